"""Kernel time of P-1 / P+1 stage 1: k_unit on a batch of residues over (1, B1], both methods, next
to k_stage1 (one curve per lane) on the same batch size and the same tape; HIP events (gecm_last_kernel_ms), one warm call
and then the median of five.
usage: python tools/unit_time.py [residues] [B1]"""
import os
import random
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "avx-ecm_amd"))
import pyecm  # noqa: E402


def median_ms(eng, launch):
    times = []
    for _ in range(6):
        launch()
        eng.stage1_extend(1, B1)
        times.append(eng.last_kernel_ms())
    return statistics.median(times[1:]), eng.last_kernel_name()


if __name__ == "__main__":
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
    B1 = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
    for bits in (415, 1030):
        rng = random.Random(bits)
        n = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
        eng = pyecm.Engine(n)
        seeds = [rng.randrange(n) for _ in range(count)]
        sig = list(range(1000, 1000 + count))
        eng.set_lanes_per_curve(1)
        row = {}
        row["ECM"] = median_ms(eng, lambda: eng.build_curves(sig))
        row["P-1"] = median_ms(eng, lambda: eng.build_seeds(pyecm.METHOD_PM1, seeds))
        row["P+1"] = median_ms(eng, lambda: eng.build_seeds(pyecm.METHOD_PP1, seeds))
        st = eng.stage1_stats()
        print("%d limbs, %d residues, (1, %d], %d tape events: " % (eng.cfg.dev_limbs, count, B1, st.tape_len) +
              "; ".join("%s %.1f ms (%s)" % (k, v[0], v[1]) for k, v in row.items()) +
              "; ECM / P-1 = %.2f, P+1 / P-1 = %.3f" % (row["ECM"][0] / row["P-1"][0], row["P+1"][0] / row["P-1"][0]), flush=True)
        eng.close()
