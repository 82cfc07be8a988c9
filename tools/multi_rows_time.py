"""Kernel time of stage 1 of a multi-modulus curve batch with the default layout (1 or 2 lanes per curve) and with 32 lanes
per curve: gecm_stage1(B1) on the same curves at a range of padded batch sizes, HIP events
(gecm_last_kernel_ms: every launch of the call, the canon pass after the row kernel included), one warm call and then the
median and the min / max of five.  The curves are spread evenly over 32 numbers of one limb class; wave packing pads every
number to 64 positions, so below 2048 positions it takes positions / 64 numbers instead.  The batch is built once per size:
the time of a launch does not depend on the points it starts from.
With --rows off it runs on a library without the setting too (the parent commit's: point --pkg at its avx-ecm_amd
directory), so that the two columns of the table come from the two trees.
usage: python tools/multi_rows_time.py [--pkg DIR] [--rows off|on|auto] [--b1 B1] [--sizes n,n,..] [--bits b,b,..]
                                       [--packings wave,lane]"""
import argparse
import os
import random
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NUMBERS = 32


def series(eng, b1):
    times = []
    for _ in range(6):
        eng.stage1(b1)
        times.append(eng.last_kernel_ms())
    t = times[1:]
    return statistics.median(t), min(t), max(t)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", default=os.path.join(ROOT, "avx-ecm_amd"))
    ap.add_argument("--rows", default="on")
    ap.add_argument("--b1", type=int, default=100000)
    ap.add_argument("--sizes", default="64,1024,4096,8192,16384,32768,65536")
    ap.add_argument("--bits", default="415,1030")
    ap.add_argument("--packings", default="wave,lane")
    a = ap.parse_args()
    sys.path.insert(0, a.pkg)
    import pyecm
    print("# %s" % pyecm.lib.gecm_version().decode(), flush=True)
    for bits in [int(b) for b in a.bits.split(",")]:
        rng = random.Random(bits)
        ns = [rng.getrandbits(bits) | (1 << (bits - 1)) | 1 for _ in range(NUMBERS)]
        for packing in a.packings.split(","):
            if packing == "lane" and bits > pyecm.lib.gecm_multi_packing_max_bits(1):
                continue
            for positions in [int(s) for s in a.sizes.split(",")]:
                numbers = NUMBERS if packing == "lane" else min(NUMBERS, positions // 64)
                each = positions // numbers
                eng = pyecm.MultiEngine(ns[:numbers])
                eng.set_packing(packing)
                if a.rows != "off":
                    eng.set_rows(a.rows)
                eng.build_curves([rng.randrange(6, 1 << 63) for _ in range(numbers * each)],
                                 [g for g in range(numbers) for _ in range(each)])
                med, lo, hi = series(eng, a.b1)
                print("%d limbs %s-packed %6d positions %2d numbers rows %-4s lanes %2d B1 %d: median %9.3f ms  min %9.3f  max %9.3f  %s"
                      % (eng.cfg.dev_limbs, packing, positions, numbers, a.rows, eng.lanes_per_curve(), a.b1, med, lo, hi,
                         eng.last_kernel_name()), flush=True)
                eng.close()
