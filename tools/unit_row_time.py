"""Kernel time of P-1 / P+1 stage 1 with one lane and with 16 lanes per residue: the same residues
over (1, B1], both methods, at 15 and 37 limbs and a range of batch sizes; HIP events (gecm_last_kernel_ms), one warm call
and then the median and the min / max of five.  With --lanes 1 it runs on a library without the setting too (the parent
commit's: point --pkg at its avx-ecm_amd directory), so that the two columns of the table come from the two trees.
usage: python tools/unit_row_time.py [--pkg DIR] [--lanes 1|16] [--b1 B1] [--sizes n,n,..] [--bits b,b,..]"""
import argparse
import os
import random
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def series(eng, method, seeds, b1):
    times = []
    for _ in range(6):
        eng.build_seeds(method, seeds)
        eng.stage1_extend(1, b1)
        times.append(eng.last_kernel_ms())
    t = times[1:]
    return statistics.median(t), min(t), max(t)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", default=os.path.join(ROOT, "avx-ecm_amd"))
    ap.add_argument("--lanes", type=int, default=16)
    ap.add_argument("--b1", type=int, default=100000)
    ap.add_argument("--sizes", default="1,64,1024,4096,16384,65536")
    ap.add_argument("--bits", default="415,1030")
    a = ap.parse_args()
    sys.path.insert(0, a.pkg)
    import pyecm
    print("# %s" % pyecm.lib.gecm_version().decode(), flush=True)
    for bits in [int(b) for b in a.bits.split(",")]:
        rng = random.Random(bits)
        n = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
        eng = pyecm.Engine(n)
        if a.lanes != 1:
            eng.set_method_lanes(a.lanes)
        pool = [rng.randrange(n) for _ in range(1024)]
        for count in [int(s) for s in a.sizes.split(",")]:
            seeds = (pool * (count // len(pool) + 1))[:count]
            for method, name in ((pyecm.METHOD_PM1, "P-1"), (pyecm.METHOD_PP1, "P+1")):
                med, lo, hi = series(eng, method, seeds, a.b1)
                print("%d limbs %6d residues %s lanes %2d (1, %d] %d events: median %9.3f ms  min %9.3f  max %9.3f  %s"
                      % (eng.cfg.dev_limbs, count, name, eng.lanes_per_curve(), a.b1, eng.stage1_stats().tape_len, med, lo, hi,
                         eng.last_kernel_name()), flush=True)
        eng.close()
