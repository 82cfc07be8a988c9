"""Kernel time of stage 1 on wide contexts: gecm_stage1(B1) on 4096 and 131072 curves of a 1039-, a
1247- and a 1311-bit number (41, 48 and 48 rows), HIP events (gecm_last_kernel_ms: every launch of the call), one warm call
and then the median and the min / max of three.  Next to them, from the same run, the library's 1030-bit number in the
32-lane layout (38 rows, the canon pass included) as the yardstick, and - where oracle/_ref holds the reference binary - the
reference on the host's cores for the same B1 on 1247 bits.  The batch is built once per size: the time of a launch does
not depend on the points it starts from; the host's build and reduction times are printed with it.
usage: python tools/wide_time.py [--b1 B1] [--sizes n,n,..] [--bits b,b,..] [--ref-threads T]"""
import argparse
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "avx-ecm_amd"))


def series(eng, b1, reps=3):
    times = []
    for _ in range(reps + 1):
        eng.stage1(b1)
        times.append(eng.last_kernel_ms())
    t = times[1:]
    return statistics.median(t), min(t), max(t)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--b1", type=int, default=100000)
    ap.add_argument("--sizes", default="4096,131072")
    ap.add_argument("--bits", default="1030,1039,1247,1311")
    ap.add_argument("--ref-threads", type=int, default=0)
    a = ap.parse_args()
    import pyecm
    print("# %s" % pyecm.lib.gecm_version().decode(), flush=True)
    for bits in [int(b) for b in a.bits.split(",")]:
        n = random.Random(bits).getrandbits(bits) | (1 << (bits - 1)) | 1
        for curves in [int(s) for s in a.sizes.split(",")]:
            eng = pyecm.Engine(n, wide=True)
            eng.set_special_form(False)
            eng.set_lanes_per_curve(32)
            t0 = time.time()
            eng.build_curves(list(range(1000, 1000 + curves)))
            t_build = time.time() - t0
            med, lo, hi = series(eng, a.b1)
            t0 = time.time()
            eng.save_line(0)                    # the download and, on a wide context, the host's reduction of every curve
            t_plain = time.time() - t0
            print("%4d bits %2d limbs wide %d %6d curves B1 %d: median %10.3f ms  min %10.3f  max %10.3f  %s   (host: build %.2f s, "
                  "plain residues %.2f s)" % (bits, eng.cfg.dev_limbs, eng.is_wide(), curves, a.b1, med, lo, hi,
                                              eng.last_kernel_name(), t_build, t_plain), flush=True)
            eng.close()
    ref = os.path.join(ROOT, "oracle", "_ref", "avx-ecm-52")
    if a.ref_threads and os.path.exists(ref):
        n = random.Random(1247).getrandbits(1247) | (1 << 1246) | 1
        curves = 8 * a.ref_threads
        with tempfile.TemporaryDirectory() as d:
            t0 = time.time()
            subprocess.run([ref, str(n), str(curves), str(a.b1), str(a.ref_threads), str(a.b1), "1000"], cwd=d, capture_output=True,
                           timeout=900)
            dt = time.time() - t0
        print("reference avx-ecm-52, 1247 bits, %d curves on %d threads, B1 %d: %.2f s wall, %.1f curves/s"
              % (curves, a.ref_threads, a.b1, dt, curves / dt), flush=True)
