"""Wall time of gecm_resume_points (plain residues, converted on the device) against gecm_upload_points (reference radix,
converted on one host thread) for one full batch on the same residues, and of gecm_build_curves, whose construction of
s = (A+2)/4 from sigma is part of every resume: one warm call, then the median of five.  DESIGN.md section 14.
usage: python tools/resume_convert_time.py [curves]"""
import ctypes
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "avx-ecm_amd"))
import pyecm  # noqa: E402


def timed(fn, runs=5):
    fn()
    ts = []
    for _ in range(runs):
        t = time.perf_counter()
        rc = fn()
        ts.append(time.perf_counter() - t)
        assert rc >= 0, pyecm.lib.gecm_last_error()
    return statistics.median(ts)


def main():
    curves = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
    for bits in (415, 1023):
        rnd = random.Random(bits)
        n = rnd.getrandbits(bits) | (1 << (bits - 1)) | 1
        eng = pyecm.Engine(n)
        xs = [rnd.randrange(n) for _ in range(curves)]
        zs = [rnd.randrange(n) for _ in range(curves)]
        x, z = eng.pack(xs), eng.pack(zs)
        sig = (ctypes.c_uint64 * curves)(*range(1000, 1000 + curves))
        h = eng._h
        t_resume = timed(lambda: pyecm.lib.gecm_resume_points(h, sig, x, z, curves, 0))
        eng.batch = curves
        back = eng.download_points_plain()
        assert back == (xs, zs)
        t_build = timed(lambda: pyecm.lib.gecm_build_curves(h, sig, curves))
        t_upload = timed(lambda: pyecm.lib.gecm_upload_points(h, x, z, x, curves))
        print("%4d bits, %d curves: gecm_resume_points %.3f s (gecm_build_curves alone %.3f s), gecm_upload_points %.3f s"
              % (bits, curves, t_resume, t_build, t_upload), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
