"""Build time of GMP-ECM's PARAM 1 and PARAM 3 curves: the device build's kernel time (HIP events,
gecm_last_kernel_ms) and the host build's wall time for one batch, one warm call and then the median of five.
usage: python tools/param_time.py [curves]"""
import os
import random
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "avx-ecm_amd"))
import pyecm  # noqa: E402


def main():
    curves = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
    for bits in (415, 1030):
        n = random.Random(bits).getrandbits(bits) | (1 << (bits - 1)) | 1
        eng = pyecm.Engine(n)
        for param in (1, 3):
            sig = [random.Random(param).randrange(1, 1 << 32) for _ in range(curves)]
            prm = [param] * curves
            out = []
            for mode in ("device", "host"):
                eng.set_curve_build(mode)
                times = []
                for _ in range(6):
                    t = time.perf_counter()
                    eng.build_curves(sig, params=prm)
                    wall = time.perf_counter() - t
                    times.append(eng.last_kernel_ms() if mode == "device" else wall * 1e3)
                out.append("%s %.3f ms (%s)" % (mode, statistics.median(times[1:]),
                                                "k_build_param, HIP events" if mode == "device" else "wall time of the call"))
            print("PARAM %d, %d limbs, %d curves: %s" % (param, eng.cfg.dev_limbs, curves, "; ".join(out)), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
