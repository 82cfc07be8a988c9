"""Wall time of gecm_build_curves with the construction on the host (worker threads, then an upload) and on the device
(k_build), and the device build's own kernel time: 131,072 curves at 415 and 1023 bits, and a multi-modulus batch of 32
numbers x 4096 curves at 415 bits.  One warm call, then the median of five, per mode; every call in this one process,
each under its own time limit (an alarm that ends the process).  DESIGN.md section 15.
usage: python tools/build_time.py [curves [numbers curves-per-number]]"""
import ctypes
import os
import random
import signal
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "avx-ecm_amd"))
import pyecm  # noqa: E402

CALL_LIMIT_S = 60


def timed(fn, runs=5):
    """(median wall seconds, median of what `fn` returns) over `runs` calls after a warm one"""
    ts, vals = [], []
    for i in range(runs + 1):
        signal.alarm(CALL_LIMIT_S)
        t = time.perf_counter()
        v = fn()
        dt = time.perf_counter() - t
        signal.alarm(0)
        if i:
            ts.append(dt)
            vals.append(v)
    return statistics.median(ts), statistics.median(vals)


def measure(label, eng, build):
    row = {}
    for mode in ("host", "device"):
        eng.set_curve_build(mode)

        def call():
            rc = build()
            assert rc >= 0, pyecm.lib.gecm_last_error()
            return eng.last_kernel_ms()
        row[mode] = timed(call)
        assert eng.curve_build() == mode
    print("%-44s host %.3f s, device %.4f s (kernel %.2f ms): %.0fx" %
          (label, row["host"][0], row["device"][0], row["device"][1], row["host"][0] / row["device"][0]), flush=True)


def main():
    curves = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
    numbers, per = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (32, 4096)
    for bits in (415, 1023):
        rnd = random.Random(bits)
        eng = pyecm.Engine(rnd.getrandbits(bits) | (1 << (bits - 1)) | 1)
        sig = (ctypes.c_uint64 * curves)(*range(1000, 1000 + curves))
        measure("%4d bits, %d curves" % (bits, curves), eng, lambda: pyecm.lib.gecm_build_curves(eng._h, sig, curves))
        eng.close()
    rnd = random.Random(32)
    eng = pyecm.MultiEngine([rnd.getrandbits(415) | (1 << 414) | 1 for _ in range(numbers)])
    total = numbers * per
    sig = (ctypes.c_uint64 * total)(*range(1000, 1000 + total))
    idx = (ctypes.c_uint32 * total)(*[k % numbers for k in range(total)])
    measure(" 415 bits, %d numbers x %d curves" % (numbers, per), eng,
            lambda: pyecm.lib.gecm_build_curves_multi(eng._h, sig, idx, total))
    eng.close()


if __name__ == "__main__":
    main()
