"""Two timings of stage-1 extension, each one warm call, then the median of five:
  - the normalisation kernel (k_normalize) on 131,072 curves at 15 and 37 limbs, from its HIP events;
  - the wall time of stage1_extend(999999, 3000000) against stage1(3000000) on the same batch of 4096 curves at 415 bits,
    next to the lengths of the two tapes.
usage: python tools/extend_time.py [curves-to-normalise] [curves-to-extend]"""
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "avx-ecm_amd"))
import pyecm  # noqa: E402


def median_of_five(fn):
    fn()
    return statistics.median(fn() for _ in range(5))


def main():
    big = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
    curves = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
    for bits, limbs in ((415, 15), (1031, 37)):
        n = random.Random(bits).getrandbits(bits) | (1 << (bits - 1)) | 1
        eng = pyecm.Engine(n)
        assert eng.cfg.dev_limbs == limbs
        eng.build_curves(list(range(1000, 1000 + big)))
        eng.stage1_extend(1, 100)                      # points with a Z other than 1

        def once():
            left = eng.normalize()                      # (normalised points go through the same instructions again)
            assert left >= 0
            return eng.last_kernel_ms()
        print("k_normalize<%d>: %d curves, %.3f ms" % (limbs, big, median_of_five(once)), flush=True)
        eng.close()

    n = random.Random(415).getrandbits(415) | (1 << 414) | 1
    eng = pyecm.Engine(n)
    sig = list(range(1000, 1000 + curves))
    tape = {}

    def run(name, fn):
        def once():
            eng.build_curves(sig)
            t = time.perf_counter()
            fn()
            dt = time.perf_counter() - t
            tape[name] = eng.stage1_stats().tape_len
            return dt
        return median_of_five(once)
    t_ext = run("extend", lambda: eng.stage1_extend(999999, 3000000))
    t_full = run("full", lambda: eng.stage1(3000000))
    print("%d curves, 415 bits, %d lane(s) per curve: stage1_extend(999999, 3000000) %.3f s, tape %d bytes; stage1(3000000) %.3f s, "
          "tape %d bytes; time ratio %.3f, tape ratio %.3f"
          % (curves, eng.lanes_per_curve(), t_ext, tape["extend"], t_full, tape["full"], t_ext / t_full,
             tape["extend"] / tape["full"]), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
