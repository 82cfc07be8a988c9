"""Multi-modulus batches against one number at a time: stage 1 of `count` random N x `curves` curves,
timed three ways on one device —
  (a) one single-N context per number, one after another (what the command line does with a list today),
  (b) up to four single-N contexts in flight at once (stage 1 is asynchronous; launched in turn, then synced),
  (c) one multi-modulus context holding every curve,
  (d) for reference, one single-N context holding as many curves of one number as (c) holds.
Curve building is outside the timed part; one untimed run of (a) and (c) first loads the code objects and tapes.
usage: python tools/multi_bench.py [--bits 415 831] [--count 32] [--curves 4096] [--b1 100000] [--out profiles/multi]"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "avx-ecm_amd"))


def run(bits, count, curves, b1):
    import pyecm
    rnd = random.Random(bits)
    ns = [rnd.getrandbits(bits) | (1 << (bits - 1)) | 1 for _ in range(count)]
    sig = [[1000 + i * curves + k for k in range(curves)] for i in range(count)]
    singles = [pyecm.Engine(n) for n in ns]
    multi = pyecm.MultiEngine(ns)

    def build_singles():
        for e, s in zip(singles, sig):
            e.build_curves(s)

    def build_multi():
        multi.build_curves([x for s in sig for x in s], [i for i, s in enumerate(sig) for _ in s])

    def seq():
        for e in singles:
            e.stage1(b1)

    def four():
        for i in range(0, count, 4):
            group = singles[i:i + 4]
            for e in group:
                e.stage1(b1, sync=False)
            for e in group:
                e.sync()

    def one():
        multi.stage1(b1)

    # untimed: load the code objects and build the tapes of B1 (stage 1 runs on the points a build leaves)
    build_singles()
    build_multi()
    seq()
    one()
    out = {"bits": bits, "numbers": count, "curves_per_number": curves, "B1": b1,
           "dev_limbs": multi.cfg.dev_limbs}
    for name, build, fn in (("a_sequential_single", build_singles, seq), ("b_four_concurrent_single", build_singles, four),
                            ("c_one_multi_batch", build_multi, one)):
        build()
        t = time.perf_counter()
        fn()
        dt = time.perf_counter() - t
        out[name] = {"seconds": round(dt, 4), "curves_per_s": round(count * curves / dt, 1)}
    # (d) the figure (c) is measured against: one number, count x curves curves in one single-N context
    big = pyecm.Engine(ns[0])
    big.build_curves([x for s in sig for x in s])
    big.stage1(b1)                              # untimed: the layout of this batch size
    big.build_curves([x for s in sig for x in s])
    t = time.perf_counter()
    big.stage1(b1)
    dt = time.perf_counter() - t
    out["d_one_single_context_all_curves"] = {"seconds": round(dt, 4), "curves_per_s": round(count * curves / dt, 1),
                                              "lanes_per_curve": big.lanes_per_curve()}
    big.close()
    out["lanes_per_curve_multi"] = multi.lanes_per_curve()
    out["lanes_per_curve_single"] = singles[0].lanes_per_curve()
    out["speedup_c_over_a"] = round(out["a_sequential_single"]["seconds"] / out["c_one_multi_batch"]["seconds"], 3)
    # the multi batch's lines are the single contexts' (one curve per number)
    for i in (0, count - 1):
        assert multi.save_line(i * curves) == singles[i].save_line(0)
    for e in singles:
        e.close()
    multi.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, nargs="+", default=[415, 831])
    ap.add_argument("--count", type=int, default=32)
    ap.add_argument("--curves", type=int, default=4096)
    ap.add_argument("--b1", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    for bits in a.bits:
        r = run(bits, a.count, a.curves, a.b1)
        print(json.dumps(r), flush=True)
        with open(os.path.join(a.out, "multi_bench_%d.json" % bits), "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
