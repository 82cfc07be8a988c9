"""Multi-modulus batches against one number at a time: stage 1 of `count` random N x `curves` curves,
timed three ways on one device —
  (a) one single-N context per number, one after another (what the command line does with a list today),
  (b) up to four single-N contexts in flight at once (stage 1 is asynchronous; launched in turn, then synced),
  (c) one multi-modulus context holding every curve,
  (d) for reference, one single-N context holding as many curves of one number as (c) holds.
Curve building is outside the timed part; one untimed run of (a) and (c) first loads the code objects and tapes.
usage: python tools/multi_bench.py [--bits 415 831] [--count 32] [--curves 4096] [--b1 100000] [--out profiles/multi]

With --curves-per-number C [C ...] it compares the two packings of a multi-modulus batch instead:
`--real-curves` curves on random N of `--bits` bits, C curves per number, stage 1 to B1 (and, with --b2, stage 2 to B2)
under every `--packing` named, in one process: one warm call, then the median of five.
usage: python tools/multi_bench.py --curves-per-number 8 16 32 64 [--packing wave lane] [--real-curves 131072]
       [--bits 415 200] [--b1 100000] [--b2 0] [--out profiles/dense]

With --stage2 it times stage 2 of a multi-modulus batch with and without sub-sequences per curve:
`--count` random N of `--bits` bits with `--curves` curves each, stage 1 to B1 once, then for every `--packing` and every
`--subseq` (1 = the plain chain, auto = by batch size) in one process: one warm stage 2 to B2, then five timed ones
(wall time of the synchronous call, median of five).  The accumulators of the first and last curve must not depend on K.
usage: python tools/multi_bench.py --stage2 --count 32 --curves 128 [--subseq 1 auto] [--packing wave lane]
       [--bits 415] [--b1 100000] [--b2 10000000] [--out profiles/subseq]"""
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


def run_dense(bits, real, cpn, packings, b1, b2, rows="off"):
    """wave against lane packing: `real` curves, cpn per number; rows: MultiEngine.set_rows"""
    import statistics
    import pyecm
    rnd = random.Random(bits * 1000 + cpn)
    count = real // cpn
    ns = [rnd.getrandbits(bits) | (1 << (bits - 1)) | 1 for _ in range(count)]
    sig = [1000 + k for k in range(count * cpn)]
    which = [i for i in range(count) for _ in range(cpn)]
    out = {"bits": bits, "numbers": count, "curves_per_number": cpn, "real_curves": count * cpn, "B1": b1, "B2": b2}
    lines = {}
    for packing in packings:
        eng = pyecm.MultiEngine(ns)
        eng.set_packing(packing)
        if rows != "off":
            eng.set_rows(rows)
        out["dev_limbs"], out["rows"] = eng.cfg.dev_limbs, rows
        t = time.perf_counter()
        eng.build_curves(sig, which)
        build_s = time.perf_counter() - t
        s1, s2 = [], []
        for call in range(6):                   # stage 1 goes on from the points the call before left: the same work
            t = time.perf_counter()
            eng.stage1(b1)
            s1.append(time.perf_counter() - t)
            if call == 0:
                lines[packing] = [eng.save_line(k) for k in (0, cpn - 1, count * cpn - 1)]
            if b2:
                t = time.perf_counter()
                eng.stage2(b2)
                s2.append(time.perf_counter() - t)
        r = {"positions": pyecm.multi_positions([cpn] * count, packing), "build_seconds": round(build_s, 3),
             "kernel": eng.last_kernel_name(), "lanes_per_curve": eng.lanes_per_curve(),
             "stage1_seconds": [round(x, 4) for x in s1], "stage1_median_of_5": round(statistics.median(s1[1:]), 4)}
        r["stage1_real_curves_per_s"] = round(count * cpn / r["stage1_median_of_5"], 1)
        if b2:
            r["stage2_seconds"] = [round(x, 4) for x in s2]
            r["stage2_median_of_5"] = round(statistics.median(s2[1:]), 4)
        out[packing] = r
        eng.close()
    if len(packings) == 2:
        a, b = out[packings[0]], out[packings[1]]
        assert lines[packings[0]] == lines[packings[1]]
        out["stage1_%s_over_%s" % tuple(packings)] = round(a["stage1_median_of_5"] / b["stage1_median_of_5"], 3)
        if b2:
            out["stage2_%s_over_%s" % tuple(packings)] = round(a["stage2_median_of_5"] / b["stage2_median_of_5"], 3)
    return out


def run_stage2(bits, count, cpn, packings, subseqs, b1, b2):
    """stage 2 with K = 1 against K by batch size, `count` numbers x `cpn` curves"""
    import statistics
    import pyecm
    rnd = random.Random(bits * 1000 + cpn)
    ns = [rnd.getrandbits(bits) | (1 << (bits - 1)) | 1 for _ in range(count)]
    sig = [1000 + k for k in range(count * cpn)]
    which = [i for i in range(count) for _ in range(cpn)]
    out = {"bits": bits, "numbers": count, "curves_per_number": cpn, "real_curves": count * cpn, "B1": b1, "B2": b2}
    for packing in packings:
        eng = pyecm.MultiEngine(ns)
        eng.set_packing(packing)
        out["dev_limbs"] = eng.cfg.dev_limbs
        eng.build_curves(sig, which)
        eng.stage1(b1)
        r = {"positions": pyecm.multi_positions([cpn] * count, packing)}
        accs = {}
        for k in subseqs:
            eng.set_stage2_subseq(k if k == "auto" else int(k))
            secs, kernel_ms = [], []
            for call in range(6):               # stage 2 starts from the stage-1 points every time: the same work
                t = time.perf_counter()
                eng.stage2(b2)
                secs.append(time.perf_counter() - t)
                kernel_ms.append(eng.last_kernel_ms())
            used, k_chunks = eng.stage2_subseq()
            accs[k] = (eng.acc(0), eng.acc(count * cpn - 1))
            r["subseq_%s" % k] = {"K": used, "k_chunks": k_chunks, "stage2_seconds": [round(x, 4) for x in secs],
                                  "stage2_median_of_5": round(statistics.median(secs[1:]), 4),
                                  "last_launch_kernel_ms": [round(x, 2) for x in kernel_ms]}
        assert len(set(accs.values())) == 1, "the accumulators depend on K"
        if len(subseqs) == 2:
            a, b = (r["subseq_%s" % k]["stage2_median_of_5"] for k in subseqs)
            r["stage2_%s_over_%s" % tuple(subseqs)] = round(a / b, 3)
        out[packing] = r
        eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves-per-number", type=int, nargs="+", default=None)
    ap.add_argument("--packing", nargs="+", choices=["wave", "lane"], default=["wave", "lane"])
    ap.add_argument("--real-curves", type=int, default=131072)
    ap.add_argument("--b2", type=int, default=0)
    ap.add_argument("--bits", type=int, nargs="+", default=[415, 831])
    ap.add_argument("--count", type=int, default=32)
    ap.add_argument("--curves", type=int, default=4096)
    ap.add_argument("--b1", type=int, default=100000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stage2", action="store_true")
    ap.add_argument("--subseq", nargs="+", default=["1", "auto"])
    ap.add_argument("--rows", choices=["off", "on", "auto"], default="off", help="with --curves-per-number: stage 1 in the row layout")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "subseq" if a.stage2 else "dense" if a.curves_per_number else "multi")
    os.makedirs(a.out, exist_ok=True)
    if a.stage2:
        for bits in a.bits:
            r = run_stage2(bits, a.count, a.curves, a.packing, a.subseq, a.b1, a.b2 or 10000000)
            print(json.dumps(r), flush=True)
            with open(os.path.join(a.out, "stage2_%d_n%d_c%d.json" % (bits, a.count, a.curves)), "w") as f:
                json.dump(r, f, indent=1)
        return
    if a.curves_per_number:
        for bits in a.bits:
            for cpn in a.curves_per_number:
                r = run_dense(bits, a.real_curves, cpn, a.packing, a.b1, a.b2, a.rows)
                print(json.dumps(r), flush=True)
                name = "dense_%d_c%d%s%s.json" % (bits, cpn, "_s2" if a.b2 else "", "" if a.rows == "off" else "_rows_" + a.rows)
                with open(os.path.join(a.out, name), "w") as f:
                    json.dump(r, f, indent=1)
        return
    for bits in a.bits:
        r = run(bits, a.count, a.curves, a.b1)
        print(json.dumps(r), flush=True)
        with open(os.path.join(a.out, "multi_bench_%d.json" % bits), "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
