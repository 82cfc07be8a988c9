"""Kernel time of P-1 / P+1 stage 2 next to an ECM batch of the same size on the same tree: the
table build (gecm_stage2_init: k_s2u_seed + k_s2u_init against k_s2_init) and the range (gecm_stage2_pair: k_s2u_gen +
k_s2_pairs against k_s2_gen + k_s2_pairs), HIP events (gecm_last_kernel_ms), one warm call and then the median of `reps`.
Under `rocprofv3 --kernel-trace --stats` (a run of its own, reps = 1) the stats file splits the range into its kernels.
Stage 1 is not run: the residues and points are stated complete to B1 (stage 2 does not care what they are).
usage: python tools/unit_s2_time.py [positions] [B1] [B2] [reps] [K: default|auto|1..32] [kinds: ecm,pm1,pp1]"""
import os
import random
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "avx-ecm_amd"))
import pyecm  # noqa: E402


def phases(eng, pairs, reps):
    init, walk = [], []
    for _ in range(reps + 1):
        eng.stage2_init()
        init.append(eng.last_kernel_ms())
        eng.stage2_pair(pairs)
        walk.append(eng.last_kernel_ms())
    return statistics.median(init[1:]), statistics.median(walk[1:])


if __name__ == "__main__":
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
    B1 = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1000000
    B2 = int(float(sys.argv[3])) if len(sys.argv) > 3 else 100000000
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    K = sys.argv[5] if len(sys.argv) > 5 else "default"
    kinds = (sys.argv[6] if len(sys.argv) > 6 else "ecm,pm1,pp1").split(",")
    rng = random.Random(415)
    n = rng.getrandbits(415) | (1 << 414) | 1
    eng = pyecm.Engine(n)
    eng.set_method_stage2(True)
    eng.set_stage2_subseq(int(K) if K.isdigit() else K)
    xs = [rng.randrange(2, n) for _ in range(count)]
    pairs = None
    for kind in kinds:
        if kind == "ecm":
            eng.build_curves(list(range(1000, 1000 + count)))
            eng.stage1_extend(1, 2)                              # a point of each curve: one doubling
            xz = eng.download_points_plain()
            eng.resume(list(range(1000, 1000 + count)), xz[0], xz[1], b1_done=B1)
        else:
            eng.build_seeds(pyecm.METHOD_PM1 if kind == "pm1" else pyecm.METHOD_PP1, None, xs=xs, b1_done=B1)
        eng.stage2_init()
        st = eng.stage2_stats()
        if pairs is None:
            pairs = pyecm.pair_primes(B1, B2, st.D, st.U)
        init_ms, walk_ms = phases(eng, pairs, reps)
        k, chunks = eng.stage2_subseq()
        print("%s: %d limbs, %d positions, B1 %d, B2 %d, D %d, U %d, %d pairs, K %d (%d chunks): table %.1f ms, range %.1f ms"
              % (kind, eng.cfg.dev_limbs, count, B1, B2, st.D, st.U, eng.stage2_stats().paired, k, chunks, init_ms, walk_ms),
              flush=True)
    eng.close()
