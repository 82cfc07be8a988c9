"""GPU: stage 2 of a multi-modulus batch with K sub-sequences per curve (include/gecm.h gecm_set_stage2_subseq,
pyecm.Engine.set_stage2_subseq), wave- and lane-packed.  The table build and the giant steps of every
curve are cut into K interleaved chains that make the same points, so every accumulator must be, bit for bit, the one
the plain chain (K = 1, the parent's path) and a single-N context of the curve's own number give; where an inversion
meets a factor, the factor reported divides the plain chain's (the rule tests/test_gpu_stage2.py pins for one N)."""
import json
import math
import os
import random

import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

S2 = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "stage2_acc.json")))}
T35 = S2["T35N_b1_1000_b2_50000"]
T35N, K1N = int(T35["N"]), int(S2["K1N_b1_2000_b2_1e5"]["N"])
R200 = random.Random(200).getrandbits(200) | (1 << 199) | 1
PACKINGS = ("wave", "lane")
GECM_ERR_ARG = -2


def _is_prime(n):
    """Miller-Rabin with 24 fixed bases (the numbers tested are random: no adversary)"""
    if n < 2 or any(n % p == 0 for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29) if n != p):
        return n in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29)
    d, r = n - 1, 0
    while d % 2 == 0:
        d, r = d // 2, r + 1
    for a in random.Random(n & 0xffff).sample(range(2, 1 << 30), 24):
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(r - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def _prime(rnd, bits):
    """A random prime of exactly `bits` bits.  The accumulators are the plain chain's for every K as long as no
    inversion of the run fails: a curve whose order modulo a prime factor of N is smooth enough fails one, the chain
    then zeroes the batch it inverted, and which entries share a batch depends on K (a random 275-bit number lost a
    case here to its factor 1569241).  A prime N has no such curve."""
    n = rnd.getrandbits(bits) | (1 << (bits - 1)) | 1
    while n.bit_length() != bits or not _is_prime(n):
        n += 2
    return n


def _interleave(groups):
    """[(modulus index, sigma)] taking one curve of every group in turn: the library has to do the grouping"""
    out, i = [], 0
    while any(i < len(g) for g in groups):
        for m, g in enumerate(groups):
            if i < len(g):
                out.append((m, g[i]))
        i += 1
    return out


def _engine(ns, order, packing):
    import pyecm
    eng = pyecm.MultiEngine(ns)
    eng.set_packing(packing)
    eng.build_curves([s for _, s in order], [m for m, _ in order])
    assert eng.packing() == packing
    return eng


def _stage2(eng, K, b2, D, U, n):
    """one stage 2 of the batch eng holds after stage 1, with K sub-sequences per curve"""
    eng.set_stage2_subseq(K)
    eng.stage2(b2, D, U)
    used, k_chunks = eng.stage2_subseq()
    eng.scan_factors(2)
    return {"K": used, "k_chunks": k_chunks, "accs": eng.accs(), "facs": [eng.stage2_factor(k) for k in range(n)],
            "flags": [eng.curve_flag(2, k) for k in range(n)]}


_SINGLE = {}


def _single(n, sig, b1, b2, D, U):
    """(accumulators, factors, flags) of a single-N context of n, computed once per argument list"""
    key = (n, tuple(sig), b1, b2, D, U)
    if key not in _SINGLE:
        import pyecm
        e = pyecm.Engine(n)
        e.build_curves(sig)
        e.stage1(b1)
        e.stage2(b2, D, U)
        e.scan_factors(2)
        _SINGLE[key] = (e.download_acc(), [e.stage2_factor(k) for k in range(len(sig))],
                        [e.curve_flag(2, k) for k in range(len(sig))])
        e.close()
    return _SINGLE[key]


def _mine(order, m):
    return [k for k, (mm, _) in enumerate(order) if mm == m]


# ---- 1. accumulators equal for every K, both packings -----------------------------------------------------------------
B1, B2, D, U = 1000, 50000, 385, 16
NS = [T35N, K1N, R200]
GROUPS = [[T35["sigma0"] + k for k in range(8)], [100 + k for k in range(8)], [5000 + k for k in range(8)]]
ORDER = _interleave(GROUPS)


@pytest.mark.parametrize("packing", PACKINGS)
def test_accumulators_and_factors_equal_the_plain_chain_for_every_k(packing):
    eng = _engine(NS, ORDER, packing)
    eng.stage1(B1)
    plain = _stage2(eng, 1, B2, D, U, len(ORDER))
    assert plain["K"] == 1 and plain["k_chunks"] == 0
    assert [plain["accs"][k] for k in _mine(ORDER, 0)] == [int(h, 16) for h in T35["acc_hex"]]
    for K in (2, 8, 32, "auto"):
        got = _stage2(eng, K, B2, D, U, len(ORDER))
        if K == "auto":             # 64 or 192 positions: far below two wavefronts per SIMD on any device this runs on
            assert got["K"] > 1 and got["K"] & (got["K"] - 1) == 0, got["K"]
        else:
            assert got["K"] == K
        assert got["accs"] == plain["accs"], (packing, K)
        assert got["facs"] == plain["facs"] and got["flags"] == plain["flags"], (packing, K)
    eng.close()


# ---- 2. the giant-step kernel really runs, and hands over to the plain chain ------------------------------------------
# B2 = 600,000 with D = 210, U = 4: about 2,850 giant steps, made in chunks of 512, so a range has six generate marks;
# the last one is the plain chain's (it reproduces the reference's last batch) and takes its two predecessors from the
# sub-sequences' scratch.
G_B1, G_B2, G_D, G_U = 2000, 600000, 210, 4
G_NS = [T35N, K1N, R200, _prime(random.Random(415), 415), _prime(random.Random(100), 100)]
G_COUNTS = [1, 63, 64, 65, 3]       # lane: a number across a wavefront boundary, several in one wavefront, a padded tail
G_SIG = [[7000 + 100 * m + k for k in range(c)] for m, c in enumerate(G_COUNTS)]


@pytest.mark.parametrize("packing", PACKINGS)
def test_giant_steps_with_sub_sequences_run_and_hand_over_to_the_plain_chain(packing):
    pick = [0, 1, 2, 3, 4] if packing == "lane" else [0, 3, 4]          # wave: 1, 65 and 3 curves
    ns, groups = [G_NS[i] for i in pick], [G_SIG[i] for i in pick]
    order = _interleave(groups)
    eng = _engine(ns, order, packing)
    eng.stage1(G_B1)
    plain = _stage2(eng, 1, G_B2, G_D, G_U, len(order))
    assert plain["k_chunks"] == 0
    for K in (8, 32):
        got = _stage2(eng, K, G_B2, G_D, G_U, len(order))
        assert got["K"] == K and got["k_chunks"] >= 2, (packing, K, got["k_chunks"])
        assert got["accs"] == plain["accs"], (packing, K)
    eng.close()
    for m, n in enumerate(ns):
        acc1, _, _ = _single(n, groups[m], G_B1, G_B2, G_D, G_U)
        assert [plain["accs"][k] for k in _mine(order, m)] == acc1, (packing, m)


# ---- 3. limb counts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packing,nl", [("wave", 8), ("wave", 15), ("wave", 23), ("wave", 37), ("lane", 8), ("lane", 10),
                                        ("lane", 15)])
def test_limb_counts(packing, nl):
    rnd = random.Random(2100 + nl)
    top = 28 * nl - 5
    ns = [_prime(rnd, top), _prime(rnd, 64), _prime(rnd, top)]
    groups = [[rnd.randrange(6, 1 << 40) for _ in range(c)] for c in (3, 5, 4)]
    order = _interleave(groups)
    eng = _engine(ns, order, packing)
    assert eng.cfg.dev_limbs == nl
    eng.stage1(300)
    plain = _stage2(eng, 1, 20000, 210, 2, len(order))
    got = _stage2(eng, 8, 20000, 210, 2, len(order))
    eng.close()
    assert got["K"] == 8 and plain["K"] == 1
    assert all(plain["accs"])                               # no inversion failed: the comparison is of real products
    assert got["accs"] == plain["accs"]


# ---- 4. amin = 0 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packing", PACKINGS)
def test_a_range_from_the_origin_keeps_the_plain_chain(packing):
    """B1 = 65 < D = 385: amin = 0, the reference's first giant steps are degenerate and every chunk is a plain chain
    (the table is still built with sub-sequences)"""
    eng = _engine(NS, ORDER, packing)
    eng.stage1(65)
    plain = _stage2(eng, 1, B2, D, U, len(ORDER))
    got = _stage2(eng, 8, B2, D, U, len(ORDER))
    eng.close()
    assert got["K"] == 8 and got["k_chunks"] == 0
    assert got["accs"] == plain["accs"] and got["facs"] == plain["facs"] and got["flags"] == plain["flags"]


# ---- 5. failure planes stay on their curves ---------------------------------------------------------------------------
# The product of the primes from 10007 up that fits 408 bits: on every sigma used here the stage-2 chain meets batch
# inversions that fail, so the factor reported comes from a failure record and not from gcd(accumulator, N).
def _small_prime_product(bits):
    n, p = 1, 10007
    while True:
        if all(p % q for q in range(3, int(p ** 0.5) + 1, 2)):
            if (n * p).bit_length() > bits:
                return n
            n *= p
        p += 2


DEGENERATE_N = _small_prime_product(408)
DEGENERATE_B1, DEGENERATE_B2 = 65, 50085


@pytest.mark.parametrize("packing", PACKINGS)
def test_failure_plane_factors_stay_on_their_curves(packing):
    sig, hsig = list(range(1000, 1008)), list(range(42, 50))
    order = _interleave([hsig, sig])
    eng = _engine([T35N, DEGENERATE_N], order, packing)
    eng.stage1(DEGENERATE_B1)
    plain = _stage2(eng, 1, DEGENERATE_B2, D, U, len(order))
    got = _stage2(eng, 8, DEGENERATE_B2, D, U, len(order))
    eng.close()
    assert got["K"] == 8
    hacc, hfac, hflag = _single(T35N, hsig, DEGENERATE_B1, DEGENERATE_B2, D, U)
    from_failure_plane = 0
    for k, (m, s) in enumerate(order):
        f = got["facs"][k]
        if m == 0:
            j = hsig.index(s)
            assert got["accs"][k] == hacc[j] and f == hfac[j] and got["flags"][k] == hflag[j], (k, s)
        else:
            f1 = plain["facs"][k]
            assert f and f1, (k, s, f, f1)
            assert 1 < f[0] < DEGENERATE_N and DEGENERATE_N % f[0] == 0 and f1[0] % f[0] == 0, (k, s, f[0], f1[0])
            if math.gcd(got["accs"][k], DEGENERATE_N) != f[0]:
                from_failure_plane += 1
    assert from_failure_plane >= 1


# ---- 6. setting and accounting ----------------------------------------------------------------------------------------
def test_setting_values_and_the_default():
    import pyecm
    eng = _engine(NS, ORDER, "wave")
    for bad in (3, 64, -2):
        assert pyecm.lib.gecm_set_stage2_subseq(eng._h, bad) == GECM_ERR_ARG, bad
    assert pyecm.lib.gecm_set_stage2_subseq(None, 8) == GECM_ERR_ARG
    assert pyecm.lib.gecm_get_stage2_subseq(None, None) == GECM_ERR_ARG
    with pytest.raises(ValueError):
        eng.set_stage2_subseq("many")
    assert eng.stage2_subseq() == (0, 0)                    # before the first stage 2
    eng.stage1(B1)
    eng.stage2(B2, D, U)                                    # nothing set: what a multi-modulus context always did
    assert eng.stage2_subseq() == (1, 0)
    accs = eng.accs()
    eng.set_stage2_subseq(8)
    assert eng.stage2_subseq() == (1, 0)                    # the setting waits for the next stage 2
    eng.set_stage2_subseq("default")
    eng.stage2(B2, D, U)
    assert eng.stage2_subseq() == (1, 0) and eng.accs() == accs
    eng.close()
    # a single-N context takes an explicit K too, and its own default is by batch size, as before
    single = pyecm.Engine(K1N)
    single.build_curves(GROUPS[1])
    single.stage1(B1)
    single.stage2(B2, D, U)
    k_default = single.stage2_subseq()[0]
    acc = single.download_acc()
    assert k_default > 1
    single.set_stage2_subseq(2)
    single.stage2(B2, D, U)
    assert single.stage2_subseq()[0] == 2 and single.download_acc() == acc
    single.set_stage2_subseq("auto")
    single.stage2(B2, D, U)
    assert single.stage2_subseq()[0] == k_default
    single.close()


def test_batch_bytes_count_the_sub_sequence_scratch():
    import pyecm
    rnd = random.Random(15)
    ns = [rnd.getrandbits(415) | (1 << 414) | 1 for _ in range(5)]
    counts = [1, 63, 64, 65, 3]
    curves = sum(counts)
    positions = pyecm.multi_positions(counts, "lane")
    eng = pyecm.MultiEngine(ns)
    eng.set_packing("lane")
    assert eng.cfg.dev_limbs == 15
    plain = eng.batch_bytes(curves, True, 1000, D, U)
    eng.set_stage2_subseq("auto")
    auto = eng.batch_bytes(curves, True, 1000, D, U)
    eng.close()
    single = pyecm.Engine(ns[0])
    assert single.cfg.dev_limbs == 15
    assert auto == single.batch_bytes(positions, True, 1000, D, U)     # the same sums
    single.close()
    assert auto > plain


@pytest.mark.parametrize("packing", PACKINGS)
def test_resume_then_stage2_with_sub_sequences_equals_the_straight_run(packing):
    import pyecm
    eng = _engine(NS, ORDER, packing)
    eng.stage1(B1)
    lines = eng.save_lines()
    straight = _stage2(eng, 1, B2, D, U, len(ORDER))
    eng.close()
    eng = pyecm.MultiEngine(NS)
    eng.set_packing(packing)
    eng.resume_lines(lines, b1_done=B1)
    assert eng.save_lines() == lines
    got = _stage2(eng, 8, B2, D, U, len(ORDER))
    eng.close()
    assert got["K"] == 8
    assert got["accs"] == straight["accs"] and got["facs"] == straight["facs"]
