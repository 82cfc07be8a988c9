"""GPU tests of P-1 and P+1 stage 2: k_s2u_seed, k_s2u_init, k_s2u_gen and their _multi / _lane twins
feeding the shared pair walk, through gecm_set_method_stage2 and the stage-2 calls.  Every expected accumulator is
tests/unit_s2_model.py's product of V_{a D}(P) - V_u(P) in Python integers, in the reference's Montgomery radix as
gecm_download_acc returns it."""
import json
import math
import os
import random

import pytest

from conftest import GOLDEN
from unit_model import (METHOD_PM1, METHOD_PP1, OFFSET, UNIT_LIMBS, class_moduli, expected, exponent, method_line,
                        random_modulus, seeds_for)
from unit_s2_model import (CLASSES, OTHER_DU, PHASE, PHASE_MID, S2_RING, WRAP, maxbits, pair_map, plain_acc, planted_case,
                           shifts_of, to_ref)

pytestmark = pytest.mark.gpu

METHODS = (METHOD_PM1, METHOD_PP1)
BATCH = 70                                   # one full block and a ragged tail
NAME = {METHOD_PM1: "P-1", METHOD_PP1: r"P\+1"}


@pytest.fixture(scope="module")
def pyecm():
    import pyecm
    return pyecm


@pytest.fixture(scope="module")
def engines(pyecm):
    """one context per modulus for the whole module, stage 2 of method batches switched on"""
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = pyecm.Engine(n)
            cache[n].set_method_stage2(True)
        return cache[n]
    yield get
    for e in cache.values():
        e.close()


def _want(pyecm, method, n, xs, cases, D, U):
    maps = [pair_map(pyecm, c) for c in cases]
    return [to_ref(plain_acc(method, x, n, maps, D, U), n, maxbits(n)) for x in xs]


def _stage1(eng, method, n, seeds, b1):
    """a fresh batch taken to b1: the plain residues, and the lines it writes"""
    eng.build_seeds(method, seeds)
    eng.stage1_extend(1, b1)
    xs = [expected(method, s, exponent(1, b1), n) for s in seeds]
    lines = eng.save_lines_std()
    assert lines == [method_line(method, b1, n, x, s) for x, s in zip(xs, seeds)]
    return xs, lines


# ---- 1. limb classes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("nl", UNIT_LIMBS)
def test_every_limb_class_both_ends(pyecm, engines, nl, method):
    b1, b2, D, U = CLASSES
    rng = random.Random(300 * nl + method)
    for n in class_moduli(nl):
        eng = engines(n)
        assert eng.cfg.dev_limbs == nl and eng.method_stage2()
        seeds = seeds_for(n, BATCH, rng)
        xs, lines = _stage1(eng, method, n, seeds, b1)
        eng.stage2(b2, D=D, U=U)
        assert eng.download_acc() == _want(pyecm, method, n, xs, [CLASSES], D, U)
        assert eng.save_lines_std() == lines                 # X and Z of the batch are untouched


# ---- 2. chunk boundary and ring wrap -----------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_more_than_two_chunks_and_a_wrapped_ring(pyecm, engines, method):
    b1, b2, D, U = WRAP
    v, u, amin = pair_map(pyecm, WRAP)
    assert 4 * U + 2 * U * shifts_of(v, u) > S2_RING and amin > 0
    n = class_moduli(15)[0]
    eng = engines(n)
    seeds = seeds_for(n, BATCH, random.Random(41 + method))
    xs, _ = _stage1(eng, method, n, seeds, b1)
    eng.stage2(b2, D=D, U=U)
    assert eng.download_acc() == _want(pyecm, method, n, xs, [WRAP], D, U)


# ---- 3. sub-sequences ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_sub_sequences_give_the_same_accumulators(pyecm, engines, method):
    b1, b2, D, U = WRAP
    n = class_moduli(15)[1]
    eng = engines(n)
    seeds = seeds_for(n, BATCH, random.Random(43 + method))
    xs, _ = _stage1(eng, method, n, seeds, b1)
    want = _want(pyecm, method, n, xs, [WRAP], D, U)
    try:
        for k in (1, 2, 8, 32, "auto"):
            eng.set_stage2_subseq(k)
            eng.stage2(b2, D=D, U=U)
            K, chunks = eng.stage2_subseq()
            assert K == k if k != "auto" else K > 1          # 70 positions: two wavefronts, far from filling the chip
            assert (chunks > 0) == (K > 1)
            assert eng.download_acc() == want, k
    finally:
        eng.set_stage2_subseq("default")


# ---- 4. phase calls --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_phase_calls_and_stats(pyecm, engines, method):
    b1, b2, D, U = CLASSES
    n = class_moduli(15)[0]
    eng = engines(n)
    seeds = seeds_for(n, BATCH, random.Random(47 + method))
    xs, lines = _stage1(eng, method, n, seeds, b1)
    want = _want(pyecm, method, n, xs, PHASE, D, U)
    maps = [pyecm.pair_primes(*c) for c in PHASE]
    eng.stage2_init(D, U)
    for m in maps:
        eng.stage2_pair(m)
    assert eng.download_acc() == want
    st = eng.stage2_stats()
    sh = [shifts_of(*pair_map(pyecm, c)[:2]) for c in PHASE]
    paired = sum(m.steps for m in maps) - sum(sh)            # every entry that is not a window shift
    assert (st.D, st.U, st.L, st.paired) == (D, U, 2 * U, paired)
    assert st.amin_last == maps[1].amin + U * sh[1]
    assert st.numinv == 1 + sum(2 + s for s in sh)
    assert st.device_inversions == (1 if method == METHOD_PM1 else 0)
    # the tape made ahead of time
    eng.stage2_init(D, U)
    eng.stage2_pair_prepare(maps[0], D, U)
    eng.stage2_pair(maps[0])
    eng.stage2_pair_prepare(maps[1], D, U)
    eng.stage2_pair(maps[1])
    assert eng.download_acc() == want
    # another (D, U) in between starts clean, and so does the one after it
    d2, u2 = OTHER_DU[2:]
    eng.stage2(b2, D=d2, U=u2)
    assert eng.download_acc() == _want(pyecm, method, n, xs, [OTHER_DU], d2, u2)
    eng.stage2_init(D, U)
    for m in maps:
        eng.stage2_pair(m)
    assert eng.download_acc() == want and eng.save_lines_std() == lines
    for m in maps:
        pyecm.lib.gecm_pairmap_release(m)


# ---- 5. multi-modulus --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packing", ["wave", "lane"])
def test_multi_modulus_both_packings(pyecm, packing):
    b1, b2, D, U = CLASSES
    rng = random.Random(53)
    ns = [random_modulus(b, rng) for b in (64, 200, 412)]
    seeds = [s for n in ns for s in (2 * pow(7, -1, n) % n, 6 * pow(5, -1, n) % n)]
    which = [i for i in range(len(ns)) for _ in range(2)]
    eng = pyecm.MultiEngine(ns)
    try:
        eng.set_method_stage2(True)
        eng.set_packing(packing)
        eng.build_seeds(METHOD_PP1, seeds, which)
        eng.stage1_extend(1, b1)
        assert eng.packing() == packing
        m = pair_map(pyecm, CLASSES)
        want = []
        for s, w in zip(seeds, which):
            x = expected(METHOD_PP1, s, exponent(1, b1), ns[w])
            want.append(to_ref(plain_acc(METHOD_PP1, x, ns[w], [m], D, U), ns[w], maxbits(ns[w])))
        for k in (1, "auto"):
            eng.set_stage2_subseq(k)
            eng.stage2(b2, D=D, U=U)
            K, chunks = eng.stage2_subseq()
            assert (K == 1) if k == 1 else (K > 1 and chunks > 0)
            assert eng.accs() == want, k
    finally:
        eng.close()


# ---- 6. factors --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_planted_factor(pyecm, engines, method):
    b1, b2, D, U = CLASSES
    n, p, r, seed = planted_case(method, b1, b2)
    eng = engines(n)
    seeds = [seed] + [s for s in seeds_for(n, BATCH + 8, random.Random(59 + method)) if math.gcd(s, n) == 1][5:BATCH + 4]
    assert len(seeds) == BATCH
    xs, _ = _stage1(eng, method, n, seeds, b1)
    s1 = [k for k, x in enumerate(xs) if 1 < math.gcd((x - OFFSET[method]) % n, n) < n]
    assert 0 not in s1
    assert eng.scan_factors(1)[0] == len(s1)
    eng.stage2(b2, D=D, U=U)
    accs = [plain_acc(method, x, n, [pair_map(pyecm, CLASSES)], D, U) for x in xs]
    gcds = [math.gcd(a, n) for a in accs]
    hits = [k for k, g in enumerate(gcds) if 1 < g < n]
    assert gcds[0] == p and 0 in hits
    count, first = eng.scan_factors(2)
    assert (count, first) == (len(hits), hits[0])
    assert [k for k in range(BATCH) if eng.curve_flag(2, k)] == hits
    assert eng.stage2_factor(0) == (p, True)
    for k in hits:
        assert eng.stage2_factor(k)[0] == gcds[k]


def test_pm1_seed_sharing_a_factor_with_n(pyecm, engines):
    b1, b2, D, U = CLASSES
    n, p, r, seed = planted_case(METHOD_PM1, b1, b2)
    eng = engines(n)
    seeds = [3 * p, 7, 5 * r, 11]
    xs, _ = _stage1(eng, METHOD_PM1, n, seeds, b1)
    assert [math.gcd(x, n) for x in xs] == [p, 1, r, 1]
    eng.stage2(b2, D=D, U=U)
    assert eng.stage2_factor(0)[0] == p and eng.stage2_factor(2)[0] == r
    eng.scan_factors(2)
    assert eng.curve_flag(2, 0) and eng.curve_flag(2, 2)
    want = _want(pyecm, METHOD_PM1, n, [xs[1], xs[3]], [CLASSES], D, U)
    got = eng.download_acc()
    assert [got[1], got[3]] == want


# ---- 7. continuation and opt-in ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_stage1_goes_on_and_the_setting_is_opt_in(pyecm, engines, method):
    b1, b2, D, U = CLASSES
    n = class_moduli(15)[0]
    eng = engines(n)
    seeds = seeds_for(n, BATCH, random.Random(61 + method))
    _stage1(eng, method, n, seeds, b1)
    eng.stage2(b2, D=D, U=U)
    eng.stage1_extend(b1, 2 * b1)
    assert eng.save_lines_std() == [method_line(method, 2 * b1, n, expected(method, s, exponent(1, 2 * b1), n), s) for s in seeds]
    pairs = pyecm.pair_primes(2 * b1, b2, D, U)
    eng.set_method_stage2(False)
    try:
        assert not eng.method_stage2()
        for call in (lambda: eng.stage2(b2), lambda: eng.stage2_prepare(b2), lambda: eng.stage2_init(), lambda: eng.stage2_pair(pairs),
                     lambda: eng.stage2_pair_prepare(pairs, D, U), lambda: eng.scan_factors(2), lambda: eng.stage2_factor(0)):
            with pytest.raises(pyecm.GecmError, match=r"\(-4\).*not available on a %s batch" % NAME[method]):
                call()
    finally:
        eng.set_method_stage2(True)
        pyecm.lib.gecm_pairmap_release(pairs)
    # the other refusals of a method batch stay with the setting on
    for call in (lambda: eng.stage1(1000), eng.normalize, eng.download_s, lambda: eng.save_line(0)):
        with pytest.raises(pyecm.GecmError, match=r"\(-4\).*not available on a %s batch" % NAME[method]):
            call()


def test_setting_changes_nothing_on_curves(pyecm):
    case = json.load(open(os.path.join(GOLDEN, "stage2_acc.json")))[0]
    eng = pyecm.Engine(int(case["N"]), digitbits=case["digitbits"])
    try:
        eng.set_method_stage2(True)
        eng.build_curves([case["sigma0"] + k for k in range(case["curves"])])
        assert eng.method_stage2()                            # it holds across builds
        eng.stage1(case["B1"])
        eng.stage2(case["B2"])
        st = eng.stage2_stats()
        assert [st.ptadds, st.numinv, st.paired] == case["stage2_counts"]
        assert eng.download_acc() == [int(h, 16) for h in case["acc_hex"]]
    finally:
        eng.close()
