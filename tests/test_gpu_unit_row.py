"""GPU tests of P-1 and P+1 stage 1 with a residue per 16-lane DPP row: k_unit_row through
gecm_set_method_lanes, gecm_build_seeds and gecm_stage1_extend, on single-N contexts and on multi-modulus contexts of both
packings.  Every comparison is of exact integers or line bytes against Python (tests/unit_model.py), as in
tests/test_gpu_unit.py: the 16-lane kernel must give the integers the one-lane kernel gives."""
import os
import random

import pytest

from unit_model import (METHOD_PM1, METHOD_PP1, OFFSET, RULE9_SEGMENT, class_moduli, expected, exponent, factor_case, jacobi,
                        method_line, py_gcd_flag, random_modulus, seeds_for)
from unit_row_model import ROW_LIMBS, row_shape

pytestmark = pytest.mark.gpu

METHODS = (METHOD_PM1, METHOD_PP1)
E1000 = exponent(1, 1000)
E9 = exponent(*RULE9_SEGMENT)
BATCH = 70                                   # one full block and a ragged tail


@pytest.fixture(scope="module")
def pyecm():
    import pyecm
    return pyecm


@pytest.fixture(scope="module")
def engines(pyecm):
    """one context per modulus for the whole module, set to 16 lanes per residue"""
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = pyecm.Engine(n)
            cache[n].set_method_lanes(16)
        return cache[n]
    yield get
    for e in cache.values():
        e.close()


def _mod(bits, seed):
    return random_modulus(bits, random.Random(seed))


N64, N200, N297, N412, N1031 = _mod(64, 64), _mod(200, 200), _mod(297, 297), _mod(412, 412), _mod(1031, 1031)


def _row_name(nl):
    return "k_unit_row<%d, %d>" % row_shape(nl)


def _check(eng, method, n_of, seeds, e, b1):
    """residues and standard lines of the batch in eng against Python: position k on n_of(k), from seeds[k] by exponent e"""
    want = [expected(method, seeds[k], e, n_of(k)) for k in range(len(seeds))]
    assert eng.save_lines_std() == [method_line(method, b1, n_of(k), want[k], seeds[k]) for k in range(len(seeds))]
    return want


# ---- 1. limb classes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("nl", ROW_LIMBS)
def test_every_limb_class_both_ends(pyecm, engines, nl, method):
    rng = random.Random(700 * nl + method)
    for n in class_moduli(nl):
        eng = engines(n)
        assert eng.cfg.dev_limbs == nl and eng.method_lanes() == 16
        seeds = seeds_for(n, BATCH, rng)
        eng.build_seeds(method, seeds)
        eng.stage1_extend(1, 1000)
        assert eng.last_kernel_name() == _row_name(nl) and eng.lanes_per_curve() == 16
        st = eng.stage1_stats()
        assert st.tape_len == 1989 and st.last_prime == 997
        want = _check(eng, method, lambda k: n, seeds, E1000, 1000)
        xs, zs = eng.download_points_plain()
        assert xs == want and zs == [1] * BATCH
        # rule 9: residues stated complete to 235536, one prime on
        eng.build_seeds(method, seeds, xs=seeds, b1_done=RULE9_SEGMENT[0])
        eng.stage1_extend(*RULE9_SEGMENT)
        assert eng.stage1_stats().tape_len == 25 and eng.last_kernel_name() == _row_name(nl)
        _check(eng, method, lambda k: n, seeds, E9, RULE9_SEGMENT[1])


# ---- 2. batch sizes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("batch", [1, 65])
def test_one_residue_alone_and_one_past_a_block(pyecm, engines, batch, method):
    n = class_moduli(15)[0]
    eng = engines(n)
    seeds = (seeds_for(n, 5, random.Random(batch)) * 14)[4:4 + batch]
    eng.build_seeds(method, seeds)
    eng.stage1_extend(1, 1000)
    assert eng.last_kernel_name() == _row_name(15) and eng.lanes_per_curve() == 16
    want = _check(eng, method, lambda k: n, seeds, E1000, 1000)
    xs, zs = eng.download_points_plain()
    assert xs == want and zs == [1] * batch


# ---- 3. a tape cut into launches -------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_tape_cut_into_launches(pyecm, engines, method):
    n = class_moduli(17)[0]
    eng = engines(n)
    seeds = seeds_for(n, BATCH, random.Random(5))
    os.environ["GECM_TAPE_CHUNK"] = "256"
    try:
        eng.build_seeds(method, seeds)
        eng.stage1_extend(1, 1000)
    finally:
        del os.environ["GECM_TAPE_CHUNK"]
    done, total = eng.stage1_progress()
    assert total >= 4 and done == total and eng.last_kernel_name() == _row_name(17)
    _check(eng, method, lambda k: n, seeds, E1000, 1000)


# ---- 4. factors ------------------------------------------------------------------------------------------------------
def _factor_setup(method):
    """(n, p, seeds, residues, (gcd, flag)s): a number whose factor p the method finds at B1 = 1000 for some seed"""
    rng = random.Random(40 + method)
    n, p, q = factor_case(method, rng)
    seeds = [3, 5, 6, 7, 10] + seeds_for(n, BATCH - 5, rng)
    seeds[5] = 1 if method == METHOD_PM1 else 2           # the degenerate seed
    res = [expected(method, s, E1000, n) for s in seeds]
    gf = [py_gcd_flag(method, x, n) for x in res]
    hits = [k for k, (g, f) in enumerate(gf) if f]
    assert hits and all(gf[k][0] == p for k in hits), "setup: no seed finds the factor"
    if method == METHOD_PP1:
        assert any(jacobi(seeds[k] * seeds[k] - 4, p) == -1 for k in hits)
    return n, p, seeds, res, gf


@pytest.mark.parametrize("method", METHODS)
def test_factors(pyecm, engines, method):
    n, p, seeds, res, gf = _factor_setup(method)
    eng = engines(n)
    eng.build_seeds(method, seeds)
    eng.stage1_extend(1, 1000)
    assert eng.lanes_per_curve() == 16
    flags = [f for g, f in gf]
    # the host gcd before any scan, then the device scan, then the gcds the scan kept
    first = flags.index(1)
    assert eng.stage1_factor(first)[0] == p and eng.stage1_factor(5) is None
    assert eng.scan_factors(1) == (sum(flags), first)
    assert [int(eng.curve_flag(1, k)) for k in range(BATCH)] == flags
    for k in range(BATCH):
        f = eng.stage1_factor(k)
        assert (f[0] if f else None) == (p if flags[k] else None), k
    # the degenerate seed: x - c = 0, g = N, no flag
    assert res[5] == OFFSET[method] and gf[5] == (n, 0) and not eng.curve_flag(1, 5)
    assert eng.save_lines_std() == [method_line(method, 1000, n, x, s) for x, s in zip(res, seeds)]


# ---- 5. multi-modulus contexts ---------------------------------------------------------------------------------------
def _multi_case(pyecm, ns, packing, method, extra=None):
    """residues interleaved across the numbers of a MultiEngine set to 16 lanes; returns (engine, which, seeds)"""
    rng = random.Random(len(ns) * 7 + method)
    me = pyecm.MultiEngine(ns)
    me.set_packing(packing)
    me.set_method_lanes(16)
    which, seeds = extra or ([], [])
    which, seeds = list(which), list(seeds)
    for j in range(9):
        for g, n in enumerate(ns):
            which.append(g)
            seeds.append(seeds_for(n, 6, rng)[(j + g) % 6] if j < 6 else rng.randrange(n))
    return me, which, seeds


def _single_n_rows(engines, method, ns, which, seeds, want):
    """per number, the 16-lane run of a single-N context gives the same residues"""
    for g, n in enumerate(ns):
        mine = [k for k in range(len(which)) if which[k] == g]
        eng = engines(n)
        eng.build_seeds(method, [seeds[k] for k in mine])
        eng.stage1_extend(1, 1000)
        assert eng.lanes_per_curve() == 16
        assert eng.download_points_plain()[0] == [want[k] for k in mine]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("ns", [(N200, N297, N412), (N200, N1031)], ids=["200_297_412", "200_1031"])
def test_multi_wave_packing(pyecm, engines, ns, method):
    me, which, seeds = _multi_case(pyecm, list(ns), "wave", method)
    me.build_seeds(method, seeds, which)
    assert me.packing() == "wave"
    me.stage1_extend(1, 1000)
    assert me.last_kernel_name() == _row_name(me.cfg.dev_limbs) and me.lanes_per_curve() == 16
    want = _check(me, method, lambda k: ns[which[k]], seeds, E1000, 1000)
    _single_n_rows(engines, method, ns, which, seeds, want)
    me.build_seeds(method, seeds, which, xs=seeds, b1_done=RULE9_SEGMENT[0])
    me.stage1_extend(*RULE9_SEGMENT)
    _check(me, method, lambda k: ns[which[k]], seeds, E9, RULE9_SEGMENT[1])
    me.close()


@pytest.mark.parametrize("method", METHODS)
def test_multi_lane_packing_with_a_64_bit_number_and_a_factor(pyecm, engines, method):
    nf, p, fseeds, fres, gf = _factor_setup(method)
    ns = [N64, N200, N412, nf]
    hit = [f for g, f in gf].index(1)
    me, which, seeds = _multi_case(pyecm, ns, "lane", method, extra=([3, 3], [fseeds[hit], fseeds[5]]))
    assert len(seeds) <= 64
    me.build_seeds(method, seeds, which)
    assert me.packing() == "lane"
    me.stage1_extend(1, 1000)
    assert me.last_kernel_name() == _row_name(15) and me.lanes_per_curve() == 16
    want = _check(me, method, lambda k: ns[which[k]], seeds, E1000, 1000)
    flags = [py_gcd_flag(method, want[k], ns[which[k]])[1] for k in range(len(seeds))]
    assert flags[0] == 1 and flags[1] == 0
    assert me.scan_factors(1) == (sum(flags), 0)
    assert [int(me.curve_flag(1, k)) for k in range(len(seeds))] == flags
    assert me.stage1_factor(0)[0] == p and me.stage1_factor(1) is None
    _single_n_rows(engines, method, ns, which, seeds, want)
    me.build_seeds(method, seeds, which, xs=seeds, b1_done=RULE9_SEGMENT[0])
    me.stage1_extend(*RULE9_SEGMENT)
    _check(me, method, lambda k: ns[which[k]], seeds, E9, RULE9_SEGMENT[1])
    me.close()


# ---- 6. the setting --------------------------------------------------------------------------------------------------
def test_settings(pyecm):
    n = class_moduli(15)[1]
    seeds = seeds_for(n, BATCH, random.Random(11))
    want = [method_line(METHOD_PP1, 1000, n, expected(METHOD_PP1, s, E1000, n), s) for s in seeds]
    eng = pyecm.Engine(n)
    try:
        assert eng.method_lanes() == 1                       # the default: the one-lane kernel, as before the setting
        eng.build_seeds(METHOD_PP1, seeds)
        eng.stage1_extend(1, 1000)
        assert "k_unit<15>" in eng.last_kernel_name() and eng.lanes_per_curve() == 1
        assert eng.save_lines_std() == want
        for bad in (0, 2, 8, 32, -2, 17):
            with pytest.raises(pyecm.GecmError, match=r"\(-2\)"):
                eng.set_method_lanes(bad)
        assert eng.method_lanes() == 1
        # curves on the same context do not see it
        sig = list(range(1000, 1008))
        lines = {}
        for lanes in (1, 16):
            eng.set_method_lanes(lanes)
            eng.build_curves(sig)
            eng.stage1(1000)
            assert "k_unit" not in eng.last_kernel_name() and eng.lanes_per_curve() != 16
            lines[lanes] = eng.save_lines()
        assert lines[1] == lines[16] and len(lines[1]) == 8
        # it survives a build
        assert eng.method_lanes() == 16
        eng.build_seeds(METHOD_PP1, seeds)
        assert eng.method_lanes() == 16
        eng.stage1_extend(1, 1000)
        assert eng.last_kernel_name() == _row_name(15) and eng.lanes_per_curve() == 16
        assert eng.save_lines_std() == want
        # "auto" at 70 positions (128 padded) picks 16; back at 1 the one-lane kernel runs again
        eng.set_method_lanes("auto")
        assert eng.method_lanes() == "auto"
        eng.build_seeds(METHOD_PP1, seeds)
        eng.stage1_extend(1, 1000)
        assert eng.last_kernel_name() == _row_name(15) and eng.lanes_per_curve() == 16
        assert eng.save_lines_std() == want
        eng.set_method_lanes(1)
        eng.build_seeds(METHOD_PP1, seeds)
        eng.stage1_extend(1, 1000)
        assert "k_unit<15>" in eng.last_kernel_name() and eng.lanes_per_curve() == 1
    finally:
        eng.close()


# ---- 7. stage 2 after a 16-lane stage 1 ------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_stage2_after_rows(pyecm, method):
    n = class_moduli(15)[0]
    seeds = seeds_for(n, BATCH, random.Random(21 + method))
    eng = pyecm.Engine(n)
    try:
        eng.set_method_stage2(True)
        accs = {}
        for lanes in (1, 16):
            eng.set_method_lanes(lanes)
            eng.build_seeds(method, seeds)
            eng.stage1_extend(1, 1000)
            assert eng.lanes_per_curve() == lanes
            eng.stage2(20000, D=210, U=2)
            accs[lanes] = eng.download_acc()
        assert len(accs[1]) == BATCH and accs[16] == accs[1]
        assert len(set(accs[1])) > BATCH // 2                # they are accumulators, not a constant
    finally:
        eng.close()
