"""GPU tests of P-1 and P+1 stage 1: k_unit, k_unit_multi, k_unit_lane and the factor scan with an offset,
through gecm_build_seeds and gecm_stage1_extend.  Every comparison is of exact integers or line bytes against Python
(tests/unit_model.py): pow, and a binary Lucas ladder for V_k.  The (1, 1000] tape has rules 3, 4, 5 and the swap; the
one-prime segment (235536, 235537] adds rule 9 (tests/test_unit_cpu.py asserts that from the tape's own counts)."""
import ctypes
import os
import random

import pytest

from unit_model import (METHOD_PM1, METHOD_PP1, OFFSET, RULE9_SEGMENT, UNIT_LIMBS, class_moduli, expected, exponent,
                        factor_case, jacobi, method_line, py_gcd_flag, random_modulus, seeds_for)

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
    """one context per modulus for the whole module"""
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = pyecm.Engine(n)
        return cache[n]
    yield get
    for e in cache.values():
        e.close()


def _mod(bits, seed):
    return random_modulus(bits, random.Random(seed))


N64, N200, N297, N412, N1031 = _mod(64, 64), _mod(200, 200), _mod(297, 297), _mod(412, 412), _mod(1031, 1031)


def _check(eng, method, n_of, seeds, start, e, b1, known=True):
    """residues and standard lines of the batch in eng against Python: position k on n_of(k), from start[k] by exponent e"""
    want = [expected(method, start[k], e, n_of(k)) for k in range(len(start))]
    lines = eng.save_lines_std()
    assert lines == [method_line(method, b1, n_of(k), want[k], seeds[k] if known else None) for k in range(len(start))]
    return want


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("nl", UNIT_LIMBS)
def test_every_limb_class_both_ends(pyecm, engines, nl, method):
    rng = random.Random(100 * nl + method)
    for n in class_moduli(nl):
        eng = engines(n)
        assert eng.cfg.dev_limbs == nl
        seeds = seeds_for(n, BATCH, rng)
        eng.set_lanes_per_curve(2)                       # one lane per residue whatever this says
        eng.build_seeds(method, seeds)
        assert eng.batch_method() == method and eng.curve_seed(3) == seeds[3] and eng.curve_seed(0) == 2
        eng.stage1_extend(1, 1000)
        assert "k_unit<%d>" % nl in eng.last_kernel_name() and eng.lanes_per_curve() == 1
        st = eng.stage1_stats()
        assert st.tape_len == 1989 and st.last_prime == 997
        want = _check(eng, method, lambda k: n, seeds, seeds, E1000, 1000)
        xs, zs = eng.download_points_plain()
        assert xs == want and zs == [1] * BATCH
        # rule 9: residues stated complete to 235536, one prime on
        eng.build_seeds(method, seeds, xs=seeds, b1_done=RULE9_SEGMENT[0])
        eng.stage1_extend(*RULE9_SEGMENT)
        assert eng.stage1_stats().tape_len == 25
        _check(eng, method, lambda k: n, seeds, seeds, E9, RULE9_SEGMENT[1])
        eng.set_lanes_per_curve(0)


@pytest.mark.parametrize("method", METHODS)
def test_tape_cut_into_launches(pyecm, engines, method):
    n = class_moduli(15)[0]
    eng = engines(n)
    seeds = seeds_for(n, BATCH, random.Random(5))
    os.environ["GECM_TAPE_CHUNK"] = "256"
    try:
        eng.build_seeds(method, seeds)
        eng.stage1_extend(1, 1000)
    finally:
        del os.environ["GECM_TAPE_CHUNK"]
    done, total = eng.stage1_progress()
    assert total >= 4 and done == total
    _check(eng, method, lambda k: n, seeds, seeds, E1000, 1000)


@pytest.mark.parametrize("method", METHODS)
def test_round_trip_through_lines(pyecm, engines, method):
    n = class_moduli(15)[1]
    eng = engines(n)
    seeds = seeds_for(n, BATCH, random.Random(9))
    eng.build_seeds(method, seeds)
    eng.stage1_extend(1, 3000)
    fresh = eng.save_lines_std()
    assert fresh == [method_line(method, 3000, n, expected(method, s, exponent(1, 3000), n), s) for s in seeds]
    eng.build_seeds(method, seeds)
    eng.stage1_extend(1, 1000)
    at1000 = eng.save_lines_std()
    recs = [pyecm.parse_resume_line_method(l) for l in at1000]
    assert all(r.method == method and r.n == n and r.b1 == 1000 and r.z == 1 and r.sigma == 0 for r in recs)
    assert [r.x0 for r in recs] == seeds
    assert {pyecm.resume_line_std_bound_method(l) for l in at1000} == {1000}
    for known in (True, False):
        eng.build_seeds(method, [r.x0 for r in recs] if known else None, xs=[r.x for r in recs], b1_done=1000)
        lines = eng.save_lines_std()                         # a batch taken from lines writes them back
        if known:
            assert lines == at1000 and eng.curve_seed(1) == seeds[1]
        else:
            assert lines == [l.replace("X0=0x%x; " % s, "") for l, s in zip(at1000, seeds)]
            assert all("X0=" not in l for l in lines) and eng.curve_seed(1) is None
            assert [pyecm.parse_resume_line_method(l).x0 for l in lines] == [None] * BATCH
        eng.stage1_extend(1000, 3000)
        assert eng.save_lines_std() == (fresh if known else [l.replace("X0=0x%x; " % s, "") for l, s in zip(fresh, seeds)])


def _factor_setup(method):
    """(n, p, seeds, residues, gcds, flags): a number whose factor p the method finds at B1 = 1000 for some seed"""
    rng = random.Random(40 + method)
    n, p, q = factor_case(method, rng)
    seeds = [3, 5, 6, 7, 10] + seeds_for(n, BATCH - 5, rng)
    seeds[5] = 1 if method == METHOD_PM1 else 2           # the degenerate seed
    res = [expected(method, s, E1000, n) for s in seeds]
    gf = [py_gcd_flag(method, x, n) for x in res]
    hits = [k for k, (g, f) in enumerate(gf) if f]
    assert hits, "setup: no seed finds the factor"
    assert all(gf[k][0] == p for k in hits)
    if method == METHOD_PP1:
        assert any(jacobi(seeds[k] * seeds[k] - 4, p) == -1 for k in hits)
    return n, p, seeds, res, gf


@pytest.mark.parametrize("method", METHODS)
def test_factors(pyecm, engines, method):
    n, p, seeds, res, gf = _factor_setup(method)
    eng = engines(n)
    eng.build_seeds(method, seeds)
    eng.stage1_extend(1, 1000)
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


def _multi_case(pyecm, ns, packing, method, extra=None):
    """residues interleaved across the numbers of a MultiEngine; returns (engine, which, seeds)"""
    rng = random.Random(len(ns) * 7 + method)
    me = pyecm.MultiEngine(ns)
    me.set_packing(packing)
    which, seeds = extra or ([], [])
    which, seeds = list(which), list(seeds)
    per = 9 if len(ns) < 10 else 1
    for j in range(per):
        for g, n in enumerate(ns):
            which.append(g)
            seeds.append(seeds_for(n, 6, rng)[(j + g) % 6] if j < 6 else rng.randrange(n))
    return me, which, seeds


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("ns", [(N200, N297, N412), (N200, N1031)], ids=["200_297_412", "200_1031"])
def test_multi_wave_packing(pyecm, engines, ns, method):
    me, which, seeds = _multi_case(pyecm, list(ns), "wave", method)
    me.build_seeds(method, seeds, which)
    assert me.batch_method() == method and me.packing() == "wave"
    me.stage1_extend(1, 1000)
    assert "k_unit_multi<" in me.last_kernel_name() and me.lanes_per_curve() == 1
    want = _check(me, method, lambda k: ns[which[k]], seeds, seeds, E1000, 1000)
    assert [me.modulus_of(k) for k in range(len(which))] == which
    for g, n in enumerate(ns):                               # and the single-N result
        mine = [k for k in range(len(which)) if which[k] == g]
        eng = engines(n)
        eng.build_seeds(method, [seeds[k] for k in mine])
        eng.stage1_extend(1, 1000)
        assert eng.download_points_plain()[0] == [want[k] for k in mine]
    me.build_seeds(method, seeds, which, xs=seeds, b1_done=RULE9_SEGMENT[0])
    me.stage1_extend(*RULE9_SEGMENT)
    _check(me, method, lambda k: ns[which[k]], seeds, seeds, E9, RULE9_SEGMENT[1])
    me.close()


@pytest.mark.parametrize("method", METHODS)
def test_multi_lane_packing_one_wavefront_with_a_factor(pyecm, method):
    nf, p, fseeds, fres, gf = _factor_setup(method)
    ns = [N64, N200, N412, nf]
    hit = [f for g, f in gf].index(1)
    me, which, seeds = _multi_case(pyecm, ns, "lane", method, extra=([3, 3], [fseeds[hit], fseeds[5]]))
    assert len(seeds) <= 64
    me.build_seeds(method, seeds, which)
    assert me.packing() == "lane"
    me.set_lanes_per_curve(2)                                # refused for curves on this packing; residues run one lane
    me.stage1_extend(1, 1000)
    assert "k_unit_lane<15>" in me.last_kernel_name() and me.lanes_per_curve() == 1
    want = _check(me, method, lambda k: ns[which[k]], seeds, seeds, E1000, 1000)
    flags = [py_gcd_flag(method, want[k], ns[which[k]])[1] for k in range(len(seeds))]
    assert flags[0] == 1 and flags[1] == 0
    assert me.scan_factors(1) == (sum(flags), 0)
    assert [int(me.curve_flag(1, k)) for k in range(len(seeds))] == flags
    assert me.stage1_factor(0)[0] == p and me.stage1_factor(1) is None
    me.build_seeds(method, seeds, which, xs=seeds, b1_done=RULE9_SEGMENT[0])
    me.stage1_extend(*RULE9_SEGMENT)
    _check(me, method, lambda k: ns[which[k]], seeds, seeds, E9, RULE9_SEGMENT[1])
    me.close()


@pytest.mark.parametrize("method", METHODS)
def test_multi_lane_packing_64_moduli_and_one_lane_in_the_second_wavefront(pyecm, method):
    rng = random.Random(64)
    ns = [random_modulus(rng.choice((64, 100, 200, 300, 412)), rng) for _ in range(64)]
    me = pyecm.MultiEngine(ns)
    me.set_packing("lane")
    which = list(range(64)) + [63]
    seeds = [seeds_for(ns[g], 6, rng)[k % 6] for k, g in enumerate(which)]
    me.build_seeds(method, seeds, which)
    me.stage1_extend(1, 1000)
    assert "k_unit_lane<15>" in me.last_kernel_name()
    _check(me, method, lambda k: ns[which[k]], seeds, seeds, E1000, 1000)
    me.close()


def test_refusals(pyecm, engines):
    n = class_moduli(15)[0]
    eng = engines(n)
    seeds = seeds_for(n, 8, random.Random(3))
    sig = list(range(1000, 1008))
    eng.build_curves(sig)
    eng.stage1_extend(1, 1000)
    eng.normalize()
    ecm_lines = eng.save_lines_std()
    assert eng.batch_method() == pyecm.METHOD_ECM
    with pytest.raises(pyecm.GecmError, match="holds curves"):
        eng.curve_seed(0)
    for method, name in ((METHOD_PM1, r"P-1"), (METHOD_PP1, r"P\+1")):
        eng.build_seeds(method, seeds)
        eng.stage1_extend(1, 1000)
        lines = eng.save_lines_std()
        pairs = pyecm.pair_primes(1000, 10000, 210, 2)
        calls = [lambda: eng.stage1(1000), lambda: eng.stage1_range(1000, 0), lambda: eng.stage2(10000),
                 lambda: eng.stage2_prepare(10000), lambda: eng.stage2_init(), lambda: eng.stage2_pair(pairs),
                 lambda: eng.stage2_pair_prepare(pairs, 210, 2), lambda: eng.normalize(), eng.download_s,
                 lambda: eng.save_line(0), lambda: eng.resume_line(0, 1000), lambda: eng.scan_factors(2),
                 lambda: eng.stage2_factor(0)]
        for call in calls:
            with pytest.raises(pyecm.GecmError, match=r"\(-4\).*not available on a %s batch" % name):
                call()
        assert eng.save_lines_std() == lines                 # none of them touched the batch
        # rejected builds leave the previous batch
        for bad in (lambda: eng.build_seeds(3, seeds), lambda: eng.build_seeds(0, seeds),
                    lambda: eng.build_seeds(method, seeds[:-1] + [n]), lambda: eng.build_seeds(method, seeds, xs=seeds[:-1] + [n + 5], b1_done=5),
                    lambda: eng.build_seeds(method, seeds, b1_done=1000), lambda: eng.build_seeds(method, seeds, xs=seeds, b1_done=0),
                    lambda: eng.build_seeds(method, [])):
            with pytest.raises((pyecm.GecmError, ValueError)):
                bad()
        assert eng.save_lines_std() == lines and eng.batch_method() == method
        # a pending parametrisation is taken and dropped
        eng._next_params([1] * 8, 8)
        eng.build_seeds(method, seeds)
        assert eng.batch_method() == method
        eng.build_curves(sig)
        assert eng.curve_param(0) == 0
        eng.build_seeds(method, seeds)
    # the other kind of context
    with pytest.raises(pyecm.GecmError, match=r"\(-4\)"):
        idx = (ctypes.c_uint32 * 8)(*([0] * 8))
        pyecm._chk(pyecm.lib.gecm_build_seeds_multi(eng._h, 1, idx, eng.pack(seeds), None, 8, 1), "gecm_build_seeds_multi")
    me = pyecm.MultiEngine([N200, N297])
    with pytest.raises(pyecm.GecmError, match=r"\(-4\)"):
        pyecm._chk(pyecm.lib.gecm_build_seeds(me._h, 1, me.pack([2, 3]), None, 2, 1), "gecm_build_seeds")
    with pytest.raises(pyecm.GecmError, match="modulus_index"):
        me.build_seeds(1, [2, 3], [0, 2])
    with pytest.raises(pyecm.GecmError, match="not below its N"):
        me.build_seeds(1, [2, N200], [1, 0])
    me.close()
    # a context with a report modulus
    rep = pyecm.Engine((1 << 127) - 1)
    rep.set_report_modulus((1 << 127) - 1)
    with pytest.raises(pyecm.GecmError, match=r"\(-4\).*report modulus"):
        rep.build_seeds(1, [3])
    rep.close()
    # back to curves: the lines it wrote before
    eng.build_curves(sig)
    assert eng.batch_method() == pyecm.METHOD_ECM
    eng.stage1_extend(1, 1000)
    eng.normalize()
    assert eng.save_lines_std() == ecm_lines
