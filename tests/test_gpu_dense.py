"""GPU: lane-packed multi-modulus batches (include/gecm.h gecm_set_multi_packing, pyecm.MultiEngine.set_packing,
DESIGN.md §16): one modulus per lane, the numbers' curves back to back, only the batch's tail padded.  Every per-curve
result must be, word for word, what the reference wrote (tests/golden), what the CPU oracle computes and what a single-N
context of the curve's own number gives — code this packing does not touch."""
import ctypes
import json
import math
import os
import random
import re

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

S1 = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "stage1.json")))}
S2 = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "stage2_acc.json")))}
COUNTS = [1, 63, 64, 65, 3, 130, 2]       # a number across a wavefront boundary, wavefronts of several numbers, a padded tail
LANE_NLS = (8, 10, 12, 14, 15)


def _n_of(case):
    return int(case["save_lines"][0].split("N=0x")[1].split(";")[0], 16)


def _sigmas(case):
    return [int(l.split("SIGMA=")[1].split(";")[0]) for l in case["save_lines"]]


def _found(lines, stage):
    """sigma -> factor of the reference's result lines of one stage"""
    return {int(re.search(r"sigma (\d+)", l).group(1)): int(re.search(r"factor (\d+) in", l).group(1))
            for l in lines if "in stage %d" % stage in l}


def _interleave(groups):
    """[(modulus index, sigma)] taking one curve of every group in turn: the library has to do the grouping"""
    out, i = [], 0
    while any(i < len(g) for g in groups):
        for m, g in enumerate(groups):
            if i < len(g):
                out.append((m, g[i]))
        i += 1
    return out


def _engine(ns, order, packing="lane"):
    import pyecm
    eng = pyecm.MultiEngine(ns)
    eng.set_packing(packing)
    eng.build_curves([s for _, s in order], [m for m, _ in order])
    assert eng.packing() == packing
    return eng


def _lines(eng):
    return [l.rstrip("\n") for l in eng.save_lines()]


@pytest.fixture(scope="module")
def orc():
    L = ctypes.CDLL(os.path.join(ROOT, "oracle", "libecm_oracle.so"))
    L.orc_create.restype = ctypes.c_void_p
    L.orc_create.argtypes = [ctypes.c_char_p, ctypes.c_int]
    L.orc_destroy.argtypes = [ctypes.c_void_p]
    L.orc_stage1_line.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t,
                                  ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)]
    L.orc_stage2.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32,
                             ctypes.c_uint32, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t,
                             ctypes.POINTER(ctypes.c_uint64)]
    return L


def _oracle_lines(orc, n, sigmas, b1):
    buf = ctypes.create_string_buffer(8192)
    c = orc.orc_create(str(n).encode(), 52)
    out = []
    for s in sigmas:
        orc.orc_stage1_line(c, s, b1, buf, len(buf), None, 0, None)
        out.append(buf.value.decode().rstrip("\n"))
    orc.orc_destroy(c)
    return out


# ---- 1. the reference's own lines, several numbers to a wavefront ---------------------------------------------------
def _check_fixtures(eng, cases, order, checked):
    lines = _lines(eng)
    for m, case in enumerate(cases):
        if case["name"] not in checked:
            continue
        mine = [k for k, (mm, _) in enumerate(order) if mm == m]
        assert [eng.modulus_of(k) for k in mine] == [m] * len(mine)
        assert [lines[k] for k in mine] == case["save_lines"], case["name"]
        want = _found(case["results_lines"], 1)
        got = {order[k][1]: eng.stage1_factor(k)[0] for k in mine if eng.stage1_factor(k)}
        assert got == want, case["name"]
    n, first = eng.scan_factors(1)
    flagged = [k for k in range(len(order)) if eng.curve_flag(1, k)]
    assert n == len(flagged)
    if flagged:
        assert first == flagged[0]
    return {order[k] for k in flagged}


@pytest.mark.parametrize("b1,names", [(1000, ("n200_b1_1000", "n415_b1_1000", "n415_bigsigma_b1_1000")),
                                      (500, ("n64_b1_500", "K1N_two_full_batches_b1_500"))], ids=["b1_1000", "b1_500"])
def test_fixture_lines_and_factors_with_several_numbers_in_a_wavefront(b1, names):
    """8 or 16 curves each, interleaved, all in one wavefront: save lines byte for byte the reference's, stage-1 factors
    and the factor scan's count the reference's result lines"""
    cases = [S1[n] for n in names]
    order = _interleave([_sigmas(c) for c in cases])
    eng = _engine([_n_of(c) for c in cases], order)
    assert eng.cfg.dev_limbs == 15
    eng.stage1(b1)
    assert eng.lanes_per_curve() == 1 and "k_stage1_lane<15>" in eng.last_kernel_name()
    flagged = _check_fixtures(eng, cases, order, names)
    assert len(flagged) == sum(len(_found(c["results_lines"], 1)) for c in cases)
    eng.close()


def test_fixture_lines_on_an_eight_limb_context():
    """n64 and n200 alone: the context has 8 limbs.  Their fixtures stand at different B1, so the batch runs twice and
    each run is compared with the fixture of its B1"""
    cases = [S1["n64_b1_500"], S1["n200_b1_1000"]]
    order = _interleave([_sigmas(c) for c in cases])
    for case in cases:
        eng = _engine([_n_of(c) for c in cases], order)
        assert eng.cfg.dev_limbs == 8
        eng.stage1(case["B1"])
        assert "k_stage1_lane<8>" in eng.last_kernel_name()
        flagged = _check_fixtures(eng, cases, order, (case["name"],))
        m = cases.index(case)
        assert len([f for f in flagged if f[0] == m]) == len(_found(case["results_lines"], 1))
        eng.close()


# ---- 2. both ends of every built limb count ---------------------------------------------------------------------------
def _class_numbers(nl):
    """seven N of one limb-count class: the top of the class twice (random), its lowest size, the 64-bit end, a size in
    between, and the 2^k - 1 and 2^k + 1 shapes that fit"""
    rnd = random.Random(1600 + nl)
    top = 28 * nl - 5
    low = {8: 65, 10: 220, 12: 276, 14: 332, 15: 388}[nl]        # one bit more than the limb count before takes
    odd = lambda b: rnd.getrandbits(b) | (1 << (b - 1)) | 1
    return [odd(top), odd(low), odd(64), (1 << (top - 1)) - 1, (1 << (top - 1)) + 1, odd(top), odd((top + 64) // 2)]


@pytest.mark.parametrize("nl", LANE_NLS)
def test_both_ends_of_every_limb_count_equal_oracle_and_wave_packing(orc, nl):
    ns = _class_numbers(nl)
    rnd = random.Random(nl)
    groups = [[rnd.randrange(6, 1 << 40) for _ in range(c)] for c in COUNTS]
    order = _interleave(groups)
    got = {}
    for packing in ("lane", "wave"):
        eng = _engine(ns, order, packing)
        assert eng.cfg.dev_limbs == nl
        eng.stage1(2000)
        assert ("k_stage1_lane<%d>" % nl in eng.last_kernel_name()) == (packing == "lane")
        got[packing] = _lines(eng)
        eng.close()
    assert got["lane"] == got["wave"]
    for m, n in enumerate(ns):
        mine = [k for k, (mm, _) in enumerate(order) if mm == m]
        assert [got["lane"][k] for k in mine] == _oracle_lines(orc, n, groups[m], 2000), (nl, m, n.bit_length())


# ---- 3. a different modulus on every lane --------------------------------------------------------------------------
def test_sixty_five_numbers_one_curve_each(orc):
    """64 lanes with 64 moduli, and one lane alone in the second wavefront"""
    rnd = random.Random(65)
    bits = [rnd.choice((64, 100, 200, 219, 220, 300, 388, 415)) for _ in range(65)]
    ns = [rnd.getrandbits(b) | (1 << (b - 1)) | 1 for b in bits]
    sig = [rnd.randrange(6, 1 << 63) for _ in ns]
    eng = _engine(ns, list(enumerate(sig)))
    eng.stage1(1000)
    lines = _lines(eng)
    eng.close()
    for k, (n, s) in enumerate(zip(ns, sig)):
        assert [lines[k]] == _oracle_lines(orc, n, [s], 1000), (k, bits[k])


# ---- 4. stage 2 -----------------------------------------------------------------------------------------------------------
def _single_stage2(n, sig, b1, b2, D=0, U=0):
    import pyecm
    e = pyecm.Engine(n)
    e.build_curves(sig)
    e.stage1(b1)
    e.stage2(b2, D, U)
    e.scan_factors(2)
    out = (e.download_acc(), [e.stage2_factor(k) for k in range(len(sig))], [e.curve_flag(2, k) for k in range(len(sig))])
    e.close()
    return out


S2_B1, S2_B2, S2_D, S2_U = 1000, 50000, 385, 16


@pytest.fixture(scope="module")
def stage2_setup():
    t35 = S2["T35N_b1_1000_b2_50000"]
    ns = [int(t35["N"]), int(S2["K1N_b1_2000_b2_1e5"]["N"]), random.Random(200).getrandbits(200) | (1 << 199) | 1]
    groups = [[t35["sigma0"] + k for k in range(8)], [100 + k for k in range(8)], [5000 + k for k in range(8)]]
    return ns, groups, _interleave(groups)


@pytest.fixture(scope="module")
def stage2_straight(stage2_setup):
    """the lane-packed straight run: save lines after stage 1, accumulators and factors after stage 2"""
    ns, groups, order = stage2_setup
    eng = _engine(ns, order)
    eng.stage1(S2_B1)
    lines = eng.save_lines()
    eng.stage2(S2_B2, S2_D, S2_U)
    n_flag, _ = eng.scan_factors(2)
    out = {"lines": lines, "accs": eng.accs(), "facs": [eng.stage2_factor(k) for k in range(len(order))], "n_flag": n_flag}
    eng.close()
    return out


def test_stage2_accumulators_and_factors_equal_single_contexts(stage2_setup, stage2_straight):
    ns, groups, order = stage2_setup
    accs, facs = stage2_straight["accs"], stage2_straight["facs"]
    assert stage2_straight["n_flag"] == sum(1 for f in facs if f)
    for m, n in enumerate(ns):
        mine = [k for k, (mm, _) in enumerate(order) if mm == m]
        acc1, fac1, _ = _single_stage2(n, groups[m], S2_B1, S2_B2, S2_D, S2_U)
        assert [accs[k] for k in mine] == acc1, m
        assert [facs[k] for k in mine] == fac1, m
    assert [accs[k] for k, (m, _) in enumerate(order) if m == 0] == [int(h, 16) for h in S2["T35N_b1_1000_b2_50000"]["acc_hex"]]


# ---- 5. failure planes ------------------------------------------------------------------------------------------------------
# The product of the primes from 10007 up that fits 408 bits (400 bits), chosen with the CPU oracle: on every sigma used
# here the reference's stage-2 chain meets batch inversions that fail (the factor it reports is not
# gcd(accumulator, N)); products of primes from 101 or 1009 up end with the accumulator at 0 and report nothing.
# degenerate.json's own number has 578 bits and does not fit 15 limbs.
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


def test_failure_plane_factors_stay_on_their_curves(orc):
    healthy = int(S2["T35N_b1_1000_b2_50000"]["N"])
    sig = list(range(1000, 1008))
    hsig = list(range(42, 50))
    order = _interleave([hsig, sig])
    eng = _engine([healthy, DEGENERATE_N], order)
    eng.stage1(DEGENERATE_B1)
    eng.stage2(DEGENERATE_B2, S2_D, S2_U)
    eng.scan_factors(2)
    got = [(eng.stage2_factor(k), eng.curve_flag(2, k), eng.acc(k)) for k in range(len(order))]
    eng.close()
    dacc, dfac, dflag = _single_stage2(DEGENERATE_N, sig, DEGENERATE_B1, DEGENERATE_B2, S2_D, S2_U)
    hacc, hfac, hflag = _single_stage2(healthy, hsig, DEGENERATE_B1, DEGENERATE_B2, S2_D, S2_U)
    from_failure_plane = 0
    for k, (m, s) in enumerate(order):
        f, flag, acc = got[k]
        if m == 1:
            j = sig.index(s)
            assert f == dfac[j] and flag == dflag[j], (k, s)
            if f and math.gcd(acc, DEGENERATE_N) != f[0]:
                from_failure_plane += 1
        else:
            j = hsig.index(s)
            assert f == hfac[j] and acc == hacc[j] and flag == hflag[j], (k, s)
    # not vacuous: the reference's chain fails an inversion on this number (the oracle says so), and the device reported
    # a factor that came from the failure record, not from the accumulator
    acch, fac = ctypes.create_string_buffer(4096), ctypes.create_string_buffer(4096)
    c = orc.orc_create(str(DEGENERATE_N).encode(), 52)
    failed = 0
    for s in sig:
        if orc.orc_stage2(c, s, DEGENERATE_B1, DEGENERATE_B2, S2_D, S2_U, acch, fac, len(fac), None) and \
                math.gcd(int(acch.value, 16), DEGENERATE_N) != int(fac.value):
            failed += 1
    orc.orc_destroy(c)
    assert failed >= 1 and from_failure_plane >= 1


# ---- 6. resume --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packing", ["lane", "wave"])
def test_resume_from_lane_packed_save_lines_equals_the_straight_run(stage2_setup, stage2_straight, packing):
    import pyecm
    ns, groups, order = stage2_setup
    eng = pyecm.MultiEngine(ns)
    eng.set_packing(packing)
    eng.resume_lines(stage2_straight["lines"], b1_done=S2_B1)
    assert eng.packing() == packing
    assert eng.save_lines() == stage2_straight["lines"]
    eng.stage2(S2_B2, S2_D, S2_U)
    assert eng.accs() == stage2_straight["accs"]
    assert [eng.stage2_factor(k) for k in range(len(order))] == stage2_straight["facs"]
    eng.close()


# ---- 7. refusals and accounting ---------------------------------------------------------------------------------------------
def test_refusals():
    import pyecm
    GecmError = pyecm.GecmError
    big = pyecm.MultiEngine([1000003, (1 << 499) + 1])
    with pytest.raises(GecmError, match=r"\(-4\): gecm_set_multi_packing: lane packing serves numbers up to 415 bits"):
        big.set_packing("lane")
    big.close()
    single = pyecm.Engine((1 << 127) - 1)
    assert pyecm.lib.gecm_set_multi_packing(single._h, pyecm.PACK_LANE) == -4
    assert b"not a multi-modulus context" in pyecm.lib.gecm_last_error()
    single.close()
    eng = pyecm.MultiEngine([1000003, (1 << 127) - 1])
    assert pyecm.lib.gecm_set_multi_packing(eng._h, 2) == -2
    assert eng.packing() == "wave"                       # before the first build
    eng.set_packing("lane")
    assert eng.packing() == "wave"                       # what the last build used, not what is asked for
    eng.build_curves([10, 11, 12], [1, 0, 1])
    assert eng.packing() == "lane"
    eng.stage1(100)
    before = eng.save_lines()
    # the device curve build has no per-lane kernel: refused, and the batch before it stays readable
    eng.set_curve_build("device")
    with pytest.raises(GecmError, match=r"\(-4\): gecm_build_curves_multi: the device curve build has no per-lane kernel"):
        eng.build_curves([20, 21], [0, 1])
    eng.batch = 3
    assert eng.save_lines() == before
    with pytest.raises(GecmError, match=r"\(-4\): gecm_resume_points_multi: the device curve build has no per-lane kernel"):
        eng.resume_lines(before, b1_done=100)
    eng.batch = 3
    assert eng.save_lines() == before and eng.packing() == "lane"
    eng.set_curve_build("host")
    # one lane per curve: 2 is refused when stage 1 is asked for, 0 and 1 run and report 1
    eng.set_lanes_per_curve(2)
    with pytest.raises(GecmError, match=r"\(-4\): gecm_stage1: a lane-packed multi-modulus batch runs one lane per curve"):
        eng.stage1(100)
    assert eng.save_lines() == before
    for lanes in (0, 1):
        eng.set_lanes_per_curve(lanes)
        eng.build_curves([10, 11, 12], [1, 0, 1])
        eng.stage1(100)
        assert eng.lanes_per_curve() == 1 and eng.save_lines() == before
    eng.set_packing("wave")
    assert eng.packing() == "lane"
    eng.build_curves([10, 11, 12], [1, 0, 1])
    assert eng.packing() == "wave"
    eng.stage1(100)
    assert eng.save_lines() == before
    eng.close()


def test_batch_bytes_count_the_tail_only():
    import pyecm
    ns = _class_numbers(15)
    curves = sum(COUNTS)
    eng = pyecm.MultiEngine(ns)
    wave = [eng.batch_bytes(curves), eng.batch_bytes(curves, True, 1000, S2_D, S2_U)]
    eng.set_packing("lane")
    lane = [eng.batch_bytes(curves), eng.batch_bytes(curves, True, 1000, S2_D, S2_U)]
    positions = pyecm.multi_positions(COUNTS, "lane")
    assert positions == 384 and pyecm.multi_positions(COUNTS, "wave") == 640
    # a batch of exactly that many curves has no tail: the same figure
    assert lane == [eng.batch_bytes(positions), eng.batch_bytes(positions, True, 1000, S2_D, S2_U)]
    eng.close()
    # and the stage-1 arrays are those of a single-N context of the same limb count with that many curves (its stage-2
    # figure is not comparable: a single-N context of a few hundred curves adds the scratch of its sub-sequences, K > 1,
    # which no multi-modulus context has)
    single = pyecm.Engine(ns[0])
    assert single.cfg.dev_limbs == 15
    assert lane[0] == single.batch_bytes(positions)
    single.close()
    assert lane[0] < wave[0] and lane[1] < wave[1]
