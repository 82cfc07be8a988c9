"""GPU tests of stage-1 extension with the standard multiplier and of normalisation.

The yardstick is exact: Python integers, tests/xladder.py, k_std(B) = stage1_multiplier(B + 1), x = X / Z mod N by pow(Z, -1, N).
Equality is of integers and of line bytes.

Moduli.  The 200- and 415-bit numbers of tests/golden/stage1.json (n200_b1_1000, n415_b1_1000) are full of small factors
(3 * 79 * 311 * 2803 and 5^3 * 79 * 89 * 1291 divide them): with sigmas 1000..1007 no curve on them has an invertible Z at
any B1 used here, so no x exists for them.  They are kept in a test of their own, with the check that is defined there (the
projective point, the Z= line, the factor).  The byte-exact cases run on numbers without small factors at the same three limb
counts: a 200-bit semiprime (8 limbs), K1's 412-bit N of the same fixture file (15 limbs) and a 1031-bit number (37 limbs);
test_yardstick_moduli_have_invertible_z checks on the CPU side that every Z met here has an inverse."""
import ctypes
import json
import math
import os
import random
import re

import pytest

from conftest import GOLDEN
from xladder import _primes, ladder_point, stage1_multiplier

pytestmark = pytest.mark.gpu

GECM_ERR_ARG, GECM_ERR_STATE = -2, -4
GECM_B1_MAX = 10 ** 12
S1 = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "stage1.json")))}
S2 = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "stage2_acc.json")))}
SIG = list(range(1000, 1008))


def _no_small_factor(bits, seed):
    """the first odd number of that many bits from the seed on that no prime below 10^5 divides"""
    small = math.prod(_primes(10 ** 5))
    n = random.Random(seed).getrandbits(bits) | (1 << (bits - 1)) | 1
    while math.gcd(n, small) != 1:
        n += 2
    return n


N_FIX200 = int(S1["n200_b1_1000"]["N"])
N_FIX415 = int(S1["n415_b1_1000"]["N"])
N64 = int(S1["n64_b1_500"]["N"])
N412 = int(S1["K1"]["N"])
N297 = int(S1["T35_46"]["N"])
N200 = _no_small_factor(200, 200)
N1031 = _no_small_factor(1031, 1031)
BY_LIMBS = {8: N200, 15: N412, 37: N1031}


def k_std(b):
    return stage1_multiplier(b + 1)


_POINTS = {}


def std_point(n, sigma, b):
    """(X, Z) of [k_std(b)]P on the Suyama curve of sigma, or None where the construction has no inverse"""
    key = (n, sigma, b)
    if key not in _POINTS:
        u, v = (sigma * sigma - 5) % n, 4 * sigma % n
        try:
            x = pow(u, 3, n) * pow(pow(v, 3, n), -1, n) % n
            a24 = pow(v - u, 3, n) * (3 * u + v) % n * pow(16 * pow(u, 3, n) * v % n, -1, n) % n
            _POINTS[key] = ladder_point(n, x, a24, k_std(b))
        except ValueError:
            _POINTS[key] = None
    return _POINTS[key]


def std_line(n, sigma, b):
    X, Z = std_point(n, sigma, b)
    return "METHOD=ECM; PARAM=0; SIGMA=%d; B1=%d; N=0x%x; X=0x%x; PROGRAM=AVX-ECM-STD;\n" % (sigma, b, n, X * pow(Z, -1, n) % n)


def std_lines(n, b, sig=SIG):
    return [std_line(n, s, b) for s in sig]


@pytest.fixture
def short_ranges():
    import pyecm
    hook = pyecm.lib.gecm_plan_set_prime_range_for_tests
    hook.argtypes = [ctypes.c_uint64]
    hook.restype = None
    yield hook
    hook(0)


def _engine(n, lanes=0):
    import pyecm
    eng = pyecm.Engine(n)
    eng.set_lanes_per_curve(lanes)
    eng.build_curves(SIG)
    return eng


def _extended(n, steps, lanes=0):
    """normalised standard lines after the extensions steps = [(from, to), ...] on fresh curves"""
    eng = _engine(n, lanes)
    for lo, hi in steps:
        eng.stage1_extend(lo, hi)
    assert eng.normalize() == 0 and eng.normalized()
    lines = eng.save_lines_std()
    eng.close()
    return lines


def test_yardstick_moduli_have_invertible_z():
    assert (N200.bit_length(), N412.bit_length(), N1031.bit_length()) == (200, 412, 1031)
    for n in (N200, N412, N1031, N297):
        for b in (342, 343, 700, 1000, 1023, 1024, 3000):
            for s in SIG:
                assert math.gcd(std_point(n, s, b)[1], n) == 1, (n.bit_length(), b, s)


# (the 32-lane layout starts at 10 limbs)
@pytest.mark.parametrize("nl,lanes", [(nl, lanes) for nl in (8, 15, 37) for lanes in (1, 2, 8, 32) if not (lanes == 32 and nl < 10)])
def test_straight(nl, lanes):
    n = BY_LIMBS[nl]
    eng = _engine(n, lanes)
    assert eng.cfg.dev_limbs == nl
    eng.stage1_extend(1, 1000)
    assert eng.lanes_per_curve() == lanes and not eng.normalized()
    assert eng.normalize() == 0
    assert eng.save_lines_std() == std_lines(n, 1000)
    eng.close()


@pytest.mark.parametrize("nl", [8, 15, 37])
def test_from_a_reference_run(nl):
    n = BY_LIMBS[nl]
    eng = _engine(n)
    eng.stage1(1000)                                   # the reference's multiplier: k_std(999)
    eng.stage1_extend(999, 3000)
    assert eng.normalize() == 0
    got = eng.save_lines_std()
    eng.close()
    assert got == _extended(n, [(1, 3000)]) == std_lines(n, 3000)


@pytest.mark.parametrize("nl", [8, 15, 37])
def test_split(nl):
    n = BY_LIMBS[nl]
    assert _extended(n, [(1, 700), (700, 3000)]) == _extended(n, [(1, 3000)]) == std_lines(n, 3000)


@pytest.mark.parametrize("b", [343, 1024])
def test_inclusive_bound(b):
    """7^3 = 343 and 2^10 = 1024: the standard multiplier to b holds the power, the reference's to b does not"""
    n = N412
    eng = _engine(n)
    eng.stage1(b)
    assert eng.normalize() == 0
    ref = [l.replace("B1=%d;" % b, "B1=*;") for l in eng.save_lines_std()]
    eng.close()
    at = [l.replace("B1=%d;" % b, "B1=*;") for l in _extended(n, [(1, b)])]
    below = [l.replace("B1=%d;" % (b - 1), "B1=*;") for l in _extended(n, [(1, b - 1)])]
    assert below == ref == [l.replace("B1=%d;" % (b - 1), "B1=*;") for l in std_lines(n, b - 1)]
    assert all(a != r for a, r in zip(at, ref))
    assert at == [l.replace("B1=%d;" % b, "B1=*;") for l in std_lines(n, b)]


def test_segments(short_ranges):
    import pyecm
    n = N412
    eng = _engine(n)
    eng.stage1_extend(1, 1000)
    one = eng.stage1_stats()
    one = (one.ptadds, one.ptdups, one.tape_len)
    assert eng.normalize() == 0
    whole = eng.save_lines_std()
    try:
        short_ranges(256)
        assert pyecm.extend_segments(1, 1000) == 4
        eng.build_curves(SIG)
        eng.stage1_extend(1, 1000)
        st = eng.stage1_stats()
        assert (st.ptadds, st.ptdups) == one[:2] and 0 < st.tape_len < one[2]      # summed; the last segment's tape
        assert eng.normalize() == 0
        assert eng.save_lines_std() == whole == std_lines(n, 1000)
        # segment by segment, normalised in between: every stop is a standard line at the segment's end
        eng.build_curves(SIG)
        for s in range(4):
            eng.stage1_extend_segment(1, 1000, s)
            assert eng.normalize() == 0
            hi = pyecm.describe_extend(1, 1000, s).hi
            assert eng.save_lines_std() == std_lines(n, hi), s
    finally:
        short_ranges(0)
    eng.close()


def test_twin():
    import pyecm
    n = (1 << 401) - 1
    sig = list(range(3000, 3064))
    out = {}
    for special in (True, False):
        eng = pyecm.Engine(n)
        eng.set_special_form(special)
        eng.set_lanes_per_curve(1)
        eng.build_curves(sig)
        eng.stage1_extend(1, 700)
        assert eng.special_form_used() == special
        left = eng.normalize()
        mid = eng.save_lines_std()
        eng.stage1_extend(700, 1000)                   # after a normalisation the launch runs modulo N
        assert not eng.special_form_used()
        assert eng.normalize() == left
        out[special] = (left, mid, eng.save_lines_std())
        eng.close()
    assert out[True] == out[False]
    for k in (0, 1, 63):
        pt = std_point(n, sig[k], 1000)
        if pt and math.gcd(pt[1], n) == 1 and math.gcd(std_point(n, sig[k], 700)[1], n) == 1:
            assert out[True][2][k] == std_line(n, sig[k], 1000)
            assert out[True][1][k] == std_line(n, sig[k], 700)


@pytest.mark.parametrize("packing", ["wave", "lane"])
def test_multi_modulus(packing):
    import pyecm
    ns = [N200, N297, N412]
    which = [0, 1, 2, 0, 2, 1, 0, 2]                   # 3, 2 and 3 curves
    multi = pyecm.MultiEngine(ns)
    multi.set_packing(packing)
    multi.build_curves(SIG, which)
    assert multi.packing() == packing
    multi.stage1_extend(1, 700)
    multi.stage1_extend(700, 1000)
    assert multi.normalize() == 0
    got = multi.save_lines_std()
    assert got == [std_line(ns[g], s, 1000) for g, s in zip(which, SIG)]
    for g, n in enumerate(ns):
        single = _extended(n, [(1, 1000)])
        assert [got[k] for k in range(8) if which[k] == g] == [single[k] for k in range(8) if which[k] == g]
    if packing == "lane":
        multi.set_lanes_per_curve(2)
        multi.build_curves(SIG, which)
        with pytest.raises(pyecm.GecmError, match="one lane per curve"):
            multi.stage1_extend(1, 1000)
        with pytest.raises(pyecm.GecmError, match="one lane per curve"):
            multi.stage1(1000)
    multi.close()


def test_z_without_inverse():
    """N = 184631 * 62429745131311 (n64_b1_500 of stage1.json): at B1 = 1000 sigmas 1002 and 1007 have an invertible Z, the
    other six have gcd(Z, N) = 184631 or 62429745131311 (checked here with the Python ladder first)"""
    import pyecm
    n, b = N64, 1000
    gcds = [math.gcd(std_point(n, s, b)[1], n) for s in SIG]
    assert gcds == [184631, 184631, 1, 62429745131311, 184631, 184631, 184631, 1]
    eng = _engine(n, 1)
    eng.stage1_extend(1, b)
    X0, Z0 = eng.download_points()
    assert eng.normalize() == 1
    X1, Z1 = eng.download_points()
    one = pow(2, eng.cfg.maxbits, n)
    lines = eng.save_lines_std()
    for k, g in enumerate(gcds):
        if g == 1:
            assert Z1[k] == one and lines[k] == std_line(n, SIG[k], b)
            assert eng.stage1_factor(k) is None
        else:
            assert (X1[k], Z1[k]) == (X0[k], Z0[k])
            rec = pyecm.parse_resume_line(lines[k])
            assert "; Z=0x" in lines[k] and lines[k].endswith("; PROGRAM=AVX-ECM-STD;\n") and "PARAM=0; " in lines[k]
            X, Z = std_point(n, SIG[k], b)
            assert (rec.x * Z - X * rec.z) % n == 0 and math.gcd(rec.z, n) == g
            assert eng.stage1_factor(k)[0] == g
    assert eng.scan_factors(1)[0] == 6
    eng.close()


@pytest.mark.parametrize("n", [N_FIX200, N_FIX415], ids=["n200", "n415"])
@pytest.mark.parametrize("lanes", [1, 2])
def test_fixture_moduli_with_small_factors(n, lanes):
    """the issue's 200- and 415-bit N: every curve Python can build ends with gcd(Z, N) > 1, so each keeps its projective
    point, which must be the ladder's, and its line carries Z="""
    import pyecm
    eng = _engine(n, lanes)
    eng.stage1_extend(1, 1000)
    assert eng.normalize() == 1
    lines = eng.save_lines_std()
    built = 0
    for k, s in enumerate(SIG):
        pt = std_point(n, s, 1000)
        if pt is None:                                   # a Suyama denominator without inverse: no yardstick
            continue
        built += 1
        g = math.gcd(pt[1], n)
        assert g > 1
        rec = pyecm.parse_resume_line(lines[k])
        assert "; Z=0x" in lines[k] and (rec.x * pt[1] - pt[0] * rec.z) % n == 0 and math.gcd(rec.z, n) == g
        f = eng.stage1_factor(k)
        assert (f[0] if f else n) == g
    assert built >= 5
    eng.close()


def test_round_trip_through_standard_lines():
    import pyecm
    n = N412
    at1000 = _extended(n, [(1, 1000)])
    assert {pyecm.resume_line_std_bound(l) for l in at1000} == {1000}
    recs = [pyecm.parse_resume_line(l) for l in at1000]
    assert all(r.z == 1 and r.b1 == 1000 and r.n == n for r in recs)
    eng = pyecm.Engine(n)
    eng.resume_lines(at1000, b1_done=0)
    eng.stage1_extend(1000, 3000)
    assert eng.normalize() == 0
    assert eng.save_lines_std() == std_lines(n, 3000)
    # the reference's own save lines of this N (B1 = 10^6, sigma0 7372562557) are standard lines of the bound 999999
    ref = S1["K1"]["save_lines"]
    assert {pyecm.resume_line_std_bound(l) for l in ref} == {999999}
    eng.close()


def test_stage2_after_normalisation():
    """T35_46 of the fixtures: the reference's save lines at B1 = 10^6, its stage 2 to 10^8 and the factor it found"""
    import pyecm
    case = S2["T35_46_b1_1e6_b2_1e8"]
    lines = S1["T35_46"]["save_lines"][:case["curves"]]
    found = {int(re.search(r"vec (\d+),", l).group(1)): int(re.search(r"factor (\d+) in stage 2", l).group(1))
             for l in case["results_lines"] if "in stage 2" in l}
    assert found
    eng = pyecm.Engine(pyecm.parse_resume_line(lines[0]).n)
    eng.resume_lines(lines, b1_done=case["B1"])
    assert eng.normalize() == 0
    assert all(pyecm.parse_resume_line(l).z == 1 for l in eng.save_lines_std())
    eng.stage2(case["B2"], case["D"], case["U"])
    for k in range(case["curves"]):
        f = eng.stage2_factor(k)
        assert (f[0] if f else None) == found.get(k), k
    eng.close()


def test_refusals():
    import pyecm
    lib = pyecm.lib
    eng = pyecm.Engine(N412)
    assert lib.gecm_stage1_extend(eng._h, 1, 1000) == GECM_ERR_STATE            # no batch
    assert lib.gecm_normalize_points(eng._h) == GECM_ERR_STATE
    eng.build_curves(SIG)
    for lo, hi in ((1001, 1000), (0, 1000), (1, GECM_B1_MAX + 1)):
        assert lib.gecm_stage1_extend(eng._h, lo, hi) == GECM_ERR_ARG
        assert lib.gecm_stage1_extend_segment(eng._h, lo, hi, 0) == GECM_ERR_ARG
        assert lib.gecm_stage1_extend_segments(lo, hi) == GECM_ERR_ARG
    assert lib.gecm_stage1_extend_segment(eng._h, 1, 1000, 1) == GECM_ERR_ARG   # one segment: 0
    eng.stage1_extend(1, 1000)
    buf = ctypes.create_string_buffer(8192)
    assert lib.gecm_format_save_line_std(eng._h, 0, buf, len(buf)) == GECM_ERR_STATE
    assert "not normalised" in lib.gecm_last_error().decode()
    assert eng.normalize() == 0 and eng.normalized()
    assert lib.gecm_format_save_line_std(eng._h, 8, buf, len(buf)) == GECM_ERR_ARG
    eng.stage1_extend(1000, 1000)                       # nothing to do, but a stage-1 call: the batch counts as new
    assert not eng.normalized()
    eng.close()
    # a report modulus: x modulo the context's modulus is not x modulo the number the lines name
    p, q = (1 << 89) - 1, (1 << 107) - 1
    eng = pyecm.Engine(p * q)
    eng.set_report_modulus(p)
    eng.build_curves(SIG)
    eng.stage1(300)
    before = eng.save_lines()
    assert lib.gecm_normalize_points(eng._h) == GECM_ERR_STATE
    assert "report modulus" in lib.gecm_last_error().decode()
    assert eng.save_lines() == before and not eng.normalized()
    eng.close()
