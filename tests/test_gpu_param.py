"""GPU tests of GMP-ECM's PARAM 1 and PARAM 3 curves: the build on the host and on the device
(k_build_param), mixed batches, a fresh standard run, the round trip through standard lines, the one-shot rule of
gecm_set_next_params, stage-1 factors, stage 2, multi-modulus batches in both packings and the special-form twin.

Every comparison is exact.  The expectation is Python (tests/param_model.py, tests/xladder.py): the plain binary ladder
from (2 : 1) on the curve with (A+2)/4 = d, d = sigma^2 / 2^64 or sigma / 2^32 mod N, and x = X / Z mod N."""
import ctypes
import json
import math
import os
import random

import pytest

from conftest import GOLDEN
from param_model import PARAM_SIGMAS, param_d, param_line, param_point
from suyama_model import suyama_plain
from xladder import _primes, ladder_point, stage1_multiplier

pytestmark = pytest.mark.gpu

GECM_ERR_ARG = -2
S1 = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "stage1.json")))}


def _no_small_factor(bits, seed):
    """the first odd number of that many bits from the seed on that no prime below 10^5 divides"""
    small = math.prod(_primes(10 ** 5))
    n = random.Random(seed).getrandbits(bits) | (1 << (bits - 1)) | 1
    while math.gcd(n, small) != 1:
        n += 2
    return n


N64 = int(S1["n64_b1_500"]["N"])
N412 = int(S1["K1"]["N"])
N297 = int(S1["T35_46"]["N"])
N200 = _no_small_factor(200, 200)
N1031 = _no_small_factor(1031, 1031)
BY_LIMBS = {8: N200, 15: N412, 37: N1031}
SIG = list(range(1000, 1008))
# (param, sigma) of every curve met here: the edge values and 1000..1007, both parametrisations
CURVES = [(p, s) for p in (1, 3) for s in PARAM_SIGMAS[p] + SIG]


def suyama_line(n, sigma, b):
    u, v = (sigma * sigma - 5) % n, 4 * sigma % n
    x = pow(u, 3, n) * pow(pow(v, 3, n), -1, n) % n
    a24 = pow(v - u, 3, n) * (3 * u + v) % n * pow(16 * pow(u, 3, n) * v % n, -1, n) % n
    X, Z = ladder_point(n, x, a24, stage1_multiplier(b + 1))
    return "METHOD=ECM; PARAM=0; SIGMA=%d; B1=%d; N=0x%x; X=0x%x; PROGRAM=AVX-ECM-STD;\n" % (sigma, b, n, X * pow(Z, -1, n) % n)


def line_of(n, param, sigma, b):
    return suyama_line(n, sigma, b) if param == 0 else param_line(n, param, sigma, b)


def _words(eng):
    X, Z = eng.download_points()
    return X, Z, eng.download_s()


def test_yardstick_curves_have_invertible_z():
    assert (N200.bit_length(), N412.bit_length(), N1031.bit_length(), N297.bit_length()) == (200, 412, 1031, 297)
    for n in (N200, N412, N1031, N297):
        for param, sigma in CURVES:
            assert math.gcd(param_point(n, param, sigma, 1000)[1], n) == 1, (n.bit_length(), param, sigma)


@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("nl", [8, 15, 37])
def test_build_holds_d_and_the_point_2_1(nl, mode):
    import pyecm
    n = BY_LIMBS[nl]
    eng = pyecm.Engine(n)
    assert eng.cfg.dev_limbs == nl
    r = pow(2, eng.cfg.maxbits, n)
    eng.set_curve_build(mode)
    for param in (1, 3):
        sig = PARAM_SIGMAS[param] + SIG
        assert eng.build_curves(sig, params=[param] * len(sig)) == 0
        assert eng.curve_build() == mode
        X, Z, s = _words(eng)
        assert X == [2 * r % n] * len(sig) and Z == [r] * len(sig)
        assert s == [param_d(param, sg, n) * r % n for sg in sig]
        assert [eng.curve_param(k) for k in range(len(sig))] == [param] * len(sig)
        if mode == "device":
            assert eng.last_kernel_ms() > 0
    eng.close()


@pytest.mark.parametrize("nl", [8, 15, 37])
def test_mixed_batch_on_host_and_device(nl):
    import pyecm
    n = BY_LIMBS[nl]
    sig = [1000 + k for k in range(70)]                      # more than one wavefront, a ragged tail
    sig[5], sig[6], sig[64] = 2**64 - 1, 2**32 - 1, 1
    params = [(0, 1, 3, 0)[k % 4] for k in range(70)]
    params[5], params[6], params[64] = 1, 3, 1
    eng = pyecm.Engine(n)
    r = pow(2, eng.cfg.maxbits, n)
    got = {}
    for mode in ("host", "device"):
        eng.set_curve_build(mode)
        assert eng.build_curves(sig, params=params) == 0
        assert eng.curve_build() == mode and [eng.curve_param(k) for k in range(70)] == params
        got[mode] = _words(eng)
    assert got["device"] == got["host"]
    X, Z, s = got["host"]
    plain = pyecm.Engine(n)
    zero = [k for k in range(70) if params[k] == 0]
    assert plain.build_curves([sig[k] for k in zero]) == 0
    pX, pZ, ps = _words(plain)
    plain.close()
    assert [X[k] for k in zero] == pX and [Z[k] for k in zero] == pZ and [s[k] for k in zero] == ps
    for k in range(70):
        if params[k]:
            assert (X[k], Z[k], s[k]) == (2 * r % n, r, param_d(params[k], sig[k], n) * r % n), k
    eng.close()


def test_mixed_batch_keeps_the_failure_record_of_a_suyama_curve():
    """N64 = 184631 * q: sigma = 184631 has v = 4 sigma = 0 modulo the factor, so both of its inversions fail"""
    import pyecm
    assert N64 % 184631 == 0 and suyama_plain(N64, 184631)[2] == 1
    sig = [1000, 184631, 1001, 1002, 1003, 1004, 7, 1]
    params = [0, 0, 1, 3, 0, 1, 3, 1]
    assert all(suyama_plain(N64, s)[2] == 0 for s, p in zip(sig, params) if p == 0 and s != 184631)
    eng = pyecm.Engine(N64)
    r = pow(2, eng.cfg.maxbits, N64)
    got = {}
    for mode in ("host", "device"):
        eng.set_curve_build(mode)
        assert eng.build_curves(sig, params=params) == 1
        got[mode] = _words(eng)
        zero = [k for k in range(8) if params[k] == 0]
        assert eng.build_curves([sig[k] for k in zero]) == 1
        pX, pZ, ps = _words(eng)
        X, Z, s = got[mode]
        assert [X[k] for k in zero] == pX and [Z[k] for k in zero] == pZ and [s[k] for k in zero] == ps
        x, a, flag = suyama_plain(N64, 184631)
        assert (X[1], s[1], flag) == (x * r % N64, a * r % N64, 1)
        # the PARAM 1 and 3 curves alone: no inversion, no flag, return value 0
        rest = [k for k in range(8) if params[k]]
        assert eng.build_curves([sig[k] for k in rest], params=[params[k] for k in rest]) == 0
    assert got["device"] == got["host"]
    eng.close()


def _fresh(n, lanes, param, sig, mode="host"):
    import pyecm
    eng = pyecm.Engine(n)
    eng.set_lanes_per_curve(lanes)
    eng.set_curve_build(mode)
    assert eng.build_curves(sig, params=[param] * len(sig)) == 0
    eng.stage1_extend(1, 1000)
    return eng


@pytest.mark.parametrize("nl,lanes", [(15, 1), (15, 2), (15, 8), (15, 32), (8, 0), (37, 0)])
def test_fresh_run_and_round_trip(nl, lanes):
    import pyecm
    n = BY_LIMBS[nl]
    for param in (1, 3):
        sig = PARAM_SIGMAS[param] + SIG
        eng = _fresh(n, lanes, param, sig, "device" if lanes in (0, 2) else "host")
        if lanes:
            assert eng.lanes_per_curve() == lanes
        assert eng.normalize() == 0
        lines = eng.save_lines_std()
        assert lines == [param_line(n, param, s, 1000) for s in sig]
        # the round trip: the lines back in, on to 3000
        with pytest.raises(pyecm.GecmError, match="PARAM"):
            eng.resume_lines(lines, b1_done=1000)
        assert eng.resume_lines(lines, b1_done=1000, params=True) == 0
        assert [eng.curve_param(k) for k in range(len(sig))] == [param] * len(sig)
        eng.stage1_extend(1000, 3000)
        assert eng.normalize() == 0
        assert eng.save_lines_std() == [param_line(n, param, s, 3000) for s in sig]
        eng.close()


def test_the_setting_is_taken_once_and_checks_its_batch_size():
    import pyecm
    n = N412
    eng = pyecm.Engine(n)
    assert eng.build_curves(SIG, params=[3] * 8) == 0
    s3 = eng.download_s()
    assert eng.build_curves(SIG) == 0                                    # no setting left: a plain Suyama build
    assert [eng.curve_param(k) for k in range(8)] == [0] * 8
    plain = pyecm.Engine(n)
    plain.build_curves(SIG)
    assert _words(eng) == _words(plain) and eng.download_s() != s3
    # a setting for another batch size: refused, and the batch before answers as before
    before = _words(eng)
    arr = (ctypes.c_uint8 * 4)(1, 1, 1, 1)
    assert pyecm.lib.gecm_set_next_params(eng._h, arr, 4) == 0
    sig = (ctypes.c_uint64 * 8)(*SIG)
    assert pyecm.lib.gecm_build_curves(eng._h, sig, 8) == GECM_ERR_ARG
    assert b"gecm_set_next_params" in pyecm.lib.gecm_last_error()
    assert _words(eng) == before and eng.curve_param(0) == 0
    assert eng.build_curves(SIG) == 0 and _words(eng) == before          # the refused call took the setting with it
    # a sigma out of its parametrisation's range: refused before the batch is given up; sigma < 6 is PARAM 0's rule only
    for sg, prm in ((0, 1), (0, 3), (2**32, 3), (5, 0)):
        with pytest.raises(pyecm.GecmError):
            eng.build_curves([1000, sg], params=[0, prm])
        eng.batch = 8
        assert _words(eng) == before
    assert eng.build_curves([1, 5, 2**32], params=[1, 3, 1]) == 0
    # NULL clears a pending setting
    assert pyecm.lib.gecm_set_next_params(eng._h, arr, 4) == 0 and pyecm.lib.gecm_set_next_params(eng._h, None, 0) == 0
    assert eng.build_curves(SIG) == 0 and _words(eng) == before
    eng.close()
    plain.close()


def test_reference_lines_carry_the_param_of_the_curve():
    import pyecm
    eng = pyecm.Engine(N412)
    eng.build_curves(SIG, params=[3, 0, 1, 0, 3, 0, 1, 0])
    eng.stage1(1000)
    plain = pyecm.Engine(N412)
    plain.build_curves(SIG)
    plain.stage1(1000)
    for k, param in enumerate([3, 0, 1, 0, 3, 0, 1, 0]):
        line = eng.save_line(k)
        if param == 0:
            assert line == plain.save_line(k) and "PARAM" not in line
            assert eng.resume_line(k, 997) == plain.resume_line(k, 997)
            continue
        assert line.startswith("METHOD=ECM; PARAM=%d; SIGMA=%d; B1=1000; N=0x%x; X=0x" % (param, SIG[k], N412))
        assert line.endswith("; PROGRAM=AVX-ECM;\n") and eng.resume_line(k, 997).startswith("METHOD=ECM; PARAM=%d; SIGMA=" % param)
        rec = pyecm.parse_resume_line_param(line)
        X, Z = param_point(N412, param, SIG[k], 999)                     # the reference's multiplier is k_std(B1 - 1)
        assert rec.param == param and rec.x * pow(rec.z, -1, N412) % N412 == X * pow(Z, -1, N412) % N412
        assert pyecm.resume_line_std_bound(line, params=True) == 999
    eng.close()
    plain.close()


def test_stage1_factors_on_the_64_bit_number():
    import pyecm
    hit = {1: [1000, 1003, 1006, 1007], 3: [1000, 1002, 1005, 1006]}
    for param in (1, 3):
        for s in SIG:
            Z = param_point(N64, param, s, 500)[1]
            assert (math.gcd(Z, N64) == 184631) == (s in hit[param]) and math.gcd(Z, N64) in (1, 184631)
        eng = pyecm.Engine(N64)
        eng.build_curves(SIG, params=[param] * 8)
        eng.stage1_extend(1, 500)
        count, first = eng.scan_factors(1)
        assert count == 4 and first == SIG.index(hit[param][0])
        assert [s for k, s in enumerate(SIG) if eng.curve_flag(1, k)] == hit[param]
        assert eng.normalize() == 1
        for k, s in enumerate(SIG):
            line = eng.save_line_std(k)
            assert line.startswith("METHOD=ECM; PARAM=%d; SIGMA=%d; B1=500; " % (param, s))
            if s in hit[param]:
                assert eng.stage1_factor(k) == (184631, True) and "; Z=0x" in line
            else:
                assert eng.stage1_factor(k) is None and line == param_line(N64, param, s, 500)
        eng.close()


def test_stage2_sees_nothing_of_the_parametrisation():
    import pyecm
    eng = _fresh(N412, 0, 1, SIG)
    X, Z, s = _words(eng)
    eng.stage2(20000)
    acc = eng.download_acc()
    other = pyecm.Engine(N412)
    other.upload_points(X, Z, s)
    other.stage1_extend(1000, 1000)                                      # launches nothing: the points are complete to 1000
    other.stage2(20000)
    assert other.download_acc() == acc and len(set(acc)) == 8
    eng.close()
    other.close()


@pytest.mark.parametrize("packing", ["wave", "lane"])
def test_multi_modulus_batches_with_mixed_params(packing):
    import pyecm
    ns = [N297, N412]
    sig = SIG + SIG + [1, 2**32 - 1, 2**64 - 1, 7]
    which = [0] * 8 + [1] * 8 + [0, 1, 0, 1]
    params = [0, 1, 3, 0, 1, 3, 0, 1] + [3, 0, 1, 3, 0, 1, 3, 0] + [1, 3, 1, 3]
    order = sorted(range(20), key=lambda k: (k * 7) % 20)                # the numbers interleaved
    sig, which, params = ([v[k] for k in order] for v in (sig, which, params))
    want = [line_of(ns[w], p, s, 1000) for s, w, p in zip(sig, which, params)]
    single = {}
    for g, n in enumerate(ns):
        eng = pyecm.Engine(n)
        mine = [k for k in range(20) if which[k] == g]
        assert eng.build_curves([sig[k] for k in mine], params=[params[k] for k in mine]) == 0
        eng.stage1_extend(1, 1000)
        assert eng.normalize() == 0
        single.update(zip(mine, eng.save_lines_std()))
        eng.close()
    assert [single[k] for k in range(20)] == want
    for mode in ("host", "device") if packing == "wave" else ("host",):
        me = pyecm.MultiEngine(ns)
        me.set_packing(packing)
        me.set_curve_build(mode)
        assert me.build_curves(sig, which, params=params) == 0
        assert me.packing() == packing and [me.curve_param(k) for k in range(20)] == params
        me.stage1_extend(1, 1000)
        assert me.normalize() == 0
        lines = me.save_lines_std()
        assert lines == want, mode
        assert me.resume_lines(lines, b1_done=1000, params=True) == 0
        assert [me.curve_param(k) for k in range(20)] == params
        me.stage1_extend(1000, 3000)
        assert me.normalize() == 0
        assert me.save_lines_std() == [line_of(ns[w], p, s, 3000) for s, w, p in zip(sig, which, params)]
        me.close()


def test_special_form_twin_runs_param_3_curves():
    import pyecm
    n = (1 << 401) - 1
    lines = {}
    for on in (True, False):
        eng = pyecm.Engine(n)
        eng.set_lanes_per_curve(1)
        eng.set_special_form(on)
        assert eng.build_curves(SIG, params=[3] * 8) == 0
        eng.stage1_extend(1, 1000)
        assert eng.special_form_used() == on
        eng.normalize()
        lines[on] = eng.save_lines_std()
        eng.close()
    assert lines[True] == lines[False]
    for k, s in enumerate(SIG):
        X, Z = param_point(n, 3, s, 1000)
        if math.gcd(Z, n) == 1:
            assert lines[True][k] == param_line(n, 3, s, 1000)
        else:
            assert "; Z=0x" in lines[True][k]
