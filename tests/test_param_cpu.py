"""CPU tests (no GPU) of GMP-ECM's PARAM 1 and PARAM 3 curves: the new entry points of the C ABI,
gecm_param_s against Python integers, the device build's sequence (tests/param_model.py) in the kernel's lazy Montgomery
arithmetic with its operand bounds, gecm_parse_resume_line_param on every line the old parser takes and on the PARAM
variants, and the argument checks of gecm_set_next_params that need no context."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from param_model import PARAM_SIGMAS, PARAM_WIDTH, ParamModel, param_d, shift_constant
from suyama_model import LIMB_BITS, N40, N65, N415
from test_resume_cpu import LINE, LINES, _split

GECM_ERR_ARG = -2
# the top and the bottom of the 8- and 37-limb classes (tests/test_build_cpu.py: K = 2N .. 32N)
EXTREMES = [(8, (1 << (28 * 8 - 5)) - 1), (8, 3), (37, (1 << (28 * 37 - 5)) - 1), (37, (1 << (28 * 37 - 5 - 27)) + 1)]
MODULI = [N40, N65, N415, EXTREMES[0][1], EXTREMES[2][1]]


@pytest.fixture(scope="module")
def pyecm():
    import pyecm
    return pyecm


def test_library_exports_the_entry_points_as_documented(pyecm):
    lib = pyecm.lib
    hdr = open(os.path.join(ROOT, "include", "gecm.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    for proto in ("int gecm_param_s(int param, uint64_t sigma, const char *n_str, char *hex, size_t hexlen);",
                  "int gecm_set_next_params(gecm_ctx *ctx, const uint8_t *param, size_t batch);",
                  "int gecm_curve_param(const gecm_ctx *ctx, size_t k);",
                  "int gecm_parse_resume_line_param(const char *line, gecm_resume_rec *rec, int *param);",
                  "int gecm_resume_line_std_bound_param(const char *line, uint64_t *from);"):
        assert proto in flat, proto
    for name, value in (("GECM_PARAM_SUYAMA", 0), ("GECM_PARAM_BATCH_SQUARE", 1), ("GECM_PARAM_BATCH_32", 3)):
        assert re.search(r"#define %s %d\b" % (name, value), hdr), name
    names = ("gecm_param_s", "gecm_set_next_params", "gecm_curve_param", "gecm_parse_resume_line_param",
             "gecm_resume_line_std_bound_param")
    raw = ctypes.CDLL(lib._name)
    for name in names:
        assert hasattr(raw, name), name
    c = ctypes
    assert lib.gecm_param_s.argtypes == [c.c_int, c.c_uint64, c.c_char_p, c.c_char_p, c.c_size_t] and lib.gecm_param_s.restype is c.c_int
    assert lib.gecm_set_next_params.argtypes == [c.c_void_p, c.POINTER(c.c_uint8), c.c_size_t] and lib.gecm_set_next_params.restype is c.c_int
    assert lib.gecm_curve_param.argtypes == [c.c_void_p, c.c_size_t] and lib.gecm_curve_param.restype is c.c_int
    assert lib.gecm_parse_resume_line_param.argtypes == [c.c_char_p, c.POINTER(pyecm.ResumeRec), c.POINTER(c.c_int)]
    assert lib.gecm_parse_resume_line_param.restype is c.c_int
    assert set(names) <= set(pyecm.EXPORTS)
    assert (pyecm.PARAM_SUYAMA, pyecm.PARAM_BATCH_SQUARE, pyecm.PARAM_BATCH_32) == (0, 1, 3)
    import inspect
    for cls, meth, arg in ((pyecm.Engine, "build_curves", "params"), (pyecm.MultiEngine, "build_curves", "params"),
                           (pyecm.Engine, "resume", "params"), (pyecm.MultiEngine, "resume", "params"),
                           (pyecm.Engine, "resume_lines", "params")):
        assert inspect.signature(getattr(cls, meth)).parameters[arg].default in (None, False), (cls, meth)
    assert callable(pyecm.Engine.curve_param) and pyecm.MultiEngine.curve_param is pyecm.Engine.curve_param
    assert callable(pyecm.param_s) and callable(pyecm.parse_resume_line_param)


@pytest.mark.parametrize("n", MODULI, ids=["n40", "n65", "n415", "top8", "top37"])
def test_param_s_equals_python(pyecm, n):
    for param, sigmas in PARAM_SIGMAS.items():
        for sigma in sigmas:
            assert pyecm.param_s(param, sigma, n) == param_d(param, sigma, n), (param, sigma)
    if n == N40:
        assert any(s >= n for s in PARAM_SIGMAS[1])
    # hex and decimal N name the same number; the digits come back lower case without prefix, and their count
    buf = ctypes.create_string_buffer(2048)
    got = pyecm.lib.gecm_param_s(1, 2**64 - 1, hex(n).encode(), buf, len(buf))
    want = "%x" % param_d(1, 2**64 - 1, n)
    assert got == len(want) and buf.value.decode() == want


def test_param_s_on_the_bottom_of_the_limb_classes(pyecm):
    for _, n in (EXTREMES[1], EXTREMES[3]):
        for param, sigmas in PARAM_SIGMAS.items():
            for sigma in sigmas:
                assert pyecm.param_s(param, sigma, n) == param_d(param, sigma, n)


def test_param_s_refusals(pyecm):
    lib = pyecm.lib
    buf = ctypes.create_string_buffer(256)
    n = str(N65).encode()
    for param in (0, 2, 4, -1):
        assert lib.gecm_param_s(param, 7, n, buf, len(buf)) == GECM_ERR_ARG, param
        assert b"gecm_param_s" in lib.gecm_last_error()
    for param in (1, 3):
        assert lib.gecm_param_s(param, 0, n, buf, len(buf)) == GECM_ERR_ARG
        assert b"SIGMA" in lib.gecm_last_error()
    assert lib.gecm_param_s(3, 2**32, n, buf, len(buf)) == GECM_ERR_ARG and b"SIGMA" in lib.gecm_last_error()
    assert lib.gecm_param_s(3, 2**32 - 1, n, buf, len(buf)) > 0
    for bad in (b"", b"12x", b"10", b"1", None):
        assert lib.gecm_param_s(1, 7, bad, buf, len(buf)) == GECM_ERR_ARG, bad
    assert lib.gecm_param_s(1, 7, n, None, 0) == GECM_ERR_ARG
    assert lib.gecm_param_s(1, 2**64 - 1, n, buf, 3) == GECM_ERR_ARG        # the digits do not fit


def test_the_constant_is_one_bit_of_one_limb():
    for nl in (8, 15, 37):
        assert shift_constant(nl, 1) == (nl - 3, 20) and shift_constant(nl, 3) == (nl - 2, 24)
        for param, w in PARAM_WIDTH.items():
            limb, bit = shift_constant(nl, param)
            assert LIMB_BITS * limb + bit == LIMB_BITS * nl - w and 0 <= bit < LIMB_BITS and 0 <= limb < nl
            assert 1 << (LIMB_BITS * limb + bit) < 1 << (LIMB_BITS * nl - 5)       # below R/32 <= K


@pytest.mark.parametrize("n", [N40, N65, N415], ids=["n40", "n65", "n415"])
def test_kernel_sequence_in_montgomery_arithmetic_equals_the_formulae(n):
    k = ParamModel(n)
    for param, sigmas in PARAM_SIGMAS.items():
        for sigma in sigmas + [0]:                   # the kernel computes sigma = 0 (a padding lane) like any other
            X, Z, S = k.build_param(param, sigma)    # asserts the operand bounds of every multiply on the way
            d = (sigma * sigma if param == 1 else sigma) * pow(2, -PARAM_WIDTH[param], n) % n
            assert (X, Z, S) == (2 * k.R % n, k.R % n, d * k.R % n), (param, sigma)
            assert 0 <= X < n and 0 <= S < n


def test_kernel_sequence_at_the_limb_count_extremes():
    for nl, n in EXTREMES:
        k = ParamModel(n, nl)
        for param, sigmas in PARAM_SIGMAS.items():
            for sigma in sigmas:
                assert k.build_param(param, sigma) == (2 * k.R % n, k.R % n, param_d(param, sigma, n) * k.R % n)
    k = ParamModel(N415, 15)
    assert k.nl == 15 and k.build_param(3, 7)[2] == param_d(3, 7, N415) * k.R % N415


def test_param_parser_agrees_with_the_old_one_on_every_line_it_takes(pyecm):
    assert len(LINES) > 400
    for line in LINES:
        assert tuple(pyecm.parse_resume_line_param(line)) == tuple(pyecm.parse_resume_line(line)) + (0,) == _split(line) + (0,)
    for skip in ("", "\n", "# a comment"):
        assert pyecm.parse_resume_line_param(skip) is None


def test_param_variants(pyecm):
    sigma, b1, n, x, z = want = _split(LINE)
    fields = [p.strip() for p in LINE.rstrip(";").split(";")]
    for param in (1, 3):
        sg = sigma if param == 1 else 1234567
        body = [("SIGMA=%d" % sg if f.startswith("SIGMA=") else f) for f in fields]
        for name, line in (("first", "PARAM=%d; " % param + "; ".join(body) + ";"),
                           ("last", "; ".join(body) + "; PARAM=%d" % param),
                           ("hex", "; ".join(body[:1] + ["PARAM=0x%x" % param] + body[1:]) + ";\r\n")):
            got = pyecm.parse_resume_line_param(line)
            assert tuple(got) == (sg,) + want[1:] + (param,), (param, name)
            assert got.param == param
    one = LINE.replace("SIGMA=%d;" % sigma, "SIGMA=1;")
    assert pyecm.parse_resume_line_param(one.replace("METHOD=ECM;", "METHOD=ECM; PARAM=1;")).sigma == 1
    assert pyecm.parse_resume_line_param(one + " PARAM=3;").param == 3
    top = LINE.replace("SIGMA=%d;" % sigma, "SIGMA=%d;" % (2**64 - 1))
    assert pyecm.parse_resume_line_param("PARAM=1; " + top).sigma == 2**64 - 1
    rec, prm = pyecm.ResumeRec(), ctypes.c_int(77)
    cases = [(one, "SIGMA"), (one.replace("METHOD=ECM;", "METHOD=ECM; PARAM=0;"), "SIGMA"),
             (LINE.replace("METHOD=ECM;", "METHOD=ECM; PARAM=2;"), "PARAM"),
             (LINE.replace("METHOD=ECM;", "METHOD=ECM; PARAM=4;"), "PARAM"),
             (LINE + " PARAM=%d;" % 2**40, "PARAM"),
             (LINE.replace("SIGMA=%d;" % sigma, "SIGMA=0;").replace("METHOD=ECM;", "METHOD=ECM; PARAM=1;"), "SIGMA"),
             (LINE.replace("SIGMA=%d;" % sigma, "SIGMA=0; PARAM=3;"), "SIGMA"),
             (LINE.replace("SIGMA=%d;" % sigma, "SIGMA=4294967296; PARAM=3;"), "SIGMA"),
             ("PARAM=3; " + LINE.replace("SIGMA=%d;" % sigma, "SIGMA=4294967296;"), "SIGMA"),
             (LINE.replace("METHOD=ECM;", "METHOD=ECM; PARAM=1; PARAM=3;"), "PARAM")]
    for line, field in cases:
        assert pyecm.lib.gecm_parse_resume_line_param(line.encode(), ctypes.byref(rec), ctypes.byref(prm)) == GECM_ERR_ARG, line
        msg = pyecm.lib.gecm_last_error().decode()
        assert "gecm_parse_resume_line" in msg and re.search(r"\b%s\b" % field, msg), (line, msg)
    assert pyecm.parse_resume_line_param(LINE.replace("SIGMA=%d;" % sigma, "SIGMA=4294967295; PARAM=3;")).sigma == 2**32 - 1
    assert pyecm.lib.gecm_parse_resume_line_param(LINE.encode(), ctypes.byref(rec), None) == GECM_ERR_ARG
    # the old function still refuses both, and the old bound with it; the new bound reads them
    for param in (1, 3):
        line = LINE.replace("METHOD=ECM;", "METHOD=ECM; PARAM=%d;" % param)
        with pytest.raises(pyecm.GecmError, match="PARAM"):
            pyecm.parse_resume_line(line)
        with pytest.raises(pyecm.GecmError, match="PARAM"):
            pyecm.resume_line_std_bound(line)
        assert pyecm.resume_line_std_bound(line, params=True) == b1 - 1          # PROGRAM=AVX-ECM: the reference's multiplier
        assert pyecm.resume_line_std_bound(line.replace("PROGRAM=AVX-ECM;", "PROGRAM=GMP-ECM 7.0.5;"), params=True) == b1
    assert pyecm.resume_line_std_bound(LINE, params=True) == pyecm.resume_line_std_bound(LINE)


def test_set_next_params_rejects_a_null_context_and_unknown_values(pyecm):
    lib = pyecm.lib
    ok = (ctypes.c_uint8 * 4)(0, 1, 3, 0)
    assert lib.gecm_set_next_params(None, ok, 4) == GECM_ERR_ARG
    assert b"gecm_set_next_params" in lib.gecm_last_error()
    assert lib.gecm_set_next_params(None, None, 0) == GECM_ERR_ARG
    assert lib.gecm_curve_param(None, 0) == GECM_ERR_ARG
    # a value other than 0, 1, 3 is refused before the context is looked at: any non-NULL pointer shows it
    dummy = ctypes.cast(ctypes.create_string_buffer(1 << 16), ctypes.c_void_p)
    for bad in (2, 4, 255):
        arr = (ctypes.c_uint8 * 4)(0, 1, bad, 3)
        assert lib.gecm_set_next_params(dummy, arr, 4) == GECM_ERR_ARG, bad
        assert b"gecm_set_next_params" in lib.gecm_last_error()
    assert lib.gecm_set_next_params(dummy, ok, 0) == GECM_ERR_ARG             # an empty batch has no build
