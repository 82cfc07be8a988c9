"""CPU tests (no GPU) of the P-1 / P+1 layer: the ABI and the Python surface, the method line parser and
its bound function, the PRAC tape interpreted on one residue against pow and a binary Lucas ladder, and the operand
bounds of the device sequence (tests/unit_model.py) at both ends of five limb classes."""
import ctypes
import json
import os
import random
import re

import pytest

from conftest import GOLDEN, ROOT
from unit_model import (METHOD_PM1, METHOD_PP1, RULE9_SEGMENT, SEGMENTS, UNIT_LIMBS, UnitModel, class_bits, class_moduli,
                        expected, exponent, extend_tape, lucas_v, plain_unit, seeds_for)

GECM_OK, GECM_ERR_ARG = 0, -2
NEW = ["gecm_build_seeds", "gecm_build_seeds_multi", "gecm_batch_method", "gecm_curve_seed", "gecm_parse_resume_line_method",
       "gecm_resume_line_std_bound_method"]


@pytest.fixture(scope="module")
def pyecm():
    import pyecm
    return pyecm


def _fixture_lines():
    out = []
    for f in ("stage1.json", "multirange.json", "special.json", "degenerate.json"):
        for c in json.load(open(os.path.join(GOLDEN, f))):
            out += c.get("save_lines", []) + c.get("checkpoint_lines", [])
    return out


def test_prototypes_exports_signatures_and_methods(pyecm):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gecm.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in pyecm.EXPORTS and hasattr(pyecm.lib, name)
        assert getattr(pyecm.lib, name).argtypes is not None
    for c, v in (("GECM_METHOD_ECM", 0), ("GECM_METHOD_PM1", 1), ("GECM_METHOD_PP1", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (c, v), hdr)
    assert (pyecm.METHOD_ECM, pyecm.METHOD_PM1, pyecm.METHOD_PP1) == (0, 1, 2)
    assert len(pyecm.lib.gecm_build_seeds.argtypes) == 6 and len(pyecm.lib.gecm_build_seeds_multi.argtypes) == 7
    assert len(pyecm.lib.gecm_parse_resume_line_method.argtypes) == 5
    for cls in (pyecm.Engine, pyecm.MultiEngine):
        for m in ("build_seeds", "batch_method", "curve_seed"):
            assert callable(getattr(cls, m))
    assert pyecm.MultiEngine.build_seeds is not pyecm.Engine.build_seeds
    assert callable(pyecm.parse_resume_line_method) and callable(pyecm.resume_line_std_bound_method)
    # without a context the calls answer, they do not crash
    assert pyecm.lib.gecm_batch_method(None) == 0
    assert pyecm.lib.gecm_build_seeds(None, 1, None, None, 1, 1) == GECM_ERR_ARG
    assert pyecm.lib.gecm_build_seeds_multi(None, 1, None, None, None, 1, 1) == GECM_ERR_ARG


def test_ecm_lines_parse_as_with_the_param_parser(pyecm):
    lines = _fixture_lines()
    assert len(lines) > 300
    extra = ["METHOD=ECM; PARAM=1; SIGMA=7; B1=3000; N=91; X=5; PROGRAM=GMP-ECM 7.0.5;",
             "PARAM=3; SIGMA=9; B1=11; N=0x5b; X=0x5; Z=3", "# comment", "", "   \r\n"]
    for line in lines + extra:
        a, b = pyecm.parse_resume_line_param(line), pyecm.parse_resume_line_method(line)
        if a is None:
            assert b is None
            continue
        assert tuple(b[:6]) == tuple(a) and b.method == pyecm.METHOD_ECM and b.x0 is None
        bounds = []
        for fn in (pyecm.resume_line_std_bound_method, lambda l: pyecm.resume_line_std_bound(l, params=True)):
            try:
                bounds.append(fn(line))
            except pyecm.GecmError as e:            # a reference line above one prime range: refused alike
                bounds.append(str(e).split(": ", 1)[1])
        assert bounds[0] == bounds[1]
    # an X0 on an ECM line stays ignored
    b = pyecm.parse_resume_line_method("METHOD=ECM; SIGMA=7; B1=10; N=91; X=5; X0=3;")
    assert b.x0 is None and b.method == 0
    # and its refusals are the param parser's, text and all
    for bad in ("METHOD=ECM; SIGMA=5; B1=10; N=91; X=5;", "METHOD=ECM; PARAM=2; SIGMA=7; B1=10; N=91; X=5;",
                "METHOD=ECM; SIGMA=7; B1=10; N=91;"):
        texts = []
        for fn in (pyecm.parse_resume_line_param, pyecm.parse_resume_line_method):
            with pytest.raises(pyecm.GecmError) as e:
                fn(bad)
            texts.append(str(e.value).split(": ", 1)[1])
        assert texts[0] == texts[1]


def test_method_lines(pyecm):
    n, x, x0 = (1 << 89) - 1, 0x1234567890abcdef, 0x2f
    for name, meth in (("P-1", METHOD_PM1), ("P+1", METHOD_PP1)):
        fields = ["METHOD=%s" % name, "B1=1000", "N=0x%x" % n, "X=0x%x" % x, "X0=0x%x" % x0, "PROGRAM=AVX-ECM-STD"]
        want = (0, 1000, n, x, 1, 0, meth, x0)
        rng = random.Random(7)
        for _ in range(12):                                             # fields in any order
            rng.shuffle(fields)
            line = "; ".join(fields) + ";\n"
            assert tuple(pyecm.parse_resume_line_method(line)) == want
            assert pyecm.resume_line_std_bound_method(line) == 1000
        line = "; ".join(fields) + ";"
        assert tuple(pyecm.parse_resume_line_method(line + "\r\n")) == want            # CRLF
        assert tuple(pyecm.parse_resume_line_method(line.rstrip(";"))) == want         # no last ';'
        assert tuple(pyecm.parse_resume_line_method(line.rstrip(";") + "\r\n")) == want
        no_seed = "; ".join(f for f in fields if not f.startswith("X0")) + ";"
        assert tuple(pyecm.parse_resume_line_method(no_seed)) == want[:7] + (None,)
        # SIGMA and PARAM are ignored, wherever they stand and whatever they hold; decimal numbers; Z = 1
        for extra in ("SIGMA=3", "SIGMA=0", "PARAM=2", "PARAM=1; SIGMA=0", "Z=1", "Z=0x1", "Z=0001", "CHECKSUM=12; WHO=me"):
            assert tuple(pyecm.parse_resume_line_method(extra + "; " + line)) == want
            assert tuple(pyecm.parse_resume_line_method(line + " " + extra)) == want
        dec = "METHOD=%s; B1=77; N=%d; X=%d; X0=%d" % (name, n, x, x0)
        assert tuple(pyecm.parse_resume_line_method(dec)) == (0, 77, n, x, 1, 0, meth, x0)
        assert pyecm.resume_line_std_bound_method(dec) == 77
        # a P-1 / P+1 line is a standard line whatever PROGRAM says
        assert pyecm.resume_line_std_bound_method(dec + "; PROGRAM=AVX-ECM;") == 77
        assert pyecm.resume_line_std_bound_method(dec + "; PROGRAM=GMP-ECM 7.0.5;") == 77
        # refusals
        for bad, text in ((line.replace("METHOD=%s" % name, "METHOD=FOO"), "METHOD"),
                          ("Z=2; " + line, r"field Z of a %s line is not 1" % re.escape(name)),
                          ("Z=0; " + line, "field Z"),
                          (line.replace("X=0x%x; " % x, "").replace("X=0x%x;" % x, ""), r"field X is missing"),
                          (line + " X=5;", "field X appears twice"), (line + " X0=5;", "field X0 appears twice"),
                          (line + " B1=5;", "field B1 appears twice"), (line + " N=5;", "field N appears twice"),
                          (line.replace("B1=1000", "B1=1e3"), r"\bfield B1\b"), (line.replace("N=0x", "N=0xg"), r"\bfield N\b")):
            for fn in (pyecm.parse_resume_line_method, pyecm.resume_line_std_bound_method):
                with pytest.raises(pyecm.GecmError, match=text):
                    fn(bad)
        # the older parsers and bound functions refuse the method as they always did
        for fn in (pyecm.parse_resume_line, pyecm.parse_resume_line_param, pyecm.resume_line_std_bound,
                   lambda l: pyecm.resume_line_std_bound(l, params=True)):
            with pytest.raises(pyecm.GecmError) as e:
                fn("SIGMA=7; " + line)
            assert str(e.value).endswith("gecm_parse_resume_line: field METHOD is not ECM")
    # bad arguments
    lib = pyecm.lib
    rec, prm, meth, x0n = pyecm.ResumeRec(), ctypes.c_int(0), ctypes.c_int(0), pyecm.ResumeNum()
    good = b"METHOD=P-1; B1=5; N=91; X=3;"
    assert lib.gecm_parse_resume_line_method(good, ctypes.byref(rec), ctypes.byref(prm), ctypes.byref(meth), ctypes.byref(x0n)) == 0
    assert lib.gecm_parse_resume_line_method(None, ctypes.byref(rec), ctypes.byref(prm), ctypes.byref(meth), ctypes.byref(x0n)) == GECM_ERR_ARG
    assert lib.gecm_parse_resume_line_method(good, None, ctypes.byref(prm), ctypes.byref(meth), ctypes.byref(x0n)) == GECM_ERR_ARG
    assert lib.gecm_parse_resume_line_method(good, ctypes.byref(rec), ctypes.byref(prm), None, ctypes.byref(x0n)) == GECM_ERR_ARG
    assert lib.gecm_parse_resume_line_method(good, ctypes.byref(rec), ctypes.byref(prm), ctypes.byref(meth), None) == GECM_ERR_ARG
    assert lib.gecm_resume_line_std_bound_method(good, None) == GECM_ERR_ARG
    assert lib.gecm_resume_line_std_bound_method(None, ctypes.byref(ctypes.c_uint64(0))) == GECM_ERR_ARG


def test_lucas_ladder_against_the_recurrence():
    n = (1 << 61) - 1
    for x in (0, 1, 2, 3, n - 2, n - 1, 123456789):
        v = [2 % n, x % n]
        for k in range(2, 70):
            v.append((x * v[-1] - v[-2]) % n)
        assert [lucas_v(x, k, n) for k in range(70)] == v
    assert lucas_v(5, 6 * 35, n) == lucas_v(lucas_v(5, 6, n), 35, n)          # V_a(V_b) = V_ab


@pytest.mark.parametrize("lo,hi", SEGMENTS)
def test_tape_on_one_residue_is_pow_and_lucas(pyecm, lo, hi):
    ops, rules, swaps = extend_tape(pyecm.lib, lo, hi)
    e = exponent(lo, hi)
    rng = random.Random(lo + hi)
    n = rng.getrandbits(200) | (1 << 199) | 1
    for x in seeds_for(n, 8, rng) + [0, 1]:
        assert plain_unit(ops, x, METHOD_PM1, n) == pow(x, e, n)
        assert plain_unit(ops, x, METHOD_PP1, n) == lucas_v(x, e, n)
    if (lo, hi) == (1, 1000):
        assert len(ops) == 1989 and swaps == 1054 and rules[0] and rules[1] and rules[2] and rules[3] == 0
    if (lo, hi) == RULE9_SEGMENT:
        # the one-prime chain the GPU tests use for rule 9: all four rules and the swap
        assert e == hi and len(ops) == 25 and rules == [18, 3, 1, 1] and swaps == 15


def test_rule_9_is_absent_below_108223(pyecm):
    ops, rules, swaps = extend_tape(pyecm.lib, 1, 50000)
    assert rules == [85137, 5444, 1298, 0]
    assert extend_tape(pyecm.lib, 108222, 108223)[1][3] >= 1


@pytest.mark.parametrize("nl", UNIT_LIMBS)
def test_device_sequence_keeps_the_bounds(pyecm, nl):
    """tests/unit_model.py: operands below 1.675 K and products below 0.675 K at every multiply, a normalised subtrahend
    below K at every subtraction, a canonical output; and the value is Python's"""
    top, bottom = class_bits(nl)
    rng = random.Random(nl)
    for n, bits in zip(class_moduli(nl), (top, bottom)):
        assert n.bit_length() == bits
        m = UnitModel(n, nl)
        for lo, hi in ((1, 1000), (108222, 108223), RULE9_SEGMENT):
            ops = extend_tape(pyecm.lib, lo, hi)[0]
            e = exponent(lo, hi)
            for x in seeds_for(n, 7, rng):
                for method in (METHOD_PM1, METHOD_PP1):
                    assert m.unit(ops, x, method) == expected(method, x, e, n)
        assert m.subtractions > 1000 and m.multiplies > 1000


def test_sub_full_edges():
    """fe_sub_full at the values where its two chains part: a = b, a = b -+ 1, b = 0, a = 0, b = K - 1"""
    for nl in UNIT_LIMBS:
        m = UnitModel(class_moduli(nl)[0], nl)
        hi = 675 * m.K // 1000 - 1
        for a, b in ((0, 0), (5, 5), (5, 6), (6, 5), (0, m.K - 1), (hi, m.K - 1), (hi, 0), (0, 1), (1 << 28, 1), (1, 1 << 28),
                     ((1 << 56) - 1, 1 << 56), (hi, hi), (hi - 1, hi)):
            m.sub_full(a, b)
