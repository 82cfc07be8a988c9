"""CPU tests (no GPU) of P-1 / P+1 stage 1 with a residue per DPP row: the ABI and the Python surface of
the setting, the rule of gecm_method_lanes_auto, and the kernel's sequence in Python integers with signed limbs
(tests/unit_row_model.py) at both ends of six limb classes: every operand bound, every quotient and every 32-bit word of
the P+1 reduction asserted, and the value Python's pow / Lucas ladder."""
import os
import random
import re

import pytest

from conftest import ROOT
from unit_model import METHOD_PM1, METHOD_PP1, RULE9_SEGMENT, class_bits, class_moduli, expected, exponent, extend_tape, seeds_for
from unit_row_model import ROW_LIMBS, TOP_MIN_BITS, UnitRowModel, row_shape

GECM_ERR_ARG = -2
NEW = ["gecm_set_method_lanes", "gecm_get_method_lanes", "gecm_method_lanes_auto"]
SHAPES = {8: (1, 9), 15: (1, 16), 17: (2, 18), 30: (2, 31), 32: (3, 33), 37: (3, 38)}


@pytest.fixture(scope="module")
def pyecm():
    import pyecm
    return pyecm


def test_prototypes_exports_and_methods(pyecm):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gecm.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in pyecm.EXPORTS and hasattr(pyecm.lib, name)
    assert re.search(r"#define\s+GECM_METHOD_LANES_AUTO\s+\(-1\)", hdr) and pyecm.METHOD_LANES_AUTO == -1
    for cls in (pyecm.Engine, pyecm.MultiEngine):
        assert callable(cls.set_method_lanes) and callable(cls.method_lanes)
    # without a context the calls answer, they do not crash
    assert pyecm.lib.gecm_set_method_lanes(None, 16) == GECM_ERR_ARG
    assert pyecm.lib.gecm_get_method_lanes(None) == 1
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "GECM_METHOD_LANES" in readme and "set_method_lanes" in readme


def test_auto_rule(pyecm):
    """monotone in the positions, 16 at one position, 1 beyond the crossover; nothing but 1 and 16"""
    auto = pyecm.method_lanes_auto
    for limbs in (8, 15, 26, 37):
        for cus in (1, 64, 256, 304):
            got = [auto(p, limbs, cus) for p in [1, 2, 63, 64, 65] + list(range(128, 65536 + 64, 64))]
            assert set(got) <= {1, 16} and got[0] == 16 and got[-1] == 1
            assert got == sorted(got, reverse=True), "16 again after 1"
    # the measured table of DESIGN.md §22 on 256 compute units: 16 lanes win up to 16,384 positions and lose at 65,536
    for limbs in (15, 37):
        assert [auto(p, limbs, 256) for p in (1, 64, 1024, 4096, 16384, 65536)] == [16, 16, 16, 16, 16, 1]
    assert auto(16384 + 64, 15, 256) == 1 and auto(1 << 20, 37, 256) == 1
    assert auto(0, 15, 256) == 1 and auto(64, 15, 0) == 1 and auto(64, 15, -3) == 1


def test_shapes_and_the_modulus_band():
    """N'' is -1 modulo 2^28, a multiple of N, and its top limb lies in [2^20, 2^23 (1 + 2^-3)) at both ends of every
    class — the bottom of class 8 is the 64-bit N whose N' = m N has no top limbs at all"""
    for nl in ROW_LIMBS:
        assert row_shape(nl) == SHAPES[nl]
        for n, bits in zip(class_moduli(nl), class_bits(nl)):
            assert n.bit_length() == bits
            m = UnitRowModel(n, nl)
            assert 1 << TOP_MIN_BITS <= m.Ml[m.L - 1] < (1 << 23) + (1 << 20)
            assert len(m.two) == m.L and (2 * m.Rp - sum(d << (28 * i) for i, d in enumerate(m.two))) % m.M == 0
    small = UnitRowModel(class_moduli(8)[1], 8)
    assert small.n.bit_length() == 64 and small.t > 0 and (small.rho * small.n) >> (28 * 8) == 0
    # a small number on a large context (a multi-modulus batch): scaled to the same band
    wide = UnitRowModel(class_moduli(8)[1], 37)
    assert wide.L == 38 and wide.Ml[37] >= 1 << TOP_MIN_BITS


@pytest.mark.parametrize("nl", ROW_LIMBS)
def test_row_sequence_keeps_the_bounds(pyecm, nl):
    """tests/unit_row_model.py at both ends of the class: the tapes (1, 1000] and the rule-9 segment, seeds_for plus 0"""
    rng = random.Random(nl)
    for n in class_moduli(nl):
        m = UnitRowModel(n, nl)
        for lo, hi in ((1, 1000), RULE9_SEGMENT):
            ops = extend_tape(pyecm.lib, lo, hi)[0]
            e = exponent(lo, hi)
            for x in seeds_for(n, 6, rng) + [0]:
                for method in (METHOD_PM1, METHOD_PP1):
                    assert m.unit(ops, x, method) == expected(method, x, e, n)
        assert m.reductions > 1000 and m.multiplies > 1000 and 1 <= m.max_q <= 2


def test_small_number_on_a_wide_context(pyecm):
    """a multi-modulus batch: a 64-bit and a 219-bit number with the 38 rows of a 37-limb context"""
    ops = extend_tape(pyecm.lib, 1, 1000)[0]
    e = exponent(1, 1000)
    rng = random.Random(7)
    for n in (class_moduli(8)[1], class_moduli(8)[0]):
        m = UnitRowModel(n, 37)
        for x in seeds_for(n, 6, rng) + [0]:
            for method in (METHOD_PM1, METHOD_PP1):
                assert m.unit(ops, x, method) == expected(method, x, e, n)
