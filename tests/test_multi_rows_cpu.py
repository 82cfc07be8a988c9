"""CPU tests of the multi-modulus row layout's setting (include/gecm.h gecm_set_multi_rows): the rule
behind "auto", the ABI without a device, and the bounds argument for a small number in a large class.

The bounds argument.  k_stage1_row_multi runs the body of k_stage1_row with the constants of every number of the context
at the context's shape, so a 64-bit N is worked on with up to 38 rows.  The analysis of the multiply (csrc/gecm_row.hpp,
DESIGN.md §5e) uses N' = m N only through N' = -1 mod 2^28, the limbs of N' from ROWS up being zero, and R' >= 32 N'; a
short N' satisfies all three with room.  tests/row_bias_model.py is the register-level model of the one-limb-per-lane
multiply: it takes up to 16 rows, so 9 and 16 rows run on it as they stand.  At 38 rows (three limbs per lane, a form
the model does not cover) the same operands go through the multiply's definition on integers — one Montgomery digit per
row, the digit the low limb itself — and the value contract of fer_mul is checked on every row and on the result."""
import ctypes
import os

import pytest

import row_bias_model as B
from conftest import ROOT
from unit_model import random_modulus
import random

LIB = os.path.join(ROOT, "avx-ecm_amd", "libgecm.so")
N64 = random_modulus(64, random.Random(6464))


@pytest.fixture(scope="module")
def lib():
    L = ctypes.CDLL(LIB)
    L.gecm_multi_rows_auto.argtypes = [ctypes.c_size_t, ctypes.c_int, ctypes.c_int]
    L.gecm_get_multi_rows.argtypes = [ctypes.c_void_p]
    L.gecm_set_multi_rows.argtypes = [ctypes.c_void_p, ctypes.c_int]
    return L


def test_the_rule(lib):
    import pyecm
    for limbs in (8, 15, 17, 37):
        for cus in (1, 64, 256, 304):
            assert lib.gecm_multi_rows_auto(0, limbs, cus) == 0
            sizes = sorted({64, 256, 1024, 4096, 8192, 16384, 32768, 65536} | {cus * k for k in range(1, 300)})
            sizes = [s for s in sizes if s < 1024 * cus] + [1024 * cus, 64 * 1024 * cus]
            got = [lib.gecm_multi_rows_auto(s, limbs, cus) for s in sizes]
            assert set(got) <= {0, 1} and got[0] == 1 and got[-1] == 0
            assert got == sorted(got, reverse=True), (limbs, cus)          # 1 up to its threshold, 0 beyond
            assert got == [pyecm.multi_rows_auto(s, limbs, cus) for s in sizes]
        for cus in (0, -1, -256):
            assert lib.gecm_multi_rows_auto(4096, limbs, cus) == 0
    # the boundaries DESIGN.md section 23 measured on 256 compute units: the last size at which rows won, the first at which they lost
    assert [pyecm.multi_rows_auto(s, 15, 256) for s in (4096, 8192, 16384, 32768)] == [1, 1, 0, 0]
    assert [pyecm.multi_rows_auto(s, 37, 256) for s in (4096, 16384, 32768, 65536)] == [1, 1, 0, 0]
    for limbs in (8, 14, 17, 34):                            # not measured: the smaller bound
        assert [pyecm.multi_rows_auto(s, limbs, 256) for s in (8192, 16384)] == [1, 0]
    # one MI355X: a 256-position batch runs rows, a batch that fills the chip many times over does not
    assert pyecm.multi_rows_auto(256, 15, 256) == 1 and pyecm.multi_rows_auto(1 << 20, 15, 256) == 0


def test_the_abi_without_a_device(lib):
    import pyecm
    for name in ("gecm_set_multi_rows", "gecm_get_multi_rows", "gecm_multi_rows_auto"):
        assert hasattr(lib, name) and name in pyecm.EXPORTS
    assert (pyecm.MULTI_ROWS_OFF, pyecm.MULTI_ROWS_ON, pyecm.MULTI_ROWS_AUTO) == (0, 1, -1)
    assert lib.gecm_get_multi_rows(None) == pyecm.MULTI_ROWS_OFF
    for rows in (0, 1, -1, 2):
        assert lib.gecm_set_multi_rows(None, rows) == -2                   # GECM_ERR_ARG: no context
    hdr = open(os.path.join(ROOT, "include", "gecm.h")).read()
    for text in ("#define GECM_MULTI_ROWS_OFF 0", "#define GECM_MULTI_ROWS_ON 1", "#define GECM_MULTI_ROWS_AUTO (-1)"):
        assert text in hdr


def _montgomery_rows(a, b, nprime, rows):
    """a b / 2^(28 rows) modulo N' = -1 mod 2^28 as the rows compute it, on integers: row i adds limb i of a times b and
    the digit (the low limb itself) times N', and drops the low limb.  Checked on the way: after every row the window
    stays inside the bound the next row's analysis starts from, |T| < |b| 2^29 + 2 N'."""
    vb = B.value(b)
    T = 0
    for i in range(rows):
        T += (a[i] if i < len(a) else 0) * vb
        q = T & B.M28
        T += q * nprime
        assert T & B.M28 == 0
        T >>= B.LIMB
        assert abs(T) < abs(vb) * (1 << 29) + 2 * nprime
    return T


@pytest.mark.parametrize("rows", [9, 16, 38])
def test_a_64_bit_number_in_a_large_class_meets_the_multiplys_bounds(rows):
    np_ = B.row_multiple(N64)
    R = 1 << (B.LIMB * rows)
    assert N64.bit_length() == 64 and np_ % N64 == 0 and np_ & B.M28 == B.M28
    assert R >= 32 * np_ and np_.bit_length() <= 92                        # the top limbs of N' are zero at every shape
    pairs = B.operand_pairs(np_, min(rows, B.LANES), "multi rows:%d" % rows, 48)
    assert len(pairs) > 100
    for a, b in pairs:
        va, vb = B.value(a), B.value(b)
        if rows <= B.LANES:
            a4, b4 = [4 * x for x in a], [4 * x for x in b]
            for new in (False, True):
                res = B.fer_mul4(a4, b4, np_, rows, new=new)               # its own asserts hold
                assert res.top_carry == 0 and not res.overflow, res.overflow[:3]
                assert all(x % 4 == 0 for x in res.limbs4) and not any(res.limbs4[rows:])
                r = [x // 4 for x in res.limbs4]
                assert all(abs(x) <= (1 << 27) + 4 for x in r[:rows - 1]) and abs(r[rows - 1]) < 1 << 25
                vr = B.value(r)
                assert (vr * R - va * vb) % np_ == 0
                assert abs(vr) * R < abs(va) * abs(vb) + np_ * R
                assert 10 * abs(vr) < 12 * np_
        else:
            vr = _montgomery_rows(a, b, np_, rows)
            assert (vr * R - va * vb) % np_ == 0
            assert abs(vr) * R < abs(va) * abs(vb) + np_ * R
            assert 10 * abs(vr) < 12 * np_
            limbs = B.balanced(vr, rows)
            assert B.value(limbs) == vr and not any(limbs[4:])             # the result is as short as N'
