"""The end of a multiply of the 32-lane kernel at one limb per lane, with the rounding bias carried by the last two
hand-overs instead of a 64-bit add (avx-ecm_amd/csrc/gecm_row.hpp), on the integer model of
tests/row_bias_model.py.  For every one-limb-per-lane shape (9, 11, 13, 15 and 16 rows), moduli at both ends of the limb
class, and operands random and extreme (limbs at +-(2^29 - 1), the top limb at the value bound):

 * the new form delivers the limbs the old form delivers, register for register;
 * what leaves the top lane is 0 (that is what lets lane 0 take lane 15's high word by row_ror:1);
 * no accumulator leaves the signed 64-bit range with 2^27 in its high word, and no high word leaves 32 bits;
 * and the model itself is a Montgomery multiply: result x R' = a x b (mod N'), |result| < |a||b| / R' + N'."""
import pytest

import row_bias_model as B

CASES = [(nl, name, n) for nl in B.NQ1_LIMBS for name, n in B.class_moduli(nl)]


@pytest.mark.parametrize("nl,name,n", CASES, ids=["nl%d-%s" % (c[0], c[1].replace(" ", "_").replace(",", "")) for c in CASES])
def test_new_end_is_the_old_end(nl, name, n):
    rows = nl + 1
    np_ = B.row_multiple(n)
    assert np_ % n == 0 and np_ & B.M28 == B.M28 and np_ < 1 << (B.LIMB * rows - 5)
    R = 1 << (B.LIMB * rows)
    for a, b in B.operand_pairs(np_, rows, "row bias:%d:%s" % (nl, name), 48):
        a4, b4 = [4 * x for x in a], [4 * x for x in b]
        old = B.fer_mul4(a4, b4, np_, rows, new=False)
        new = B.fer_mul4(a4, b4, np_, rows, new=True)
        assert new.limbs4 == old.limbs4
        assert old.top_carry == 0 and new.top_carry == 0
        assert not old.overflow and not new.overflow, (old.overflow[:3], new.overflow[:3])
        assert all(x % 4 == 0 for x in new.limbs4) and not any(new.limbs4[rows:])
        r = [x // 4 for x in new.limbs4]
        assert all(abs(x) <= (1 << 27) + 4 for x in r[:rows - 1]) and abs(r[rows - 1]) < 1 << 25
        va, vb, vr = B.value(a), B.value(b), B.value(r)
        assert (vr * R - va * vb) % np_ == 0
        assert abs(vr) * R < abs(va) * abs(vb) + np_ * R
        assert 10 * abs(vr) < 12 * np_


def test_the_identity_on_single_registers():
    """T a multiple of 16 in the signed 64-bit range, c the carry of the lane below: old and new end give the same word"""
    lows = [0, 16, (1 << 31) - 16, 1 << 31, (1 << 31) + 16, (1 << 32) - 16, 0x12345670, 0xfedcba90]
    for hi in (-(1 << 30), -5, -1, 0, 1, 7, (1 << 30) - 1):
        for lo in lows:
            t = (hi << 32) + lo
            tn = t + (1 << 31) + (B.Z << 32)                      # what the two hand-overs leave
            assert -(1 << 63) <= tn < 1 << 63
            carry = (t + (1 << 31)) >> 32
            assert B.i32(tn >> 32) == carry + B.Z
            for below in (-8, -1, 0, 1, 8):
                old = B.i32((B.i32(t) >> 2) + (below << 2))
                new = B.i32(((tn & 0xffffffff) >> 2) + ((below + B.Z) << 2))
                assert old == new


def test_the_bias_leaves_room_in_64_bits():
    """the last row's accumulator with K in its high word, at fer_mul's operand bound (|4 x limb| <= 4 (2^29 - 1)) and the
    largest digit and modulus limb: below 2^63; and its high word, which the last hand-over reads as a signed operand"""
    op = 4 * B.OPERAND_LIMB_MAX
    hi_max = (op * op + ((1 << 32) - 16) * B.M28 + (1 << 36)) >> 32         # a row before the last one
    t_max = 16 * hi_max + (1 << 32) + op * op + ((1 << 32) - 16) * B.M28 + (B.K << 32)
    t_min = -16 * hi_max - op * op + (B.K << 32)
    assert t_max < 1 << 63 and t_min >= -(1 << 63)
    assert (t_max >> 32) < 1 << 31 and (t_min >> 32) >= -(1 << 31)
    assert 16 * (t_max >> 32) + (1 << 32) + (B.Z << 32) >= -(1 << 63)
