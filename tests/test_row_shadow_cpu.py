"""Which operand of a one-limb-per-lane multiply is scanned does not change the product (avx-ecm_amd/csrc/gecm_row.hpp:
fer_scan / fer_mul_scanned).  A point addition of the 32-lane kernel scans the form of the kept point in its
first multiply and the difference point's coordinate in its third, where it used to scan the new point's form and the fresh
square.  On the integer model of tests/row_bias_model.py (the rows as the kernel runs them, every register write checked
against its width), for moduli at both ends of every one-limb class and operands random and extreme:

 * rows(scan of a, b) and rows(scan of b, a) are the same integer (the quotient by N' is fixed by a x b mod R'; only how the
   carries are spread over the limbs may differ);
 * both stay inside the registers and inside the bounds a multiply promises, and nothing leaves the top lane."""
import pytest

import row_bias_model as B

CASES = [(nl, name, n) for nl in B.NQ1_LIMBS for name, n in B.class_moduli(nl)]


@pytest.mark.parametrize("nl,name,n", CASES, ids=["nl%d-%s" % (c[0], c[1].replace(" ", "_").replace(",", "")) for c in CASES])
def test_either_operand_scanned_gives_the_same_integer(nl, name, n):
    rows = nl + 1
    np_ = B.row_multiple(n)
    R = 1 << (B.LIMB * rows)
    for a, b in B.operand_pairs(np_, rows, "row shadow:%d:%s" % (nl, name), 24):
        a4, b4 = [4 * x for x in a], [4 * x for x in b]
        ab = B.fer_mul4(a4, b4, np_, rows, new=True)          # a scanned, b the lane's own limb
        ba = B.fer_mul4(b4, a4, np_, rows, new=True)
        assert not ab.overflow and not ba.overflow, (ab.overflow[:3], ba.overflow[:3])
        assert ab.top_carry == 0 and ba.top_carry == 0
        for res in (ab, ba):
            assert all(x % 4 == 0 for x in res.limbs4) and not any(res.limbs4[rows:])
            assert all(abs(x) <= 4 * ((1 << 27) + 4) for x in res.limbs4[:rows - 1])
        vab, vba = B.value(ab.limbs4), B.value(ba.limbs4)
        assert vab == vba
        assert (vab // 4 * R - B.value(a) * B.value(b)) % np_ == 0
