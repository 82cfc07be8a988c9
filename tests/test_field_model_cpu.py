"""The limb-level model of csrc/gecm_field.hpp (tests/field_model.py) on its own directed operands, at every built limb
count: the smallest and the largest modulus of the limb count in five kinds, and the special forms ff_setup accepts
there.  Every operand is inside the contract, no register leaves its width, every raw product is a product again
(limbs below 2^28 under the top one, value below PRODUCT_BOUND K) and is the value KernelModel.mul gives; and the set
is hard enough: the 64-bit column accumulator is driven to 90 % of NL La Lb for every pair of operand classes, and past
2^63 wherever NL La Lb is.  The GPU counterpart (tests/test_gpu_field_raw.py) compares the device's limbs with these."""
from fractions import Fraction

import pytest

import divsteps_model as D
import field_model as F
from suyama_model import KernelModel

EDGE = {}
for _nl, _bits in D.edge_bits():
    EDGE.setdefault(_nl, []).append(_bits)


def generic_fields(nl):
    return [F.Field(D.modulus(bits, kind), nl, "K") for bits in EDGE[nl] for kind in D.KINDS]


def special_fields(nl):
    return [F.Field(F.special_modulus(fl, k, c), nl, fl) for fl, k, c in F.special_cases(nl)]


def run_set(f):
    """the directed set of one modulus through the model: every check that is the same for every flavour"""
    km = KernelModel(f.N, f.nl)
    assert km.K == f.K
    cases = F.directed(f)
    assert set(cases) == set(F.OPS)
    for op in ("mul", "sqr"):
        for lab, a, b in cases[op]:
            for v in (a, b) if b is not None else (a,):
                assert F.operand_class(f, v), (f.nl, f.flavour, op, lab, "operand outside the contract")
            r = f.apply(op, a, b)                        # Width, or the self-check against (a b + q N) / R, fails in here
            assert all(d <= F.M28 for d in r[:-1]) and f.in_contract(r, "M"), (f.nl, f.flavour, op, lab)
            assert F.value(r) == km.mul(F.value(a), F.value(a if b is None else b))
    for lab, a, b in cases["add"]:
        assert f.in_contract(a, "M") and f.in_contract(b, "M"), lab
        r = f.apply("add", a, b)
        assert F.value(r) == F.value(a) + F.value(b) and f.in_contract(r, "A"), lab
    for lab, a, b in cases["sub"]:
        assert F.operand_class(f, a) in ("M", "A") and f.in_contract(b, "M"), lab
        raw, r = f.sub_raw(a, b), f.apply("sub", a, b)
        assert F.value(raw) == F.value(r) == F.value(a) + f.K - F.value(b), lab
        assert r == (f.weak_norm(raw) if F.norm_sub(f.nl) else raw), lab
        if f.in_contract(a, "M"):                        # a difference of two products: an operand of class S
            assert all(d < 3 << F.LIMB for d in raw) and f.in_contract(r, "S"), lab
    for lab, a, _ in cases["condsub"]:
        v = F.value(a)
        assert v < 2 * f.N and all(d <= F.M28 for d in a), lab
        assert f.apply("condsub", a, None) == F.limbs_of(v - f.N if v >= f.N else v, f.nl), lab
    return cases


def class_pair_peaks(f):
    """{(class a, class b): largest column value of the multiply of the two class maxima}"""
    out = {}
    for ca in F.CLASSES:
        for cb in F.CLASSES:
            f.peak = 0
            f.mul(F.class_max(f, ca), F.class_max(f, cb))
            out[ca + cb] = f.peak
    return out


PEAKS = {}       # limb count -> (largest column value of the whole set over the generic moduli, {pair: peak / (NL La Lb)})


@pytest.mark.parametrize("nl", D.BUILT)
def test_directed_set_on_generic_moduli(nl):
    peak, ratio = 0, {}
    for f in generic_fields(nl):
        f.peak = 0
        run_set(f)
        peak = max(peak, f.peak)
        for pair, p in class_pair_peaks(f).items():
            full = nl * f.limb_max(pair[0]) * f.limb_max(pair[1])
            ratio[pair] = max(ratio.get(pair, 0), Fraction(p, full))
    PEAKS[nl] = (peak, ratio)
    lmax = max(F.Field(D.modulus(EDGE[nl][1], "2^k-1"), nl).limb_max(c) for c in F.CLASSES)
    print("nl %2d: column peak %.3f 2^64; of NL La Lb: %s%s" % (
        nl, peak / 2.0 ** 64, " ".join("%s %.2f" % (p, float(r)) for p, r in sorted(ratio.items())),
        "; NL Lmax^2 >= 2^63" if nl * lmax * lmax >= 1 << 63 else ""))
    for pair, r in ratio.items():
        assert r >= Fraction(9, 10), (nl, pair, float(r))
    if nl * lmax * lmax >= 1 << 63:
        assert peak > 1 << 63, (nl, peak / 2.0 ** 64)
    assert peak < 1 << 64


@pytest.mark.parametrize("nl", D.BUILT)
def test_directed_set_on_special_forms(nl):
    """the same through the F-, P- and C-form column code: k at both ends of the limb count, c = 3, the c with the largest
    low correction limb, the largest c below a reference limb.  (That the special multiply leaves the integers of the
    generic one is part of every call: both are checked against the definition of the raw product.)"""
    fields = special_fields(nl)
    assert [f.flavour for f in fields] == ["F", "F", "P", "P"] + ["C"] * 6
    for f in fields:
        assert D.dev_limbs(f.N.bit_length()) == nl
        cases = run_set(f)
        g = F.Field(f.N, nl, "K")
        for lab, a, b in cases["mul"][:40]:
            assert g.mul(a, b) == f.mul(a, b), lab


@pytest.mark.parametrize("nl", D.BUILT)
def test_product_bound_of_0_675_is_not_closed_and_0_6755_is(nl):
    """The finding of this model: on the largest modulus of a limb count (N close to R / 32 = K / 2) two operands below
    1.675 K have a product that is not below 0.675 K: the fixed point of m -> (1 + m)^2 / 16 + 1 / 2 is 7 - sqrt(40) =
    0.675445.  The case stays in the directed set; the bound is PRODUCT_BOUND = 0.6755, which is closed."""
    f = F.Field(D.modulus(EDGE[nl][1], "2^k-1"), nl)
    fp = F.fixed_point_case(f)
    assert fp, "the seeded search found no pair"
    a, b = fp
    old = Fraction(675, 1000)
    assert f.below(F.value(a), 1 + old) and f.below(F.value(b), 1 + old)
    r = f.mul(a, b)
    assert not f.below(F.value(r), old) and f.in_contract(r, "M")
    assert ("fixed point", a, b) in F.directed(f)["mul"]
    m = F.PRODUCT_BOUND
    assert (1 + m) ** 2 / 16 + Fraction(1, 2) < m and (1 + old) ** 2 / 16 + Fraction(1, 2) > old


def test_width_checks_fire_outside_the_contract():
    """the model is not blind: operands outside the contract leave a register"""
    f = F.Field(D.modulus(EDGE[23][1], "2^k-1"), 23)
    wide = [(1 << 32) - 1] * 23
    with pytest.raises(F.Width, match="column accumulator"):
        f.mul(wide, wide)
    with pytest.raises(F.Width, match="a2 = a << 1"):
        f.sqr([1 << 31] + [0] * 22)
    with pytest.raises(F.Width, match="fe_sub limb"):
        f.sub([0] * 23, [1 << 30] * 23)
    with pytest.raises(F.Width, match="misreads the sign"):
        f.cond_sub_n([(1 << 32) - 1] + [0] * 22)
    g = F.Field(F.special_modulus("F", 28 * 37 - 5, 1), 37, "F")
    with pytest.raises(F.Width):
        g.mul([(1 << 30) - 1] * 37, [(1 << 30) - 1] * 37)


def test_kp_is_what_gecm_mod_make_kp_builds():
    for nl, bits in D.edge_bits():
        for kind in D.KINDS:
            n = D.modulus(bits, kind)
            kp = F.make_kp(n, nl)
            k = n << (F.LIMB * nl - 4 - bits)
            assert F.value(kp) == k and (1 << (F.LIMB * nl)) // 32 <= k < (1 << (F.LIMB * nl)) // 16
            assert kp[0] >= 1 << F.LIMB and all(d >= F.M28 for d in kp[1:-1])
