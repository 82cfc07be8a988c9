"""The field functions of csrc/gecm_field.hpp on the device, on lazy operands at the edge of their contract: k_l0_raw
through gecm_vecrawop, the limbs it leaves against the limb model of tests/field_model.py, word for word.  The operands
are the model's directed set (classes M, A, S at their limb maxima and value bounds and at their minima, one hot limb in
every position pair, the REDC digits all 2^28 - 1 and all 0, the pair at the fixed point of the product bound, seeded
random operands of every class pair, fe_add / fe_sub / fe_cond_sub_n at their edges), at every built limb count:

  ModK   the smallest and the largest modulus of the limb count (the largest: 2^k - 1, where the column accumulator
         peaks), the expected limbs by the limb code of the model;
  ModF, ModP, ModC   the same set on the special-form twin, for every special form of field_model.special_cases;
  ModV   the same set on one lane-packed batch at 8 .. 15 limbs, ten moduli (both ends of the limb count, five kinds)
         alternating lane by lane, so that a lane reading its neighbour's N, rho or K' column shows.

For the last two the expected products are the model's definition of the raw product, (a b + q N) / R, which
tests/test_field_model_cpu.py shows its limb code to equal on these very sets.  One launch per (modulus or batch,
operator).  Independent of the model: every product the device returns has limbs below 2^28 under the top one and a value
below PRODUCT_BOUND K."""
import pytest

import divsteps_model as D
import field_model as F

pytestmark = pytest.mark.gpu

EDGE = {}
for _nl, _bits in D.edge_bits():
    EDGE.setdefault(_nl, []).append(_bits)
LANE_NLS = [nl for nl in D.BUILT if nl <= 15]


def _code(op):
    import pyecm
    return {"mul": pyecm.RAW_MUL, "sqr": pyecm.RAW_SQR, "add": pyecm.RAW_ADD, "sub": pyecm.RAW_SUB,
            "condsub": pyecm.RAW_CONDSUB}[op]


def _product_ok(f, r):
    return all(d <= F.M28 for d in r[:-1]) and f.below(F.value(r), F.PRODUCT_BOUND)


def _run_set(eng, f, target, by_definition):
    for op, cases in F.directed(f).items():
        a = [c[1] for c in cases]
        b = None if cases[0][2] is None else [c[2] for c in cases]
        got = eng.vecrawop(_code(op), a, b, target=target, limbs=f.nl)
        assert len(got) == len(cases)
        for k, (lab, x, y) in enumerate(cases):
            assert got[k] == f.apply(op, x, y, by_definition), (f.nl, f.flavour, hex(f.N), op, lab)
            if op in ("mul", "sqr"):
                assert _product_ok(f, got[k]), (f.nl, f.flavour, op, lab)


@pytest.mark.parametrize("nl", D.BUILT)
def test_generic_multiply_on_both_edge_moduli(nl):
    import pyecm
    for bits, kind in ((EDGE[nl][0], "random"), (EDGE[nl][1], "2^k-1")):
        f = F.Field(D.modulus(bits, kind), nl, "K")
        eng = pyecm.Engine(f.N)
        assert eng.cfg.dev_limbs == nl
        _run_set(eng, f, pyecm.RAW_OWN, False)
        eng.close()


SPECIAL = [(nl,) + c for nl in D.BUILT for c in F.special_cases(nl)]


@pytest.mark.parametrize("nl,fl,k,c", SPECIAL, ids=["nl%d_%s_k%d_c%x" % s for s in SPECIAL])
def test_special_multiplies_on_the_twin(nl, fl, k, c):
    import pyecm
    f = F.Field(F.special_modulus(fl, k, c), nl, fl)
    eng = pyecm.Engine(f.N)
    on, tk, limbs = eng.special_form()
    assert on and tk == (-k if fl == "P" else k) and limbs == nl == eng.cfg.dev_limbs
    _run_set(eng, f, pyecm.RAW_TWIN, True)
    eng.close()


@pytest.mark.parametrize("nl", LANE_NLS)
def test_a_modulus_per_lane(nl):
    import pyecm
    fields = [F.Field(D.modulus(bits, kind), nl, "V") for kind in D.KINDS for bits in EDGE[nl]]
    sets = [F.directed(f) for f in fields]
    m = len(fields)
    rounds = max(len(s[op]) for s in sets for op in F.OPS)
    eng = pyecm.MultiEngine([f.N for _ in range(rounds) for f in fields])        # position p works modulo fields[p % m].N
    assert eng.cfg.dev_limbs == nl
    eng.set_packing("lane")
    eng.build_seeds(pyecm.METHOD_PM1, [3] * (rounds * m), list(range(rounds * m)))
    assert eng.packing() == "lane"                      # the numbers lie back to back in their order: position p is number p
    positions = pyecm.multi_positions([1] * (rounds * m), "lane")
    zero = [0] * nl
    for op in F.OPS:
        a, b, want = [], [], []
        for p in range(positions):
            f, s = fields[p % m], sets[p % m][op]
            lab, x, y = s[p // m] if p < rounds * m and p // m < len(s) else ("padding", zero, zero)
            a.append(x)
            b.append(y if y is not None else zero)
            want.append((lab, f.apply(op, x, y, True)) if p < rounds * m else None)
        got = eng.vecrawop(_code(op), a, b, target=pyecm.RAW_BATCH)
        for p in range(rounds * m):
            assert got[p] == want[p][1], (nl, p, p % m, op, want[p][0])
            if op in ("mul", "sqr"):
                assert _product_ok(fields[p % m], got[p]), (nl, p, op)
    eng.close()


def test_sizes_and_state_are_checked_and_values_are_not():
    import pyecm
    n = D.modulus(EDGE[15][1], "random")
    eng = pyecm.Engine(n)
    nl = eng.cfg.dev_limbs
    wild = [[0xffffffff] * nl] * 65                                              # far outside the contract: unspecified limbs
    assert len(eng.vecrawop(pyecm.RAW_MUL, wild, wild)) == 65
    with pytest.raises(pyecm.GecmError, match="no special-form twin"):
        eng.vecrawop(pyecm.RAW_MUL, wild, wild, target=pyecm.RAW_TWIN, limbs=nl)
    with pytest.raises(pyecm.GecmError, match="GECM_RAW_BATCH needs"):
        eng.vecrawop(pyecm.RAW_MUL, wild, wild, target=pyecm.RAW_BATCH)
    with pytest.raises(pyecm.GecmError, match="bad argument"):
        eng.vecrawop(7, wild, wild)
    f = F.Field(n, nl)
    one = [1] + [0] * (nl - 1)
    assert eng.vecrawop(pyecm.RAW_MUL, [one], [F.limbs_of(f.N, nl)]) == [F.limbs_of(f.N, nl)]   # usable after the refusals
    eng.close()
    multi = pyecm.MultiEngine([n, n - 2])
    with pytest.raises(pyecm.GecmError, match="not available on a multi-modulus context"):
        multi.vecrawop(pyecm.RAW_MUL, [one], [one])
    with pytest.raises(pyecm.GecmError, match="GECM_RAW_BATCH needs"):             # no batch yet
        multi.vecrawop(pyecm.RAW_MUL, [one], [one], target=pyecm.RAW_BATCH)
    multi.build_seeds(pyecm.METHOD_PM1, [3, 3], [0, 1])                            # wave-packed: not served
    with pytest.raises(pyecm.GecmError, match="GECM_RAW_BATCH needs"):
        multi.vecrawop(pyecm.RAW_MUL, [one] * 128, [one] * 128, target=pyecm.RAW_BATCH)
    multi.close()
