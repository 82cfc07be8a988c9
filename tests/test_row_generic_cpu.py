"""row_dup_scanned of avx-ecm_amd/csrc/gecm_row.hpp on the limb model of tests/row_bias_model.py, the
rows as the kernel runs them with every register write checked against its width.  The double of the one-limb DPP form
reads the caller's scan of fA in its first multiply, scans p1 (the Z rows' s4, the X rows' own square) in its second and w
in its third, where row_dup scans fA, p1 and r1 + q:

 * with either choice the X rows and the Z rows deliver the same integers, the residues of 4 U V and 4 (s w + V) w;
 * fA, p1, p2, w and r1 + q are inside fer_mul's bound on an operand limb, 4 x (2^29 - 1), whether scanned or the lane's
   own, and no multiply leaves its registers.

Operands: the coordinates X, Z and the curve constant s4 are results of a multiply, balanced limbs and |value| < 1.2 N'.
Directed ones put every limb below the top one at the edge of a product's limb bound, +-(2^27 + 4), in the same, in
alternating and in seeded random signs, with the top limb the largest that keeps the value inside 1.2 N'; and, in the way
of field_model.fixed_point_case, a seeded search keeps of 400 coordinate pairs just under 1.2 N' the one whose first
square comes out largest.  Moduli: the largest and the smallest of the 15- and of the 8-limb class and the special shapes of
row_bias_model.class_moduli (N' of full limbs, N' of zero limbs)."""
import random

import pytest

import row_bias_model as B

PRODUCT_LIMB_MAX = (1 << 27) + 4
CASES = [(nl, name, n) for nl in (15, 8) for name, n in B.class_moduli(nl)]


def product_value(nprime, rows, sign, pattern):
    """limbs below the top one at +-(2^27 + 4), the top limb the largest that keeps |value| <= 1.2 N'"""
    lim = 12 * nprime // 10
    rows = min(rows, (lim.bit_length() - 1) // B.LIMB + 1)
    low = []
    for l in range(rows - 1):
        s = sign if pattern == "same" else (sign if l % 2 == 0 else -sign) if pattern == "alternate" else pattern.choice((-1, 1))
        low.append(s * PRODUCT_LIMB_MAX)
    w = B.LIMB * (rows - 1)
    top = (sign * lim - B.value(low)) >> w if sign > 0 else -((lim + B.value(low)) >> w)
    limbs = low + [top] + [0] * (B.LANES - rows)
    assert abs(B.value(limbs)) <= lim
    return limbs


def near_top(rng, nprime, rows):
    lim = 12 * nprime // 10
    return B.balanced(rng.choice((-1, 1)) * (lim - rng.randrange(lim >> 12)), rows)


def dup(x4, z4, s4, nprime, rows, scanned):
    """(own of the X rows, own of the Z rows, the multiplies, the operands) of D = 2A for A = (x4 : z4), every value
    times 4, limb by limb as row_dup (scanned = False) or row_dup_scanned (True) makes it"""
    mul = lambda scan, own: B.fer_mul4(scan, own, nprime, rows, new=True)
    fa = {"X": [z + x for x, z in zip(x4, z4)], "Z": [x - z for x, z in zip(x4, z4)]}      # row_sd: oth + own, oth - own
    q = {r: mul(fa[r], fa[r]) for r in "XZ"}
    t = {"X": q["Z"].limbs4, "Z": q["X"].limbs4}                                           # the exchange
    out, muls, operands = {}, list(q.values()), list(fa.values())
    for r in "XZ":
        w = [a - b for a, b in zip(t[r], q[r].limbs4)]
        p1, p2 = (s4, w) if r == "Z" else (q[r].limbs4, t[r])
        r1 = mul(p1, p2)
        u = [a + b for a, b in zip(r1.limbs4, q[r].limbs4)]
        third = mul(w, u) if scanned else mul(u, w)
        out[r] = third.limbs4 if r == "Z" else r1.limbs4
        muls += [r1, third]
        operands += [p1, p2, w, u]
    return out["X"], out["Z"], muls, operands


def points(nprime, rows, seed):
    rng = random.Random(seed)
    ex = [product_value(nprime, rows, s, p) for s in (1, -1) for p in ("same", "alternate", rng)]
    pts = [(x, z, rng.choice(ex)) for x in ex for z in ex]
    top = [(near_top(rng, nprime, rows), near_top(rng, nprime, rows)) for _ in range(400)]
    lim = 12 * nprime // 10
    x, z = max(top, key=lambda p: abs(B.value(p[0]) + B.value(p[1])))
    pts.append((x, z, ex[0]))
    for _ in range(16):
        pts.append(tuple(B.balanced(rng.randrange(-lim, lim + 1), rows) for _ in range(3)))
    zero = [0] * B.LANES
    return pts + [(zero, ex[0], ex[1]), (ex[0], zero, ex[1])]


@pytest.mark.parametrize("nl,name,n", CASES, ids=["nl%d-%s" % (c[0], c[1].replace(" ", "_").replace(",", "")) for c in CASES])
def test_scanned_double_gives_the_residues_of_the_plain_one(nl, name, n):
    rows = nl + 1
    np_ = B.row_multiple(n)
    R = 1 << (B.LIMB * rows)
    Ri = pow(R, -1, np_)
    for x, z, s in points(np_, rows, "row generic:%d:%s" % (nl, name)):
        x4, z4, s4 = ([4 * v for v in c] for c in (x, z, s))
        px, pz, pm, po = dup(x4, z4, s4, np_, rows, scanned=False)
        sx, sz, sm, so = dup(x4, z4, s4, np_, rows, scanned=True)
        for res in pm + sm:
            assert not res.overflow and res.top_carry == 0, res.overflow[:3]
            assert all(v % 4 == 0 for v in res.limbs4) and not any(res.limbs4[rows:])
            assert all(abs(v) <= 4 * PRODUCT_LIMB_MAX for v in res.limbs4[:rows - 1])
        for limbs in po + so:
            assert all(abs(v) <= 4 * B.OPERAND_LIMB_MAX for v in limbs)
        assert B.value(sx) == B.value(px) and B.value(sz) == B.value(pz)
        # the residues: U = (X + Z)^2, V = (X - Z)^2 as the model's multiply delivers them (times R'^-1 each time)
        X, Z, S = B.value(x), B.value(z), B.value(s)
        U, V = (X + Z) ** 2 * Ri % np_, (X - Z) ** 2 * Ri % np_
        W = U - V
        assert (B.value(sx) // 4 - U * V * Ri) % np_ == 0
        assert (B.value(sz) // 4 - (S * W * Ri + V) * W * Ri) % np_ == 0
