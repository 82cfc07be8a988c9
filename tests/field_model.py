"""The one-lane field arithmetic of avx-ecm_amd/csrc/gecm_field.hpp on Python integers, limb for limb: K' as
gecm_mod_make_kp builds it, fe_add, fe_sub with fe_weak_norm above 25 limbs, fe_cond_sub_n, and the product-scanning
fe_mul / fe_sqr of the five flavours — ModK and ModV (generic REDC; they differ in where the constants come from, not in
a single integer), ModF (2^k - 1: class sums T.t[] as 32-bit words), ModP (2^k + 1) and ModC (2^k - c: the signed
correction terms) — each with ONE 64-bit column accumulator fed in chains of at most GECM_MAD_CHUNK multiply-adds.

Every register write is checked against the width of the register (Width is raised otherwise): a column accumulator
that leaves 64 bits, a class sum that leaves 32, a doubled limb of fe_sqr that loses its top bit, a borrow test of
fe_cond_sub_n that misreads the sign, a top limb that does not fit the 32-bit word it is stored in.  The multiply keeps
the largest column value it saw (Field.peak).

The raw result of a multiply has a definition of its own, (a b + q N) / R with q = -a b / N mod R, written in limbs
below 2^28 with the top limb taking the rest: Field.mul and Field.sqr check themselves against it on every call.

The contract (header of gecm_field.hpp), with m = PRODUCT_BOUND:
  product     M  limbs < 2^28 (top limb: the rest), value < m K
  sum         A  of two products: limbs < 2^29, value < 2 m K
  difference  S  a + K' - b of two products: limbs < 3 2^28 (renormalised above 25 limbs: <= 2^28 + 1), value < (1 + m) K
  every operand of a multiply is below (1 + m) K, and its result is a product again.
The second half of this file makes the directed operands at the edge of that contract which the CPU and the GPU tests
share (directed())."""
import random
from fractions import Fraction
from operator import mul as _times

from divsteps_model import BUILT

LIMB = 28
M28 = (1 << LIMB) - 1
MAD_CHUNK = 14                      # GECM_MAD_CHUNK: multiply-adds per asm statement
U32, U64 = 1 << 32, 1 << 64
# The bound of a product, as a fraction of K.  The map m -> (1 + m)^2 / 16 + 1 / 2 (operands below (1 + m) K, K < R / 16,
# N <= K / 2) has its fixed point at 7 - sqrt(40) = 0.675445: a bound below it is not closed (operands below 1.675 K give
# products up to 0.67535 K: fixed_point_case() makes one), every bound from there to 13 is.
PRODUCT_BOUND = Fraction(6755, 10000)
SUM_BOUND = 2 * PRODUCT_BOUND
OPERAND_BOUND = 1 + PRODUCT_BOUND


class Width(AssertionError):
    """a value that does not fit the register the kernel keeps it in"""


def _fits(x, width, what):
    if not 0 <= x < width:
        raise Width("%s = %#x leaves %d bits" % (what, x, width.bit_length() - 1))
    return x


def fpolicy(nl):
    """(G, NF, NC) of FPolicy<NL>"""
    g = 4 if nl in (26, 37) else 2 if nl in (8, 15) else 3
    nf = nl - g
    return g, nf, (nf + 14) // 15


def norm_sub(nl):
    """LazyPolicy<NL>::norm_sub"""
    return nl > 25


def limbs_of(v, nl):
    """v >= 0 in limbs below 2^28, the top limb taking the rest"""
    assert v >= 0
    return [(v >> (LIMB * i)) & M28 for i in range(nl - 1)] + [v >> (LIMB * (nl - 1))]


def value(limbs):
    return sum(d << (LIMB * i) for i, d in enumerate(limbs))


def make_kp(n, nl):
    """gecm_mod_make_kp: K = 2^j N in [R/32, R/16) with + 2^28 at limb 0, + 2^28 - 1 in the middle, - 1 at the top"""
    k = limbs_of(n << (LIMB * nl - 4 - n.bit_length()), nl)
    kp = [k[i] + (1 << LIMB) if i == 0 else k[i] + M28 if i < nl - 1 else k[i] - 1 for i in range(nl)]
    assert value(kp) == value(k) and all(M28 <= d < 1 << 29 for d in kp[:-1]) and 0 <= kp[-1] < 1 << 29
    return kp


class Field:
    """one modulus at nl limbs and one flavour of the multiply: "K" (ModK), "V" (ModV: the same integers), "F", "P", "C" """

    def __init__(self, n, nl, flavour="K"):
        assert n & 1 and n >= 3 and flavour in "KVFPC"
        self.N, self.nl, self.flavour = n, nl, flavour
        self.R = 1 << (LIMB * nl)
        assert self.R >= 32 * n
        self.n = limbs_of(n, nl)
        self.kp = make_kp(n, nl)
        self.K = value(self.kp)
        assert self.R // 32 <= self.K < self.R // 16 and self.K % n == 0
        self.rho = (-pow(n, -1, 1 << LIMB)) % (1 << LIMB)
        self.nprime = (-pow(n, -1, self.R)) % self.R
        self.G, self.NF, self.NC = fpolicy(nl)
        if flavour in "FC":                      # what ff_setup checks before it chooses the special multiply
            assert all(d == M28 for d in self.n[2 if flavour == "C" else 0:self.NF])
        if flavour == "F":
            assert self.rho == 1
        if flavour == "P":
            assert self.n[0] == 1 and not any(self.n[1:self.NF]) and self.rho == M28
        if flavour == "C":
            assert self.NF >= 3
        self.peak = 0

    # ---- bounds of the contract -----------------------------------------------------------------------------------
    def below(self, v, bound):
        return v * bound.denominator < bound.numerator * self.K

    def limb_max(self, cls):
        """the largest limb below the top one of an operand of class M, A or S"""
        return {"M": M28, "A": 2 * M28, "S": (1 << LIMB) + 1 if norm_sub(self.nl) else 3 * (1 << LIMB) - 1}[cls]

    def value_bound(self, cls):
        return {"M": PRODUCT_BOUND, "A": SUM_BOUND, "S": OPERAND_BOUND}[cls]

    def in_contract(self, limbs, cls):
        """limbs: an operand of that class?  (The top limb is bounded by the value.)"""
        return (len(limbs) == self.nl and all(0 <= d <= self.limb_max(cls) for d in limbs[:-1]) and 0 <= limbs[-1] < U32
                and self.below(value(limbs), self.value_bound(cls)))

    # ---- fe_add, fe_sub, fe_weak_norm, fe_cond_sub_n ----------------------------------------------------------------
    def add(self, a, b):
        return [_fits(x + y, U32, "fe_add limb") for x, y in zip(a, b)]

    def weak_norm(self, r):
        nl = self.nl
        o = [r[0] & M28] + [(r[i] & M28) + (r[i - 1] >> LIMB) for i in range(1, nl - 1)]
        return o + [_fits(r[nl - 1] + (r[nl - 2] >> LIMB), U32, "fe_weak_norm top limb")]

    def sub_raw(self, a, b):
        """a + K' - b limb-wise, before any renormalisation"""
        return [_fits(_fits(x + k, U32, "fe_sub a + K'") - y, U32, "fe_sub limb") for x, k, y in zip(a, self.kp, b)]

    def sub(self, a, b):
        r = self.sub_raw(a, b)
        return self.weak_norm(r) if norm_sub(self.nl) else r

    def cond_sub_n(self, r):
        t, borrow = [], 0
        for i in range(self.nl):
            exact = r[i] - self.n[i] - borrow
            d = exact % U32
            borrow = (d >> 31) & 1
            if borrow != (exact < 0):
                raise Width("fe_cond_sub_n: bit 31 of limb %d misreads the sign of %d" % (i, exact))
            t.append(d if i == self.nl - 1 else d & M28)
        return list(r) if borrow else t

    # ---- the multiply -------------------------------------------------------------------------------------------------
    def _mad(self, acc, xs, ys):
        """one chain of multiply-adds: every factor a 32-bit register, the sum in the 64-bit accumulator (the carry-out
        of v_mad_u64_u32 is ignored: it must not happen)"""
        assert 1 <= len(xs) == len(ys) <= MAD_CHUNK
        acc += sum(map(_times, xs, ys))             # the terms are not negative: the last partial sum is the largest
        if acc > self.peak:
            self.peak = acc
        return _fits(acc, U64, "column accumulator")

    def _col(self, acc, x, y, c, i0, i1):
        """col_vv / col_vs: acc += sum over i in [i0, i1) of x[i] y[c - i], in chunks of GECM_MAD_CHUNK"""
        while i0 < i1:
            hi = min(i0 + MAD_CHUNK, i1)
            acc = self._mad(acc, x[i0:hi], y[c - hi + 1:c - i0 + 1][::-1])
            i0 = hi
        return acc

    def _ab_col(self, acc, a, b, a2, c):
        """the a b half of column c: fe_mul's, or fe_sqr's with the doubled operand a2"""
        nl = self.nl
        lo = max(0, c - nl + 1)
        if a2 is None:
            return self._col(acc, a, b, c, lo, min(c + 1, nl))
        acc = self._col(acc, a, a2, c, lo, (c + 1) // 2)                      # i < c - i
        if c % 2 == 0 and c // 2 < nl:
            acc = self._col(acc, a, a, c, c // 2, c // 2 + 1)
        return acc

    def _redc_f_col(self, acc, T, q, c):
        """redc_f_col<C>: the class sums times F and the generic terms in one chain"""
        nl, nf, nc = self.nl, self.NF, self.NC
        if 0 <= c - nf <= nl - 1:
            T[(c - nf) % nc] = _fits(T[(c - nf) % nc] - q[c - nf], U32, "class sum")
        w_lo, w_hi = max(c - nf + 1, 0), min(c - 1, nl - 1)
        cnt = min(max(w_hi - w_lo + 1, 0), nc)
        i_lo, i_hi = max(c - nl + 1, 0), min(c - nf, nl - 1)
        gen = max(i_hi - i_lo + 1, 0)
        if cnt + gen:
            xs = [T[(w_lo + j) % nc] for j in range(cnt)] + [q[i_lo + j] for j in range(gen)]
            ys = [M28] * cnt + [self.n[c - i_lo - j] for j in range(gen)]
            acc = self._mad(acc, xs, ys)
        return acc

    def _store(self, acc, c):
        """o.v[c - NL]: masked, but for the top limb, which takes the whole low word"""
        if c == 2 * self.nl - 1:
            return _fits(acc, U32, "top limb of the product")
        return acc & M28

    def _mulsqr(self, a, b):
        """b None: fe_sqr(a)"""
        nl, fl = self.nl, self.flavour
        for d in a + (b or []):
            _fits(d, U32, "operand limb")
        a2 = None if b is not None else [_fits(d << 1, U32, "a2 = a << 1") for d in a]
        q, o, acc = [0] * nl, [0] * nl, 0
        T = [0] * self.NC
        e1 = M28 - self.n[1]
        for c in range(2 * nl):
            acc = self._ab_col(acc, a, b, a2, c)
            if fl in "KV":
                acc = self._col(acc, q, self.n, c, max(0, c - nl + 1), min(c, nl))
            elif fl == "P":
                i_lo, i_hi = max(c - nl + 1, 0), min(c - self.NF, nl - 1)
                if i_hi >= i_lo:
                    acc = self._col(acc, q, self.n, c, i_lo, i_hi + 1)
            else:
                acc = self._redc_f_col(acc, T, q, c)
                if fl == "C" and 1 <= c <= nl:                                  # mad_neg: acc -= e1 q[c - 1], signed
                    _fits(e1, 1 << LIMB, "e1")
                    acc = _fits(acc - e1 * q[c - 1], U64, "column accumulator after the signed correction")
            if c >= nl:
                o[c - nl] = self._store(acc, c)
                acc >>= LIMB
                continue
            lo = acc & (U32 - 1)
            if fl in "KV":
                q[c] = (lo * self.rho) % U32 & M28
                acc = self._mad(acc, [q[c]], [self.n[0]])
            elif fl == "P":
                q[c] = (0 - lo) % U32 & M28                                     # rho = -1
                acc = _fits(acc + q[c], U64, "column accumulator")                # limb 0 of the modulus is 1
                self.peak = max(self.peak, acc)
            elif fl == "F":
                q[c] = lo & M28                                                 # rho = 1
            else:
                q[c] = (lo * self.rho) % U32 & M28
                acc = self._mad(acc, [q[c]], [self.n[0]])
            if fl == "F":
                acc = _fits((acc >> LIMB) + q[c], U64, "column accumulator")     # (acc + q F) >> 28
            else:
                if acc & M28:
                    raise Width("column %d is not 0 mod 2^28 after its digit" % c)
                acc >>= LIMB
            if fl in "FC":
                T[c % self.NC] = _fits(T[c % self.NC] + q[c], U32, "class sum")
        return o, value(q)

    def _checked(self, a, b, o, q):
        """the limbs against the definition of the raw product"""
        t = value(a) * value(b)
        want_q = t * self.nprime % self.R
        r = (t + want_q * self.N) // self.R
        assert (t + want_q * self.N) % self.R == 0
        assert q == want_q, "the digits are not -a b / N mod R"
        assert o == limbs_of(r, self.nl), "the limbs are not (a b + q N) / R"
        return o

    def mul(self, a, b):
        o, q = self._mulsqr(list(a), list(b))
        return self._checked(a, b, o, q)

    def sqr(self, a):
        o, q = self._mulsqr(list(a), None)
        return self._checked(a, a, o, q)

    def product(self, a, b):
        """the raw product by its definition alone (what mul and sqr check their limbs against): for the callers that
        want the expected limbs of many products quickly, on operands the limb code has been run over elsewhere"""
        t = value(a) * value(b)
        return limbs_of((t + t * self.nprime % self.R * self.N) // self.R, self.nl)

    def apply(self, op, a, b, by_definition=False):
        """what k_l0_raw leaves for that operator"""
        if by_definition and op in ("mul", "sqr"):
            return self.product(a, a if op == "sqr" else b)
        return {"mul": lambda: self.mul(a, b), "sqr": lambda: self.sqr(a), "add": lambda: self.add(a, b),
                "sub": lambda: self.sub(a, b), "condsub": lambda: self.cond_sub_n(a)}[op]()


OPS = ("mul", "sqr", "add", "sub", "condsub")
CLASSES = "MAS"


# ---- the directed operands --------------------------------------------------------------------------------------------
def _top_under(f, lower, bound, cap):
    """the operand with those lower limbs whose value sits just under bound K: the largest top limb that keeps it there"""
    unit = 1 << (LIMB * (f.nl - 1))
    limit = -(-bound.numerator * f.K // bound.denominator) - 1                # the largest value below bound K
    top = min((limit - value(lower)) // unit, cap)
    assert top >= 0
    return lower + [top]


def class_max(f, cls):
    """every lower limb at the class maximum, the value just under the class's bound"""
    return _top_under(f, [f.limb_max(cls)] * (f.nl - 1), f.value_bound(cls), U32 - 1)


def class_min(f, cls):
    """all limbs minimal: 0 for a product, 1 (as 1 + 0) for a sum, K' itself, sub(0, 0), for a difference"""
    zero = [0] * f.nl
    return {"M": zero, "A": [1] + zero[1:], "S": f.sub(zero, zero)}[cls]


def random_operand(f, cls, rng):
    def product():
        v = rng.randrange(-(-PRODUCT_BOUND.numerator * f.K // PRODUCT_BOUND.denominator))
        if rng.random() < 0.25:                                               # close under the bound
            v = -(-PRODUCT_BOUND.numerator * f.K // PRODUCT_BOUND.denominator) - 1 - rng.getrandbits(40)
        return limbs_of(v, f.nl)
    if cls == "M":
        return product()
    return f.add(product(), product()) if cls == "A" else f.sub(product(), product())


def hot(f, i, j=None):
    """L 2^(28 i) (and + L 2^(28 j)): L the largest limb of any class, the top limb what the value bound allows"""
    nl = f.nl
    big = f.limb_max("A") if norm_sub(nl) else f.limb_max("S")
    v = [0] * nl
    for t in {i, j} - {None}:
        v[t] = big
    if v[nl - 1]:
        bound = f.value_bound("A" if norm_sub(nl) else "S")
        limit = -(-bound.numerator * f.K // bound.denominator) - 1
        v[nl - 1] = 0
        v[nl - 1] = min(big, (limit - value(v)) >> (LIMB * (nl - 1)))
    return v


def fixed_point_case(f, tries=200000):
    """operands below 1.675 K whose product is not below 0.675 K, or None: N close to K / 2 = R / 32 is needed (the
    largest modulus of a limb class).  A seeded search over pairs just under 1.675 K for one whose digits
    q = -a b / N mod R come out nearly R (one pair in 8192 does)."""
    old = Fraction(675, 1000)
    top = -(-(1 + old).numerator * f.K // (1 + old).denominator) - 1
    if 10000 * f.K < 624 * f.R:                             # 1.675^2 K / R + 1 / 2 >= 0.675 needs K / R >= 0.06237
        return None
    rng = random.Random("fixed point:%d:%d" % (f.nl, f.N))
    for _ in range(tries):
        a, b = top - rng.randrange(top >> 12), top - rng.randrange(top >> 12)
        q = a * b * f.nprime % f.R
        if q >= f.R - (f.R >> 13) and not f.below((a * b + q * f.N) // f.R, old):
            return limbs_of(a, f.nl), limbs_of(b, f.nl)
    return None


def directed(f, seed="field", randoms=24):
    """{operator: [(label, a, b)]}: the operands of every operator for this modulus (b None: one operand)"""
    nl, rng = f.nl, random.Random("%s:%d:%d" % (seed, f.nl, f.N))               # the same set for every flavour
    ext = {c + "max": class_max(f, c) for c in CLASSES}
    ext.update({c + "min": class_min(f, c) for c in CLASSES})
    mulc, sqrc = [], []
    for ka, va in ext.items():                                                  # classes: every pair, every square
        sqrc.append((ka, va, None))
        for kb, vb in ext.items():
            mulc.append((ka + "*" + kb, va, vb))
    hots = [hot(f, i) for i in range(nl)]
    for i in range(nl):                                                         # one hot limb each, two for the square
        for j in range(nl):
            mulc.append(("hot%d*hot%d" % (i, j), hots[i], hots[j]))
            if i <= j:
                sqrc.append(("hot%d+%d" % (i, j), hot(f, i, j), None))
    one, zero = [1] + [0] * (nl - 1), [0] * nl
    half = (nl + 1) // 2
    mulc += [("digits F: 1*N", one, limbs_of(f.N, nl)), ("digits 0: a*0", ext["Smax"], zero),
             ("digits 0: a b = R", limbs_of(1 << (LIMB * half), nl), limbs_of(1 << (LIMB * (nl - half)), nl))]
    sqrc += [("digits 0: 0", zero, None), ("1", one, None)]
    fp = fixed_point_case(f)
    if fp:
        mulc.append(("fixed point", fp[0], fp[1]))
    for ca in CLASSES:
        for cb in CLASSES:
            for r in range(randoms):
                mulc.append(("rnd %s*%s %d" % (ca, cb, r), random_operand(f, ca, rng), random_operand(f, cb, rng)))
        for r in range(randoms):
            sqrc.append(("rnd %s %d" % (ca, r), random_operand(f, ca, rng), None))
    # fe_add and fe_sub: the subtrahend a product with every limb 2^28 - 1 and the largest top limb its bound allows, the
    # minuend a sum; the operands of fe_add have normalised limbs
    full = _top_under(f, [M28] * (nl - 1), PRODUCT_BOUND, U32 - 1)
    subc = [("Amax-full", ext["Amax"], full), ("Mmax-full", ext["Mmax"], full), ("0-full", zero, full), ("0-0", zero, zero),
            ("full-0", full, zero), ("Amax-0", ext["Amax"], zero)]
    addc = [("full+full", full, full), ("Mmax+Mmin", ext["Mmax"], ext["Mmin"]), ("0+0", zero, zero), ("1+0", one, zero)]
    for r in range(randoms):
        subc.append(("rnd A-M %d" % r, random_operand(f, "A", rng), random_operand(f, "M", rng)))
        subc.append(("rnd M-M %d" % r, random_operand(f, "M", rng), random_operand(f, "M", rng)))
        addc.append(("rnd M+M %d" % r, random_operand(f, "M", rng), random_operand(f, "M", rng)))
    cond = [(lab, limbs_of(v, nl), None) for lab, v in (("0", 0), ("1", 1), ("N-1", f.N - 1), ("N", f.N), ("N+1", f.N + 1),
                                                        ("2N-1", 2 * f.N - 1))]
    for r in range(randoms):
        cond.append(("rnd %d" % r, limbs_of(rng.randrange(2 * f.N), nl), None))
    return {"mul": mulc, "sqr": sqrc, "add": addc, "sub": subc, "condsub": cond}


def operand_class(f, limbs):
    """the first of M, A, S the operand is in the contract of, or None"""
    return next((c for c in CLASSES if f.in_contract(limbs, c)), None)


# ---- the moduli ---------------------------------------------------------------------------------------------------------
def special_cases(nl):
    """[(flavour, k, c)]: the special forms ff_setup accepts at this limb count (Mw = 2^k - 1, 2^k + 1, 2^k - c of nl limbs
    whose limbs below nl - G are all F, or 1, 0, .. 0), k at both ends; for 2^k - c: c = 3, the c whose low correction
    limb (c - 1) mod 2^28 is the largest an odd c has (2^28 - 2, with a correction of 1 in limb 1), and the largest c below
    one 52-bit reference limb"""
    g, nf, _ = fpolicy(nl)
    prev = BUILT[BUILT.index(nl) - 1] if BUILT.index(nl) else 0
    out = []
    for fl, extra in (("F", 0), ("P", 1), ("C", 0)):
        k_lo = max(LIMB * nf, LIMB * prev - 4 - extra, 64)                      # more limbs than the limb count before
        k_hi = LIMB * nl - 5 - extra                                            # R >= 32 Mw
        for k in (k_lo, k_hi):
            for c in ((3, (1 << 29) - 1, (1 << 51) - 1) if fl == "C" else (1,)):
                out.append((fl, k, c))
    return out


def special_modulus(fl, k, c):
    return (1 << k) + 1 if fl == "P" else (1 << k) - c
