"""Wide contexts: the numbers the tests run on, and a Python-integer model of the three-limbs-per-lane
row multiply (avx-ecm_amd/csrc/gecm_row.hpp: fer_mul at NQ = 3, the C-written path) as stage1_row uses it at the wide
shapes, register by register, the way tests/row_bias_model.py models the one-limb form.

A row of 16 lanes holds 48 limbs, lane l the limbs 3l, 3l + 1, 3l + 2.  Every lane keeps three signed 64-bit
accumulators T[0..2], each 16 x (its slot of the window); the roles rotate with the row number.  Row i:
  Q      = the low register of lane 0's T[i % 3]                  (16 x the Montgomery digit, as 32 unsigned bits; rho = 1)
  T[(t + i) % 3] += Q * n[t]              for t = 0, 1, 2         (unsigned 32 x 32 -> 64, wrapping like the hardware)
  T[(t + i + 1) % 3] += A[i + 1] * b4[t]  for t = 0, 1            (A[j] = 4 x limb j of a, broadcast; signed 32 x 32)
  hi, lo = the two registers of T[i % 3];  lo moves one lane down (row_shl:1: lane l takes lane l + 1's, lane 15 takes 0)
  T[(i + 1) % 3] += hi * 16
  T[i % 3]      = A[i + 1] * b4[2] + lo   (the last row: lo alone)
and after ROWS rows the balanced normalisation of fer_mul's end.  The model keeps the accumulators as Python integers
and RECORDS the largest magnitude written (`peak_acc`: the kernel's are signed 64-bit) and the largest high word read
as a multiply-add operand (`peak_hi`: v_mad_i64_i32 takes a signed 32-bit operand); the low register of an accumulator is
its value modulo 2^32, which is what the hardware keeps whenever the value fits 64 bits."""
import random

LIMB = 28
MASK = (1 << LIMB) - 1
NQ = 3
LANES = 16
WIDE_ROWS = (41, 44, 48)                 # csrc/gecm_rowk.h: GECM_ROW_WIDE_SHAPES
WIDE_NL = (40, 43, 47)
WIDE_MAX_BITS = 1311
# (limb count, fewest bits, most bits) of every wide class: 28 nl >= bits + 5, from the first length gecm_create refuses
WIDE_CLASSES = ((40, 1032, 1115), (43, 1116, 1199), (47, 1200, 1311))


def wide_nl(bits):
    """the limb rule of gecm_create_wide: the smallest of 40, 43, 47 with 28 nl >= bits + 5; 0 above 1311 bits"""
    for nl in WIDE_NL:
        if LIMB * nl >= bits + 5:
            return nl
    return 0


def modulus(bits, kind):
    """the modulus of that kind with exactly `bits` bits (the kinds and the seeding of tests/divsteps_model.modulus, which
    stops at the built limb counts)"""
    rng = random.Random("modulus:%d:%s" % (bits, kind))
    top = 1 << (bits - 1)
    if kind == "random":
        n = rng.getrandbits(bits) | top | 1
    elif kind == "2^k-1":
        n = (1 << bits) - 1
    elif kind == "2^k+1":
        n = top + 1
    elif kind == "1mod2^28":
        n = ((rng.getrandbits(bits) | top) >> LIMB << LIMB) | 1
    else:
        raise ValueError(kind)
    assert n.bit_length() == bits and n & 1
    return n


# ---- the constants of gecm_mod_row_consts for the stage-1 kernel ----
def row_consts(n, nl):
    """N' = m N = -1 mod 2^28, the entry factor R'^2 / R mod N, R mod N, K' of N (as its limbs), rho of N"""
    rows = nl + 1
    m = (-pow(n, -1, 1 << LIMB)) % (1 << LIMB)
    np_ = m * n
    assert np_ & MASK == MASK and np_.bit_length() + 5 <= LIMB * rows
    cin = pow(2, 2 * LIMB * rows - LIMB * nl, n)
    one = pow(2, LIMB * nl, n)
    k = n << (LIMB * nl - 4 - n.bit_length())
    kp = [(k >> (LIMB * i)) & MASK for i in range(nl)]
    kp = [kp[i] + ((1 << LIMB) if i == 0 else (1 << LIMB) - 1 if i < nl - 1 else -1) for i in range(nl)]
    return {"np": np_, "cin": cin, "one": one, "kp": kp, "rho": m, "rows": rows}


def limbs_of(v, count):
    """the unsigned 28-bit limbs of v >= 0"""
    assert 0 <= v < 1 << (LIMB * count)
    return [(v >> (LIMB * i)) & MASK for i in range(count)]


def value_of(limbs):
    return sum(x << (LIMB * i) for i, x in enumerate(limbs))


def _s32(x):
    x &= 0xffffffff
    return x - (1 << 32) if x >> 31 else x


class RowMul:
    """fer_mul<3, ROWS, RHO1, false, A4, B4, R4> on the 48 limbs of a row; limbs are signed Python integers"""

    def __init__(self, rows):
        assert 2 * LANES < rows <= 3 * LANES
        self.rows = rows
        self.peak_acc = 0        # largest |accumulator| written
        self.peak_hi = 0         # largest |high word| read as a multiply-add operand
        self.peak_op = 0         # largest |operand limb| x 4 read by a multiply-add

    def _acc(self, v):
        self.peak_acc = max(self.peak_acc, abs(v))
        return v

    def mul(self, a, b, mod_limbs, rho=1, a4=False, b4=False, r4=False):
        """a, b: 48 signed limbs each (zero from `rows` up), mod_limbs: the 48 unsigned limbs of the modulus.  Returns
        the 48 signed limbs of the result (times 4 with r4) and the digits used."""
        rows = self.rows
        A = [x if a4 else _s32(x << 2) for x in a]
        B = [x if b4 else _s32(x << 2) for x in b]
        for x in A + B:
            self.peak_op = max(self.peak_op, abs(x))
        T = [[self._acc(A[0] * B[NQ * l + t]) for t in range(NQ)] for l in range(LANES)]
        digits = []
        for i in range(rows):
            rot, nxt = i % NQ, (i + 1) % NQ
            q = (T[0][rot] & 0xffffffff) * rho & 0xffffffff        # 16 x the digit, 32 unsigned bits
            digits.append(q)
            ac = A[i + 1] if i + 1 < rows else 0
            los = []
            for l in range(LANES):
                Tl = T[l]
                for t in range(NQ):
                    Tl[(t + rot) % NQ] = self._acc(Tl[(t + rot) % NQ] + q * mod_limbs[NQ * l + t])
                if i + 1 < rows:
                    for t in range(NQ - 1):
                        Tl[(t + nxt) % NQ] = self._acc(Tl[(t + nxt) % NQ] + ac * B[NQ * l + t])
                los.append(Tl[rot] & 0xffffffff)
            assert los[0] == 0, "the digit clears the low register of lane 0"
            for l in range(LANES):
                Tl = T[l]
                hi = Tl[rot] >> 32
                self.peak_hi = max(self.peak_hi, abs(hi))
                lo = los[l + 1] if l + 1 < LANES else 0
                Tl[nxt] = self._acc(Tl[nxt] + hi * 16)
                Tl[rot] = self._acc(ac * B[NQ * l + NQ - 1] + lo) if i + 1 < rows else lo
        # balanced normalisation in the accumulators' own scale
        out = [0] * (NQ * LANES)
        tops = []
        for l in range(LANES):
            Tl = T[l]
            carry = 0
            lo = [0] * NQ
            for t in range(NQ - 1):
                u16 = Tl[(t + rows) % NQ] + (1 << 31)
                if t > 0:
                    u16 += carry * 16
                self._acc(u16)
                carry = u16 >> 32
                self.peak_hi = max(self.peak_hi, abs(carry))
                lo[t] = (((u16 & 0xffffffff) >> 4) & MASK) - (1 << 27)
            full = (Tl[(NQ - 1 + rows) % NQ] >> 4) + carry + (1 << 27)
            assert -(1 << 31) <= full < 1 << 31, "the top slot of a lane fits its 32-bit register"
            lo[NQ - 1] = (full & MASK) - (1 << 27)
            tops.append(full >> LIMB)
            out[NQ * l:NQ * l + NQ] = lo
        assert tops[LANES - 1] == 0, "nothing leaves the top lane"
        for l in range(1, LANES):
            out[NQ * l] += tops[l - 1]
        if r4:
            out = [_s32(x << 2) for x in out]
        return out, digits


def signed_value(limbs, scale=1):
    v = sum(x << (LIMB * i) for i, x in enumerate(limbs))
    assert v % scale == 0
    return v // scale


class Stage1Ends:
    """The entry multiply, the exit multiply and the + K' pass of stage1_row for one modulus at a wide shape."""

    def __init__(self, n, nl):
        self.n, self.nl = n, nl
        self.c = row_consts(n, nl)
        self.rows = self.c["rows"]
        self.mul = RowMul(self.rows)
        pad = NQ * LANES
        self.np_limbs = limbs_of(self.c["np"], pad)
        self.n_limbs = limbs_of(n, pad)
        self.cin = limbs_of(self.c["cin"], pad)
        self.one = limbs_of(self.c["one"], pad)
        self.kp = self.c["kp"] + [0] * (pad - nl)
        self.Rp = 1 << (LIMB * self.rows)

    def entry(self, raw):
        """raw: nl words as the device buffer holds them -> the 48 limbs of 4 x (x R'), modulo N'"""
        a = list(raw) + [0] * (NQ * LANES - self.nl)
        out, digits = self.mul.mul(a, self.cin, self.np_limbs, r4=True)
        q = sum((d >> 4) << (LIMB * i) for i, d in enumerate(digits))
        want = value_of(raw) * self.c["cin"] + q * self.c["np"]
        assert want % self.Rp == 0 and signed_value(out, 4) == want // self.Rp
        assert all(x == 0 for x in out[self.rows:])
        return out

    def exit(self, p4):
        """the 48 limbs of 4 x value modulo N' -> the nl words the kernel writes back"""
        out, digits = self.mul.mul(p4, self.one, self.n_limbs, rho=self.c["rho"], a4=True)
        q = sum((d >> 4) << (LIMB * i) for i, d in enumerate(digits))
        want = signed_value(p4, 4) * self.c["one"] + q * self.n
        assert want % self.Rp == 0 and signed_value(out) == want // self.Rp
        assert all(x == 0 for x in out[self.rows:])
        t = signed_value(out)
        u = [(out[i] + self.kp[i]) & 0xffffffff for i in range(NQ * LANES)]
        words = []
        for i in range(self.nl):
            v = (u[i] & MASK) + (u[i - 1] >> LIMB if i else 0)
            if i == self.nl - 1:
                v += u[i] & ~MASK & 0xffffffff
            words.append(v)
        # limb nl of t is zero (|t| < 1.07 N < 2^(28 nl - 4)): the nl words hold t + K' exactly
        assert all(x == 0 for x in out[self.nl:]) and value_of(words) == t + value_of(self.c["kp"])
        return words, t

    def interp(self, a4, b4):
        """a multiply of the tape interpreter: operands and result times 4, modulo N'"""
        out, digits = self.mul.mul(a4, b4, self.np_limbs, a4=True, b4=True, r4=True)
        q = sum((d >> 4) << (LIMB * i) for i, d in enumerate(digits))
        want = signed_value(a4, 4) * signed_value(b4, 4) + q * self.c["np"]
        assert want % self.Rp == 0 and signed_value(out, 4) == want // self.Rp
        assert all(x == 0 for x in out[self.rows:])
        assert all(abs(x) <= 4 * PRODUCT_LIMB_MAX for x in out[:self.rows - 1])
        return out


# ---- operands as the tape interpreter makes them (times 4: the scale its multiplies read and deliver) ----
PRODUCT_LIMB_MAX = (1 << 27) + 4           # a multiply's result limbs below the top one, fer_mul's contract
OPERAND4_MAX = 4 * 2 * PRODUCT_LIMB_MAX    # a sum or a difference of two of them, times 4: 2^30 + 32


def balanced(v, rows):
    """the limbs of v in [-2^27, 2^27), the top one whatever is left; 48 limbs"""
    out = []
    for _ in range(rows - 1):
        d = ((v + (1 << 27)) & MASK) - (1 << 27)
        out.append(d)
        v = (v - d) >> LIMB
    return out + [v] + [0] * (NQ * LANES - rows)


def extreme_operand4(nprime, rows, sign, pattern):
    """times 4: limbs below the top one at +-(2^30 + 32) (pattern "same", "alternate" or a random.Random), the top limb
    the largest for which |value| stays inside 2.4 N' (tests/row_bias_model.extreme_operand at this layout's bound)"""
    lim = 24 * nprime // 10
    rows = min(rows, (lim.bit_length() - 1) // LIMB + 1)
    low = []
    for l in range(rows - 1):
        sg = sign if pattern == "same" else (sign if l % 2 == 0 else -sign) if pattern == "alternate" else pattern.choice((-1, 1))
        low.append(sg * (OPERAND4_MAX // 4))
    base = sum(x << (LIMB * i) for i, x in enumerate(low))
    w = LIMB * (rows - 1)
    top = (sign * lim - base) >> w if sign > 0 else -((lim + base) >> w)
    limbs = low + [top] + [0] * (NQ * LANES - rows)
    assert abs(signed_value(limbs)) <= lim and abs(top) <= OPERAND4_MAX // 4
    return [4 * x for x in limbs]


def random_operand4(rng, nprime, rows):
    """times 4: a sum or a difference of two balanced values of (-1.2 N', 1.2 N'), limb by limb"""
    lim = 12 * nprime // 10
    x, y = (balanced(rng.randrange(-lim, lim + 1), rows) for _ in range(2))
    sg = rng.choice((-1, 1))
    return [4 * (a + sg * b) for a, b in zip(x, y)]


def balanced_times4(v, rows):
    return [4 * x for x in balanced(v, rows)]
