"""The multiply of the 32-lane stage-1 kernel at one limb per lane (fer_mul of avx-ecm_amd/csrc/gecm_row.hpp, NQ = 1, rho = 1,
operands and result times 4) on Python integers, register by register: sixteen lanes, one signed 64-bit accumulator each,
the row loop as the kernel runs it, and the end of the multiply in two forms:

  old   u16 = T + 2^31 (a 64-bit add); limb x 4 = (T.lo read as signed) >> 2; carry = u16.hi; the carry of the lane below
        comes by row_shr:1 (lane 0: 0) and enters times 4
  new   the hand-over into the last row adds K = 2^27 to the accumulator's high word, the last hand-over adds Z = -2^27 to
        the high word of what it leaves: T' = T + 2^31 - 2^59.  limb x 4 + 2^29 = T'.lo >> 2 (unsigned), T'.hi = carry - 2^27
        comes by row_ror:1 (lane 0: from lane 15) and enters times 4, which takes the 2^29 away.

Every register write is checked against its width: an accumulator that leaves the signed 64-bit range, or a high word that
leaves the signed 32-bit range where a multiply-add reads it as an operand, is recorded in Result.overflow."""
import random

LIMB = 28
LANES = 16
M28 = (1 << LIMB) - 1
K = 1 << 27
Z = -(1 << 27)
NQ1_LIMBS = (8, 10, 12, 14, 15)         # the built limb counts with one limb per lane: 9, 11, 13, 15 and 16 rows
OPERAND_LIMB_MAX = (1 << 29) - 1        # fer_mul's bound on an operand limb (before the times 4)


def i32(x):
    x &= 0xffffffff
    return x - ((x & 0x80000000) << 1)


def row_multiple(n):
    """N' = m N = -1 mod 2^28, the modulus of the row kernel"""
    return ((-pow(n, -1, 1 << LIMB)) % (1 << LIMB)) * n


def limbs_unsigned(v, cnt=LANES):
    assert 0 <= v < 1 << (LIMB * cnt)
    return [(v >> (LIMB * i)) & M28 for i in range(cnt)]


def balanced(v, rows):
    """the limbs of v (any sign) as a multiply leaves them: [-2^27, 2^27) below the top one, the top one what is left"""
    out = []
    for _ in range(rows - 1):
        d = ((v + (1 << 27)) & M28) - (1 << 27)
        out.append(d)
        v = (v - d) >> LIMB
    return out + [v] + [0] * (LANES - rows)


def value(limbs):
    return sum(d << (LIMB * i) for i, d in enumerate(limbs))


class Result:
    def __init__(self, limbs4, top_carry, overflow):
        self.limbs4 = limbs4            # 4 x limb per lane, as the 32-bit register holds it (signed)
        self.top_carry = top_carry      # what leaves lane 15 (old: u16.hi; new: T'.hi + 2^27)
        self.overflow = overflow        # [(row, lane, what)]


def fer_mul4(a4, b4, nprime, rows, new):
    """a4, b4: sixteen signed 32-bit values per operand (4 x limb; zero from `rows` up); nprime: N' (its limbs from `rows`
    up are zero)"""
    assert len(a4) == len(b4) == LANES and 2 <= rows <= LANES
    assert all(-(1 << 31) <= x < 1 << 31 for x in a4 + b4)
    n = limbs_unsigned(nprime)
    assert n[0] == M28 and not any(n[rows:]) and not any(a4[rows:]) and not any(b4[rows:])
    bad = []

    def chk64(x, row, lane, what):
        if not -(1 << 63) <= x < 1 << 63:
            bad.append((row, lane, what))
        return x

    T = [chk64(a4[0] * b4[l], 0, l, "first product") for l in range(LANES)]
    for i in range(rows):
        q = T[0] & 0xffffffff                                                   # row_newbcast:0 of the low register
        T = [chk64(T[l] + q * n[l], i, l, "digit product") for l in range(LANES)]     # v_mad_u64_u32
        assert T[0] & 0xffffffff == 0
        lo = [T[l + 1] & 0xffffffff for l in range(LANES - 1)] + [0]            # row_shl:1, bound_ctrl
        h = 0
        if new and i + 2 == rows:
            h = K
        if new and i + 1 == rows:
            h = Z
        nxt = []
        for l in range(LANES):
            hi = T[l] >> 32
            if not -(1 << 31) <= hi < 1 << 31:
                bad.append((i, l, "high word as an operand"))
            t = chk64(16 * hi + ((h << 32) + lo[l]), i, l, "hand-over")         # v_mad_i64_i32 hi, 16, {lo, h}
            if i + 1 < rows:
                t = chk64(t + a4[i + 1] * b4[l], i, l, "next product")
            nxt.append(t)
        T = nxt
    out = []
    if new:
        his = [i32(t >> 32) for t in T]
        for l in range(LANES):
            out.append(i32(((T[l] & 0xffffffff) >> 2) + (his[(l - 1) % LANES] << 2)))       # row_ror:1
        top = his[LANES - 1] - Z
    else:
        u16 = [chk64(t + (1 << 31), rows, l, "rounding add") for l, t in enumerate(T)]
        car = [i32(u >> 32) for u in u16]
        for l in range(LANES):
            out.append(i32((i32(T[l]) >> 2) + ((car[l - 1] if l else 0) << 2)))              # row_shr:1, bound_ctrl
        top = car[LANES - 1]
    return Result(out, top, bad)


# ---- operands ------------------------------------------------------------------------------------------------------
def class_moduli(nl):
    """[(name, N)]: moduli at both ends of the limb class nl, by length and by what their multiple N' looks like"""
    import divsteps_model as M
    i = M.BUILT.index(nl)
    lo_bits = LIMB * (M.BUILT[i - 1] if i else 7) - 4
    hi_bits = LIMB * nl - 5
    out = [("bottom, random", M.modulus(lo_bits, "random")), ("top, random", M.modulus(hi_bits, "random")),
           ("top, 2^k-1", (1 << hi_bits) - 1)]
    if i == 0:
        out.append(("64 bits", M.modulus(64, "random")))
    # N = 1 mod 2^28: m = 2^28 - 1, N' as long as the class allows and nearly every limb 2^28 - 1
    m = (1 << LIMB) - 1
    n = ((1 << (hi_bits + LIMB)) - 1) // m
    n -= (n - 1) % (1 << LIMB)
    if n.bit_length() == hi_bits:
        out.append(("top, full limbs", n))
    # N = -1 mod 2^28: m = 1, N' = N, limbs 1 .. nl - 2 zero
    out.append(("top, zero limbs", (1 << (hi_bits - 1)) + (1 << LIMB) - 1))
    for _, n in out:
        assert n & 1 and M.dev_limbs(n.bit_length()) == nl
    return out


def extreme_operand(nprime, rows, sign, pattern):
    """limbs below the top one at +-(2^29 - 1) (pattern: "same", "alternate" or a random.Random), the top limb the largest
    for which |value| stays inside 2.4 N': what the point formulas feed to a multiply is a sum or a difference of two
    values of (-1.2 N', 1.2 N').  (The top one: the highest limb that 2.4 N' reaches, limb rows - 1 unless N' is short for
    its class; the limbs above it are zero.)"""
    lim = 24 * nprime // 10
    rows = min(rows, (lim.bit_length() - 1) // LIMB + 1)
    low = []
    for l in range(rows - 1):
        s = sign if pattern == "same" else (sign if l % 2 == 0 else -sign) if pattern == "alternate" else pattern.choice((-1, 1))
        low.append(s * OPERAND_LIMB_MAX)
    base = value(low)
    w = LIMB * (rows - 1)
    top = (sign * lim - base) >> w if sign > 0 else -((lim + base) >> w)
    limbs = low + [top] + [0] * (LANES - rows)
    assert abs(value(limbs)) <= lim and abs(top) <= OPERAND_LIMB_MAX
    return limbs


def random_operand(rng, nprime, rows):
    """a sum or difference of two balanced values of (-1.2 N', 1.2 N'), limb by limb, as row_sd / row_ds make it"""
    lim = 12 * nprime // 10
    x, y = (balanced(rng.randrange(-lim, lim + 1), rows) for _ in range(2))
    s = rng.choice((-1, 1))
    return [a + s * b for a, b in zip(x, y)]


def operand_pairs(nprime, rows, seed, count):
    rng = random.Random(seed)
    ex = [extreme_operand(nprime, rows, s, p) for s in (1, -1) for p in ("same", "alternate", rng)]
    pairs = [(a, b) for a in ex for b in ex]
    rnd = [random_operand(rng, nprime, rows) for _ in range(count)]
    pairs += [(rng.choice(ex), r) for r in rnd[:count // 2]] + [(r, rng.choice(ex)) for r in rnd[:count // 4]]
    pairs += [(rnd[i], rnd[(i * 7 + 3) % count]) for i in range(count)]
    pairs += [(r, r) for r in rnd[:count // 2]]                    # squares
    zero = [0] * LANES
    one = [1] + [0] * (LANES - 1)
    pairs += [(zero, ex[0]), (ex[1], zero), (one, ex[0]), (one, one)]
    return pairs
