"""P-1 and P+1 stage 2 in Python: the accumulator a method batch must hold after a stage 2, in exact
integers, and the device sequence (csrc/gecm_stage2.hpp: s2u_seed, s2u_init, s2u_gen and one step of s2_pairs) restated
over tests/unit_model.py's UnitModel with the operand bounds asserted.  Shared by tests/test_unit_s2_cpu.py and the GPU
tests."""
import math

from suyama_model import LIMB_BITS, is_probable_prime
from unit_model import METHOD_PM1, METHOD_PP1, UnitModel, lucas_v
from xladder import _primes

S2_CHUNK, S2_RING = 512, 1024                          # host/gecm_api.c: S2_GIANT_CHUNK, S2_RING
GEN = 0xffffffff
MASK = (1 << LIMB_BITS) - 1


# ---- the plan and the pair map (host/gecm_pair.c) ----
def plan_map(D, U):
    """gecm_s2_plan_init: j -> table index for j in [0, U D], 0 = not stored"""
    m = [0] * (U * (D + 1) + 3)
    m[1], m[2], nxt = 1, 2, 3
    for blk in range(U):
        for j in range(1 if blk else 3, (D - 1 if blk else D) + 1):
            if math.gcd(j, D) == 1 or (blk == 0 and j == D):
                m[blk * D + j] = nxt
                nxt += 1
    return m, nxt


def map_lists(pairs):
    """(v, u, amin) of a pyecm.Pairs as Python lists"""
    return list(pairs.pairmap_v[:pairs.steps]), list(pairs.pairmap_u[:pairs.steps]), pairs.amin


def walk(v, u, amin, U):
    """the entries of a pair map as (a, u, valid): the factor is V_{a D} - V_u with a = run_amin + v; valid is
    gecm_s2_tape_build's own rule for the entry (without the table lookup)"""
    run = amin
    for vv, uu in zip(v, u):
        if vv == 0 and uu == 0:
            run += U
            continue
        yield run + vv, uu, vv >= run and vv - run < 4 * U


def shifts_of(v, u):
    return sum(1 for vv, uu in zip(v, u) if vv == 0 and uu == 0)


def tape(v, u, amin, D, U, chunk=S2_CHUNK, ring=S2_RING):
    """gecm_s2_tape_build: [(GEN, n)] marks and (ring slot, j) pairs in the order of the map (the device sorts the pairs
    between two marks by slot; a product does not care).  j is the table's j, not map[j]."""
    L = 2 * U
    E = 2 * L + 2 * U * shifts_of(v, u)
    g0 = E - 2 * U if shifts_of(v, u) else 0
    out, generated, run, base = [], 0, amin, 2 * amin

    def need(upto):
        nonlocal generated
        while generated < upto:
            lim = g0 if generated < g0 else E
            n = min(lim - generated, chunk)
            out.append((GEN, n))
            generated += n
    need(2 * L)
    for vv, uu in zip(v, u):
        if vv == 0 and uu == 0:
            run += U
            need(2 * run - base + 2 * L)
        else:
            out.append(((2 * run - base + (vv - run)) & (ring - 1), uu))
    return out, E


# ---- exact integers ----
def method_p(method, x, n):
    """P with V_k(P) = x^k + x^-k: x itself for P+1, x + 1/x for P-1 (None where x has no inverse)"""
    if method == METHOD_PP1:
        return x % n
    if math.gcd(x, n) != 1:
        return None
    return (x + pow(x, -1, n)) % n


def plain_acc(method, x, n, maps, D, U):
    """the accumulator of a position whose stage-1 residue is x, after the maps [(v, u, amin), ..]: the product of
    V_{a D}(P) - V_u(P) over their entries, a plain residue"""
    P = method_p(method, x, n)
    vt = [2 % n, P]
    for j in range(2, U * D + 1):
        vt.append((vt[-1] * P - vt[-2]) % n)
    vd, giant, acc = vt[D], {}, 1
    for v, u, amin in maps:
        for a, uu, _ in walk(v, u, amin, U):
            if a not in giant:
                if a - 1 in giant and a - 2 in giant:
                    giant[a] = (giant[a - 1] * vd - giant[a - 2]) % n
                else:
                    giant[a] = lucas_v(vd, a, n)
            acc = acc * (giant[a] - vt[uu]) % n
    return acc


def to_ref(acc, n, maxbits):
    """what gecm_download_acc / gecm_curve_acc return for the plain accumulator: the reference's Montgomery radix"""
    return acc * pow(2, maxbits, n) % n


# ---- planted factors ----
def planted_prime(method, b1, b2, bits, rng, a, b=1):
    """(p, q): a prime p with p - 1 (P-1) or p + 1 (P+1) = (a b1-smooth number) * q, q one prime in (b1, b2), such that
    stage 1 to b1 from the seed a / b misses p and stage 2 to b2 finds it: for P+1 jacobi(s^2 - 4, p) = -1 for the seed's
    residue s modulo p, so that the order of its x divides p + 1, and for both methods that order keeps q"""
    from unit_model import expected, exponent, jacobi
    small = [s for s in _primes(b1) if s > 2]
    big = [s for s in _primes(b2) if s > b1]
    sign = -1 if method == METHOD_PM1 else +1
    while True:
        q = rng.choice(big)
        m = 2 * q
        for s in rng.sample(small, len(small)):
            if m.bit_length() >= bits:
                break
            m *= s
        p = m - sign
        if not is_probable_prime(p) or a % p == 0 or b % p == 0:
            continue
        s = a * pow(b, -1, p) % p
        if method == METHOD_PP1 and jacobi(s * s - 4, p) != -1:
            continue
        if expected(method, s, exponent(1, b1), p) == (1 if method == METHOD_PM1 else 2):
            continue                                   # the seed's order lost q: stage 1 would find p
        return p, q


# ---- the device sequence, with its bounds ----
class S2Model(UnitModel):
    """s2u_seed, s2u_init, s2u_gen and the step of s2_pairs on Python integers.  Every multiply of the three builders goes
    through KernelModel.mul (operands below 1.675 K, product below 0.675 K), every subtraction through
    UnitModel.sub_full (subtrahend normalised and below K, words inside 32 bits, result normalised and below K).  The
    pair step has its own statement: its second operand t = x + K' - y is below 2 K, not 1.675 K."""

    def to_mont(self, x):
        X = self.mul(x, self.r2)                          # k_to_mont, then k_unit's canonical store
        return X - self.n if X >= self.n else X

    def inv_mont(self, a):
        """fe_inv_mont: (x^-1 R as a product, None) or (0, gcd)"""
        c = self.canon(a)
        g = math.gcd(c, self.n)
        if g != 1:
            return 0, g
        return self.mul(pow(c, -1, self.n), self.r3), None

    def seed(self, X, method):
        """(P in canonical Montgomery form, failure record or None)"""
        assert 0 <= X < self.n
        fail = None
        if method == METHOD_PM1:
            inv, fail = self.inv_mont(X)
            xl, il = self.limbs(X), self.limbs(inv)       # both normalised: fe_add's limbs stay below 2^29
            assert all(a + b < 1 << 29 for a, b in zip(xl, il))
            X = X + inv
        P = self.canon(X)
        assert 0 <= P < self.n, "P not canonical"
        return P, fail

    def step(self, a, b, c):
        return self.sub_full(self.mul(a, b), c)

    def ladder(self, Q, k):
        """lucas_ladder: (V_k(Q), V_{k+1}(Q))"""
        two = self.two()
        a, b = two, Q
        if k == 0:
            return a, b
        for bit in bin(k)[2:]:
            t = self.step(a, b, Q)
            s = b if bit == "1" else a
            s = self.sub_full(self.mul(s, s), two)
            a, b = (t, s) if bit == "1" else (s, t)
        return a, b

    def init(self, P, K, D, U):
        """s2u_init for every sub-sequence r: ({j: V_j} for the kept j, V_D, V_{K D} or None)"""
        pmap, _ = plan_map(D, U)
        two, umax, table = self.two(), U * D, {}
        for r in range(K):
            c0, c1, p1, p2, i = two, P, P, two, 1
            while True:
                if i == r:
                    p1 = c1
                if i == K - r:
                    p2 = c1
                if i == K:
                    break
                c0, c1 = c1, self.step(c1, P, c0)
                i += 1
            vk = c1
            if r == 0:
                p1, p2 = vk, two
            j = r if r else K
            while j <= umax:
                if pmap[j]:
                    assert j not in table
                    table[j] = self.canon(p1)             # the walk's subtrahend: canonical (see pair)
                p1, p2 = self.step(p1, vk, p2), p1
                j += K
        assert sorted(table) == [j for j in range(umax + 1) if pmap[j]]
        vd = self.ladder(P, D)[0]
        vkd = self.ladder(vd, K)[0] if K > 1 else None
        return table, vd, vkd

    def gen(self, ring, state, vd, vkd, K, base, first_abs, n, ring_size=S2_RING):
        """s2u_gen for every sub-sequence r: giant steps [first_abs, first_abs + n) into ring (slot -> value); state[r] =
        (next member, the one before), the scratch entries 1 and 0"""
        step = vkd if K > 1 else vd
        for r in range(K):
            s0 = first_abs + (r + K - first_abs % K) % K
            if s0 >= first_abs + n:
                continue
            cnt = (first_abs + n - 1 - s0) // K + 1
            if s0 < K:
                p1 = self.ladder(vd, abs(base + s0))[0]
                p2 = self.ladder(vd, abs(base + s0 - K))[0]
            else:
                p1, p2 = state[r]
            for j in range(cnt):
                ring[(s0 + j * K) & (ring_size - 1)] = p1
                p1, p2 = self.step(p1, step, p2), p1
            state[r] = (p1, p2)

    def pair(self, acc, x, y):
        """one step of s2_pairs: acc <- acc (x - y) / R with x a ring entry, y a table entry"""
        K = self.K
        # the minuend as the chain leaves it, the subtrahend canonical: fe_sub has no carry, and K' has K's top limb less
        # one, so a subtrahend K - (something small) would leave the top word of t at -1
        assert 0 <= x < K, "ring entry not below K"
        assert 0 <= y < self.n, "table entry not canonical"
        xl, yl = self.limbs(x), self.limbs(y)             # normalised: limbs() asserts the value fits NL limbs
        t = [a + k - b for a, k, b in zip(xl, self.kp, yl)]
        assert all(0 <= w < 3 << LIMB_BITS for w in t), "fe_sub word outside [0, 3 2^28)"
        if self.nl > 25:                                  # LazyPolicy::norm_sub: fe_weak_norm
            o = [t[0] & MASK] + [(t[i] & MASK) + (t[i - 1] >> LIMB_BITS) for i in range(1, self.nl - 1)]
            o.append(t[-1] + (t[-2] >> LIMB_BITS))
            assert all(w < (1 << LIMB_BITS) + 4 for w in o[:-1]) and o[-1] < 1 << 32
            assert sum(w << (LIMB_BITS * i) for i, w in enumerate(o)) == sum(w << (LIMB_BITS * i) for i, w in enumerate(t))
            t = o
        # the 64-bit column accumulator of fe_mul: NL products of a limb of acc and a limb of t, NL of a digit and a limb of N
        assert self.nl * (MASK * max(t) + MASK * MASK) < 1 << 64
        tv = x + K - y
        assert tv == sum(w << (LIMB_BITS * i) for i, w in enumerate(t)) and tv < 2 * K
        assert 0 <= acc and 1000 * acc < 675 * K, "accumulator above 0.675 K"
        p = acc * tv
        r = (p + (p * self.nprime % self.R) * self.n) // self.R
        assert 1000 * r < 675 * K, "pair product above 0.675 K"
        self.multiplies += 1
        return r

    def stage2(self, x, method, maps, D, U, K=1, chunk=S2_CHUNK, ring_size=S2_RING):
        """(the plain accumulator the device's output stands for, failure record): x the plain stage-1 residue"""
        X = self.to_mont(x)
        P, fail = self.seed(X, method)
        table, vd, vkd = self.init(P, K, D, U)
        acc = self.one
        for v, u, amin in maps:
            ring, state = {}, {}
            words, _ = tape(v, u, amin, D, U, chunk, ring_size)
            generated = 0
            for w0, w1 in words:
                if w0 == GEN:
                    self.gen(ring, state, vd, vkd, K, 2 * amin, generated, w1, ring_size)
                    generated += w1
                else:
                    acc = self.pair(acc, ring[w0], table[w1])
        out = self.canon(acc)
        assert 0 <= out < self.n, "accumulator not canonical"
        return out * pow(self.R, -1, self.n) % self.n, fail


# ---- what the GPU tests run: every (B1, B2, D, U) whose pair map one of them walks ----
CLASSES = (200, 20000, 210, 2)                         # B1 < D: amin = 0, the first ring entry is V_0
WRAP = (3000, 250000, 210, 4)                          # more than two chunks of giant steps, a wrapped ring
PHASE_MID = 6000
PHASE = [(200, PHASE_MID, 210, 2), (PHASE_MID, 20000, 210, 2)]
OTHER_DU = (200, 20000, 385, 4)
CLI = (1000, 30000, 385, 16)                           # the driver's D and U for B1 = 1000
GPU_CASES = [CLASSES, WRAP, OTHER_DU, CLI] + PHASE

_MAPS = {}


def pair_map(pyecm, case):
    """(v, u, amin) of pyecm.pair_primes for a case, computed once"""
    if case not in _MAPS:
        p = pyecm.pair_primes(*case)
        _MAPS[case] = map_lists(p)
        pyecm.lib.gecm_pairmap_release(p)
    return _MAPS[case]


def maxbits(n, digitbits=52):
    """MAXBITS of the reference for n: its Montgomery radix is 2^MAXBITS"""
    step = 208 if digitbits == 52 else 128
    return step * (n.bit_length() // step + 1)


_FACTOR = {}


def planted_case(method, b1, b2, frac=None):
    """(N, p, r, seed) for the factor tests: N = p r, stage 1 to b1 from `seed` finds nothing, stage 2 to b2 finds p; r a
    random prime of 100 bits.  The seed is 3 (P-1) or 5 (P+1), or with frac = (a, b) the residue a / b mod N, as the
    command line makes its own.  The same in every test."""
    import random
    key = (method, b1, b2, frac)
    if key not in _FACTOR:
        a, b = frac or ((3, 1) if method == METHOD_PM1 else (5, 1))
        rng = random.Random(7000 + method + 10 * a + b)
        p, _ = planted_prime(method, b1, b2, 80, rng, a, b)
        while True:
            r = rng.getrandbits(100) | (1 << 99) | 1
            if is_probable_prime(r):
                break
        _FACTOR[key] = (p * r, p, r, a * pow(b, -1, p * r) % (p * r))
    return _FACTOR[key]
