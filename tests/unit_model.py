"""P-1 and P+1 stage 1 on the PRAC tape in Python: the values a method batch must hold (pow, and a binary
Lucas ladder for V_k), the tape interpreter of csrc/gecm_curve.hpp (run_tape_unit) over any add / dup, and the device
sequence restated in the kernel's lazy Montgomery arithmetic over tests/suyama_model.py's KernelModel with the operand
bounds asserted.  Shared by tests/test_unit_cpu.py and the GPU tests."""
import ctypes
import math
import random

from suyama_model import LIMB_BITS, LIMBS, KernelModel
from xladder import _primes, stage1_multiplier

METHOD_PM1, METHOD_PP1 = 1, 2
METHOD_NAME = {METHOD_PM1: "P-1", METHOD_PP1: "P+1"}
OFFSET = {METHOD_PM1: 1, METHOD_PP1: 2}                # the factor test is gcd(x - OFFSET, N)

# csrc/gecm_tape.h
OP_NOP, OP_PRAC_BEGIN, OP_PRAC_END, OP_STEP, OP_SWAP, OP_RULE_MASK = 0, 1, 2, 8, 4, 3
RULE3, RULE4, RULE5, RULE9 = 0, 1, 2, 3

UNIT_LIMBS = [8, 15, 23, 26, 37]                       # 25 -> 26 limbs is where LazyPolicy::norm_sub switches on
SEGMENTS = [(1, 1000), (1000, 3000), (108222, 108223), (235536, 235537)]
RULE9_SEGMENT = (235536, 235537)                       # one prime: 25 events, all four rules and the swap


class Tape(ctypes.Structure):
    _fields_ = [("ops", ctypes.POINTER(ctypes.c_uint8)), ("len", ctypes.c_size_t), ("ptadds", ctypes.c_uint64),
                ("ptdups", ctypes.c_uint64), ("prac_calls", ctypes.c_uint64), ("last_prime", ctypes.c_uint64),
                ("rule_count", ctypes.c_uint64 * 4), ("swaps", ctypes.c_uint64)]


_TAPES = {}


def extend_tape(lib, lo, hi):
    """(ops, rule_count, swaps) of the extension segment (lo, hi] as host/gecm_plan.c compiles it"""
    if (lo, hi) not in _TAPES:
        lib.gecm_tape_build_extend.argtypes = [ctypes.POINTER(Tape), ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int]
        lib.gecm_tape_free.argtypes = [ctypes.POINTER(Tape)]
        lib.gecm_tape_free.restype = None
        t = Tape()
        assert lib.gecm_tape_build_extend(ctypes.byref(t), lo, hi, 1) == 0
        _TAPES[(lo, hi)] = (bytes(t.ops[:t.len]), list(t.rule_count), t.swaps)
        lib.gecm_tape_free(ctypes.byref(t))
    return _TAPES[(lo, hi)]


def k_std(b):
    return stage1_multiplier(b + 1)


def exponent(lo, hi):
    """E of an extension from lo to hi"""
    q, r = divmod(k_std(hi), k_std(lo))
    assert r == 0
    return q


def lucas_v(x, k, n):
    """V_k(x) mod n by the binary ladder on (V_m, V_{m+1}): V_0 = 2, V_1 = x, V_{2m} = V_m^2 - 2,
    V_{2m+1} = V_m V_{m+1} - x"""
    if k == 0:
        return 2 % n
    a, b = x % n, (x * x - 2) % n
    for bit in bin(k)[3:]:
        if bit == "1":
            a, b = (a * b - x) % n, (b * b - 2) % n
        else:
            a, b = (a * a - 2) % n, (a * b - x) % n
    return a


_EXPECTED = {}


def expected(method, x, e, n):
    """the residue of a method batch: x^e or V_e(x) modulo n"""
    key = (method, x, e, n)
    if key not in _EXPECTED:
        _EXPECTED[key] = pow(x, e, n) if method == METHOD_PM1 else lucas_v(x, e, n)
    return _EXPECTED[key]


def method_line(method, b1, n, x, x0=None):
    """the standard line of a P-1 / P+1 residue"""
    seed = "" if x0 is None else "X0=0x%x; " % x0
    return "METHOD=%s; B1=%d; N=0x%x; X=0x%x; %sPROGRAM=AVX-ECM-STD;\n" % (METHOD_NAME[method], b1, n, x, seed)


def run_unit_tape(ops, x, add, dup):
    """run_tape_unit: the tape on one residue, with the register renamings of run_tape (BEGIN, END, swap, rules 3/4/5/9).
    add(X, Y, W) is the addition with difference W, dup(X) the doubling."""
    A = B = C = x
    for op in ops:
        if op == OP_NOP:
            continue
        if op == OP_PRAC_BEGIN:
            B = C = A
            A = dup(A)
            continue
        if op == OP_PRAC_END:
            A = add(B, A, C)
            continue
        assert op >= OP_STEP
        if op & OP_SWAP:
            A, B = B, A
        rule = op & OP_RULE_MASK
        if rule == RULE3:                         # T = B + A (C); (B, C) <- (T, B)
            B, C = add(B, A, C), B
        elif rule == RULE4:                       # B = B + A (C); A = 2A
            B, A = add(B, A, C), dup(A)
        elif rule == RULE5:                       # C = C + A (B); A = 2A
            C, A = add(C, A, B), dup(A)
        else:                                     # rule 9: C = C + B (A); B = 2B
            C, B = add(C, B, A), dup(B)
    return A


def plain_unit(ops, x, method, n):
    """the tape in plain integers modulo n"""
    if method == METHOD_PM1:
        return run_unit_tape(ops, x % n, lambda X, Y, W: X * Y % n, lambda X: X * X % n)
    return run_unit_tape(ops, x % n, lambda X, Y, W: (X * Y - W) % n, lambda X: (X * X - 2) % n)


class UnitModel(KernelModel):
    """k_unit's sequence: every multiply through KernelModel.mul (operands below 1.675 K, product below 0.675 K), every
    subtraction through sub_full, which is fe_sub_full limb by limb in 32-bit words: the subtrahend normalised and below
    K, the result normalised and below K"""

    def __init__(self, n, nl):
        KernelModel.__init__(self, n, nl)
        mask = (1 << LIMB_BITS) - 1
        kl = [(self.K >> (LIMB_BITS * i)) & mask for i in range(nl)]
        # gecm_mod_make_kp: + 2^28 at limb 0, + 2^28 - 1 in the middle, - 1 at the top
        self.kp = [kl[i] + (1 << LIMB_BITS) if i == 0 else kl[i] + mask if i < nl - 1 else kl[i] - 1 for i in range(nl)]
        assert sum(v << (LIMB_BITS * i) for i, v in enumerate(self.kp)) == self.K
        self.subtractions = 0

    def limbs(self, v):
        mask = (1 << LIMB_BITS) - 1
        assert 0 <= v < 1 << (LIMB_BITS * self.nl)
        return [(v >> (LIMB_BITS * i)) & mask for i in range(self.nl)]

    def sub_full(self, a, b):
        assert 0 <= b < self.K, "subtrahend not below K"
        assert 0 <= a < self.K
        al, bl = self.limbs(a), self.limbs(b)             # normalised limbs: both are values of a multiply or of this
        mask, top = (1 << LIMB_BITS) - 1, self.nl - 1
        p, q, cp, cq = [], [], 0, 0
        for i in range(self.nl):
            u = al[i] + self.kp[i] - bl[i] + cp
            s = al[i] - bl[i] + cq
            assert 0 <= u < 1 << 32 and -(1 << 31) <= s < 1 << 31
            p.append(u if i == top else u & mask)
            q.append(s if i == top else s & mask)
            cp, cq = u >> LIMB_BITS, s >> LIMB_BITS       # s >> 28 is arithmetic: 0 or -1
        r = p if q[top] < 0 else q
        assert all(0 <= v <= mask for v in r), "limbs not normalised"
        v = sum(w << (LIMB_BITS * i) for i, w in enumerate(r))
        assert v == (a - b if a >= b else a - b + self.K) and v < self.K
        self.subtractions += 1
        return v

    def two(self):
        t = 2 * self.one                                  # unit_const: carry pass, one conditional subtraction of N
        return t - self.n if t >= self.n else t

    def unit(self, ops, x, method):
        """the plain residue the kernel's output stands for, x the plain canonical input"""
        assert 0 <= x < self.n
        X = self.mul(x, self.r2)                          # k_to_mont
        X = X - self.n if X >= self.n else X
        if method == METHOD_PM1:
            A = run_unit_tape(ops, X, lambda P, Q, W: self.mul(P, Q), lambda P: self.mul(P, P))
        else:
            two = self.two()
            A = run_unit_tape(ops, X, lambda P, Q, W: self.sub_full(self.mul(P, Q), W),
                              lambda P: self.sub_full(self.mul(P, P), two))
        out = self.canon(A)
        assert 0 <= out < self.n, "output not canonical"
        return out * pow(self.R, -1, self.n) % self.n


_SMALL = None


def random_modulus(bits, rng):
    """random, odd, exactly `bits` bits, no factor below 2^20"""
    global _SMALL
    if _SMALL is None:
        _SMALL = _primes(1 << 20)
    while True:
        n = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
        if all(n % p for p in _SMALL):
            return n


def class_bits(nl):
    """(top, bottom) bit sizes of the limb class nl: 28 nl - 5 bits, and one more than the class below holds"""
    below = LIMBS[LIMBS.index(nl) - 1] if LIMBS.index(nl) else None
    return LIMB_BITS * nl - 5, (LIMB_BITS * below - 5 + 1) if below else 64


_MODULI = {}


def class_moduli(nl):
    """[top, bottom]: one modulus at each end of the class, the same in every test"""
    if nl not in _MODULI:
        rng = random.Random(2000 + nl)
        _MODULI[nl] = [random_modulus(b, rng) for b in class_bits(nl)]
    return _MODULI[nl]


def seeds_for(n, count, rng):
    """2, 3, N - 1, N - 2, 2/7 mod N, then random ones: `count` seeds"""
    fixed = [2, 3, n - 1, n - 2, 2 * pow(7, -1, n) % n]
    return (fixed + [rng.randrange(n) for _ in range(max(0, count - len(fixed)))])[:count]


def smooth_prime(bits, bound, sign, rng):
    """a prime p of about `bits` bits with p + sign = 2 times distinct odd primes below `bound`: a divisor of k_std(bound)"""
    small = [q for q in _primes(bound) if q > 2]
    from suyama_model import is_probable_prime
    while True:
        m = 2
        for q in rng.sample(small, len(small)):
            if m.bit_length() >= bits:
                break
            m *= q
        p = m - sign
        if is_probable_prime(p):
            return p


def is_smooth(m, bound):
    for q in _primes(bound):
        while m % q == 0:
            m //= q
    return m == 1


def factor_case(method, rng):
    """N = p q for the factor tests: P-1: p - 1 is 1000-smooth and q - 1 is not; P+1: p + 1 is 1000-smooth, q -+ 1 are
    not.  q is a random prime.  Returns (n, p, q)."""
    from suyama_model import is_probable_prime
    p = smooth_prime(90, 1000, -1 if method == METHOD_PM1 else +1, rng)
    assert k_std(1000) % (p - 1 if method == METHOD_PM1 else p + 1) == 0
    while True:
        q = rng.getrandbits(100) | (1 << 99) | 1
        if is_probable_prime(q) and not is_smooth(q - 1, 1000) and not is_smooth(q + 1, 1000):
            return p * q, p, q


def jacobi(a, n):
    a %= n
    r = 1
    while a:
        while a % 2 == 0:
            a //= 2
            if n % 8 in (3, 5):
                r = -r
        a, n = n, a
        if a % 4 == 3 and n % 4 == 3:
            r = -r
        a %= n
    return r if n == 1 else 0


def py_gcd_flag(method, x, n):
    """(gcd, flag) of the factor test on the residue x"""
    g = math.gcd((x - OFFSET[method]) % n, n)
    return g, 1 if 1 < g < n else 0
