"""The curve construction of the device build (csrc/gecm_kernels.hip: build_curve) restated in Python, operation for
operation, in the kernel's lazy Montgomery arithmetic, next to the plain Suyama values it must equal.
Shared by tests/test_build_cpu.py, which pins the algebra without a GPU, and tests/test_gpu_curve_build.py, whose directed
inputs get their expectation here."""
import json
import math
import os

LIMBS = [8, 10, 12, 14, 15, 17, 19, 21, 23, 26, 28, 30, 32, 34, 37]
LIMB_BITS = 28

Q415 = 0xba2e8ba2e8ba2e8ba2e8ba2e8ba2e8ba2e8ba2e8ba2e8ba2e8ba2e8ba2e8ba2e8ba2e8ba2e8ba2e8ba2e8ba2e8ba2e8ba1f46e3
N11Q = 11 * Q415                      # 415 bits: sigma = 15 has u = 0, sigma = 22 has v = 0 modulo 11
N40 = (1 << 39) + 23                  # below 2^64: sigma >= N happens
N65 = (1 << 64) + 13                  # 65 bits: 4 sigma and sigma^2 pass N, 8 limbs with R = 2^224
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage1.json")) as _f:
    N415 = int(next(c for c in json.load(_f) if c["name"] == "n415_b1_1000")["N"])       # the 415-bit bench number
SIGMA_EDGES = [6, 7, 2**32 - 1, 2**32, 2**32 + 1, 2**63, 2**64 - 1]


def is_probable_prime(n, bases=(2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)):
    if n < 2 or n % 2 == 0:
        return n == 2
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in bases:
        if a % n == 0:
            continue
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def pick_nl(nbits):
    need = (nbits + 5 + LIMB_BITS - 1) // LIMB_BITS        # R = 2^(28 nl) >= 32 N
    return next(nl for nl in LIMBS if nl >= need)


def suyama_plain(n, sigma):
    """(X, s, flag): plain residues of the curve the reference builds for sigma modulo n, with its stale operands where
    a denominator has no inverse (ecm.c:1745, 1759), and whether one had none"""
    u, v = sigma * sigma - 5, 4 * sigma
    x3, z3 = pow(u, 3, n), pow(v, 3, n)
    num = pow(v - u, 3, n) * ((3 * u + v) % n) % n
    den = 16 * x3 * v % n
    flag = 0
    if math.gcd(den, n) == 1:
        di = pow(den, -1, n)
    else:
        di, flag = 16 * x3 % n, 1
    if math.gcd(z3, n) == 1:
        zi = pow(z3, -1, n)
    else:
        zi, flag = num, 1
    return x3 * zi % n, num * di % n, flag


class KernelModel:
    """build_curve's sequence on Python integers: the same REDC (so the same lazy representatives), the same order, and
    the operand bounds of csrc/gecm_field.hpp asserted at every multiply"""

    def __init__(self, n, nl=None):
        self.n = n
        self.nl = nl or pick_nl(n.bit_length())
        self.R = 1 << (LIMB_BITS * self.nl)
        assert self.R >= 32 * n
        self.K = n << (LIMB_BITS * self.nl - 4 - n.bit_length())     # gecm_mod_make_kp: K in [R/32, R/16)
        assert self.R // 32 <= self.K < self.R // 16
        self.nprime = (-pow(n, -1, self.R)) % self.R
        self.one = self.R % n
        self.r2 = self.R * self.R % n
        self.r3 = self.r2 * self.R % n
        self.multiplies = 0

    def mul(self, a, b):
        # 0.6755, not 0.675: operands below 1.675 K reach products of 0.67535 K; the closed bound is 7 - sqrt(40) = 0.675445
        # (tests/field_model.py: PRODUCT_BOUND, fixed_point_case)
        assert 0 <= a and 10000 * a < 16755 * self.K, "operand above 1.6755 K"
        assert 0 <= b and 10000 * b < 16755 * self.K, "operand above 1.6755 K"
        t = a * b
        r = (t + (t * self.nprime % self.R) * self.n) // self.R
        assert 10000 * r < 6755 * self.K
        self.multiplies += 1
        return r

    def sub(self, a, b):
        assert b < self.R // 16                   # a subtrahend with normalised limbs: a product
        return a + self.K - b

    def canon(self, a):
        r = self.mul(a, self.one)
        assert r < 2 * self.n
        return r - self.n if r >= self.n else r

    def invert(self, a):
        """build_invert: the Montgomery form of the inverse of the Montgomery-form a, or None"""
        c = self.canon(a)
        if math.gcd(c, self.n) != 1:
            return None
        return self.mul(pow(c, -1, self.n), self.r3)

    def build(self, sigma):
        """(X, Z, S, flag) as the kernel stores them: canonical, Montgomery form"""
        assert 0 <= sigma < 1 << 64
        m, r2 = self.mul, self.r2
        w = m(sigma, r2)
        v = m(w, m(4, r2))
        u = self.sub(m(w, w), m(5, r2))
        u = m(u, self.one)
        x3 = m(m(u, u), u)
        d16 = m(x3, m(16, r2))
        den = m(d16, v)
        z3 = m(m(v, v), v)
        t = m(m(3, r2), u) + v
        w = self.sub(v, u)
        num = m(m(m(w, w), w), t)
        flag = 0
        inv = self.invert(m(den, z3))
        if inv is not None:
            di, zi = m(inv, z3), m(inv, den)
        else:
            di, zi = self.invert(den), self.invert(z3)
            if di is None:
                di, flag = d16, 1
            if zi is None:
                zi, flag = num, 1
        return self.canon(m(x3, zi)), self.one, self.canon(m(num, di)), flag
