"""P-1 and P+1 stage 1 with a residue per 16-lane DPP row in Python integers: the constants
host/gecm_api.c makes (row_consts), and k_unit_row's sequence of csrc/gecm_row.hpp with signed limbs as the kernel holds
them: the entry multiply, the tape events with fer_mul's contract as the multiply, the subtraction and its reduction limb
by limb in 32-bit words, the carry pass and the exit.  Every bound DESIGN.md §22 claims is asserted where it is used.
Shared by tests/test_unit_row_cpu.py and the GPU tests."""
import numpy as np

from suyama_model import LIMB_BITS
from unit_model import METHOD_PM1, UnitModel, run_unit_tape

ROW_LIMBS = [8, 15, 17, 30, 32, 37]                    # shapes (1,9) (1,16) (2,18) (2,31) (3,33) (3,38)
TOP_MIN_BITS = 20                                      # GECM_UROW_TOP_MIN_BITS
MASK = (1 << LIMB_BITS) - 1
HALF = 1 << (LIMB_BITS - 1)
I32 = 1 << 31


def row_shape(nl):
    """gecm_row_shape: (limbs per lane, rows of a multiply = limbs in use)"""
    return (nl + 1 + 15) // 16, nl + 1


def balanced(v, L):
    """v in L signed limbs: [-2^27, 2^27) below the top one, which takes the rest"""
    out = []
    for _ in range(L - 1):
        d = ((v + HALF) & MASK) - HALF
        out.append(d)
        v = (v - d) >> LIMB_BITS
    return out + [v]


def value(limbs):
    return sum(d << (LIMB_BITS * i) for i, d in enumerate(limbs))


def in_i32(x):
    return -I32 <= x < I32


class UnitRowModel:
    """one modulus n on a context of nl limbs"""

    def __init__(self, n, nl):
        self.n, self.nl = n, nl
        self.nq, self.L = row_shape(nl)
        L = self.L
        self.R = 1 << (LIMB_BITS * nl)                 # the device buffers' radix
        self.Rp = 1 << (LIMB_BITS * L)                 # the kernel's
        self.B = 1 << (LIMB_BITS * (L - 1))
        m = (-pow(n, -1, 1 << LIMB_BITS)) % (1 << LIMB_BITS)
        low = self.B << TOP_MIN_BITS
        M = m * n
        self.t = 0
        if M < low:
            step = n << LIMB_BITS
            self.t = (low - M + step - 1) // step
            M += self.t * step
        self.M = M
        # what host/gecm_api.c checks, and DESIGN.md §22 states
        assert M % n == 0 and M & MASK == MASK
        assert low <= M < (self.Rp >> 5) + (self.Rp >> 8)
        assert self.Rp > 28 * M
        self.Ml = [(M >> (LIMB_BITS * i)) & MASK for i in range(L)]
        self.cin = self.Rp * self.Rp // self.R % n
        assert self.cin == pow(2, 2 * LIMB_BITS * L - LIMB_BITS * nl, n)
        self.one = self.R % n
        um = UnitModel(n, nl)
        self.K, self.kp = um.K, um.kp
        two = 2 * self.Rp % M
        self.two = balanced(two - M if 2 * two > M else two, L)
        assert all(-HALF <= d <= HALF for d in self.two[:-1]) and abs(value(self.two)) <= M // 2 + 1
        scaled = float(self.Ml[L - 1]) + float(self.Ml[L - 2]) / 268435456.0 + float(self.Ml[L - 3]) / 72057594037927936.0
        self.minv = np.float32(1.0 / scaled)
        self.rho = m
        self.inv = {M: pow(M, -1, self.Rp), n: pow(n, -1, self.Rp)}
        self.multiplies = self.reductions = 0
        self.max_q = 0
        # the operand bound of a multiply: P+1 values are reduced ones, P-1 values products of products
        self.bound = {True: M // 2 + (M >> 19), False: 104 * M // 100}
        self.reduced = M // 2 + (M >> 19)

    # ---- fer_mul: r = a b / R' modulo `mod` (M with rho = 1, or n with its own rho), digits in [0, 2^28) -----------------
    def mul(self, a, b, mod, pp1=None):
        assert all(abs(d) < 1 << 29 for d in a) and all(abs(d) < 1 << 29 for d in b), "operand limb not below 2^29"
        va, vb = value(a), value(b)
        if pp1 is not None:
            assert abs(va) <= self.bound[pp1] and abs(vb) <= self.bound[pp1], "operand outside the value bound"
        q = (-va * vb * self.inv[mod]) % self.Rp
        r, rem = divmod(va * vb + q * mod, self.Rp)
        assert rem == 0 and abs(r) < abs(va * vb) // self.Rp + mod + 1
        self.multiplies += 1
        return balanced(r, self.L)                     # limbs in +-(2^27 + 4), the top one free: the contract

    # ---- fer_reduce ------------------------------------------------------------------------------------------------------
    def reduce(self, v):
        L = self.L
        v0 = value(v)
        assert all(abs(d) <= (1 << 28) + 8 for d in v[:-1]) and abs(v0) <= 21 * self.M // 10
        top = v[L - 1]
        assert in_i32(top)
        q = int(np.rint(np.float32(top) * self.minv))
        assert abs(q) <= 2, "quotient outside the claimed range"
        self.max_q = max(self.max_q, abs(q))
        x = [v[i] - q * self.Ml[i] for i in range(L)]
        assert all(in_i32(q * self.Ml[i]) and in_i32(x[i]) and in_i32(x[i] + HALF) for i in range(L))
        c = [(x[i] + HALF) >> LIMB_BITS if i < L - 1 else 0 for i in range(L)]
        lo = [x[i] - (c[i] << LIMB_BITS) for i in range(L)]
        out = [lo[i] + (c[i - 1] if i else 0) for i in range(L)]
        assert all(in_i32(d) for d in lo + out)
        assert value(out) == v0 - q * self.M
        assert all(-HALF - 3 <= d <= HALF + 2 for d in out[:-1]), "limb outside the balanced range"
        assert abs(value(out)) <= self.reduced, "reduced value outside (1/2 + 2^-19) M"
        self.reductions += 1
        return out

    def add(self, X, Y, W, pp1):
        T = self.mul(X, Y, self.M, pp1)
        if not pp1:
            return T
        D = [T[i] - W[i] for i in range(self.L)]
        assert all(in_i32(d) for d in D)
        return self.reduce(D)

    # ---- the kernel: plain canonical x in, the plain residue its output stands for out -----------------------------------
    def unit(self, ops, x, method):
        n, nl, L = self.n, self.nl, self.L
        pp1 = method != METHOD_PM1
        assert 0 <= x < n
        X = x * self.R % n                                               # the upload's canonical Montgomery form
        load = [(X >> (LIMB_BITS * i)) & MASK for i in range(nl)] + [0] * (L - nl)
        cin = [(self.cin >> (LIMB_BITS * i)) & MASK for i in range(nl)] + [0] * (L - nl)
        A = self.mul(load, cin, self.M)
        assert abs(value(A)) <= 1001 * self.M // 1000
        A = self.reduce(A)
        A = run_unit_tape(ops, A, lambda P, Q, W: self.add(P, Q, W, pp1), lambda P: self.add(P, P, self.two, pp1))
        assert abs(value(A)) <= self.bound[pp1]
        one = [(self.one >> (LIMB_BITS * i)) & MASK for i in range(nl)] + [0] * (L - nl)
        t = self.mul(A, one, n)                                          # modulo N itself, with N's rho
        assert -n // 16 < value(t) < 17 * n // 16 and t[nl] == 0
        u = [t[i] + self.kp[i] for i in range(nl)]
        assert all(0 <= w < 1 << 32 for w in u), "exit limb negative or above 32 bits"
        out = [(u[i] & MASK) + ((u[i - 1] >> LIMB_BITS) if i else 0) for i in range(nl)]
        out[nl - 1] += u[nl - 1] & ~MASK
        assert all(0 <= w < (1 << 28) + 16 for w in out[:-1]) and 0 <= out[nl - 1] < 1 << 32
        lazy = value(out)
        assert lazy == value(t) + self.K and lazy < self.K + 2 * n       # what k_canon takes
        return lazy % n * pow(self.R, -1, n) % n
