"""GMP-ECM's PARAM 1 and PARAM 3 curves in Python integers, and the device build of them
(csrc/gecm_kernels.hip: k_build_param) restated operation for operation in the kernel's lazy Montgomery arithmetic, with the
REDC and the operand bounds of tests/suyama_model.py's KernelModel.  Shared by tests/test_param_cpu.py and the GPU tests.

The curve is B y^2 = x^3 + A x^2 + x with A = 4d - 2, so s = (A+2)/4 = d, and the start point is (2 : 1):
  PARAM 1: d = sigma^2 / 2^64 mod N, 1 <= sigma < 2^64;   PARAM 3: d = sigma / 2^32 mod N, 1 <= sigma < 2^32."""
from suyama_model import LIMB_BITS, KernelModel
from xladder import ladder_point, stage1_multiplier

PARAM_WIDTH = {1: 64, 3: 32}          # the power of two d is divided by
PARAM_SIGMAS = {1: [1, 2, 7, 2**32 - 1, 2**32, 2**32 + 1, 2**63, 2**64 - 1], 3: [1, 2, 7, 2**32 - 1]}


def param_d(param, sigma, n):
    w = PARAM_WIDTH[param]
    assert 1 <= sigma < 1 << w
    return (sigma * sigma if param == 1 else sigma) * pow(2, -w, n) % n


def k_std(b):
    return stage1_multiplier(b + 1)


_POINTS = {}


def param_point(n, param, sigma, b):
    """(X, Z) of [k_std(b)](2 : 1) on the curve of (param, sigma) modulo n, by the plain binary ladder"""
    key = (n, param, sigma, b)
    if key not in _POINTS:
        _POINTS[key] = ladder_point(n, 2, param_d(param, sigma, n), k_std(b))
    return _POINTS[key]


def param_line(n, param, sigma, b):
    """the standard line of a curve whose Z has an inverse"""
    X, Z = param_point(n, param, sigma, b)
    return "METHOD=ECM; PARAM=%d; SIGMA=%d; B1=%d; N=0x%x; X=0x%x; PROGRAM=AVX-ECM-STD;\n" % (param, sigma, b, n, X * pow(Z, -1, n) % n)


def shift_constant(nl, param):
    """(limb, bit) of 2^(28 nl - w): the one set bit of the operand that divides by 2^w in a Montgomery multiply"""
    e = LIMB_BITS * nl - PARAM_WIDTH[param]
    return e // LIMB_BITS, e % LIMB_BITS


class ParamModel(KernelModel):
    """k_build_param's sequence: every multiply through KernelModel.mul, which asserts both operands below 1.675 K and the
    product below 0.675 K"""

    def build_param(self, param, sigma):
        """(X, Z, S) as the kernel stores them: canonical, Montgomery form"""
        assert 0 <= sigma < 1 << 64
        m = self.mul
        limb, bit = shift_constant(self.nl, param)
        c = 1 << (LIMB_BITS * limb + bit)
        assert 0 <= limb < self.nl and c < 1 << (LIMB_BITS * self.nl - 5) and c <= self.K
        w = m(sigma, self.r2)                     # sigma R, sigma's 64 bits in three limbs
        if param == 1:
            w = m(w, w)                           # sigma^2 R
        w = m(w, c)                               # d R = a b / R with b = R / 2^w
        return self.canon(m(2, self.r2)), self.one, self.canon(w)
