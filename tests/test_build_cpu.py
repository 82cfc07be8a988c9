"""CPU tests of the device curve build: the new entry points of the C ABI, and the kernel's formula
sequence — restated in tests/suyama_model.py in the kernel's own lazy Montgomery arithmetic — against the plain Suyama
values with pow(., -1, N) and math.gcd, stale operands of a failed inversion included.  This pins the algebra (sigma >= N,
sigma = 2^64 - 1, the failure rule) where no GPU is needed and gives tests/test_gpu_curve_build.py's directed inputs a
CPU-checked expectation."""
import ctypes
import math
import os
import random
import re

import pytest

from conftest import ROOT
from suyama_model import (N11Q, N40, N65, N415, Q415, SIGMA_EDGES, KernelModel, is_probable_prime, pick_nl,
                          suyama_plain)

GECM_ERR_ARG = -2


@pytest.fixture(scope="module")
def lib():
    import pyecm
    return pyecm.lib


def test_library_exports_the_three_entry_points_as_documented(lib):
    hdr = open(os.path.join(ROOT, "include", "gecm.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    for proto in ("int gecm_set_curve_build(gecm_ctx *ctx, int where);",
                  "int gecm_get_curve_build(const gecm_ctx *ctx);",
                  "int gecm_download_s(gecm_ctx *ctx, void *s);"):
        assert proto in flat
    assert re.search(r"#define GECM_BUILD_HOST 0\b", hdr) and re.search(r"#define GECM_BUILD_DEVICE 1\b", hdr)
    raw = ctypes.CDLL(lib._name)
    for name in ("gecm_set_curve_build", "gecm_get_curve_build", "gecm_download_s"):
        assert hasattr(raw, name), name
    import pyecm
    assert lib.gecm_set_curve_build.argtypes == [ctypes.c_void_p, ctypes.c_int] and lib.gecm_set_curve_build.restype is ctypes.c_int
    assert lib.gecm_get_curve_build.argtypes == [ctypes.c_void_p] and lib.gecm_get_curve_build.restype is ctypes.c_int
    assert lib.gecm_download_s.argtypes == [ctypes.c_void_p, ctypes.c_void_p] and lib.gecm_download_s.restype is ctypes.c_int
    assert {"gecm_set_curve_build", "gecm_get_curve_build", "gecm_download_s"} <= set(pyecm.EXPORTS)
    for meth in ("set_curve_build", "curve_build", "download_s"):
        assert callable(getattr(pyecm.Engine, meth))
    assert pyecm.MultiEngine.set_curve_build is pyecm.Engine.set_curve_build
    assert pyecm.MultiEngine.curve_build is pyecm.Engine.curve_build


def test_set_curve_build_rejects_a_null_context_and_unknown_values(lib):
    for where in (0, 1, 2, -1):
        assert lib.gecm_set_curve_build(None, where) == GECM_ERR_ARG
    assert b"gecm_set_curve_build" in lib.gecm_last_error()
    assert lib.gecm_get_curve_build(None) == GECM_ERR_ARG
    # a value other than 0 / 1 is refused before the context is looked at: any non-NULL pointer shows it
    dummy = ctypes.create_string_buffer(1 << 16)
    for where in (2, -1, 1 << 20):
        assert lib.gecm_set_curve_build(ctypes.cast(dummy, ctypes.c_void_p), where) == GECM_ERR_ARG


def test_the_directed_moduli_are_what_the_tests_say():
    assert is_probable_prime(Q415) and N11Q.bit_length() == 415 and N11Q % 11 == 0
    assert N65.bit_length() == 65 and N65 % 2 == 1 and N40 < 2**63 and N40 % 2 == 1
    assert N415.bit_length() == 415 and pick_nl(415) == 15 and pick_nl(65) == 8 and pick_nl(1030) == 37
    # sigma = 15: u = 220 = 0 mod 11, v = 60: only 16u^3v has no inverse, v^3 has one
    u, v = 15 * 15 - 5, 4 * 15
    assert math.gcd(u, N11Q) == 11 and math.gcd(v, N11Q) == 1
    assert math.gcd(16 * u**3 * v, N11Q) == 11 and math.gcd(v**3, N11Q) == 1
    # sigma = 22: v = 88 = 0 mod 11: both denominators fail
    u, v = 22 * 22 - 5, 4 * 22
    assert math.gcd(v, N11Q) == 11 and math.gcd(16 * u**3 * v, N11Q) == 11 and math.gcd(v**3, N11Q) == 11
    for s in (14, 16, 21, 23):
        assert suyama_plain(N11Q, s)[2] == 0
    assert suyama_plain(N11Q, 15)[2] == 1 and suyama_plain(N11Q, 22)[2] == 1
    x, _, _ = suyama_plain(N11Q, 15)                 # X of sigma = 15 is still a true quotient
    assert x * pow(4 * 15, 3, N11Q) % N11Q == pow(15 * 15 - 5, 3, N11Q)


def _sigmas(rnd, count):
    return SIGMA_EDGES + [15, 22, 14, 16, 21, 23] + [rnd.randrange(6, 1 << 64) for _ in range(count)]


@pytest.mark.parametrize("n", [N40, N65, N415, N11Q], ids=["n40", "n65", "n415", "n11q"])
def test_kernel_sequence_in_montgomery_arithmetic_equals_plain_suyama(n):
    k = KernelModel(n)
    flagged = 0
    for sigma in _sigmas(random.Random(n % 1000003), 40):
        X, Z, S, flag = k.build(sigma)               # asserts the operand bounds of every multiply on the way
        x, s, want = suyama_plain(n, sigma)
        assert (X, Z, S, flag) == (x * k.R % n, k.R % n, s * k.R % n, want), sigma
        assert 0 <= X < n and 0 <= S < n
        flagged += flag
    if n == N11Q:
        assert flagged >= 2
    if n == N40:
        assert any(s >= n for s in SIGMA_EDGES)


def test_kernel_sequence_meets_every_failure_pattern_modulo_a_small_composite():
    """N = 3 * 5 * 7 * 11 * 13 + a large prime cofactor would hide them: modulo 1155 * p with small sigma every
    combination (none, 16u^3v only, both) occurs; v^3 alone cannot fail, v divides 16u^3v"""
    n = 3 * 5 * 7 * 11 * Q415
    k = KernelModel(n)
    seen = set()
    for sigma in range(6, 400):
        X, Z, S, flag = k.build(sigma)
        x, s, want = suyama_plain(n, sigma)
        assert (X, S, flag) == (x * k.R % n, s * k.R % n, want), sigma
        u, v = sigma * sigma - 5, 4 * sigma
        seen.add((math.gcd(16 * u**3 * v, n) != 1, math.gcd(v**3, n) != 1))
    assert seen == {(False, False), (True, False), (True, True)}


def test_limb_count_extremes_keep_the_bounds():
    """a modulus at the bottom and at the top of a limb class, at both ends of the range: K = 2N .. 32N"""
    for nl in (8, 37):
        for n in ((1 << (28 * nl - 5)) - 1, (1 << (28 * nl - 5 - 27)) + 1 if nl > 8 else 3):
            k = KernelModel(n, nl)
            for sigma in SIGMA_EDGES:
                X, _, S, flag = k.build(sigma)
                x, s, want = suyama_plain(n, sigma)
                assert (X, S, flag) == (x * k.R % n, s * k.R % n, want)
