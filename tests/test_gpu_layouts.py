"""Every stage-1 layout (one, two, eight and 32 lanes per curve: k_stage1, k_stage1_pair, k_stage1_quad, k_stage1_row) at
the smallest and the largest modulus of every built limb count, on the five modulus kinds of tests/divsteps_model.py,
with the kernel that ran asserted by name:
 * save lines of all 33 curves against the oracle, in each of the four layouts;
 * the crossbar variant of the 32-lane kernel (k_stage1_row<1, rows, true>) at each of its five shapes, against the
   one-lane kernel on the whole batch and against the oracle on a sample;
 * chosen start points (edges of [0, N), limb boundaries, R mod N) through gecm_upload_points: the four layouts against
   each other, and against a plain binary ladder on Python integers (tests/xladder.py).
All comparisons are exact, on integers or on the bytes of a save line."""
import ctypes
import math
import os
import random

import pytest

import divsteps_model as M
from conftest import ROOT
from xladder import ladder_point, stage1_multiplier

pytestmark = pytest.mark.gpu

LAYOUTS = (1, 2, 8, 32)
EDGES = M.edge_bits()
EDGE_IDS = ["nl%d_%dbit" % c for c in EDGES]


def _kernel(nl, lanes, crossbar=False):
    """the instantiation gecm_last_kernel_name must report for that layout"""
    if lanes == 32:
        return "k_stage1_row<%d, %d, %s>" % ((nl + 1 + 15) // 16, nl + 1, "true" if crossbar else "false")
    return {1: "k_stage1<%d>", 2: "k_stage1_pair<%d>", 8: "k_stage1_quad<%d>"}[lanes] % nl


def _digitbits(bits):
    return 52 if bits < 1000 else 32


@pytest.fixture(scope="module")
def orc():
    L = ctypes.CDLL(os.path.join(ROOT, "oracle", "libecm_oracle.so"))
    L.orc_create.restype = ctypes.c_void_p
    L.orc_create.argtypes = [ctypes.c_char_p, ctypes.c_int]
    L.orc_destroy.argtypes = [ctypes.c_void_p]
    L.orc_stage1_line.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t,
                                  ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)]
    return L


def _oracle_lines(orc, n, digitbits, sigmas, b1):
    c = orc.orc_create(str(n).encode(), digitbits)
    line = ctypes.create_string_buffer(16384)
    out = []
    for s in sigmas:
        orc.orc_stage1_line(c, s, b1, line, len(line), None, 0, None)
        out.append(line.value.decode())
    orc.orc_destroy(c)
    return out


# ---- 1. layout x limb count x modulus kind, against the oracle ---------------------------------------------------
@pytest.mark.parametrize("nl,bits", EDGES, ids=EDGE_IDS)
def test_every_layout_writes_the_oracles_lines(orc, nl, bits):
    """33 curves (a wavefront that is not full; a ragged second quad or row group), one B1 of a few hundred, generic
    REDC in all four layouts (the 2^k -/+ 1 kinds with the special form switched off)"""
    import pyecm
    digitbits = _digitbits(bits)
    for kind in M.KINDS:
        n = M.modulus(bits, kind)
        rng = random.Random("layouts:%d:%s" % (bits, kind))
        sig = [rng.randrange(6, 1 << 63) for _ in range(33)]
        b1 = rng.randrange(150, 401 if nl < 26 else 251)                # the oracle's time on the CPU grows with the square of nl
        want = _oracle_lines(orc, n, digitbits, sig, b1)
        eng = pyecm.Engine(n, digitbits=digitbits)
        assert eng.cfg.dev_limbs == nl
        eng.set_special_form(False)
        facs = {}
        for lanes in LAYOUTS:
            eng.set_lanes_per_curve(lanes)
            eng.build_curves(sig)
            eng.stage1(b1)
            assert eng.lanes_per_curve() == lanes and not eng.special_form_used()
            assert eng.last_kernel_name() == _kernel(nl, lanes), (kind, lanes)
            lines = eng.save_lines()
            for k in range(len(sig)):
                assert lines[k] == want[k], (kind, lanes, b1, k, sig[k])
            facs[lanes] = [eng.stage1_factor(k) for k in range(len(sig))]
        eng.close()
        assert facs[1] == facs[2] == facs[8] == facs[32], kind


# ---- 2. the crossbar variant of the 32-lane kernel ---------------------------------------------------------------
CROSSBAR_BATCH = 4096 + 130       # just over 16 curves per CU on 256 CUs, not a multiple of 64


@pytest.mark.parametrize("nl", [8, 10, 12, 14, 15])
def test_row_kernel_crossbar_variant(orc, nl):
    """One limb per lane, more than 16 curves per CU: operand limbs go through the LDS crossbar.  A library that picks the
    DPP variant here fails this test: nothing else in the suite would then run the crossbar variant."""
    import pyecm
    bits = M.LIMB * nl - 5
    for kind in ("random", "2^k-1"):
        n = M.modulus(bits, kind)
        rng = random.Random("crossbar:%d:%s" % (bits, kind))
        sig = [rng.randrange(6, 1 << 63) for _ in range(CROSSBAR_BATCH)]
        b1 = rng.randrange(90, 111)
        last = CROSSBAR_BATCH - 1
        sample = sorted({0, 1, 31, 32, 63, 64, 4095, 4096, last} | {rng.randrange(CROSSBAR_BATCH) for _ in range(12)})
        eng = pyecm.Engine(n, digitbits=52)
        assert eng.cfg.dev_limbs == nl
        eng.set_special_form(False)
        eng.set_lanes_per_curve(32)
        eng.build_curves(sig)
        eng.stage1(b1)
        assert eng.lanes_per_curve() == 32 and not eng.special_form_used()
        assert eng.last_kernel_name() == "k_stage1_row<1, %d, true>" % (nl + 1), kind
        rows = eng.save_lines()
        eng.set_lanes_per_curve(1)
        eng.build_curves(sig)
        eng.stage1(b1)
        assert eng.last_kernel_name() == _kernel(nl, 1)
        one = eng.save_lines()
        assert len(rows) == len(one) == CROSSBAR_BATCH
        differ = [k for k in range(CROSSBAR_BATCH) if rows[k] != one[k]]
        assert not differ, (kind, len(differ), differ[:8])
        want = _oracle_lines(orc, n, 52, [sig[k] for k in sample], b1)
        for k, w in zip(sample, want):
            assert rows[k] == w, (kind, k, sig[k])
        # the same curves in a batch below the threshold: the DPP variant, the same lines
        eng.set_lanes_per_curve(32)
        eng.build_curves(sig[:64])
        eng.stage1(b1)
        assert eng.last_kernel_name() == _kernel(nl, 32, crossbar=False)
        assert eng.save_lines() == rows[:64], kind
        eng.close()


# ---- 3. chosen start points through gecm_upload_points -----------------------------------------------------------
POINT_KINDS = ("random", "2^k-1")
MIN_CHECKED_BITS = 64


def _coprime_part(n, z):
    """the largest divisor of n that is coprime to z"""
    g = math.gcd(n, z)
    while g != 1:
        n //= g
        g = math.gcd(n, g)
    return n


def _point_inputs(n, bits, kind, nl, R):
    """(b1, regular, degenerate): lists of (X, Z, s) as plain residues"""
    rng = random.Random("start points:%d:%s" % (bits, kind))
    b1 = rng.randrange(180, 221)
    ops = M.fixed_operands(n, bits, kind, nl, R % n)
    assert ops[0] == 0
    xs = list(dict.fromkeys(v for v in ops if v))                       # without the zero; each value once
    off = rng.randrange(1, len(xs))
    regular = [(x, 1, s) for x, s in zip(xs, xs[off:] + xs[:off])]
    x0, s0 = rng.randrange(2, n - 1), rng.randrange(2, n - 1)
    degenerate = [(x0, 0, s0), (1, 0, s0), (0, 1, s0), (0, n - 1, s0), (0, 0, s0), (x0, x0, s0), (1, 1, s0), (n - 1, n - 1, s0),
                  (x0, 1, 0), (n - 1, 1, 0), (x0, 1, n - 1), (1, 1, n - 1), (0, 0, 0), (n - 1, n - 1, n - 1)]
    return b1, regular, degenerate


def _unchecked(n, regular, k):
    """the ladder's point for every regular input, and the inputs on which the cross-product says too little"""
    pts = [ladder_point(n, x, s, k) for x, _, s in regular]
    weak = [i for i, (_, Z) in enumerate(pts) if _coprime_part(n, Z).bit_length() <= MIN_CHECKED_BITS]
    return pts, weak


@pytest.mark.parametrize("nl,bits", EDGES, ids=EDGE_IDS)
def test_chosen_start_points_in_every_layout(nl, bits):
    """Regular points (x over the fixed operands of the modulus, Z = 1, s over the same list rotated): the four layouts
    bit-identical, every coordinate canonical, and X_dev Z_py = X_py Z_dev (mod N) with the plain ladder's (X_py, Z_py).
    Degenerate points (Z = 0, X = 0, X = Z, s = 0, s = N - 1): the four layouts bit-identical and canonical only.

    When is the cross-product vacuous?  It says nothing modulo the primes of N that divide Z_py, and these moduli are not
    primes: 2^k - 1 and a random odd number have small factors p modulo which [k]P is the point at infinity on every
    curve (the group order modulo 3, 5, 7, 11, ... divides the stage-1 multiplier of a B1 near 200), so gcd(Z_py, N) = 1
    holds for none of the inputs of 49 of the 60 moduli, whatever the seeds (counted on Python integers).  What is
    required instead: the divisor of N coprime to Z_py, modulo which the comparison is a real one, has more than 64 bits
    (a wrong residue passes with probability 2^-64), on all but 2 % of the regular inputs of any modulus; asserted.
    Counted with the ladder alone over the 60 moduli: 2 inputs of every modulus fall short, x = 1 and x = N - 1, the
    points of order 4 ([k]P is the point at infinity modulo N itself); no other input does, and on the rest the coprime
    divisor is never shorter than 81 bits (220-bit 2^k - 1) and within 60 bits of N on the random moduli but one."""
    import pyecm
    for kind in POINT_KINDS:
        n = M.modulus(bits, kind)
        eng = pyecm.Engine(n, digitbits=_digitbits(bits))
        assert eng.cfg.dev_limbs == nl
        R = 1 << eng.cfg.maxbits
        b1, regular, degenerate = _point_inputs(n, bits, kind, nl, R)
        pts = regular + degenerate
        X, Z, S = ([v[j] * R % n for v in pts] for j in range(3))
        eng.set_special_form(False)
        got = {}
        for lanes in LAYOUTS:
            eng.set_lanes_per_curve(lanes)
            eng.upload_points(X, Z, S)
            eng.stage1(b1)
            assert eng.lanes_per_curve() == lanes and not eng.special_form_used()
            assert eng.last_kernel_name() == _kernel(nl, lanes), (kind, lanes)
            got[lanes] = (eng.download_points(), eng.download_points_plain())
        eng.close()
        (Xr, Zr), (xp, zp) = got[1]
        for lanes in LAYOUTS[1:]:
            for a, b in zip(got[1][0] + got[1][1], got[lanes][0] + got[lanes][1]):
                differ = [k for k in range(len(pts)) if a[k] != b[k]]
                assert not differ, (kind, lanes, differ[:8])
        assert all(v < n for v in Xr + Zr + xp + zp), kind
        assert Xr == [v * R % n for v in xp] and Zr == [v * R % n for v in zp], kind
        py, weak = _unchecked(n, regular, stage1_multiplier(b1))
        print("%s: B1 %d, %d regular inputs, %d with a coprime divisor of %d bits or less: %r"
              % (kind, b1, len(regular), len(weak), MIN_CHECKED_BITS, weak))
        assert len(weak) * 100 <= 2 * len(regular), (kind, weak)
        for k, (Xpy, Zpy) in enumerate(py):
            assert (xp[k] * Zpy - Xpy * zp[k]) % n == 0, (kind, k, hex(regular[k][0]), hex(regular[k][2]))
