"""Wide contexts without a device: the limb rule and the bit limit of the library, and the model of the
three-limbs-per-lane row multiply at 41, 44 and 48 rows (tests/wide_row_model.py): on moduli at both ends of every wide
class and operands at the tape interpreter's bounds, every accumulator write stays inside signed 64 bits, every high word
read as a multiply-add operand inside signed 32 bits, the value is (a b + q N') / R', limbs from ROWS up stay zero, and the
lazy exit value of one launch is inside the contract of the next launch's entry multiply (a cut tape needs no canonical
form in between)."""
import os
import random
import subprocess

import pytest

import wide_row_model as W
from conftest import ROOT

KINDS = ("random", "2^k-1", "1mod2^28")
CASES = [(nl, bits, kind) for nl, lo, hi in W.WIDE_CLASSES for bits in (lo, hi) for kind in KINDS]
I64, I32 = 1 << 63, 1 << 31


def test_the_library_limit_and_limb_rule():
    import pyecm
    assert pyecm.wide_max_bits() == W.WIDE_MAX_BITS == 1311
    assert "gecm_create_wide" in pyecm.EXPORTS and "gecm_is_wide" in pyecm.EXPORTS and "gecm_wide_max_bits" in pyecm.EXPORTS
    assert pyecm.lib.gecm_is_wide(None) == 0


def test_limb_rule():
    assert [W.wide_nl(b) for b in (1032, 1115, 1116, 1199, 1200, 1311, 1312)] == [40, 40, 43, 43, 47, 47, 0]
    for nl, lo, hi in W.WIDE_CLASSES:
        assert W.LIMB * nl >= hi + 5 and W.LIMB * nl < hi + 1 + 5
        assert nl + 1 in W.WIDE_ROWS and 2 * W.LANES < nl + 1 <= 3 * W.LANES


def test_headroom_is_exact_for_n_1_mod_2_28():
    """N = 1 mod 2^28 has m = 2^28 - 1: N' is as long as it gets, bits(N') + 5 = 28 ROWS at the top of a class"""
    for nl, _, hi in W.WIDE_CLASSES:
        c = W.row_consts(W.modulus(hi, "1mod2^28"), nl)
        assert c["np"].bit_length() + 5 == W.LIMB * c["rows"]


@pytest.mark.parametrize("nl,bits,kind", CASES, ids=["nl%d_%d_%s" % c for c in CASES])
def test_row_multiply_at_three_limbs_per_lane(nl, bits, kind):
    n = W.modulus(bits, kind)
    assert W.wide_nl(bits) == nl
    ends = W.Stage1Ends(n, nl)
    rows, nprime = ends.rows, ends.c["np"]
    rng = random.Random("wide model:%d:%s" % (bits, kind))
    ex = [W.extreme_operand4(nprime, rows, sg, p) for sg in (1, -1) for p in ("same", "alternate", rng)]
    rnd = [W.random_operand4(rng, nprime, rows) for _ in range(4)]
    pairs = [(ex[0], ex[0]), (ex[0], ex[3]), (ex[1], ex[1]), (ex[1], ex[4]), (ex[2], ex[5]), (ex[3], ex[3])]
    pairs += [(rnd[0], ex[1]), (ex[4], rnd[1]), (rnd[2], rnd[3]), (rnd[0], rnd[0])]
    results = [ends.interp(a, b) for a, b in pairs]
    # the exit of interpreter values, and the raw words fed back through the entry multiply (the cut tape)
    for p4 in results[:4] + [W.balanced_times4(rng.randrange(-12 * nprime // 10, 12 * nprime // 10), rows)]:
        words, t = ends.exit(p4)
        assert -n // 16 < t < 17 * n // 16 + 1
        assert all(0 <= w < (1 << W.LIMB) + 16 for w in words[:-1]) and 0 <= words[-1]
        assert 0 < W.value_of(words) < (1 << (W.LIMB * nl)) // 16 + 2 * n
        back = ends.entry(words)
        assert (W.signed_value(back, 4) - W.signed_value(p4, 4)) % n == 0      # x R' again, modulo N
        assert all(abs(x) <= 4 * W.PRODUCT_LIMB_MAX for x in back[:rows - 1])
    # canonical words (a fresh batch) through the entry multiply
    for v in (0, 1, n - 1, rng.randrange(n)):
        ends.entry(W.limbs_of(v, nl))
    assert ends.mul.peak_acc < I64, ends.mul.peak_acc.bit_length()
    assert ends.mul.peak_hi < I32, ends.mul.peak_hi.bit_length()
    assert ends.mul.peak_op < I32


def test_host_side_under_the_sanitizers():
    """tools/wide_sanitize.sh: a program of its own over mpl.c and gecm_mod.c (CPU only), built and run with
    AddressSanitizer + UBSan"""
    p = subprocess.run([os.path.join(ROOT, "tools", "wide_sanitize.sh")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "wide_sanitize: ok" in p.stdout, p.stdout + p.stderr
