"""The device inversion (fe_invert / fe_inv_mont, csrc/gecm_stage2.hpp) on chosen inputs, through gecm_vecinvmod and
through the whole-batch factor scan.  Every comparison is an exact integer against pow(x, -1, n) and math.gcd; the
inputs are those of tests/divsteps_model.py (edges of [0, N), limb boundaries, multiples of known divisors, the latest
convergers of the seeded search), on moduli at both ends of every built limb count."""
import json
import math
import os
import random

import pytest

import divsteps_model as M
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

CASES = [(nl, bits, 52) for nl, bits in M.edge_bits()] + \
        [(nl, bits, 32) for nl, bits in M.edge_bits() if nl in (8, 21, 37)]
IDS = ["nl%d_%dbit_d%d" % c for c in CASES]
BIG = 301           # the large batch: more than four wavefronts, not a multiple of 64


def _expected(n, R, a):
    """(inv, gcd) by Python integers for the operand a = x R mod n"""
    x = a * pow(R, -1, n) % n
    assert x * R % n == a
    g = math.gcd(x * R % n, n)
    return (pow(x, -1, n) * R % n if g == 1 else 0), g


@pytest.mark.parametrize("nl,bits,digitbits", CASES, ids=IDS)
def test_vecinvmod_equals_python_on_directed_inputs(nl, bits, digitbits):
    import pyecm
    for kind in M.KINDS:
        n = M.modulus(bits, kind)
        eng = pyecm.Engine(n, digitbits=digitbits)
        assert eng.cfg.dev_limbs == nl and eng.cfg.maxbits == M.ref_maxbits(bits, digitbits)
        R = 1 << eng.cfg.maxbits
        a = M.operands(n, bits, kind, nl, R % n)
        rng = random.Random("pad:%d:%s" % (bits, kind))
        a += [rng.randrange(n) for _ in range(BIG - len(a))]            # up to the large batch (longer lists stay)
        want = [_expected(n, R, v) for v in a]
        assert want[0] == (0, n) and want[1][1] == 1                    # a = 0: no inverse, gcd N
        if kind == "composite":
            assert {M.P, n // M.P} <= {g for _, g in want}
        inv, g = eng.vecinvmod(a)
        for k, v in enumerate(a):
            assert (inv[k], g[k]) == want[k], (kind, k, hex(v))
            assert inv[k] < n and g[k] <= n
        ok = [k for k in range(len(a)) if want[k][1] == 1]
        assert eng.vecmulmod([a[k] for k in ok], [inv[k] for k in ok]) == [R % n] * len(ok)
        # the same values in other batch shapes: one lane, one short of a wavefront, one over
        for lo, cnt in ((7, 1), (0, 63), (len(a) - 65, 65)):
            inv, g = eng.vecinvmod(a[lo:lo + cnt])
            assert list(zip(inv, g)) == want[lo:lo + cnt], (kind, lo, cnt)
        eng.close()


def test_vecinvmod_rejects_non_canonical_and_multi_modulus():
    import pyecm
    n = (1 << 100) + 277
    eng = pyecm.Engine(n)
    with pytest.raises(pyecm.GecmError, match="not < N"):
        eng.vecinvmod([1, n])
    one = pow(2, eng.cfg.maxbits, n)
    assert eng.vecinvmod([one]) == ([one], [1])                         # the context is usable after the rejection
    eng.close()
    multi = pyecm.MultiEngine([(1 << 127) - 1, 1000003])
    with pytest.raises(pyecm.GecmError, match=r"\(-4\): the L0 operators: not available on a multi-modulus context"):
        multi.vecinvmod([1])
    multi.close()


def _probable_prime(n):
    """Miller-Rabin on 24 seeded bases (after trial division by the small primes)"""
    small = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97)
    if any(n % p == 0 for p in small):
        return n in small
    s = (n - 1 & -(n - 1)).bit_length() - 1
    rng = random.Random(n)
    for _ in range(24):
        y = pow(rng.randrange(2, n - 1), n >> s, n)
        if y in (1, n - 1):
            continue
        for _ in range(s - 1):
            y = y * y % n
            if y == n - 1:
                break
        else:
            return False
    return True


def _prime_of(bits):
    """the first probable prime from the random modulus of that length downwards (upwards could leave the length)"""
    n = M.modulus(bits, "random")
    while not _probable_prime(n):
        n -= 2
    assert n.bit_length() == bits
    return n


@pytest.mark.parametrize("nl,bits", M.edge_bits(), ids=["nl%d_%dbit" % c for c in M.edge_bits()])
def test_factor_scan_on_chosen_values(nl, bits):
    """gecm_scan_factors(1) over uploaded Z: the flag of every curve, gecm_stage1_factor, the count and `first` against
    1 < gcd(Z_k, N) < N.  Each operand is uploaded twice: as it is, and scaled so that the device's fe_invert, which
    sees Z in the internal radix 2^(28 nl), is handed exactly that operand.  Three moduli: the composite (its known
    divisors must be flagged), the random odd one (a third of them have small prime factors that the operands meet: the
    flags follow Python's gcd, whatever they are) and a prime, on which nothing may be flagged."""
    import pyecm
    for kind in ("composite", "random", "prime"):
        n = _prime_of(bits) if kind == "prime" else M.modulus(bits, kind)
        eng = pyecm.Engine(n)
        R = 1 << eng.cfg.maxbits
        ops = M.fixed_operands(n, bits, kind, nl, R % n) if kind == "prime" else M.operands(n, bits, kind, nl, R % n)
        to_ref = R * pow(1 << (M.LIMB * eng.cfg.dev_limbs), -1, n) % n
        Z = ops + [v * to_ref % n for v in ops]
        one = [R % n] * len(Z)
        eng.upload_points(one, Z, one)                                   # Z = 0 is accepted (first operand)
        assert Z[0] == 0
        want = [math.gcd(z, n) for z in Z]
        flag = [1 < g < n for g in want]
        cnt, first = eng.scan_factors(1)
        assert [eng.curve_flag(1, k) for k in range(len(Z))] == flag, kind
        assert cnt == sum(flag) and first == (flag.index(True) if cnt else None)
        if kind == "composite":
            assert {M.P, n // M.P} <= {g for g, fl in zip(want, flag) if fl}
        if kind == "prime":
            assert cnt == 0
        for k in range(len(Z)):
            f = eng.stage1_factor(k)
            assert (f[0] if f else None) == (want[k] if flag[k] else None), (kind, k)
        eng.close()


def test_stage2_factor_equals_vecinvmod_gcd_of_the_accumulator():
    """a composite whose stage-2 batch inversions fail on some curves: where the downloaded accumulator itself carries
    the factor, gecm_stage2_factor reports the gcd gecm_vecinvmod computes of it"""
    import pyecm
    s1 = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "stage1.json")))}
    k1n = int(s1["K1"]["save_lines"][0].split("N=0x")[1].split(";")[0], 16)      # as tests/test_gpu_stage2.py
    n = M.P * k1n
    sig = list(range(1000, 1000 + 130))
    eng = pyecm.Engine(n)
    eng.build_curves(sig)
    eng.stage1(300)
    eng.stage2(3000, 0, 2)
    cnt, _ = eng.scan_factors(2)
    flagged = [k for k in range(len(sig)) if eng.curve_flag(2, k)]
    assert cnt == len(flagged) > 0
    acc = eng.download_acc()
    facs = {k: eng.stage2_factor(k) for k in flagged}
    inv, g = eng.vecinvmod(acc)
    assert g == [math.gcd(v, n) for v in acc]
    carried = [k for k in flagged if 1 < g[k] < n]
    print("stage 2: %d curves flagged, the accumulator carries the factor on %d" % (len(flagged), len(carried)))
    assert carried
    for k in carried:
        assert facs[k] is not None and facs[k][0] == g[k], k
        assert inv[k] == 0
    eng.close()
