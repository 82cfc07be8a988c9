"""GPU parity across every built limb count (NL = 8 ... 37, 15 sizes) and ragged batch
sizes.  Inputs without small factors are built from Mersenne primes so that no curve hits the
degenerate "factor already found" path.  Checks: L0 operators against Python integers (the
mathematical definition the reference's operators satisfy, verified in tests/golden/l0.json),
stage 1 and stage 2 against the oracle.  The stage-1 checks here run in the library's choice of layout, which is 32 lanes
per curve at these batch sizes; the matrix of layouts, limb counts and moduli is tests/test_gpu_layouts.py."""
import ctypes
import math
import os
import random

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

M = {p: (1 << p) - 1 for p in (13, 17, 19, 31, 61, 89, 107, 127, 521, 607)}
# bits -> device limb count NL = smallest built size >= ceil((bits+5)/28)
CASES = [
    ("M89*M107", M[89] * M[107], 8),                       # 196 bits
    ("M127*M107", M[127] * M[107], 10),                    # 234 bits
    ("M127*M107*M89*M61", M[127] * M[107] * M[89] * M[61], 14),            # 384 bits
    ("M127*M107*M89*M61*M31*M19*M17*M13", M[127] * M[107] * M[89] * M[61] * M[31] * M[19] * M[17] * M[13], 17),  # 464
    ("M521*M61", M[521] * M[61], 21),                      # 582 bits
    ("M607*M127*M31*M13", M[607] * M[127] * M[31] * M[13], 28),            # 778 bits
    ("M607*M127*M107*M31*M17", M[607] * M[127] * M[107] * M[31] * M[17], 32),  # 889 bits
    ("M127*M89*M107", M[127] * M[89] * M[107], 12),        # 323 bits
    ("M521", M[521], 19),                                  # 521 bits
    ("M521*M127", M[521] * M[127], 26),                    # 648 bits
    ("M607*M127*M89", M[607] * M[127] * M[89], 30),        # 823 bits
    ("M607*M127*M107*M89", M[607] * M[127] * M[107] * M[89], 34),           # 930 bits
    ("M607*M127*M107*M89*M61", M[607] * M[127] * M[107] * M[89] * M[61], 37),  # 991 bits
]


@pytest.fixture(scope="module")
def orc():
    L = ctypes.CDLL(os.path.join(ROOT, "oracle", "libecm_oracle.so"))
    L.orc_create.restype = ctypes.c_void_p
    L.orc_create.argtypes = [ctypes.c_char_p, ctypes.c_int]
    L.orc_destroy.argtypes = [ctypes.c_void_p]
    L.orc_stage1_line.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t,
                                  ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)]
    L.orc_stage2.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32,
                             ctypes.c_uint32, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t,
                             ctypes.POINTER(ctypes.c_uint64)]
    return L


@pytest.mark.parametrize("name,n,nl", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("digitbits", [52, 32])
def test_every_limb_count(orc, name, n, nl, digitbits):
    import pyecm
    rng = random.Random(nl * 100 + digitbits)
    eng = pyecm.Engine(n, digitbits=digitbits)
    assert eng.cfg.dev_limbs == nl
    # L0 against the definition, Montgomery radix of the chosen reference limb format
    R = 1 << eng.cfg.maxbits
    Ri = pow(R, -1, n)
    a = [rng.randrange(n) for _ in range(70)] + [0, 1, n - 1]
    b = [rng.randrange(n) for _ in range(70)] + [n - 1, n - 1, n - 1]
    assert eng.vecmulmod(a, b) == [x * y * Ri % n for x, y in zip(a, b)]
    assert eng.vecsqrmod(a) == [x * x * Ri % n for x in a]
    s, d = eng.vecaddsubmod(a, b)
    assert s == [(x + y) % n for x, y in zip(a, b)] and d == [(x - y) % n for x, y in zip(a, b)]
    # stage 1 + stage 2 against the oracle
    sig = [rng.randrange(6, 1 << 63) for _ in range(65)]
    b1, b2, D, U = 600, 30000, 385, 2
    eng.build_curves(sig)
    eng.stage1(b1)
    lines = eng.save_lines()
    eng.stage2(b2, D, U)
    acc = eng.download_acc()
    eng.close()
    c = orc.orc_create(str(n).encode(), digitbits)
    line = ctypes.create_string_buffer(16384)
    acch = ctypes.create_string_buffer(8192)
    for k in (0, 63, 64):
        orc.orc_stage1_line(c, sig[k], b1, line, len(line), None, 0, None)
        assert line.value.decode() == lines[k]
        orc.orc_stage2(c, sig[k], b1, b2, D, U, acch, None, 0, None)
        assert int(acch.value, 16) == acc[k]
    orc.orc_destroy(c)


@pytest.mark.parametrize("name,n,nl", CASES, ids=[c[0] for c in CASES])
def test_pair_walk_long_segments_every_limb_count(orc, name, n, nl, monkeypatch):
    """The pair walk in one slice per curve over segments of thousands of pairs: blocks of 64 tape entries, the rows in
    flight across block boundaries and the tail of a segment, for every limb count (hand-placed loads with four or two
    rows in flight, and the compiler-scheduled variant from 32 limbs on)."""
    import pyecm
    monkeypatch.setenv("GECM_S2_SLICES", "1")
    rng = random.Random(nl)
    sig = [rng.randrange(6, 1 << 63) for _ in range(65)]
    b1, b2, D, U = 400, 400000, 2310, 8
    eng = pyecm.Engine(n)
    assert eng.cfg.dev_limbs == nl
    eng.build_curves(sig)
    eng.stage1(b1)
    eng.stage2(b2, D, U)
    acc = eng.download_acc()
    st = eng.stage2_stats()
    facs = {k: eng.stage2_factor(k) for k in (0, 1, 64)}
    eng.close()
    assert st.paired > 10000
    c = orc.orc_create(str(n).encode(), 52)
    acch = ctypes.create_string_buffer(8192)
    fac = ctypes.create_string_buffer(4096)
    for k in (0, 1, 64):
        found = orc.orc_stage2(c, sig[k], b1, b2, D, U, acch, fac, len(fac), None)
        if found:
            # the composite with 2^17-1 and 2^31-1 in it: most curves find a factor.  The factor reported is the
            # reference's; the accumulator itself is compared only when no inversion failed on the way (after a failed
            # inversion the reference multiplies on with what mpz_invert left behind, which nobody defines)
            assert facs[k][0] == int(fac.value)
        if not found or math.gcd(int(acch.value, 16), n) == int(fac.value):
            assert int(acch.value, 16) == acc[k]
    orc.orc_destroy(c)


@pytest.mark.parametrize("batch", [1, 2, 63, 64, 65, 127, 129])
def test_ragged_batches(orc, batch):
    import pyecm
    n = M[127] * M[89] * M[107] * M[61]
    sig = list(range(77, 77 + batch))
    eng = pyecm.Engine(n)
    eng.build_curves(sig)
    eng.stage1(1000)
    lines = eng.save_lines()
    assert len(lines) == batch
    eng.close()
    c = orc.orc_create(str(n).encode(), 52)
    line = ctypes.create_string_buffer(8192)
    for k in sorted({0, batch // 2, batch - 1}):
        orc.orc_stage1_line(c, sig[k], 1000, line, len(line), None, 0, None)
        assert line.value.decode() == lines[k]
    orc.orc_destroy(c)


def test_upload_points_roundtrip_and_reference_radix():
    """gecm_upload_points / gecm_download_points: vec operands in the reference's Montgomery radix"""
    import pyecm
    n = M[521]
    eng = pyecm.Engine(n)
    R = 1 << eng.cfg.maxbits
    rng = random.Random(3)
    xs = [rng.randrange(n) for _ in range(9)]
    zs = [rng.randrange(1, n) for _ in range(9)]
    ss = [rng.randrange(n) for _ in range(9)]
    eng.upload_points([x * R % n for x in xs], [z * R % n for z in zs], [s * R % n for s in ss])
    X, Z = eng.download_points()
    assert X == [x * R % n for x in xs] and Z == [z * R % n for z in zs]
    x, z = eng.download_points_plain()
    assert x == xs and z == zs
    eng.close()


ADVERSARIAL = [
    # K = 2^k N is the subtraction bias; these moduli put it at the two ends of its range [R/32, R/16)
    # and make every limb of N (hence every q*N product) maximal or minimal.
    ("2^415-1", (1 << 415) - 1),            # all-ones limbs, K just below R/16   (NL=15)
    ("2^414+1", (1 << 414) + 1),            # K just above R/32
    ("2^387+2^200+1", (1 << 387) + (1 << 200) + 1),   # smallest size that still needs NL=15
    ("2^639-1", (1 << 639) - 1),            # NL=23, the largest count without sub renormalisation
    ("2^723-1", (1 << 723) - 1),            # NL=26, the smallest count with it
    ("2^835-1", (1 << 835) - 1),            # NL=30, all-ones
    ("2^1031-1", (1 << 1031) - 1),          # NL=37, all-ones, largest supported size
]


@pytest.mark.parametrize("name,n", ADVERSARIAL, ids=[a[0] for a in ADVERSARIAL])
def test_extreme_moduli_against_oracle(orc, name, n):
    """lazy-reduction bounds (csrc/gecm_field.hpp) at their extremes: residues after 2,000+ point
    operations still equal the oracle's canonical ones"""
    import pyecm
    rng = random.Random(len(name))
    sig = [rng.randrange(6, 1 << 64) for _ in range(64)]
    eng = pyecm.Engine(n)
    eng.build_curves(sig)
    eng.stage1(1500)
    lines = eng.save_lines()
    R = 1 << eng.cfg.maxbits
    Ri = pow(R, -1, n)
    a = [n - 1, n - 1, 1, (n + 1) // 2, n - 2] + [rng.randrange(n) for _ in range(59)]
    b = [n - 1, 1, n - 1, (n - 1) // 2, n - 2] + [rng.randrange(n) for _ in range(59)]
    assert eng.vecmulmod(a, b) == [x * y * Ri % n for x, y in zip(a, b)]
    assert eng.vecsubmod(a, b) == [(x - y) % n for x, y in zip(a, b)]
    eng.close()
    c = orc.orc_create(str(n).encode(), 52)
    line = ctypes.create_string_buffer(16384)
    for k in range(0, 64, 7):
        orc.orc_stage1_line(c, sig[k], 1500, line, len(line), None, 0, None)
        assert line.value.decode() == lines[k], (name, sig[k])
    orc.orc_destroy(c)
