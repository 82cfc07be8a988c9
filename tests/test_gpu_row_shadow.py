"""The 32-lane stage-1 kernel at one limb per lane (k_stage1_row<1, rows, false>) with the operand broadcasts of a point
addition's first and third multiply issued while the X <-> Z exchange that the multiply waits for is in flight
(avx-ecm_amd/csrc/gecm_row.hpp: fer_scan, fer_mul_scanned, row_add_scanned).  Those two multiplies now scan
the OTHER operand (the kept point's form, the difference point's coordinate), and the renaming picks that read the old C
have moved up behind its scan.

 1. every one-limb-per-lane shape (9, 11, 13, 15 and 16 rows) at the smallest and at the largest modulus of its limb class:
    64 curves (two curves per wavefront, 32 wavefronts), B1 = 2000 (rules 3, 4, 5 and 9, the begin and the end of every PRAC
    chain), the 32-lane layout forced, the kernel asserted by name, the save line of every curve (canonical X and Z) equal
    to the oracle's, byte for byte, as in tests/test_gpu_row_bias.py;
 2. a short tape on which a rule-5 step and a rule-9 step each follow a rule-3 step directly (its primes are searched from
    the tape builder): those steps fetch the old C's own coordinate from a C that the rule-3 step before renamed behind its
    scan.  Compared with the one-lane-per-curve layout of the same library on the same points, exact, as in
    tests/test_gpu_row_scaled.py."""
import ctypes
import os
import random

import pytest

import divsteps_model as M
from conftest import ROOT
from unit_model import OP_PRAC_BEGIN, OP_PRAC_END, OP_RULE_MASK, OP_STEP, OP_SWAP, RULE3, RULE5, RULE9, extend_tape

B1 = 2000
CURVES = 64
NQ1_EDGES = [(nl, bits) for nl, bits in M.edge_bits() if nl <= 15]       # 9, 11, 13, 15 and 16 rows: both ends of each class
PRIME_LIMIT = 120000


@pytest.fixture(scope="module")
def orc():
    L = ctypes.CDLL(os.path.join(ROOT, "oracle", "libecm_oracle.so"))
    L.orc_create.restype = ctypes.c_void_p
    L.orc_create.argtypes = [ctypes.c_char_p, ctypes.c_int]
    L.orc_destroy.argtypes = [ctypes.c_void_p]
    L.orc_stage1_line.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t,
                                  ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)]
    return L


def _oracle_lines(orc, n, sigmas):
    c = orc.orc_create(str(n).encode(), 52)
    line = ctypes.create_string_buffer(16384)
    out = []
    for s in sigmas:
        orc.orc_stage1_line(c, s, B1, line, len(line), None, 0, None)
        out.append(line.value.decode())
    orc.orc_destroy(c)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("nl,bits", NQ1_EDGES, ids=["nl%d_%dbit" % c for c in NQ1_EDGES])
def test_one_limb_shapes_at_both_ends_of_the_class(orc, nl, bits):
    import pyecm
    n = M.modulus(bits, "random")
    rng = random.Random("row shadow:%d" % bits)
    sig = [rng.randrange(6, 1 << 63) for _ in range(CURVES)]
    want = _oracle_lines(orc, n, sig)
    eng = pyecm.Engine(n, digitbits=52)
    assert eng.cfg.dev_limbs == nl
    eng.set_special_form(False)
    eng.set_lanes_per_curve(32)
    eng.build_curves(sig)
    eng.stage1(B1)
    assert eng.lanes_per_curve() == 32 and not eng.special_form_used()
    assert eng.last_kernel_name() == "k_stage1_row<1, %d, false>" % (nl + 1)
    got = eng.save_lines()
    eng.close()
    assert len(got) == CURVES
    differ = [k for k in range(CURVES) if got[k] != want[k]]
    assert not differ, (nl, bits, differ[:8])
    assert all("X=0x" in l and "Z=0x" in l for l in got)


def _primes_from(lo, limit):
    sieve = bytearray([1]) * limit
    sieve[0:2] = b"\0\0"
    for i in range(2, int(limit ** 0.5) + 1):
        if sieve[i]:
            sieve[i * i::i] = bytes(len(range(i * i, limit, i)))
    return [i for i in range(lo, limit) if sieve[i]]


def _follows_rule_3(ops, rule):
    """positions of a step of that rule whose predecessor is a rule-3 step (with or without swap)"""
    is3 = lambda o: o >= OP_STEP and o & OP_RULE_MASK == RULE3
    return [i for i in range(1, len(ops)) if ops[i] >= OP_STEP and ops[i] & OP_RULE_MASK == rule and is3(ops[i - 1])]


_FOUND = {}


def _tape_with_5_and_9_behind_3(lib):
    """(lo, hi, ops) of the shortest extension tape that has both a rule-5 and a rule-9 step directly behind a rule-3 step.
    Rule 9 behind rule 3 is rare (16 primes below 400,000) and no chain of a single prime below 400,000 has both, so the
    tape is that of the primes in (lo, hi]: hi the smallest prime with a rule 9 behind a rule 3, lo + 1 the nearest prime
    below it with a rule 5 behind a rule 3."""
    if not _FOUND:
        primes = _primes_from(11, PRIME_LIMIT)
        chain = lambda p: extend_tape(lib, p - 1, p)[0]
        i9 = next(i for i, p in enumerate(primes) if _follows_rule_3(chain(p), RULE9))
        i5 = next(i for i in range(i9 - 1, -1, -1) if _follows_rule_3(chain(primes[i]), RULE5))
        lo, hi = primes[i5] - 1, primes[i9]
        _FOUND["hit"] = (lo, hi, extend_tape(lib, lo, hi)[0])
    return _FOUND["hit"]


def test_the_tape_builder_has_such_a_tape():
    import pyecm
    lo, hi, ops = _tape_with_5_and_9_behind_3(pyecm.lib)
    assert hi - lo < 200 and ops[0] == OP_PRAC_BEGIN and ops[-1] == OP_PRAC_END
    i5, i9 = _follows_rule_3(ops, RULE5)[0], _follows_rule_3(ops, RULE9)[0]
    assert ops[i5 - 1] & ~OP_SWAP == OP_STEP | RULE3 and ops[i9 - 1] & ~OP_SWAP == OP_STEP | RULE3


@pytest.mark.gpu
@pytest.mark.parametrize("nl", [15, 8])
def test_rules_5_and_9_directly_behind_rule_3(nl):
    import pyecm
    lo, hi, ops = _tape_with_5_and_9_behind_3(pyecm.lib)
    n = M.modulus(M.LIMB * nl - 5, "random")
    rng = random.Random("5 and 9 behind 3:%d" % nl)
    eng = pyecm.Engine(n, digitbits=52)
    assert eng.cfg.dev_limbs == nl
    R = 1 << eng.cfg.maxbits
    X, Z, S = ([rng.randrange(1, n) * R % n for _ in range(CURVES)] for _ in range(3))
    eng.set_special_form(False)
    got = {}
    for lanes in (32, 1):
        eng.set_lanes_per_curve(lanes)
        eng.upload_points(X, Z, S)
        eng.stage1_extend(lo, hi)
        assert eng.lanes_per_curve() == lanes and not eng.special_form_used()
        if lanes == 32:
            assert eng.last_kernel_name() == "k_stage1_row<1, %d, false>" % (nl + 1)
        assert eng.stage1_stats().tape_len == len(ops)
        got[lanes] = eng.download_points()
    eng.close()
    for a, b in zip(got[32], got[1]):
        differ = [k for k in range(CURVES) if a[k] != b[k]]
        assert not differ, (lo, hi, differ[:8])
    assert got[32][0] != X and all(v < n for v in got[32][0] + got[32][1])
