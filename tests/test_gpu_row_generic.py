"""The events of the 32-lane stage-1 kernel at one limb per lane that are not rule-3 steps (avx-ecm_amd/csrc/gecm_row.hpp:
run_tape_row_dpp, row_dup_scanned): the begin and the end of a PRAC chain and the add-and-double steps of
rules 4, 5 and 9 are three paths of their own, an add-and-double step renames by conditional moves, reads ONE scan of fA in
its addition and in its double, fetches C's own coordinate on rules 5 and 9 alone, and treats rule 9 as rule 5 with A and B
exchanged before and after.

The tape is the shortest extension tape (primes searched from the tape builder, as tests/test_gpu_row_shadow.py does)
that has every transition this code treats differently: rules 4, 5 and 9 each with and without the swap bit, each
directly behind a rule-3 step and directly behind another event that is not one, a rule-3 step directly behind rule 4 and
behind rule 5, the end of a chain followed by the begin of the next, and a begin on a word boundary, where the tape-cut
hook can start a launch.  Two things about that search:

 * rule 9 without the swap bit is rare: 5 primes below 8,000,000 have one, none below 1,000,000, so the search window is
   the thousand numbers around the first of them whose chain has all of the rest as well (6,720,533: 33 events);
 * a rule-3 step never follows rule 9 directly.  PRAC takes rule 9 (e even: e <- e / 2) only where rule 3 does not
   apply, d >= 4e; behind it d >= 8e, and rule 3 still does not apply.  No chain of a prime below 8,000,000 has one.  The
   test asserts that the tape has none, so that a change of the tape builder that makes one possible shows up here.

The yardstick is exact: Python integers, the plain binary ladder of tests/xladder.py on the Suyama curve of every sigma,
as in tests/test_gpu_extend.py (the C oracle has no entry for an extension); the projective points are compared by cross
multiplication.  70 curves (a ragged batch: two curves per wavefront, more than one wavefront), the 16-row shape (a
415-bit N) and the 9-row shape (the smallest one-limb class), the 32-lane layout forced and the kernel asserted by name.

 1. primes: the tape in one launch;
 2. cut: the same tape cut into launches by the tape-cut hook (GECM_TAPE_CHUNK = 4, its smallest).  The hook starts a
    launch only at a begin on a word boundary, because a launch hands over the point A alone: a cut behind any other
    event is not something the kernels can run, so the state handed over is that behind the end of a chain;
 3. layout: the same curves through one lane per curve give the same save lines."""
import math
import random

import pytest

from unit_model import OP_PRAC_BEGIN, OP_PRAC_END, OP_RULE_MASK, OP_STEP, OP_SWAP, RULE3, RULE4, RULE5, RULE9, extend_tape
from xladder import _primes, ladder_point

CURVES = 70
WINDOW = (6720000, 6721000)
SHAPES = [15, 8]                        # device limbs: 16 rows (415 bits) and 9 rows (219 bits)
GENERIC = (RULE4, RULE5, RULE9)
WANT = ({("op", r, s) for r in GENERIC for s in (False, True)}
        | {(k, r) for k in ("behind rule 3", "behind generic") for r in GENERIC}
        | {("rule 3 behind", RULE4), ("rule 3 behind", RULE5), ("end, begin",), ("begin on a word boundary",)})


def _is3(o):
    return o >= OP_STEP and o & OP_RULE_MASK == RULE3


def transitions(ops):
    f = set()
    for i, o in enumerate(ops):
        if o >= OP_STEP and not _is3(o):
            r = o & OP_RULE_MASK
            f.add(("op", r, bool(o & OP_SWAP)))
            if i:
                f.add(("behind rule 3" if _is3(ops[i - 1]) else "behind generic", r))
            if i + 1 < len(ops) and _is3(ops[i + 1]):
                f.add(("rule 3 behind", r))
        if o == OP_PRAC_BEGIN and i:
            if ops[i - 1] == OP_PRAC_END:
                f.add(("end, begin",))
            if i % 4 == 0:
                f.add(("begin on a word boundary",))
    return f


_FOUND = {}


def _tape(lib):
    """(lo, hi, ops, primes) of the shortest extension tape of consecutive primes of the window with every transition of
    WANT, or None"""
    if "hit" not in _FOUND:
        small = _primes(int(WINDOW[1] ** 0.5) + 1)
        primes = [p for p in range(*WINDOW) if all(p % q for q in small)]
        best = None
        for i in range(len(primes)):
            for j in range(i + 1, min(i + 8, len(primes))):
                lo, hi = primes[i] - 1, primes[j]
                ops = extend_tape(lib, lo, hi)[0]
                if best is not None and len(ops) >= len(best[2]):
                    break
                if WANT <= transitions(ops):
                    best = (lo, hi, ops, primes[i:j + 1])
        _FOUND["hit"] = best
    return _FOUND["hit"]


def test_the_tape_has_every_transition():
    import pyecm
    hit = _tape(pyecm.lib)
    assert hit is not None, "no run of consecutive primes in %r has every transition" % (WINDOW,)
    lo, hi, ops, primes = hit
    got = transitions(ops)
    assert WANT <= got, WANT - got
    assert ("rule 3 behind", RULE9) not in got           # (see above: PRAC cannot make one)
    assert ops[0] == OP_PRAC_BEGIN and ops[-1] == OP_PRAC_END and len(ops) < 200
    assert ops.count(OP_PRAC_BEGIN) == len(primes) >= 2     # one chain per prime: no prime power in (lo, hi]


def _launch_starts(ops, chunk):
    """the offsets at which gecm_dev_set_tape starts a launch"""
    cuts, want = [0], chunk
    while want < len(ops):
        off = (want + 3) & ~3
        while off < len(ops) and ops[off] != OP_PRAC_BEGIN:
            off += 4
        if off >= len(ops):
            break
        cuts.append(off)
        want = off + chunk
    return cuts


def _modulus(nl):
    """the first odd number of 28 nl - 5 bits from a seed on that no prime below 10^5 divides (every Z has an inverse)"""
    bits = 28 * nl - 5
    small = math.prod(_primes(10 ** 5))
    n = random.Random("row generic:%d" % nl).getrandbits(bits) | (1 << (bits - 1)) | 1
    while math.gcd(n, small) != 1:
        n += 2
    return n


_CASES = {}


def _case(nl):
    """(n, sigmas, [(X, Z)] of the exact ladder), made once per shape and left unchanged"""
    if nl not in _CASES:
        import pyecm
        lo, hi, ops, primes = _tape(pyecm.lib)
        n = _modulus(nl)
        rng = random.Random("row generic sigmas:%d" % nl)
        sig = [rng.randrange(6, 1 << 63) for _ in range(CURVES)]
        k = math.prod(primes)
        want = []
        for s in sig:
            u, v = (s * s - 5) % n, 4 * s % n
            x = pow(u, 3, n) * pow(pow(v, 3, n), -1, n) % n
            a24 = pow(v - u, 3, n) * (3 * u + v) % n * pow(16 * pow(u, 3, n) * v % n, -1, n) % n
            want.append(ladder_point(n, x, a24, k))
        _CASES[nl] = (n, sig, want)
    return _CASES[nl]


def _run(nl, lanes):
    """(plain X, plain Z, save lines, launches) of the curves of the case after the tape"""
    import pyecm
    lo, hi, ops, primes = _tape(pyecm.lib)
    n, sig, want = _case(nl)
    eng = pyecm.Engine(n, digitbits=52)
    assert eng.cfg.dev_limbs == nl
    eng.set_special_form(False)
    eng.set_lanes_per_curve(lanes)
    eng.build_curves(sig)
    eng.stage1_extend(lo, hi)
    assert eng.lanes_per_curve() == lanes and not eng.special_form_used()
    if lanes == 32:
        assert eng.last_kernel_name() == "k_stage1_row<1, %d, false>" % (nl + 1)
    assert eng.stage1_stats().tape_len == len(ops)
    launches = eng.stage1_progress()
    X, Z = eng.download_points_plain()
    lines = eng.save_lines()
    eng.close()
    return X, Z, lines, launches


def _assert_points(nl, X, Z):
    n, sig, want = _case(nl)
    assert len(X) == len(Z) == CURVES
    differ = [k for k in range(CURVES) if Z[k] % n == 0 or (X[k] * want[k][1] - want[k][0] * Z[k]) % n]
    assert not differ, (nl, differ[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("nl", SHAPES)
def test_primes(nl):
    X, Z, lines, launches = _run(nl, 32)
    assert launches == (1, 1)
    _assert_points(nl, X, Z)


@pytest.mark.gpu
@pytest.mark.parametrize("nl", SHAPES)
def test_cut(nl, monkeypatch):
    import pyecm
    ops = _tape(pyecm.lib)[2]
    starts = _launch_starts(ops, 4)
    assert len(starts) >= 2 and all(ops[s] == OP_PRAC_BEGIN and ops[s - 1] == OP_PRAC_END for s in starts[1:])
    monkeypatch.setenv("GECM_TAPE_CHUNK", "4")
    X, Z, lines, launches = _run(nl, 32)
    assert launches == (len(starts), len(starts))
    _assert_points(nl, X, Z)


@pytest.mark.gpu
@pytest.mark.parametrize("nl", SHAPES)
def test_layout(nl):
    X32, Z32, lines32, _ = _run(nl, 32)
    X1, Z1, lines1, _ = _run(nl, 1)
    _assert_points(nl, X1, Z1)
    assert lines32 == lines1 and all("X=0x" in l and "Z=0x" in l for l in lines32)
