"""CPU tests (no GPU) of the extension planner: the tape of every extension segment, interpreted over
plain XZ arithmetic in Python integers, multiplies a point by k_std(to) / k_std(from); the segment rule under the
shortened prime range; gecm_resume_line_std_bound; and the bounds at the top of the B1 range.

The yardstick is tests/xladder.py: k_std(B) = stage1_multiplier(B + 1), points by ladder_point."""
import ctypes
import time

import pytest

from xladder import _primes, ladder_point, stage1_multiplier

GECM_OK, GECM_ERR_ARG = 0, -2
GECM_B1_MAX = 10 ** 12
P61 = (1 << 61) - 1          # the small curve's prime modulus

# csrc/gecm_tape.h
OP_PRAC_BEGIN, OP_PRAC_END, OP_STEP, OP_SWAP, OP_RULE_MASK = 1, 2, 8, 4, 3
RULE3, RULE4, RULE5, RULE9 = 0, 1, 2, 3


class Tape(ctypes.Structure):
    _fields_ = [("ops", ctypes.POINTER(ctypes.c_uint8)), ("len", ctypes.c_size_t), ("ptadds", ctypes.c_uint64),
                ("ptdups", ctypes.c_uint64), ("prac_calls", ctypes.c_uint64), ("last_prime", ctypes.c_uint64),
                ("rule_count", ctypes.c_uint64 * 4), ("swaps", ctypes.c_uint64)]


@pytest.fixture(scope="module")
def pyecm():
    import pyecm
    lib = pyecm.lib
    lib.gecm_tape_build_extend.argtypes = [ctypes.POINTER(Tape), ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int]
    lib.gecm_tape_free.argtypes = [ctypes.POINTER(Tape)]
    lib.gecm_tape_free.restype = None
    lib.gecm_extend_segment_bounds.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32,
                                               ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    lib.gecm_plan_set_prime_range_for_tests.argtypes = [ctypes.c_uint64]
    lib.gecm_plan_set_prime_range_for_tests.restype = None
    return pyecm


@pytest.fixture
def short_ranges(pyecm):
    yield pyecm.lib.gecm_plan_set_prime_range_for_tests
    pyecm.lib.gecm_plan_set_prime_range_for_tests(0)


def k_std(b):
    return stage1_multiplier(b + 1)


def e_p(p, x):
    e = 0
    while p ** (e + 1) <= x:
        e += 1
    return e


def _curve():
    """x and (A + 2) / 4 of the Suyama curve of sigma = 11 modulo P61"""
    n, s = P61, 11
    u, v = (s * s - 5) % n, 4 * s % n
    x = pow(u, 3, n) * pow(pow(v, 3, n), -1, n) % n
    a24 = pow(v - u, 3, n) * (3 * u + v) % n * pow(16 * pow(u, 3, n) * v % n, -1, n) % n
    return x, a24


def interpret(ops, A, a24, n=P61):
    """the tape ops of csrc/gecm_tape.h on the point A = (X, Z), as the device interpreter reads them"""
    def dbl(P):
        s, d = (P[0] + P[1]) ** 2 % n, (P[0] - P[1]) ** 2 % n
        t = (s - d) % n
        return s * d % n, t * (d + a24 * t) % n

    def add(P, Q, D):                   # P + Q, D = P - Q
        a, b = (P[0] - P[1]) * (Q[0] + Q[1]) % n, (P[0] + P[1]) * (Q[0] - Q[1]) % n
        return D[1] * (a + b) ** 2 % n, D[0] * (a - b) ** 2 % n

    B = C = A
    for op in ops:
        if op == OP_PRAC_BEGIN:
            B, C, A = A, A, dbl(A)
        elif op == OP_PRAC_END:
            A = add(A, B, C)
        else:
            assert op & OP_STEP
            if op & OP_SWAP:
                A, B = B, A
            rule = op & OP_RULE_MASK
            if rule == RULE3:
                B, C = add(B, A, C), B
            elif rule == RULE4:
                B, A = add(B, A, C), dbl(A)
            elif rule == RULE5:
                C, A = add(C, A, B), dbl(A)
            else:
                C, B = add(C, B, A), dbl(B)
    return A


def same_point(P, Q, n=P61):
    return (P[0] * Q[1] - Q[0] * P[1]) % n == 0 and P != (0, 0) and Q != (0, 0)


def build(pyecm, lo, hi, threads=2):
    t = Tape()
    assert pyecm.lib.gecm_tape_build_extend(ctypes.byref(t), lo, hi, threads) == 0
    ops = bytes(t.ops[i] for i in range(t.len))
    out = (ops, t.ptadds, t.ptdups, t.prac_calls, t.last_prime)
    pyecm.lib.gecm_tape_free(ctypes.byref(t))
    return out


def segments(pyecm, lo, hi):
    n = pyecm.extend_segments(lo, hi)
    out = []
    for s in range(n):
        a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
        assert pyecm.lib.gecm_extend_segment_bounds(lo, hi, s, ctypes.byref(a), ctypes.byref(b)) == 0
        d = pyecm.describe_extend(lo, hi, s)
        assert (d.lo, d.hi) == (a.value, b.value)
        out.append((a.value, b.value))
    return out


@pytest.mark.parametrize("lo,hi", [(1, 1000), (999, 3000), (1, 343), (342, 343), (1023, 1024), (960, 961), (996, 997),
                                   (500, 500)])
def test_tape_of_every_segment_multiplies_by_the_quotient(pyecm, lo, hi):
    x, a24 = _curve()
    assert segments(pyecm, lo, hi) == [(lo, hi)]
    ops, ptadds, ptdups, prac_calls, last_prime = build(pyecm, lo, hi)
    q, r = divmod(k_std(hi), k_std(lo))
    assert r == 0
    assert (len(ops) == 0) == (q == 1)
    assert same_point(interpret(ops, (x, 1), a24), ladder_point(P61, x, a24, q))
    odd = [p for p in _primes(hi) if p > 2]
    assert prac_calls == sum(e_p(p, hi) - e_p(p, lo) for p in odd)
    doublings = ops.count(OP_PRAC_BEGIN) - prac_calls
    assert doublings == e_p(2, hi) - e_p(2, lo)
    assert ops[:doublings] == bytes([OP_PRAC_BEGIN]) * doublings
    assert ptdups >= doublings and ptadds >= prac_calls
    gained = [p for p in odd if e_p(p, hi) > e_p(p, lo)]
    assert last_prime == (gained[-1] if gained else 2 if doublings else 0)
    d = pyecm.describe_extend(lo, hi, 0)
    assert d.nprimes == sum(1 for p in _primes(hi) if p > lo)
    assert d.nprimes + d.power_steps == prac_calls + doublings and d.last_prime == last_prime


def test_slices_compiled_on_threads_join_in_order(pyecm):
    assert build(pyecm, 1, 200000, 1) == build(pyecm, 1, 200000, 8)


def test_short_segments(pyecm, short_ranges):
    x, a24 = _curve()
    whole = interpret(build(pyecm, 1, 1000)[0], (x, 1), a24)
    short_ranges(256)
    assert segments(pyecm, 1, 1000) == [(1, 256), (256, 512), (512, 768), (768, 1000)]
    assert segments(pyecm, 256, 512) == [(256, 512)] and segments(pyecm, 255, 257) == [(255, 256), (256, 257)]
    assert segments(pyecm, 700, 700) == [(700, 700)]
    P = (x, 1)
    for lo, hi in segments(pyecm, 1, 1000):
        P = interpret(build(pyecm, lo, hi)[0], P, a24)
        assert same_point(P, ladder_point(P61, x, a24, k_std(hi)))      # a checkpoint is a standard point at hi
    assert same_point(P, whole)
    short_ranges(0)
    assert segments(pyecm, 1, 1000) == [(1, 1000)]


def test_std_bound_of_a_line(pyecm, short_ranges):
    lib = pyecm.lib
    line = "METHOD=ECM; SIGMA=1000; B1=1000; N=0x7fffffffffffffff; X=0x123; Z=0x45; PROGRAM=AVX-ECM;"
    assert pyecm.resume_line_std_bound(line) == 999
    assert pyecm.resume_line_std_bound(line + "\r\n") == 999
    assert pyecm.resume_line_std_bound(line.rstrip(";")) == 999
    for program in ("AVX-ECM-STD", "GMP-ECM 7.0.5"):
        std = line.replace("PROGRAM=AVX-ECM;", "PROGRAM=%s;" % program)
        assert pyecm.resume_line_std_bound(std) == 1000
        assert pyecm.resume_line_std_bound(std.rstrip(";") + "\r\n") == 1000
    assert pyecm.resume_line_std_bound(line.replace(" PROGRAM=AVX-ECM;", "")) == 1000
    assert pyecm.resume_line_std_bound("METHOD=ECM; PARAM=0; SIGMA=7; B1=3000; N=91; X=5; PROGRAM=GMP-ECM 7.0.5;") == 3000
    assert pyecm.resume_line_std_bound("# comment") is None and pyecm.resume_line_std_bound("") is None
    # a reference line above one prime range has no standard multiplier
    short_ranges(512)
    b = ctypes.c_uint64(77)
    assert lib.gecm_resume_line_std_bound(line.encode(), ctypes.byref(b)) == GECM_ERR_ARG and b.value == 77
    assert "a reference run over several prime ranges has no standard multiplier" in lib.gecm_last_error().decode()
    assert pyecm.resume_line_std_bound(line.replace("B1=1000", "B1=512")) == 511
    assert pyecm.resume_line_std_bound(line.replace("AVX-ECM;", "AVX-ECM-STD;")) == 1000     # a standard line is not bound by it
    short_ranges(0)
    assert pyecm.resume_line_std_bound(line.replace("B1=1000", "B1=100000000")) == 99999999
    with pytest.raises(pyecm.GecmError, match="several prime ranges"):
        pyecm.resume_line_std_bound(line.replace("B1=1000", "B1=100000001"))
    # what the parser refuses, this refuses
    with pytest.raises(pyecm.GecmError, match=r"\bfield X\b"):
        pyecm.resume_line_std_bound(line.replace("X=0x123; ", ""))
    with pytest.raises(pyecm.GecmError, match=r"\bfield B1\b"):
        pyecm.resume_line_std_bound(line.replace("B1=1000", "B1=1e3"))


def test_bounds_at_the_top_of_the_range(pyecm):
    ops, ptadds, ptdups, prac_calls, last_prime = build(pyecm, GECM_B1_MAX, GECM_B1_MAX)
    assert (ops, ptadds, ptdups, prac_calls, last_prime) == (b"", 0, 0, 0, 0)
    assert pyecm.extend_segments(GECM_B1_MAX, GECM_B1_MAX) == 1
    assert pyecm.extend_segments(1, GECM_B1_MAX) == 10 ** 4
    for bad in ((0, 10), (11, 10), (1, GECM_B1_MAX + 1)):
        with pytest.raises(pyecm.GecmError):
            pyecm.extend_segments(*bad)
    # the last stretch below 10^12: the base primes up to 10^6 and 1000 numbers are all that is sieved
    t0 = time.time()
    lo, hi = GECM_B1_MAX - 1000, GECM_B1_MAX
    d = pyecm.describe_extend(1, GECM_B1_MAX, 10 ** 4 - 1)
    assert (d.lo, d.hi) == (GECM_B1_MAX - 10 ** 8, GECM_B1_MAX)
    d = pyecm.describe_extend(lo, hi, 0)
    took = time.time() - t0
    small = _primes(10 ** 6)
    primes = [v for v in range(lo + 1, hi + 1) if all(v % p for p in small)]
    assert (d.lo, d.hi, d.nprimes, d.last_prime) == (lo, hi, len(primes), primes[-1])
    # 10^12 = 2^12 5^12 is itself no prime power beyond those: 2^39 < 10^12 < 2^40 and so on were all there at lo
    assert d.power_steps == sum(e_p(p, hi) - e_p(p, lo) for p in small)
    ops, _, _, prac_calls, last_prime = build(pyecm, lo, hi)
    assert prac_calls == len(primes) + d.power_steps and last_prime == primes[-1]
    assert took < 60                    # (sieving everything below 10^12 would take hours)
