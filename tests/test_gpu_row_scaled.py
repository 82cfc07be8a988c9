"""The 32-lane stage-1 kernel at one limb per lane (k_stage1_row<1, rows, false>) keeps every value of the tape
interpreter times 4, the scale the rows of its multiply read, keeps of a point its own and the other coordinate only, and
renames the points of a rule-3 step after the addition (avx-ecm_amd/csrc/gecm_row.hpp).  Where that can go wrong:

 1. the shortest tapes: B1 = 2 (empty), B1 = 3 (one doubling), and the smallest B1 whose tape has rules 4, 5 and 9, found
    from the tape builder;
 2. the end of a tape: one-prime tapes whose last step before PRAC_END is a rule 3 with and without swap, and, as no
    chain ends in another rule, the tapes on which rules 4, 5 and 9 come nearest to the end (the primes are searched on
    the CPU from the tape builder); and a stage 1 cut into launches as short as the tape allows;
 3. limbs at the ends of their ranges: a modulus whose multiple N' has 2^28 - 1 in all limbs but two, one with thirteen
    zero limbs, start points (N - 1, 1) and (1, N - 1); and on the CPU the bounds of the times-4 scale;
 4. 2 curves (one wavefront, most rows empty) and 130 curves (a partial last workgroup).

Every GPU comparison is between the 32-lane layout and the one-lane-per-curve layout of the same library on the same
curves, exact, as in tests/test_gpu_layouts.py."""
import ctypes
import random

import pytest

import divsteps_model as M
from unit_model import OP_PRAC_BEGIN, OP_PRAC_END, OP_RULE_MASK, OP_STEP, OP_SWAP, RULE3, RULE4, RULE5, RULE9, Tape, extend_tape

LIMB = M.LIMB
M28 = M.M28


def _row_kernel(nl):
    return "k_stage1_row<1, %d, false>" % (nl + 1)


def _modulus(nl):
    """the largest random modulus of that limb count (tests/test_gpu_layouts.py takes the same)"""
    return M.modulus(LIMB * nl - 5, "random")


def _stage1_tape(lib, b1):
    lib.gecm_tape_build_stage1.argtypes = [ctypes.POINTER(Tape), ctypes.c_uint64]
    lib.gecm_tape_free.argtypes = [ctypes.POINTER(Tape)]
    lib.gecm_tape_free.restype = None
    t = Tape()
    assert lib.gecm_tape_build_stage1(ctypes.byref(t), b1) == 0
    out = (bytes(t.ops[:t.len]), list(t.rule_count))
    lib.gecm_tape_free(ctypes.byref(t))
    return out


def _smallest_b1_with_rules_4_5_9(lib):
    """the tape of B1 holds the tape of every smaller B1's primes, so "has all three rules" is monotone: bisection"""
    has = lambda b1: all(_stage1_tape(lib, b1)[1][r] > 0 for r in (RULE4, RULE5, RULE9))
    lo, hi = 3, 1 << 12
    while not has(hi):
        lo, hi = hi, 2 * hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if has(mid) else (mid, hi)
    return hi


def _both_layouts(eng, nl, prepare, run, read):
    """read() after prepare() and run() in the 32-lane layout and in the one-lane layout"""
    got = {}
    for lanes in (32, 1):
        eng.set_lanes_per_curve(lanes)
        prepare()
        run()
        assert eng.lanes_per_curve() == lanes and not eng.special_form_used()
        if lanes == 32:
            assert eng.last_kernel_name() == _row_kernel(nl)
        got[lanes] = read()
    return got[32], got[1]


# ---- 1. the shortest tapes ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nl", [15, 8])
def test_shortest_tapes(nl):
    import pyecm
    b1_all = _smallest_b1_with_rules_4_5_9(pyecm.lib)
    ops2, ops3 = _stage1_tape(pyecm.lib, 2)[0], _stage1_tape(pyecm.lib, 3)[0]
    assert len(ops2) == 0 and set(ops3) <= {OP_PRAC_BEGIN, OP_PRAC_END} and len(ops3) >= 1
    rules = _stage1_tape(pyecm.lib, b1_all)[1]
    assert all(rules[r] >= 1 for r in (RULE3, RULE4, RULE5, RULE9)), (b1_all, rules)
    assert not all(_stage1_tape(pyecm.lib, b1_all - 1)[1][r] >= 1 for r in (RULE4, RULE5, RULE9))
    n = _modulus(nl)
    rng = random.Random("shortest tapes:%d" % nl)
    sig = [rng.randrange(6, 1 << 63) for _ in range(64)]             # one pair of wavefronts
    eng = pyecm.Engine(n, digitbits=52)
    assert eng.cfg.dev_limbs == nl
    eng.set_special_form(False)
    for b1 in (2, 3, 5, 7, b1_all):                              # 5: ends BEGIN, END (the prime 3); 7: one rule-3 step
        rows, one = _both_layouts(eng, nl, lambda: eng.build_curves(sig), lambda: eng.stage1(b1), eng.save_lines)
        differ = [k for k in range(len(sig)) if rows[k] != one[k]]
        assert not differ, (b1, differ[:8])
    eng.close()


# ---- 2. the end of a tape ----------------------------------------------------------------------------------------
# A launch's tape ends where a prime's chain ends (gecm_dev_set_tape cuts at PRAC_BEGIN bytes only: between chains only A
# is live), and a PRAC chain always ends in a rule-3 step, with or without swap, then PRAC_END: the Euclidean descent
# finishes on (d, e) = (2, 1) -> (1, 1), which rule 3 takes.  So "the last step is a rule 4, 5 or 9" does not exist on
# any tape the library can run (asserted below from the tape builder, for every prime below PRIME_LIMIT); what exists, and
# is run here, is the one-prime tape on which that rule comes NEAREST to the end, so that the points it makes reach the
# exit through the fewest renamings: rule 4 as the second-last step, rule 5 as the third-last, rule 9 as the fourth-last.
PRIME_LIMIT = 120000
LAST_STEPS = ("rule 3 with swap", "rule 3 without swap", "rule 4", "rule 5", "rule 9")
_CHAINS = {}


def _primes_below(limit):
    sieve = bytearray([1]) * limit
    sieve[0:2] = b"\0\0"
    for i in range(2, int(limit ** 0.5) + 1):
        if sieve[i]:
            sieve[i * i::i] = bytes(len(range(i * i, limit, i)))
    return [i for i in range(limit) if sieve[i]]


def _chain_ends(lib):
    """{case: (prime, ops, steps between the case's rule and PRAC_END)} over the one-prime tapes (the extension (p - 1, p])
    of every prime from 11 below PRIME_LIMIT, the smallest prime at the smallest distance; and the set of last steps seen"""
    if not _CHAINS:
        best, last_seen = {}, set()
        for p in _primes_below(PRIME_LIMIT):
            if p < 11:
                continue
            ops = extend_tape(lib, p - 1, p)[0]
            assert ops[0] == OP_PRAC_BEGIN and ops[-1] == OP_PRAC_END and all(o >= OP_STEP for o in ops[1:-1]), p
            last_seen.add(ops[-2])
            for case, rule, swap in (("rule 3 with swap", RULE3, True), ("rule 3 without swap", RULE3, False),
                                     ("rule 4", RULE4, None), ("rule 5", RULE5, None), ("rule 9", RULE9, None)):
                hit = [i for i in range(2, len(ops)) if ops[-i] & OP_RULE_MASK == rule
                       and (swap is None or bool(ops[-i] & OP_SWAP) == swap)]
                if hit and (case not in best or hit[0] - 1 < best[case][2]):
                    best[case] = (p, ops, hit[0] - 1)
        _CHAINS.update(best=best, last_seen=last_seen)
    return _CHAINS["best"], _CHAINS["last_seen"]


def test_every_chain_ends_in_rule_3():
    import pyecm
    best, last_seen = _chain_ends(pyecm.lib)
    assert last_seen == {OP_STEP | RULE3, OP_STEP | OP_SWAP | RULE3}
    assert {c: best[c][2] for c in LAST_STEPS} == {"rule 3 with swap": 1, "rule 3 without swap": 1, "rule 4": 2, "rule 5": 3,
                                                   "rule 9": 4}
    # the same on the tape of a whole stage 1: every PRAC_END follows a rule-3 step, or PRAC_BEGIN at once (the prime 3)
    ops = _stage1_tape(pyecm.lib, 20000)[0]
    before_end = {ops[i - 1] for i in range(len(ops)) if ops[i] == OP_PRAC_END}
    assert before_end == {OP_PRAC_BEGIN, OP_STEP | RULE3, OP_STEP | OP_SWAP | RULE3}


@pytest.mark.gpu
@pytest.mark.parametrize("last", LAST_STEPS)
def test_end_of_tape_roles(last):
    import pyecm
    nl = 15
    p, ops, _ = _chain_ends(pyecm.lib)[0][last]
    n = _modulus(nl)
    rng = random.Random("end of tape:%s" % last)
    cnt = 64
    eng = pyecm.Engine(n, digitbits=52)
    assert eng.cfg.dev_limbs == nl
    R = 1 << eng.cfg.maxbits
    X, Z, S = ([rng.randrange(1, n) * R % n for _ in range(cnt)] for _ in range(3))
    eng.set_special_form(False)
    rows, one = _both_layouts(eng, nl, lambda: eng.upload_points(X, Z, S), lambda: eng.stage1_extend(p - 1, p),
                              eng.download_points)
    assert eng.stage1_stats().tape_len == len(ops)
    eng.close()
    for a, b in zip(rows, one):
        differ = [k for k in range(cnt) if a[k] != b[k]]
        assert not differ, (last, p, differ[:8])
    assert rows[0] != X and all(v < n for v in rows[0] + rows[1])


@pytest.mark.gpu
def test_every_launch_as_short_as_the_tape_allows():
    """the hook for cut tapes (GECM_TAPE_CHUNK, tests/test_gpu_multirange.py) at its smallest value: every launch ends at
    the first chain end it can, so the exit runs after chains of every length, ending with and without swap"""
    import os
    import pyecm
    nl = 15
    n = _modulus(nl)
    sig = list(range(5000, 5064))
    eng = pyecm.Engine(n, digitbits=52)
    eng.set_special_form(False)
    out = {}
    try:
        for chunk in (0, 4):
            if chunk:
                os.environ["GECM_TAPE_CHUNK"] = str(chunk)
            out[chunk] = _both_layouts(eng, nl, lambda: eng.build_curves(sig), lambda: eng.stage1(600), eng.save_lines)
    finally:
        os.environ.pop("GECM_TAPE_CHUNK", None)
        eng.close()
    assert out[0][0] == out[0][1] == out[4][0] == out[4][1]


# ---- 3. limbs at the ends of their ranges ------------------------------------------------------------------------
def _row_multiple(n):
    """N' = m N = -1 mod 2^28, the modulus of the row kernel (gecm_row.hpp)"""
    m = (-pow(n, -1, 1 << LIMB)) % (1 << LIMB)
    return m * n


def _limbs(v, cnt=16):
    return [(v >> (LIMB * i)) & M28 for i in range(cnt)]


def _full_limbs_modulus():
    """415 bits, N = 1 mod 2^28, so m = 2^28 - 1 and N' = m N lies within 2^57 of 2^442: every limb of N' but limbs 1 and 15
    is 2^28 - 1 (limb 15 is the top one: 2^22 - 1, all the bits a 442-bit N' has there)"""
    m = (1 << LIMB) - 1
    n = ((1 << 442) - 1) // m
    n -= (n - 1) % (1 << LIMB)
    return n


def _zero_limbs_modulus():
    """415 bits, N = -1 mod 2^28, so m = 1 and N' = N = 2^414 + 2^28 - 1: limbs 1 to 13 are zero"""
    return (1 << 414) + (1 << LIMB) - 1


def test_extreme_moduli_are_what_they_claim():
    n = _full_limbs_modulus()
    assert n.bit_length() == 415 and n & 1 and M.dev_limbs(415) == 15
    l = _limbs(_row_multiple(n))
    assert [i for i in range(16) if l[i] != M28] == [1, 15] and l[15] == (1 << 22) - 1
    n = _zero_limbs_modulus()
    assert n.bit_length() == 415 and _row_multiple(n) == n
    l = _limbs(n)
    assert l[0] == M28 and l[1:14] == [0] * 13 and l[14] == 1 << 22 and l[15] == 0


def test_scale_4_fits_the_signed_multiplier_operand():
    """gecm_row.hpp, on Python integers.  A multiply delivers limbs in [-2^27 - 4, 2^27 + 4] (its documented bound); the
    forms the point formulas feed to a multiply are sums or differences of two such values, limb by limb: row_sd, row_ds,
    e = t +- w (row_add), w = t - q and t = r1 + q (row_dup).  Four times the largest of them must fit v_mad_i64_i32's
    signed 32-bit operand, and so must four times anything within fer_mul's operand bound |.| < 2^29."""
    product = (1 << 27) + 4
    form = 2 * product
    assert form < 1 << 29
    assert 4 * form == (1 << 30) + 32 and 4 * form < 1 << 31 and -4 * form >= -(1 << 31)
    assert 4 * ((1 << 29) - 1) < 1 << 31 and -4 * ((1 << 29) - 1) >= -(1 << 31)
    # the end of a multiply in the scaled form against the plain one: the accumulator T (64 bits, signed) is a multiple
    # of 16; limb = ((T + 2^31 mod 2^32) >> 4) - 2^27, carry = (T + 2^31) >> 32; scaled: the low word read as signed,
    # shifted right by 2 arithmetically, is 4 x limb
    i32 = lambda x: (x & 0xffffffff) - ((x & 0x80000000) << 1)
    lows = [0, 16, (1 << 31) - 16, 1 << 31, (1 << 31) + 16, (1 << 32) - 16, 0x12345670, 0xfedcba90]
    for hi in (-(1 << 31), -5, -1, 0, 1, 7, (1 << 31) - 1):
        for lo in lows:
            t = (hi << 32) + lo
            u = t + (1 << 31)
            limb = (((u & 0xffffffff) >> 4) & M28) - (1 << 27)
            carry = u >> 32
            assert limb + (carry << 28) == t >> 4 and -(1 << 27) <= limb < 1 << 27
            assert i32(t) >> 2 == 4 * limb
            for below in (-8, -1, 0, 1, 8):                       # the neighbour's carry enters times 4
                assert i32((i32(t) >> 2) + (below << 2)) == 4 * (limb + below)


@pytest.mark.gpu
@pytest.mark.parametrize("modulus", ["full limbs", "zero limbs"])
def test_limbs_at_the_ends_of_their_ranges(modulus):
    import pyecm
    nl = 15
    n = _full_limbs_modulus() if modulus == "full limbs" else _zero_limbs_modulus()
    rng = random.Random("extreme limbs:%s" % modulus)
    b1 = 300
    pts = [(n - 1, 1), (1, n - 1)]
    svals = [1, n - 1, (n - 1) // 2] + [rng.randrange(2, n - 1) for _ in range(5)]
    pts = [(x, z, s) for x, z in pts for s in svals]
    eng = pyecm.Engine(n, digitbits=52)
    assert eng.cfg.dev_limbs == nl
    R = 1 << eng.cfg.maxbits
    X, Z, S = ([v[j] * R % n for v in pts] for j in range(3))
    eng.set_special_form(False)
    read = lambda: eng.download_points() + eng.download_points_plain()
    rows, one = _both_layouts(eng, nl, lambda: eng.upload_points(X, Z, S), lambda: eng.stage1(b1), read)
    eng.close()
    for a, b in zip(rows, one):
        differ = [k for k in range(len(pts)) if a[k] != b[k]]
        assert not differ, (modulus, differ[:8])
    assert all(v < n for part in rows for v in part)


# ---- 4. sizes ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("curves", [2, 130])
def test_batch_sizes(curves):
    import pyecm
    nl = 15
    n = _modulus(nl)
    rng = random.Random("sizes:%d" % curves)
    sig = [rng.randrange(6, 1 << 63) for _ in range(curves)]
    b1 = rng.randrange(300, 401)
    eng = pyecm.Engine(n, digitbits=52)
    eng.set_special_form(False)
    rows, one = _both_layouts(eng, nl, lambda: eng.build_curves(sig), lambda: eng.stage1(b1), eng.save_lines)
    eng.close()
    assert len(rows) == len(one) == curves
    differ = [k for k in range(curves) if rows[k] != one[k]]
    assert not differ, (curves, b1, differ[:8])
