"""GPU tests of resume: plain residues of save and checkpoint lines go back into a context through the
device conversion (k_to_mont / k_to_mont_multi), on single-N, special-form and multi-modulus contexts, and what runs
from there — the remaining prime ranges, stage 2 — equals the reference's files, the oracle and an uninterrupted run."""
import ctypes
import json
import os
import random
import re

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

GECM_ERR_ARG, GECM_ERR_STATE = -2, -4
LIMBS = [8, 10, 12, 14, 15, 17, 19, 21, 23, 26, 28, 30, 32, 34, 37]
S1 = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "stage1.json")))}
MR = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "multirange.json")))}
S2 = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "stage2_acc.json")))}
BATCHES = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "batches.json")))}


def _oracle():
    L = ctypes.CDLL(os.path.join(ROOT, "oracle", "libecm_oracle.so"))
    L.orc_create.restype = ctypes.c_void_p
    L.orc_create.argtypes = [ctypes.c_char_p, ctypes.c_int]
    L.orc_destroy.argtypes = [ctypes.c_void_p]
    L.orc_stage1_ranges_line.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                         ctypes.c_int, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
                                         ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int)]
    L.orc_stage1_line.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t,
                                  ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)]
    return L


class Oracle:
    """the CPU restatement of the reference on one N: resume lines after `stop_after` ranges (0: the save line)"""

    def __init__(self, n, digitbits=52):
        self.L = _oracle()
        self.c = self.L.orc_create(str(n).encode(), digitbits)

    def line(self, sigma, b1, prange, stop_after):
        buf = ctypes.create_string_buffer(8192)
        self.L.orc_stage1_ranges_line(self.c, sigma, b1, b1, prange, stop_after, 0 if stop_after else b1, buf, len(buf), None, 0,
                                      None, None)
        return buf.value.decode()

    def save_line(self, sigma, b1):
        buf = ctypes.create_string_buffer(8192)
        self.L.orc_stage1_line(self.c, sigma, b1, buf, len(buf), None, 0, None)
        return buf.value.decode()

    def close(self):
        self.L.orc_destroy(self.c)


@pytest.fixture
def short_ranges():
    import pyecm
    hook = pyecm.lib.gecm_plan_set_prime_range_for_tests
    hook.argtypes = [ctypes.c_uint64]
    hook.restype = None
    yield hook
    hook(0)


def _top_of_class(nl):
    """an odd modulus at the top of the limb class: R = 2^(28 nl) >= 32 N"""
    return (1 << (28 * nl - 5)) - 1 - 2 * random.Random(nl).randrange(1 << 20)


def _residues(n, count, rnd, rot=0):
    """count pairs (x, z): first the edge values 0, 1, N-1, each x paired with another edge value as z and the pairing
    rotated by rot, so that a batch of 1 meets them too; random values after them"""
    edge = [0, 1, n - 1]
    xs = [edge[(k + rot) % 3] for k in range(3)] + [rnd.randrange(n) for _ in range(count)]
    zs = [edge[(k + rot + 2) % 3] for k in range(3)] + [rnd.randrange(n) for _ in range(count)]
    xs, zs = xs[:count], zs[:count]
    if count >= 3:
        assert {0, 1, n - 1} <= set(xs) and {0, 1, n - 1} <= set(zs)
    return xs, zs


def _line_fields(line):
    return int(re.search(r"X=0x([0-9a-f]+);", line).group(1), 16), int(re.search(r"Z=0x([0-9a-f]+);", line).group(1), 16)


# ---- 1. the conversion alone -------------------------------------------------------------------------------------
@pytest.mark.parametrize("nl", LIMBS)
def test_conversion_returns_the_residues_given(nl):
    import pyecm
    n = _top_of_class(nl)
    eng = pyecm.Engine(n)
    assert eng.cfg.dev_limbs == nl
    rnd = random.Random(1000 + nl)
    for rot, batch in enumerate((1, 63, 65)):
        xs, zs = _residues(n, batch, rnd, rot)
        sig = [rnd.randrange(6, 1 << 64) for _ in range(batch)]
        eng.resume(sig, xs, zs, b1_done=2)
        assert eng.download_points_plain() == (xs, zs), batch
        for k in {0, batch // 2, batch - 1}:
            line = eng.save_line(k)
            assert _line_fields(line) == (xs[k], zs[k])
            assert line.startswith("METHOD=ECM; SIGMA=%d; B1=2; N=0x%x; " % (sig[k], n))
    eng.close()


def _three_numbers(nl, rnd):
    """three numbers of different bit lengths in the limb class of nl limbs"""
    top = 28 * nl - 5
    return [rnd.getrandbits(b) | (1 << (b - 1)) | 1 for b in (top - 20, top - 9, top)]


@pytest.mark.parametrize("nl", [8, 15, 37])
def test_conversion_on_a_multi_modulus_context(nl):
    import pyecm
    rnd = random.Random(2000 + nl)
    ns = _three_numbers(nl, rnd)
    eng = pyecm.MultiEngine(ns)
    assert eng.cfg.dev_limbs == nl
    for counts in ((1, 1, 1), (63, 1, 65), (5, 64, 70)):
        which = [g for g, c in enumerate(counts) for _ in range(c)]
        rnd.shuffle(which)
        xs, zs = [], []
        per = {g: _residues(ns[g], c, rnd, g) for g, c in enumerate(counts)}
        seen = [0, 0, 0]
        for g in which:
            xs.append(per[g][0][seen[g]])
            zs.append(per[g][1][seen[g]])
            seen[g] += 1
        sig = [rnd.randrange(6, 1 << 64) for _ in which]
        eng.resume(sig, which, xs, zs, b1_done=2)
        for k in range(len(which)):
            line = eng.save_line(k)
            assert _line_fields(line) == (xs[k], zs[k]), (counts, k)
            assert "SIGMA=%d; B1=2; N=0x%x; " % (sig[k], ns[which[k]]) in line
    eng.close()


# ---- 2. the reference's bytes ------------------------------------------------------------------------------------
def test_single_range_checkpoint_of_the_reference_is_the_final_residue():
    import pyecm
    c = MR["n204_b1_1e8_single_range_checkpoint"]
    b1 = c["B1"]
    field = pyecm.parse_resume_line(c["checkpoint_lines"][0]).b1
    assert pyecm.stage1_resume_range(b1, field) == pyecm.stage1_ranges(b1) == 1
    eng = pyecm.Engine(pyecm.parse_resume_line(c["checkpoint_lines"][0]).n)
    eng.resume_lines(c["checkpoint_lines"], b1_done=b1)
    assert [l.rstrip("\n") for l in eng.save_lines()] == [l.rstrip("\n") for l in c["save_lines"]]
    with pytest.raises(pyecm.GecmError):
        eng.stage1_stats()                     # no stage-1 launch was made
    eng.close()


def test_checkpoint_of_the_reference_resumed_through_the_last_range():
    """range 1 of B1 = 1.1e8: 541,911 primes on the reference's own checkpoint lines; the save lines are its bytes"""
    import pyecm
    c = MR["n204_b1_1.1e8"]
    b1 = c["B1"]
    rec = pyecm.parse_resume_line(c["checkpoint_lines"][0])
    assert pyecm.stage1_resume_range(b1, rec.b1) == 1 and pyecm.stage1_ranges(b1) == 2
    eng = pyecm.Engine(rec.n)
    eng.resume_lines(c["checkpoint_lines"])
    eng.stage1_range(b1, 1)
    assert [l.rstrip("\n") for l in eng.save_lines()] == [l.rstrip("\n") for l in c["save_lines"]]
    eng.close()


# ---- 3. checkpoint resume against the oracle, every layout -------------------------------------------------------
_ORACLE_LINES = {}


def _oracle_lines(bits, b1, prange, sig):
    """per stop_after (0 = final) the oracle's lines of every curve; computed once per case"""
    key = (bits, b1, prange)
    if key not in _ORACLE_LINES:
        n = random.Random(bits).getrandbits(bits) | (1 << (bits - 1)) | 1
        o = Oracle(n)
        nr = -(-b1 // prange)
        _ORACLE_LINES[key] = (n, {r: [o.line(s, b1, prange, r) for s in sig] for r in range(1, nr)},
                              {k: o.line(sig[k], b1, prange, 0) for k in (0, 1, 63, 64, 69)})
        o.close()
    return _ORACLE_LINES[key]


@pytest.mark.parametrize("lanes", [1, 2, 8, 32])
@pytest.mark.parametrize("bits,b1,prange", [(415, 5000, 2000), (200, 2500, 1250), (729, 2013, 503)])
def test_checkpoint_resume_against_the_oracle(short_ranges, bits, b1, prange, lanes):
    import pyecm
    short_ranges(prange)
    sig = list(range(1000, 1000 + 70))
    n, per_range, final = _oracle_lines(bits, b1, prange, sig)
    nr = pyecm.stage1_ranges(b1)
    assert nr == -(-b1 // prange) and nr >= 2
    eng = pyecm.Engine(n)
    if lanes == 32 and eng.cfg.dev_limbs < 10:
        lanes = 8
    eng.set_lanes_per_curve(lanes)
    eng.build_curves(sig)
    eng.stage1(b1)
    whole = eng.save_lines()
    for r in range(1, nr):
        field = pyecm.parse_resume_line(per_range[r][0]).b1
        if field:                                            # (a range without any prime writes the field 0)
            assert pyecm.stage1_resume_range(b1, field) == r
        fresh = pyecm.Engine(n)
        fresh.set_lanes_per_curve(lanes)
        fresh.resume_lines(per_range[r])
        for rr in range(r, nr):
            fresh.stage1_range(b1, rr)
        got = fresh.save_lines()
        fresh.close()
        for k, want in final.items():
            assert got[k] == want, (r, k)
        assert got == whole, r
    eng.close()


# ---- 4. stage 2 from save lines, against the reference's stg2acc -------------------------------------------------
def _reference_save_lines(case):
    for fx in list(S1.values()) + list(BATCHES.values()):
        if fx["B1"] == case["B1"] and fx["sigma0"] == case["sigma0"] and fx["digitbits"] == case["digitbits"] and \
                fx["N"] == case["N"] and len(fx["save_lines"]) >= case["curves"]:
            return fx["save_lines"][:case["curves"]]
    return None


@pytest.mark.parametrize("name", ["K1N_b1_2000_b2_1e5", "T35N_b1_1000_b2_50000", "M607xM127xM89_b1_800_b2_40000",
                                  "K1N_d32_b1_300_b2_20000", "T35_46_b1_1e6_b2_1e8"])
def test_stage2_from_save_lines(name):
    import pyecm
    case = S2[name]
    lines = _reference_save_lines(case)
    if name == "T35_46_b1_1e6_b2_1e8":
        assert lines is not None            # the reference's own save lines are in stage1.json (T35_46)
    n = int(case["N"]) if lines is None else pyecm.parse_resume_line(lines[0]).n
    if lines is None:
        o = Oracle(n, case["digitbits"])
        lines = [o.save_line(case["sigma0"] + k, case["B1"]) for k in range(case["curves"])]
        o.close()
    eng = pyecm.Engine(n, digitbits=case["digitbits"])
    eng.resume_lines(lines, b1_done=case["B1"])
    eng.stage2(case["B2"], case["D"], case["U"])
    st = eng.stage2_stats()
    assert (st.D, st.U, st.L) == (case["D"], case["U"], case["L"])
    assert [st.ptadds, st.numinv, st.paired] == case["stage2_counts"]
    assert eng.download_acc() == [int(h, 16) for h in case["acc_hex"]]
    found = {int(re.search(r"vec (\d+),", l).group(1)): int(re.search(r"factor (\d+) in stage 2", l).group(1))
             for l in case["results_lines"] if "in stage 2" in l}
    if name == "T35_46_b1_1e6_b2_1e8":
        assert found
    for k in range(case["curves"]):
        f = eng.stage2_factor(k)
        assert (f[0] if f else None) == found.get(k), k
    eng.close()


# ---- 5. multi-modulus ---------------------------------------------------------------------------------------------
def test_multi_modulus_resume_equals_single_contexts_and_the_oracle(short_ranges):
    import pyecm
    b1, prange, b2 = 2500, 1000, 60000
    short_ranges(prange)
    rnd = random.Random(55)
    ns = [rnd.getrandbits(b) | (1 << (b - 1)) | 1 for b in (380, 400, 415)]
    counts = (5, 64, 70)
    which = [g for g, c in enumerate(counts) for _ in range(c)]
    rnd.shuffle(which)
    sig = [3000 + k for k in range(len(which))]
    orcs = [Oracle(n) for n in ns]
    after0 = [orcs[g].line(s, b1, prange, 1) for g, s in zip(which, sig)]
    final = [orcs[g].line(s, b1, prange, 0) for g, s in zip(which, sig)]
    for o in orcs:
        o.close()
    assert pyecm.stage1_resume_range(b1, pyecm.parse_resume_line(after0[0]).b1) == 1
    multi = pyecm.MultiEngine(ns)
    multi.resume_lines(after0)
    assert [multi.modulus_of(k) for k in range(len(which))] == which
    with pytest.raises(pyecm.GecmError, match="stage 1"):
        multi.stage2_init()
    for r in (1, 2):
        multi.stage1_range(b1, r)
    got = multi.save_lines()
    assert got == final
    multi.stage2(b2)
    accs = multi.accs()
    multi.close()
    for g, n in enumerate(ns):
        mine = [k for k, w in enumerate(which) if w == g]
        eng = pyecm.Engine(n)
        eng.resume_lines([after0[k] for k in mine])
        for r in (1, 2):
            eng.stage1_range(b1, r)
        assert eng.save_lines() == [got[k] for k in mine]
        eng.stage2(b2)
        assert eng.download_acc() == [accs[k] for k in mine], g
        eng.close()


# ---- 6. states and errors -----------------------------------------------------------------------------------------
def test_states_and_errors():
    import pyecm
    lib = pyecm.lib
    p, q = (1 << 89) - 1, (1 << 107) - 1
    n = p * q
    eng = pyecm.Engine(n)
    sig = [100, 101, 102]
    eng.build_curves(sig)
    eng.stage1(500)
    before = eng.save_lines()
    one = lambda v: eng.pack([v, 1, 1])
    arr = (ctypes.c_uint64 * 3)(*sig)
    # sigma 5 and x = N are refused before the old batch is dropped
    bad_sigma = (ctypes.c_uint64 * 3)(100, 5, 102)
    assert lib.gecm_resume_points(eng._h, bad_sigma, one(1), one(1), 3, 0) == GECM_ERR_ARG
    assert "sigma[1]" in lib.gecm_last_error().decode()
    assert lib.gecm_resume_points(eng._h, arr, one(n), one(1), 3, 0) == GECM_ERR_ARG
    assert "x[0]" in lib.gecm_last_error().decode()
    assert lib.gecm_resume_points(eng._h, arr, one(1), one(n), 3, 0) == GECM_ERR_ARG
    assert eng.save_lines() == before
    # the wrong kind of context
    idx = (ctypes.c_uint32 * 3)(0, 0, 0)
    assert lib.gecm_resume_points_multi(eng._h, arr, idx, one(1), one(1), 3, 0) == GECM_ERR_STATE
    multi = pyecm.MultiEngine([n, p * p + 2])
    assert lib.gecm_resume_points(multi._h, arr, multi.pack([1, 1, 1]), multi.pack([1, 1, 1]), 3, 0) == GECM_ERR_STATE
    assert lib.gecm_resume_points_multi(multi._h, arr, (ctypes.c_uint32 * 3)(0, 2, 0), multi.pack([1, 1, 1]),
                                        multi.pack([1, 1, 1]), 3, 0) == GECM_ERR_ARG
    # x below the largest number but not below its own
    assert lib.gecm_resume_points_multi(multi._h, arr, (ctypes.c_uint32 * 3)(0, 1, 0), multi.pack([1, p * p + 2, 1]),
                                        multi.pack([1, 1, 1]), 3, 0) == GECM_ERR_ARG
    assert "x[1]" in lib.gecm_last_error().decode()
    multi.close()
    # mid stage 1: stage 2 wants stage 1 first
    eng.resume(sig, [2, 3, 4], [1, 1, 1], b1_done=0)
    with pytest.raises(pyecm.GecmError, match="stage 1"):
        eng.stage2_init()
    with pytest.raises(pyecm.GecmError):
        eng.stage2(5000)
    # stage 1 taken as finished: the factor scan flags the curve whose Z is a factor of N
    eng.resume(sig, [2, 3, 4], [1, p, 7], b1_done=500)
    assert eng.scan_factors(1) == (1, 1)
    assert eng.stage1_factor(1)[0] == p and eng.stage1_factor(0) is None
    assert [eng.curve_flag(1, k) for k in range(3)] == [False, True, False]
    eng.stage2_init()
    eng.close()


# ---- 7. special form keeps its multiply ---------------------------------------------------------------------------
def test_special_form_keeps_its_multiply(short_ranges):
    import pyecm
    prange, b1 = 1500, 4000
    short_ranges(prange)
    n = (1 << 401) - 1
    sig = list(range(1000, 1000 + 200))
    check = (0, 63, 64, 199)
    o = Oracle(n)
    after0 = [o.line(s, b1, prange, 1) for s in sig]
    final = {k: o.line(sig[k], b1, prange, 0) for k in check}
    o.close()
    out = {}
    for special in (True, False):
        eng = pyecm.Engine(n)
        eng.set_special_form(special)
        eng.set_lanes_per_curve(1)
        eng.resume_lines(after0)
        for r in range(1, pyecm.stage1_ranges(b1)):
            eng.stage1_range(b1, r)
            assert eng.special_form_used() == special
        out[special] = eng.save_lines()
        eng.close()
    assert out[True] == out[False]
    for k in check:
        assert out[True][k] == final[k]
