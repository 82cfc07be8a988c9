"""GPU: multi-modulus batches (include/gecm.h gecm_create_multi, pyecm.MultiEngine).  Curves on many
numbers in one launch must give, curve by curve, what a single-N context of the curve's own number gives — and what the
reference wrote for it (tests/golden) — in both layouts the multi path has, with the padding to whole wavefronts
never leaking into a result."""
import ctypes
import json
import os
import random
import re

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

S1 = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "stage1.json")))}
S2 = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "stage2_acc.json")))}


def _n_of(case):
    return int(case["save_lines"][0].split("N=0x")[1].split(";")[0], 16)


def _sigmas(case):
    return [int(l.split("SIGMA=")[1].split(";")[0]) for l in case["save_lines"]]


def _found(lines, stage):
    """sigma -> factor of the reference's result lines of one stage"""
    return {int(re.search(r"sigma (\d+)", l).group(1)): int(re.search(r"factor (\d+) in", l).group(1))
            for l in lines if "in stage %d" % stage in l}


def _interleave(groups):
    """[(modulus index, sigma)] taking one curve of every group in turn: the library has to do the grouping"""
    out, i = [], 0
    while any(i < len(g) for g in groups):
        for m, g in enumerate(groups):
            if i < len(g):
                out.append((m, g[i]))
        i += 1
    return out


@pytest.fixture(scope="module")
def orc():
    L = ctypes.CDLL(os.path.join(ROOT, "oracle", "libecm_oracle.so"))
    L.orc_create.restype = ctypes.c_void_p
    L.orc_create.argtypes = [ctypes.c_char_p, ctypes.c_int]
    L.orc_destroy.argtypes = [ctypes.c_void_p]
    L.orc_stage1_line.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t,
                                  ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)]
    return L


@pytest.mark.parametrize("lanes", [1, 2])
def test_fixture_save_lines_and_factors_on_four_sizes_in_one_batch(lanes):
    """200-, 415-, 623- and 831-bit N of stage1.json in one context (37 limbs for all), 8 curves each (7/8 of every
    wavefront is padding), curves interleaved: every save line byte for byte the reference's, every stage-1 factor
    the reference's"""
    import pyecm
    cases = [S1[n] for n in ("n200_b1_1000", "n415_b1_1000", "n623_b1_1000", "n831_b1_1000")]
    order = _interleave([_sigmas(c) for c in cases])
    eng = pyecm.MultiEngine([_n_of(c) for c in cases])
    eng.set_lanes_per_curve(lanes)
    eng.build_curves([s for _, s in order], [m for m, _ in order])
    eng.stage1(1000)
    assert eng.lanes_per_curve() == lanes
    lines = [l.rstrip("\n") for l in eng.save_lines()]
    for m, case in enumerate(cases):
        mine = [k for k, (mm, _) in enumerate(order) if mm == m]
        assert [eng.modulus_of(k) for k in mine] == [m] * len(mine)
        assert [lines[k] for k in mine] == case["save_lines"], case["name"]
        want = _found(case["results_lines"], 1)
        got = {order[k][1]: eng.stage1_factor(k)[0] for k in mine if eng.stage1_factor(k)}
        assert got == want, case["name"]
    n, first = eng.scan_factors(1)
    flagged = [k for k in range(len(order)) if eng.curve_flag(1, k)]
    assert n == len(flagged) == sum(len(_found(c["results_lines"], 1)) for c in cases)
    assert first == flagged[0]
    eng.close()


def test_mixed_sizes_and_uneven_counts_equal_oracle_and_single_contexts(orc):
    """ten random odd N from the 8-limb class to 1031 bits, 1 to 200 curves each, interleaved; B1 = 2000"""
    import pyecm
    rnd = random.Random(20261016)
    bits = [200, 1031, 300, 415, 520, 640, 700, 831, 960, 250]
    counts = [1, 63, 64, 65, 200, 1, 3, 64, 2, 17]
    ns = [rnd.getrandbits(b) | (1 << (b - 1)) | 1 for b in bits]
    groups = [[rnd.randrange(6, 1 << 40) for _ in range(c)] for c in counts]
    order = _interleave(groups)
    eng = pyecm.MultiEngine(ns)
    assert eng.cfg.dev_limbs == 37 and eng.cfg.nbits == 1031
    assert eng.batch_bytes(len(order)) >= eng.batch_bytes(1) * (sum((c + 63) // 64 for c in counts))
    eng.build_curves([s for _, s in order], [m for m, _ in order])
    eng.stage1(2000)
    lines = [l.rstrip("\n") for l in eng.save_lines()]
    eng.close()
    buf = ctypes.create_string_buffer(8192)
    for m, n in enumerate(ns):
        mine = [k for k, (mm, _) in enumerate(order) if mm == m]
        single = pyecm.Engine(n)
        single.build_curves(groups[m])
        single.stage1(2000)
        assert [lines[k] for k in mine] == [l.rstrip("\n") for l in single.save_lines()], (m, bits[m])
        single.close()
        c = orc.orc_create(str(n).encode(), 52)
        for k, s in zip(mine, groups[m]):
            orc.orc_stage1_line(c, s, 2000, buf, len(buf), None, 0, None)
            assert lines[k] == buf.value.decode().rstrip("\n"), (m, bits[m], s)
        orc.orc_destroy(c)


def _single_stage2(n, sig, b1, b2, D=0, U=0):
    import pyecm
    e = pyecm.Engine(n)
    e.build_curves(sig)
    e.stage1(b1)
    e.stage2(b2, D, U)
    out = (e.download_acc(), [e.stage2_factor(k) for k in range(len(sig))])
    e.close()
    return out


def test_stage2_accumulators_and_factors_equal_single_contexts():
    """three N of stage2_acc.json at B1 = 1000, B2 = 50000, D = 385, U = 16 in one context: every accumulator and
    stage-2 factor is the single-N context's, and the T35N curves' accumulators are the reference's stg2acc"""
    import pyecm
    t35 = S2["T35N_b1_1000_b2_50000"]
    cases = [t35, S2["K1N_b1_2000_b2_1e5"], S2["M607xM127xM89_b1_800_b2_40000"]]
    groups = [[c["sigma0"] + k for k in range(c["curves"])] for c in cases]
    order = _interleave(groups)
    eng = pyecm.MultiEngine([int(c["N"]) for c in cases])
    eng.build_curves([s for _, s in order], [m for m, _ in order])
    eng.stage1(1000)
    eng.stage2(50000, 385, 16)
    accs = eng.accs()
    facs = [eng.stage2_factor(k) for k in range(len(order))]
    n_flag, _ = eng.scan_factors(2)
    assert n_flag == sum(1 for f in facs if f)
    eng.close()
    for m, case in enumerate(cases):
        mine = [k for k, (mm, _) in enumerate(order) if mm == m]
        acc1, fac1 = _single_stage2(int(case["N"]), groups[m], 1000, 50000, 385, 16)
        assert [accs[k] for k in mine] == acc1, case["name"]
        assert [facs[k] for k in mine] == fac1, case["name"]
    assert [accs[k] for k, (m, _) in enumerate(order) if m == 0] == [int(h, 16) for h in t35["acc_hex"]]


def test_stage2_failure_records_stay_on_their_curves():
    """degenerate.json (every stage-2 batch inversion fails) next to a healthy N: the degenerate curves report the
    reference's own stage-2 factors (one sub-sequence per curve is the reference's chain), the healthy ones what a
    single-N context reports"""
    import pyecm
    case = json.load(open(os.path.join(GOLDEN, "degenerate.json")))[0]
    n = _n_of(case)
    healthy = int(S2["T35N_b1_1000_b2_50000"]["N"])
    sig = [case["sigma0"] + k for k in range(8)]
    hsig = list(range(42, 42 + 8))
    order = _interleave([hsig, sig])
    eng = pyecm.MultiEngine([healthy, n])
    eng.build_curves([s for _, s in order], [m for m, _ in order])
    eng.stage1(case["B1"])
    lines = [l.rstrip("\n") for l in eng.save_lines()]
    eng.stage2(case["B2"])
    eng.scan_factors(2)
    want2 = _found(case["results_lines"], 2)
    hacc, hfac = _single_stage2(healthy, hsig, case["B1"], case["B2"])
    for k, (m, s) in enumerate(order):
        f = eng.stage2_factor(k)
        if m == 1:
            assert lines[k] == case["save_lines"][sig.index(s)]
            assert f and f[0] == want2[s] and eng.curve_flag(2, k), (k, s)
        else:
            j = hsig.index(s)
            assert f == hfac[j] and eng.acc(k) == hacc[j] and eng.curve_flag(2, k) == bool(hfac[j]), (k, s)
    eng.close()


def test_a_group_with_a_stage1_factor_changes_nothing_next_to_it():
    """n415_b1_1000 finds factors in stage 1; the curves of two other numbers give the same lines and factors with it
    in the batch as without it"""
    import pyecm
    fac = S1["n415_b1_1000"]
    others = [S1["n623_b1_1000"], S1["n200_b1_1000"]]
    rnd = random.Random(7)
    quiet = rnd.getrandbits(500) | (1 << 499) | 1
    ns = [_n_of(c) for c in others] + [quiet]
    groups = [_sigmas(c) for c in others] + [list(range(5000, 5070))]

    def run(with_fac):
        g = groups + ([_sigmas(fac)] if with_fac else [])
        order = _interleave(g)
        eng = pyecm.MultiEngine(ns + ([_n_of(fac)] if with_fac else []))
        eng.build_curves([s for _, s in order], [m for m, _ in order])
        eng.stage1(1000)
        out = {(m, s): (eng.save_line(k), eng.stage1_factor(k)) for k, (m, s) in enumerate(order) if m < len(ns)}
        eng.close()
        return out

    assert run(True) == run(False)


def test_errors_and_calls_without_a_meaning_on_a_multi_context():
    import pyecm
    GecmError = pyecm.GecmError
    with pytest.raises(GecmError, match="empty"):
        pyecm.MultiEngine([])
    with pytest.raises(GecmError, match=r"N\[1\] must be an odd integer"):
        pyecm.MultiEngine([1000003, 1000004])
    with pytest.raises(GecmError, match=r"N\[0\] of 1100 bits is larger"):
        pyecm.MultiEngine([(1 << 1099) + 1, 1000003])
    eng = pyecm.MultiEngine([1000003, (1 << 127) - 1])
    with pytest.raises(GecmError, match=r"modulus_index\[1\] = 2"):
        eng.build_curves([10, 11], [0, 2])
    with pytest.raises(GecmError, match="no curves"):
        eng.stage1(100)
    with pytest.raises(GecmError, match="1 or 2 lanes"):
        eng.set_lanes_per_curve(8)
    eng.build_curves([10, 11, 12], [1, 0, 1])
    eng.stage1(100)
    calls = {"the L0 operators": lambda: eng.vecmulmod([1], [2]),
             "gecm_upload_points": lambda: eng.upload_points([1], [1], [1]),
             "gecm_download_points": eng.download_points,
             "gecm_download_points_plain": eng.download_points_plain,
             "gecm_download_acc": eng.download_acc,
             "gecm_set_special_form": lambda: eng.set_special_form(False),
             "gecm_set_report_modulus": lambda: eng.set_report_modulus(7),
             "gecm_build_curves": lambda: pyecm.Engine.build_curves(eng, [10])}
    for name, call in calls.items():
        with pytest.raises(GecmError, match=r"\(-4\): %s: not available on a multi-modulus context" % name):
            call()
    # the refused calls left the batch alone (save_line: straight to the library, whatever pyecm's count says)
    assert "N=0x%x;" % ((1 << 127) - 1) in eng.save_line(2) and "N=0x%x;" % 1000003 in eng.save_line(1)
    with pytest.raises(GecmError, match="no such curve"):
        eng.save_line(3)
    eng.close()
    single = pyecm.Engine((1 << 127) - 1)
    with pytest.raises(GecmError, match=r"\(-4\): gecm_build_curves_multi: not a multi-modulus context"):
        pyecm.MultiEngine.build_curves(single, [10], [0])
    assert pyecm.lib.gecm_moduli(single._h) == 1
    single.close()
