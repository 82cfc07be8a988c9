"""Every stage-1 launch path of the device layer, one row of a table each: the kernel named exactly, the tape run as
several launches, and the result against the oracle (curves; oracle/libecm_oracle.so as tests/test_gpu_layouts.py and
tests/test_gpu_wide.py use it) or against Python integers (P-1 and P+1 residues; tests/unit_model.py).  Every row runs 33
curves or residues (a block of 64 positions with padding; two moduli share them 20 and 13) to B1 = 1000 with
GECM_TAPE_CHUNK = 64.  The limb counts are 15 (one limb per lane of a row, 16 rows), 17 (two per lane, 18 rows) and 40 (a
wide context, 41 rows).

The second part pins the refusals of a stage-1 launch that the public API reaches before anything is launched: exact
text, return code, and the batch as it was.  Both are on contexts that refuse gecm_download_points (a multi-modulus and a
wide one), so "the batch as it was" is read through gecm_format_save_line, which downloads the same points.  The two
other refusals one could wish for here — rows ON, and method lanes 16, on a context one of whose numbers has no row
constants — cannot be constructed: gecm_mod_row_consts makes both sets for every odd N that fits its limb count (N below
2^(28 nl - 5) gives m N below 2^(28 (nl + 1) - 5), which is the only bound of the curve kernel's set, and the method
kernel's N'' lies below 2^(28 nl + 20) + 2^28 N, which is its upper bound)."""
import ctypes
import os
import random
from concurrent.futures import ThreadPoolExecutor

import pytest

import wide_row_model as W
from conftest import ROOT
from unit_model import METHOD_PM1, METHOD_PP1, class_moduli, expected, exponent, method_line, seeds_for

pytestmark = pytest.mark.gpu

B1 = 1000
COUNT = 33
SPLIT = (20, 13)
E1000 = exponent(1, B1)
GECM_ERR_STATE = -4

N15, N15B = class_moduli(15)
N17 = class_moduli(17)[0]
NF = (1 << 401) - 1                          # tests/test_gpu_fform.py: (401, 1), 15 limbs, the 2^k - 1 multiply
NWIDE = W.modulus(1039, "random")
TWO = (N15, N15B)


@pytest.fixture(scope="module")
def pyecm():
    import pyecm
    return pyecm


@pytest.fixture(scope="module")
def orc():
    L = ctypes.CDLL(os.path.join(ROOT, "oracle", "libecm_oracle.so"))
    L.orc_create.restype = ctypes.c_void_p
    L.orc_create.argtypes = [ctypes.c_char_p, ctypes.c_int]
    L.orc_destroy.argtypes = [ctypes.c_void_p]
    L.orc_stage1_line.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t,
                                  ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)]
    return L


def _sigmas(n):
    rng = random.Random("stage-1 paths:%d" % n.bit_length())
    return [rng.randrange(6, 1 << 63) for _ in range(COUNT)]


_ORACLE = {}


def _oracle_lines(orc, n):
    """the oracle's save line of every sigma of _sigmas(n), computed once per number (threads: a wide curve takes it
    a twentieth of a second, and the library keeps no state outside a context)"""
    if n not in _ORACLE:
        sig = _sigmas(n)

        def some(part):
            c = orc.orc_create(str(n).encode(), 52)
            line = ctypes.create_string_buffer(16384)
            out = []
            for s in part:
                orc.orc_stage1_line(c, s, B1, line, len(line), None, 0, None)
                out.append(line.value.decode())
            orc.orc_destroy(c)
            return out
        workers = max(1, min(8, os.cpu_count() or 1))
        with ThreadPoolExecutor(workers) as pool:
            res = list(pool.map(some, [sig[w::workers] for w in range(workers)]))
        lines = [None] * COUNT
        for w, r in enumerate(res):
            lines[w::workers] = r
        _ORACLE[n] = lines
    return _ORACLE[n]


def _which():
    """20 positions on number 0 and 13 on number 1, interleaved: the library does the grouping"""
    rng = random.Random("stage-1 paths: which")
    which = [0] * SPLIT[0] + [1] * SPLIT[1]
    rng.shuffle(which)
    return which


def _after_the_launch(eng, name, lanes):
    eng.sync()
    assert eng.last_kernel_name() == name
    assert eng.lanes_per_curve() == lanes
    done, total = eng.stage1_progress()
    assert total > 1 and done == total, (done, total)


# ---- 1. curves ---------------------------------------------------------------------------------------------------
# (id, number, special form, lanes per curve, kernel name, lanes reported)
SINGLE = [
    ("nl15_lanes1", N15, False, 1, "k_stage1<15>", 1),
    ("nl15_lanes2", N15, False, 2, "k_stage1_pair<15>", 2),
    ("nl15_lanes8", N15, False, 8, "k_stage1_quad<15>", 8),
    ("nl15_lanes32", N15, False, 32, "k_stage1_row<1, 16, false>", 32),
    ("nl17_lanes32", N17, False, 32, "k_stage1_row<2, 18, false>", 32),
    ("fform_lanes1", NF, True, 1, "k_stage1_f<15, ModF<15> >", 1),
    ("fform_lanes2", NF, True, 2, "k_stage1_pair_f<15, ModF<15> >", 2),
]


@pytest.mark.parametrize("n,special,lanes,name,used", [c[1:] for c in SINGLE], ids=[c[0] for c in SINGLE])
def test_single_number_curves(pyecm, orc, monkeypatch, n, special, lanes, name, used):
    monkeypatch.setenv("GECM_TAPE_CHUNK", "64")
    want = _oracle_lines(orc, n)
    eng = pyecm.Engine(n)
    try:
        assert eng.cfg.dev_limbs == (17 if n == N17 else 15)
        eng.set_special_form(special)
        eng.set_lanes_per_curve(lanes)
        eng.build_curves(_sigmas(n))
        eng.stage1(B1, sync=False)
        _after_the_launch(eng, name, used)
        assert eng.special_form_used() == special
        got = eng.save_lines()
    finally:
        eng.close()
    assert [k for k in range(COUNT) if got[k] != want[k]] == [] and len(got) == COUNT


# (id, packing, lanes per curve, rows, kernel name, lanes reported)
MULTI = [
    ("wave_lanes1", "wave", 1, "off", "k_stage1_multi<15>", 1),
    ("wave_lanes2", "wave", 2, "off", "k_stage1_pair_multi<15>", 2),
    ("lane", "lane", 0, "off", "k_stage1_lane<15>", 1),
    ("wave_rows", "wave", 0, "on", "k_stage1_row_multi<1, 16>", 32),
    ("lane_rows", "lane", 0, "on", "k_stage1_row_multi<1, 16>", 32),
]


@pytest.mark.parametrize("packing,lanes,rows,name,used", [c[1:] for c in MULTI], ids=[c[0] for c in MULTI])
def test_two_moduli_curves(pyecm, orc, monkeypatch, packing, lanes, rows, name, used):
    monkeypatch.setenv("GECM_TAPE_CHUNK", "64")
    which = _which()
    # curve k is the next unused sigma of its own number's list: the oracle's lines are shared with the single-N rows
    taken, sig, want = [0, 0], [], []
    for g in which:
        sig.append(_sigmas(TWO[g])[taken[g]])
        want.append(_oracle_lines(orc, TWO[g])[taken[g]])
        taken[g] += 1
    me = pyecm.MultiEngine(TWO)
    try:
        assert me.cfg.dev_limbs == 15
        me.set_packing(packing)
        me.set_rows(rows)
        me.set_lanes_per_curve(lanes)
        me.build_curves(sig, which)
        assert me.packing() == packing
        me.stage1(B1, sync=False)
        _after_the_launch(me, name, used)
        got = me.save_lines()
    finally:
        me.close()
    assert [k for k in range(COUNT) if got[k] != want[k]] == [] and len(got) == COUNT


def test_wide_curves(pyecm, orc, monkeypatch):
    monkeypatch.setenv("GECM_TAPE_CHUNK", "64")
    assert NWIDE.bit_length() == 1039 and W.wide_nl(1039) == 40
    want = _oracle_lines(orc, NWIDE)
    eng = pyecm.Engine(NWIDE, wide=True)
    try:
        assert eng.is_wide() and eng.cfg.dev_limbs == 40
        eng.build_curves(_sigmas(NWIDE))
        eng.stage1(B1, sync=False)
        _after_the_launch(eng, "k_stage1_row<3, 41, false>", 32)
        got = eng.save_lines()
    finally:
        eng.close()
    assert [k for k in range(COUNT) if got[k] != want[k]] == [] and len(got) == COUNT


# ---- 2. P-1 and P+1 residues -------------------------------------------------------------------------------------
# (id, context: None = single N or the packing of two moduli, method lanes, kernel name)
UNIT = [
    ("single_lanes1", None, 1, "k_unit<15>"),
    ("wave_lanes1", "wave", 1, "k_unit_multi<15>"),
    ("lane_lanes1", "lane", 1, "k_unit_lane<15>"),
    ("single_lanes16", None, 16, "k_unit_row<1, 16>"),
    ("two_moduli_lanes16", "wave", 16, "k_unit_row<1, 16>"),
]


@pytest.mark.parametrize("method", (METHOD_PM1, METHOD_PP1), ids=["pm1", "pp1"])
@pytest.mark.parametrize("packing,lanes,name", [c[1:] for c in UNIT], ids=[c[0] for c in UNIT])
def test_method_residues(pyecm, monkeypatch, packing, lanes, name, method):
    monkeypatch.setenv("GECM_TAPE_CHUNK", "64")
    rng = random.Random("stage-1 paths: seeds %s %d" % (packing, method))
    if packing is None:
        eng, ns, which = pyecm.Engine(N15), (N15,), [0] * COUNT
        seeds = seeds_for(N15, COUNT, rng)
    else:
        eng, ns, which = pyecm.MultiEngine(TWO), TWO, _which()
        per = [iter(seeds_for(n, c, rng)) for n, c in zip(TWO, SPLIT)]
        seeds = [next(per[g]) for g in which]
    try:
        assert eng.cfg.dev_limbs == 15
        if packing is not None:
            eng.set_packing(packing)
        eng.set_method_lanes(lanes)
        if packing is None:
            eng.build_seeds(method, seeds)
        else:
            eng.build_seeds(method, seeds, which)
            assert eng.packing() == packing
        eng.stage1_extend(1, B1, sync=False)
        _after_the_launch(eng, name, lanes)
        got = eng.save_lines_std()
    finally:
        eng.close()
    want = [method_line(method, B1, ns[g], expected(method, s, E1000, ns[g]), s) for g, s in zip(which, seeds)]
    assert [k for k in range(COUNT) if got[k] != want[k]] == [] and len(got) == COUNT


# ---- 3. refusals before a launch ---------------------------------------------------------------------------------
def test_lane_packed_batch_asked_for_two_lanes(pyecm):
    which = _which()
    sig = _sigmas(N15)
    me = pyecm.MultiEngine(TWO)
    try:
        me.set_packing("lane")
        me.build_curves(sig, which)
        assert me.packing() == "lane"
        before = me.save_lines()
        me.set_lanes_per_curve(2)
        assert pyecm.lib.gecm_stage1(me._h, B1) == GECM_ERR_STATE
        assert pyecm.lib.gecm_last_error().decode() == (
            "gecm_stage1: a lane-packed multi-modulus batch runs one lane per curve, and this context is set to 2 "
            "(gecm_set_lanes_per_curve)")
        assert pyecm.lib.gecm_stage1_extend(me._h, 1, B1) == GECM_ERR_STATE
        assert pyecm.lib.gecm_last_error().decode() == (
            "gecm_stage1: a lane-packed multi-modulus batch runs one lane per curve, and this context is set to 2 "
            "(gecm_set_lanes_per_curve)")
        assert me.save_lines() == before and len(before) == COUNT
    finally:
        me.close()


def test_wide_context_asked_for_eight_lanes(pyecm):
    eng = pyecm.Engine(NWIDE, wide=True)
    try:
        eng.build_curves(_sigmas(NWIDE))
        before = eng.save_lines()
        plain = eng.download_points_plain()
        eng.set_lanes_per_curve(8)
        assert pyecm.lib.gecm_stage1(eng._h, B1) == GECM_ERR_STATE
        assert pyecm.lib.gecm_last_error().decode() == (
            "gecm_stage1: a wide context (gecm_create_wide) runs 32 lanes per curve, and this context is set to 8 "
            "(gecm_set_lanes_per_curve)")
        assert eng.save_lines() == before and eng.download_points_plain() == plain and len(before) == COUNT
    finally:
        eng.close()
