"""GPU tests of stage 1 of multi-modulus curve batches in the 32-lane row layout: k_stage1_row_multi
through gecm_set_multi_rows, on both packings and through every stage-1 entry point.  The yardstick is the same context
with rows off — the path tests/test_gpu_multi.py and tests/test_gpu_dense.py pin to single-number contexts, to the
reference's files and to the oracle — and, for the 15- and 37-limb classes, the oracle itself.  Every comparison is of
line bytes or exact integers."""
import ctypes
import json
import os
import random
import re

import pytest

from conftest import GOLDEN, ROOT
from unit_model import class_moduli, random_modulus

pytestmark = pytest.mark.gpu

S1 = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "stage1.json")))}
N64 = random_modulus(64, random.Random(6464))
B1 = 1000


def _row_name(nl):
    return "k_stage1_row_multi<%d, %d>" % ((nl + 1 + 15) // 16, nl + 1)


def _interleave(groups):
    """[(modulus index, sigma)] taking one curve of every group in turn: the library has to do the grouping"""
    out, i = [], 0
    while any(i < len(g) for g in groups):
        for m, g in enumerate(groups):
            if i < len(g):
                out.append((m, g[i]))
        i += 1
    return out


def _batch(counts, seed):
    rng = random.Random(seed)
    order = _interleave([[rng.randrange(6, 1 << 63) for _ in range(c)] for c in counts])
    return [s for _, s in order], [m for m, _ in order]


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


def _oracle_lines(orc, n, sigmas, b1):
    c = orc.orc_create(str(n).encode(), 52)
    line = ctypes.create_string_buffer(16384)
    out = []
    for s in sigmas:
        orc.orc_stage1_line(c, s, b1, line, len(line), None, 0, None)
        out.append(line.value.decode())
    orc.orc_destroy(c)
    return out


def _stage1(me, rows, sig, which, b1=B1):
    me.set_rows(rows)
    me.build_curves(sig, which)
    me.stage1(b1)
    return me.save_lines()


# ---- 1. wave packing, both ends of every limbs-per-lane shape --------------------------------------------------------
@pytest.mark.parametrize("nl", [8, 15, 17, 30, 32, 37])
def test_wave_packing_both_ends_of_every_shape(pyecm, orc, nl):
    """three numbers: the top of the class (28 nl - 5 bits: the multiply's 5-bit minimum of headroom), the bottom of the
    class, and a 64-bit number whose N' has its top limbs zero; 1, 65 and 2 curves: 256 positions, a group boundary
    inside the batch"""
    top, bottom = class_moduli(nl)
    ns = [top, bottom, N64]
    assert top.bit_length() == 28 * nl - 5
    sig, which = _batch([1, 65, 2], "wave rows:%d" % nl)
    me = pyecm.MultiEngine(ns)
    try:
        assert me.cfg.dev_limbs == nl and me.packing() == "wave"
        on = _stage1(me, "on", sig, which)
        assert me.lanes_per_curve() == 32 and me.last_kernel_name() == _row_name(nl)
        assert me.last_kernel_name().startswith("k_stage1_row_multi<")
        off = _stage1(me, "off", sig, which)
        assert me.lanes_per_curve() in (1, 2) and "row" not in me.last_kernel_name()
        assert len(on) == 68 and on == off
        if nl in (15, 37):
            for g, n in enumerate(ns):
                mine = [k for k in range(len(sig)) if which[k] == g]
                ends = sorted({mine[0], mine[-1]})
                want = _oracle_lines(orc, n, [sig[k] for k in ends], B1)
                assert [on[k] for k in ends] == want, (nl, g)
    finally:
        me.close()


# ---- 2. lane packing -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nl", [8, 15])
def test_lane_packing_neighbours_on_different_numbers(pyecm, nl):
    """five numbers with 1, 1, 3, 64 and 2 curves, back to back: the two curves of a wavefront are on different numbers,
    and the tail of the 128 positions is padding"""
    top, bottom = class_moduli(nl)
    rng = random.Random(8000 + nl)
    ns = [top, N64, bottom, random_modulus(28 * nl - 17, rng), random_modulus(28 * nl - 40, rng)]
    sig, which = _batch([1, 1, 3, 64, 2], "lane rows:%d" % nl)
    me = pyecm.MultiEngine(ns)
    try:
        me.set_packing("lane")
        on = _stage1(me, "on", sig, which)
        assert me.packing() == "lane" and me.cfg.dev_limbs == nl
        assert me.lanes_per_curve() == 32 and me.last_kernel_name() == _row_name(nl)
        off = _stage1(me, "off", sig, which)
        assert me.lanes_per_curve() == 1 and me.last_kernel_name() == "k_stage1_lane<%d>" % nl
        assert len(on) == 71 and on == off
    finally:
        me.close()


# ---- 3. the other stage-1 entry points -------------------------------------------------------------------------------
def _three(nl=15):
    top, bottom = class_moduli(nl)
    return [top, bottom, N64]


@pytest.mark.parametrize("packing", ["wave", "lane"])
def test_extension_in_two_steps_and_in_one(pyecm, packing):
    ns = _three()
    sig, which = _batch([3, 66, 2], "extend rows")
    me = pyecm.MultiEngine(ns)
    try:
        me.set_packing(packing)
        got = {}
        for rows, steps in (("on", [(1, 300), (300, 1000)]), ("on", [(1, 1000)]), ("off", [(1, 1000)])):
            me.set_rows(rows)
            me.build_curves(sig, which)
            for lo, hi in steps:
                me.stage1_extend(lo, hi)
                assert (me.lanes_per_curve() == 32) == (rows == "on")
                assert me.last_kernel_name().startswith("k_stage1_row_multi<") == (rows == "on")
            left = me.normalize()                     # 1: some curve met a factor and keeps its X and Z in the line
            got[(rows, len(steps))] = (left, me.save_lines_std())
        two, one, off = got[("on", 2)], got[("on", 1)], got[("off", 1)]
        assert len(one[1]) == 71 and one == off
        # in two steps: the same point of every curve, so the same line wherever Z had an inverse (a curve left as it was
        # shows the projective X and Z its own chain of steps ended on)
        kept = [k for k, l in enumerate(one[1]) if "Z=0x" in l]
        assert two[0] == one[0] and [k for k, l in enumerate(two[1]) if "Z=0x" in l] == kept and len(kept) < 8
        assert [l for k, l in enumerate(two[1]) if k not in kept] == [l for k, l in enumerate(one[1]) if k not in kept]
        for k in kept:                                # ... and there the two are the same projective point: X Z' = X' Z
            (n2, x2, z2), (n1, x1, z1) = ([int(re.search(r"%s=0x([0-9a-f]+);" % f, l[k]).group(1), 16) for f in "NXZ"]
                                          for l in (two[1], one[1]))
            assert n1 == n2 == ns[which[k]] and (x2 * z1 - x1 * z2) % n1 == 0, k
    finally:
        me.close()


def test_param_0_1_and_3_in_one_batch(pyecm):
    ns = _three()
    rng = random.Random("param rows")
    which = [k % 3 for k in range(70)]
    params = [(0, 1, 3, 1, 0, 3, 3)[k % 7] for k in range(70)]
    sig = [rng.randrange(6, 1 << 32) for _ in range(70)]
    me = pyecm.MultiEngine(ns)
    try:
        lines = {}
        for rows in ("on", "off"):
            me.set_rows(rows)
            assert me.build_curves(sig, which, params=params) == 0
            me.stage1_extend(1, B1)
            assert (me.lanes_per_curve() == 32) == (rows == "on")
            left = me.normalize()
            lines[rows] = (left, me.save_lines_std())
        assert len(lines["on"][1]) == 70 and lines["on"] == lines["off"]
        assert {"PARAM=1" in l for l in lines["on"][1]} == {True, False}
    finally:
        me.close()


def test_resumed_batch_runs_its_remaining_range_in_rows(pyecm):
    """two prime ranges below B1 = 1000 (the test hook of tests/test_gpu_resume.py): the lines after range 0 go into a
    fresh batch, range 1 runs with rows on and with rows off"""
    hook = pyecm.lib.gecm_plan_set_prime_range_for_tests
    hook.argtypes = [ctypes.c_uint64]
    hook.restype = None
    ns = _three()
    sig, which = _batch([2, 65, 1], "resume rows")
    me = pyecm.MultiEngine(ns)
    hook(500)
    try:
        assert pyecm.stage1_ranges(B1) == 2
        field = pyecm.describe_range(B1, B1, 0).last_prime
        me.build_curves(sig, which)
        me.stage1_range(B1, 0)
        after0 = [me.resume_line(k, field) for k in range(len(sig))]
        me.stage1_range(B1, 1)
        whole = me.save_lines()
        got = {}
        for rows in ("on", "off"):
            me.set_rows(rows)
            me.resume_lines(after0)
            me.stage1_range(B1, 1)
            assert (me.lanes_per_curve() == 32) == (rows == "on")
            got[rows] = me.save_lines()
        assert got["on"] == got["off"] == whole and len(whole) == 68
    finally:
        hook(0)
        me.close()


# ---- 4. factors and stage 2 ------------------------------------------------------------------------------------------
def test_factors_and_stage2_after_rows(pyecm):
    """n415_b1_1000 of tests/golden finds factors in stage 1; a number without one sits next to it"""
    fac = S1["n415_b1_1000"]
    nf = int(fac["save_lines"][0].split("N=0x")[1].split(";")[0], 16)
    fsig = [int(l.split("SIGMA=")[1].split(";")[0]) for l in fac["save_lines"]]
    found = {int(re.search(r"sigma (\d+)", l).group(1)): int(re.search(r"factor (\d+) in", l).group(1))
             for l in fac["results_lines"] if "in stage 1" in l}
    assert found
    quiet = class_moduli(15)[1]
    order = _interleave([fsig, list(range(5000, 5000 + 66))])
    sig, which = [s for _, s in order], [m for m, _ in order]
    me = pyecm.MultiEngine([nf, quiet])
    try:
        out = {}
        for rows in ("on", "off"):
            lines = _stage1(me, rows, sig, which)
            assert (me.lanes_per_curve() == 32) == (rows == "on")
            scan = me.scan_factors(1)
            flags = [int(me.curve_flag(1, k)) for k in range(len(sig))]
            facs = [me.stage1_factor(k) for k in range(len(sig))]
            me.stage2(20000, D=210, U=2)
            out[rows] = (lines, scan, flags, facs, me.accs())
        assert out["on"] == out["off"]
        lines, scan, flags, facs, accs = out["on"]
        got = {sig[k]: facs[k][0] for k in range(len(sig)) if which[k] == 0 and facs[k]}
        assert got == found and scan[0] == sum(flags) >= len(found)
        assert [l.rstrip("\n") for k, l in enumerate(lines) if which[k] == 0] == fac["save_lines"]
        assert len(set(accs)) > len(sig) // 2
    finally:
        me.close()


# ---- 5. the setting --------------------------------------------------------------------------------------------------
def test_settings(pyecm):
    ns = _three()
    sig, which = _batch([1, 65, 2], "settings rows")
    me = pyecm.MultiEngine(ns)
    try:
        # the default is off: what ran before the setting existed
        assert me.rows() == "off"
        me.build_curves(sig, which)
        me.stage1(B1)
        default_name, want = me.last_kernel_name(), me.save_lines()
        assert default_name in ("k_stage1_multi<15>", "k_stage1_pair_multi<15>") and me.lanes_per_curve() in (1, 2)
        for bad in (2, -2, 32, "rows"):
            with pytest.raises(pyecm.GecmError, match=r"\(-2\)"):
                me.set_rows(bad)
        assert me.rows() == "off"
        # on: it holds across builds; an explicit lanes-per-curve setting wins
        me.set_rows("on")
        assert me.rows() == "on"
        me.build_curves(sig, which)
        assert me.rows() == "on"
        me.stage1(B1)
        assert me.last_kernel_name() == _row_name(15) and me.lanes_per_curve() == 32 and me.save_lines() == want
        me.set_lanes_per_curve(1)
        me.build_curves(sig, which)
        me.stage1(B1)
        assert me.last_kernel_name() == "k_stage1_multi<15>" and me.lanes_per_curve() == 1 and me.save_lines() == want
        with pytest.raises(pyecm.GecmError, match="1 or 2 lanes"):
            me.set_lanes_per_curve(32)
        me.set_lanes_per_curve(0)
        # a method batch on the same context does not see it
        me.build_seeds(pyecm.METHOD_PM1, [3] * 5, [0, 1, 2, 1, 0])
        me.stage1_extend(1, B1)
        assert me.last_kernel_name() == "k_unit_multi<15>" and me.lanes_per_curve() == 1
        # auto on a 256-position batch runs rows
        me.set_rows("auto")
        assert me.rows() == "auto"
        me.build_curves(sig, which)
        me.stage1(B1)
        assert me.last_kernel_name() == _row_name(15) and me.lanes_per_curve() == 32 and me.save_lines() == want
        me.set_rows("off")
        me.build_curves(sig, which)
        me.stage1(B1)
        assert me.last_kernel_name() == default_name and me.save_lines() == want
    finally:
        me.close()


def test_lane_packing_still_refuses_two_lanes_and_keeps_the_batch(pyecm):
    ns = _three()
    sig, which = _batch([1, 5, 2], "refusal rows")
    me = pyecm.MultiEngine(ns)
    try:
        me.set_packing("lane")
        me.set_rows("on")
        want = _stage1(me, "on", sig, which)
        assert me.lanes_per_curve() == 32
        me.set_lanes_per_curve(2)
        with pytest.raises(pyecm.GecmError, match="one lane per curve"):
            me.stage1(2000)
        assert me.save_lines() == want and me.rows() == "on"
    finally:
        me.close()


def test_setter_on_a_single_number_context(pyecm):
    eng = pyecm.Engine(class_moduli(15)[0])
    try:
        for rows in ("on", "auto", "off"):
            with pytest.raises(pyecm.GecmError, match=r"\(-4\)"):
                pyecm.MultiEngine.set_rows(eng, rows)
        with pytest.raises(pyecm.GecmError, match=r"\(-2\)"):
            pyecm.MultiEngine.set_rows(eng, 7)
        assert pyecm.lib.gecm_get_multi_rows(eng._h) == pyecm.MULTI_ROWS_OFF
    finally:
        eng.close()
