"""GPU test of batch after batch on the same contexts.  Every call that puts a batch into a context ends in the same
begin and finish steps (batch_build in host/gecm_api.c), which is where the state of one kind of batch
could leak into the next: parametrisations, seeds, the method, the layout, the stage-1 counters.  A context that has held
other batches must answer exactly as a fresh context given the same single build.  The values themselves are pinned by
the exact models of tests/test_gpu_param.py, test_gpu_unit.py and test_gpu_resume.py."""
import random

import pytest

from unit_model import METHOD_PM1, METHOD_PP1, random_modulus

pytestmark = pytest.mark.gpu

N200, N297 = random_modulus(200, random.Random(200)), random_modulus(297, random.Random(297))
# one curve on N200, 65 on N297, N200's curve second in the caller's order: 192 positions wave-packed (padding in the
# middle and at the end), 128 lane-packed
WHICH = [1, 0] + [1] * 64


def _state(eng, multi):
    method = eng.batch_method()
    if method == 0:
        eng.normalize()
    ks = range(eng.batch)
    st = eng.stage1_stats()
    return {"method": method, "params": [eng.curve_param(k) for k in ks], "lines": eng.save_lines_std(),
            "seeds": [eng.curve_seed(k) for k in ks] if method else None,
            "moduli": [eng.modulus_of(k) for k in ks] if multi else None,
            "stage1": (st.ptadds, st.ptdups, st.last_prime, st.tape_len)}


def _on_device(build):
    def go(e):
        e.set_curve_build("device")
        try:
            build(e)
        finally:
            e.set_curve_build("host")
        assert e.curve_build() == "device"
    return go


def _steps(ns, which, rng, packing, maxbits):
    """(name, build(eng), run(eng), method, params, seeds) for every batch of the sequence"""
    single = packing is None
    count = len(which)
    mod = [ns[g] for g in which]
    idx = [] if single else [which]                            # MultiEngine's calls take the modulus indices after the values
    sig = [1000 + k for k in range(count)]
    mix = [(0, 1, 3)[k % 3] for k in range(count)]
    xs, zs, x0s = ([rng.randrange(2, n) for n in mod] for _ in range(3))
    ext, ref = (lambda e: e.stage1_extend(1, 1000)), (lambda e: e.stage1(1000))
    steps = [("curves, PARAM 0/1/3 mixed", lambda e: e.build_curves(sig, *idx, params=mix), ext, 0, mix, None),
             ("P-1 residues, seeds unknown", lambda e: e.build_seeds(METHOD_PM1, None, *idx, xs=xs, b1_done=1), ext,
              METHOD_PM1, [0] * count, [None] * count),
             ("resumed plain points, mid stage 1", lambda e: e.resume(sig, *idx, xs, zs, params=mix[::-1]), ref, 0, mix[::-1], None),
             ("P+1 seeds", lambda e: e.build_seeds(METHOD_PP1, x0s, *idx), ext, METHOD_PP1, [0] * count, x0s),
             ("curves, PARAM 0", lambda e: e.build_curves(sig, *idx), ref, 0, [0] * count, None)]
    if single:
        R = 1 << maxbits                                       # gecm_upload_points takes the reference's Montgomery radix
        up = [[v * R % ns[0] for v in vec] for vec in (xs, zs, x0s)]
        steps.append(("uploaded points", lambda e: e.upload_points(*up), ref, 0, [0] * count, None))
    if packing != "lane":                                      # a lane-packed context builds on the host only
        steps.append(("curves built on the device", _on_device(steps[0][1]), ext, 0, mix, None))
    return steps


def test_a_used_context_answers_as_a_fresh_one():
    import pyecm
    for packing in (None, "wave", "lane"):
        single = packing is None

        def make():
            if single:
                return pyecm.Engine(N297)
            me = pyecm.MultiEngine([N200, N297])
            me.set_packing(packing)
            return me
        used = make()
        assert single or used.cfg.dev_limbs <= 15              # a limb class with per-lane kernels
        which = [0] * 70 if single else WHICH
        for name, build, run, method, params, seeds in _steps([N297] if single else [N200, N297], which,
                                                              random.Random(16), packing, used.cfg.maxbits):
            fresh = make()
            got = []
            for eng in (used, fresh):
                build(eng)
                assert single or (eng.packing() == packing and eng.batch == len(WHICH))
                run(eng)
                got.append(_state(eng, not single))
            fresh.close()
            where = "%s, %s" % (packing or "single N", name)
            assert got[1]["method"] == method and got[1]["params"] == params and got[1]["seeds"] == seeds, where
            assert got[1]["moduli"] == (None if single else WHICH), where
            assert len(got[1]["lines"]) == len(which) and len(set(got[1]["lines"])) == len(which), where
            assert got[0] == got[1], where
        used.close()
