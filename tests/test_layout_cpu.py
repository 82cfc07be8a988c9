"""CPU test (no GPU) of the position layout of a multi-modulus batch, gecm_layout_make in host/gecm_mod.c, against a model
written from DESIGN.md §13 (wave packing: the moduli in order, each one's curves in the caller's order, padded to whole
blocks of 64) and §16 (lane packing: back to back, the batch's tail padded on modulus 0)."""
import ctypes
import random

import pytest

PAD = 0xFFFFFFFF
u32p, szp = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_size_t)


class Layout(ctypes.Structure):
    """gecm_layout of host/gecm_mod.h"""
    _fields_ = [("nuser", ctypes.c_size_t), ("total", ctypes.c_size_t), ("ngroups", ctypes.c_size_t), ("slot", u32p),
                ("pos_user", u32p), ("pos_grp", u32p), ("blocks", u32p), ("goff", szp), ("cnt", szp)]


def model(which, ngroups, lane):
    """(total, slot, pos_user, pos_grp, blocks, goff, cnt) as DESIGN.md states the layout"""
    up = lambda v: (v + 63) // 64 * 64
    cnt = [which.count(g) for g in range(ngroups)]
    span = cnt if lane else [up(c) for c in cnt]
    goff = [sum(span[:g]) for g in range(ngroups)]
    total = up(sum(span))
    pos_user, pos_grp = [PAD] * total, [0] * total
    for g in range(ngroups):
        pos_grp[goff[g]:goff[g] + span[g]] = [g] * span[g]
    seen, slot = [0] * ngroups, []
    for i, g in enumerate(which):
        slot.append(goff[g] + seen[g])
        pos_user[slot[-1]] = i
        seen[g] += 1
    return total, slot, pos_user, pos_grp, None if lane else pos_grp[::64], goff, cnt


def _by_counts(counts, interleave=False):
    which = [g for g, c in enumerate(counts) for _ in range(c)]
    if interleave:                                   # modulus 0's curve comes second: slot is not monotone
        which = which[1:2] + which[:1] + which[2:]
    return which, len(counts)


_rng = random.Random(7300)
CASES = {"1_65_interleaved": _by_counts((1, 65), interleave=True), "64_64": _by_counts((64, 64)),
         "63_0_1": _by_counts((63, 0, 1)), "0_0_5": _by_counts((0, 0, 5)), "128": _by_counts((128,)),
         "random_7_moduli_300": ([_rng.randrange(7) for _ in range(300)], 7)}


@pytest.fixture(scope="module")
def pyecm():
    import pyecm
    return pyecm


@pytest.fixture(scope="module")
def raw(pyecm):
    lib = ctypes.CDLL(pyecm.lib._name)
    lib.gecm_layout_make.argtypes = [ctypes.POINTER(Layout), u32p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int]
    lib.gecm_layout_make.restype = ctypes.c_int
    lib.gecm_layout_free.argtypes = [ctypes.POINTER(Layout)]
    lib.gecm_layout_free.restype = None
    return lib


@pytest.mark.parametrize("packing", ["wave", "lane"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_layout_is_the_documented_one(pyecm, raw, case, packing):
    which, ngroups = CASES[case]
    lane, batch = packing == "lane", len(which)
    assert sorted(set(which) | set(range(ngroups))) == list(range(ngroups))
    lay = Layout()
    idx = (ctypes.c_uint32 * batch)(*which)
    assert raw.gecm_layout_make(ctypes.byref(lay), idx, batch, ngroups, pyecm._PACKINGS[packing]) == 0
    total = lay.total
    got = (total, lay.slot[:batch], lay.pos_user[:total], lay.pos_grp[:total], lay.blocks[:total // 64] if lay.blocks else None,
           lay.goff[:ngroups], lay.cnt[:ngroups])
    assert (lay.nuser, lay.ngroups) == (batch, ngroups)
    raw.gecm_layout_free(ctypes.byref(lay))
    assert not lay.slot and not lay.pos_user and not lay.pos_grp and not lay.blocks and not lay.goff and not lay.cnt and lay.total == 0
    raw.gecm_layout_free(ctypes.byref(lay))                    # and again: nothing left to free
    assert got == model(which, ngroups, lane)
    total, slot, pos_user, pos_grp, blocks, goff, cnt = got
    assert total == pyecm.multi_positions(cnt, packing) and total % 64 == 0 and total >= batch
    assert len(set(slot)) == batch                             # injective
    assert [pos_user[slot[i]] for i in range(batch)] == list(range(batch))
    assert [pos_grp[slot[i]] for i in range(batch)] == which
    assert sorted(p for p in pos_user if p != PAD) == list(range(batch))
    if lane:
        assert blocks is None
        assert pos_user[batch:] == [PAD] * (total - batch) and PAD not in pos_user[:batch] and total - batch < 64
        assert pos_grp[batch:] == [0] * (total - batch)
    else:
        assert len(blocks) == total // 64
        for b in range(total // 64):
            assert set(pos_grp[64 * b:64 * b + 64]) == {blocks[b]}
        assert total == sum((c + 63) // 64 * 64 for c in cnt)


def test_layout_refuses_what_it_cannot_lay_out(pyecm, raw):
    lay = Layout()
    idx = (ctypes.c_uint32 * 3)(0, 2, 1)
    for batch, ngroups in ((3, 2), (0, 3), (3, 0)):            # an index past the moduli, no curves, no moduli
        assert raw.gecm_layout_make(ctypes.byref(lay), idx, batch, ngroups, pyecm.PACK_WAVE) == -2
        assert not lay.slot and not lay.cnt and lay.total == 0
    assert raw.gecm_layout_make(ctypes.byref(lay), None, 3, 3, pyecm.PACK_LANE) == -2
