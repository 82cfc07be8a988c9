"""No device: the host side of lane packing (include/gecm.h gecm_set_multi_packing) — the symbols, the
answers that need no context, and the one rounding rule of a multi-modulus batch's positions."""
import ctypes

import pytest

COUNTS = [1, 63, 64, 65, 200, 1, 3, 64, 2, 17]
NEW = ["gecm_set_multi_packing", "gecm_get_multi_packing", "gecm_multi_positions", "gecm_multi_packing_max_bits"]


@pytest.fixture(scope="module")
def pyecm():
    import pyecm
    return pyecm


def _positions(pyecm, counts, packing):
    arr = (ctypes.c_size_t * max(1, len(counts)))(*counts)
    return pyecm.lib.gecm_multi_positions(arr, len(counts), packing)


def test_symbols_are_exported_and_listed(pyecm):
    for s in NEW:
        assert hasattr(pyecm.lib, s), s
        assert s in pyecm.EXPORTS, s
    assert (pyecm.PACK_WAVE, pyecm.PACK_LANE) == (0, 1)
    assert hasattr(pyecm.MultiEngine, "set_packing") and hasattr(pyecm.MultiEngine, "packing")


def test_null_context_answers(pyecm):
    ERR_ARG = -2
    assert pyecm.lib.gecm_set_multi_packing(None, pyecm.PACK_LANE) == ERR_ARG
    assert b"gecm_set_multi_packing" in pyecm.lib.gecm_last_error()
    assert pyecm.lib.gecm_set_multi_packing(None, pyecm.PACK_WAVE) == ERR_ARG
    assert pyecm.lib.gecm_get_multi_packing(None) == ERR_ARG


def test_a_bad_packing_value_is_an_argument_error(pyecm):
    # the value is checked before the context is looked at: any context, even none, gets GECM_ERR_ARG for it
    for bad in (-1, 2, 64):
        assert pyecm.lib.gecm_set_multi_packing(None, bad) == -2
    with pytest.raises(ValueError):
        pyecm.MultiEngine.set_packing(object(), "dense")


def test_positions_of_both_packings(pyecm):
    """wave: every number padded to whole wavefronts, 64 + 64 + 64 + 128 + 256 + 64 + 64 + 64 + 64 + 64 = 896 (the 200
    curves of one number take four wavefronts); lane: 480 curves back to back, padded once, 512"""
    assert _positions(pyecm, COUNTS, pyecm.PACK_WAVE) == 896 == sum((c + 63) // 64 * 64 for c in COUNTS)
    assert _positions(pyecm, COUNTS, pyecm.PACK_LANE) == 512 == (sum(COUNTS) + 63) // 64 * 64
    assert pyecm.multi_positions(COUNTS, "wave") == 896 and pyecm.multi_positions(COUNTS, "lane") == 512


def test_largest_number_of_each_packing(pyecm):
    assert pyecm.lib.gecm_multi_packing_max_bits(pyecm.PACK_LANE) == 415 == 28 * 15 - 5
    assert pyecm.lib.gecm_multi_packing_max_bits(pyecm.PACK_WAVE) == 0
    assert pyecm.lib.gecm_multi_packing_max_bits(2) == -2


def test_positions_of_empty_and_exact_batches(pyecm):
    for packing in (pyecm.PACK_WAVE, pyecm.PACK_LANE):
        assert _positions(pyecm, [], packing) == 0
        assert pyecm.lib.gecm_multi_positions(None, 0, packing) == 0
        assert _positions(pyecm, [64], packing) == 64
        assert _positions(pyecm, [65], packing) == 128
    # eight curves on each of sixteen numbers: the shape the packing is for
    assert _positions(pyecm, [8] * 16, pyecm.PACK_WAVE) == 1024
    assert _positions(pyecm, [8] * 16, pyecm.PACK_LANE) == 128
