"""CPU: the argument checks of the multi-modulus ABI (include/gecm.h gecm_create_multi) come before any device is
opened, so they hold on a machine without one."""
import ctypes

import pytest


def _create(ns, digitbits=52):
    import pyecm
    h = ctypes.c_void_p()
    strs = [None if n is None else str(n).encode() for n in ns]
    arr = (ctypes.c_char_p * max(1, len(strs)))(*strs)
    rc = pyecm.lib.gecm_create_multi(ctypes.byref(h), 0, arr, len(strs), digitbits)
    return rc, pyecm.lib.gecm_last_error().decode(), h


@pytest.mark.parametrize("ns, digitbits, text", [
    ([], 52, "gecm_create_multi: the list of moduli is empty"),
    ([1000003], 48, "gecm_create_multi: bad argument (digitbits must be 52 or 32)"),
    ([1000003, 1000004], 52, "gecm_create_multi: N[1] must be an odd integer >= 3"),
    ([1], 52, "gecm_create_multi: N[0] must be an odd integer >= 3"),
    ([1000003, None], 52, "gecm_create_multi: N[1] must be an odd integer >= 3"),
    ([1000003, "12x"], 52, "gecm_create_multi: N[1] must be an odd integer >= 3"),
    ([(1 << 1099) + 1], 32, "gecm_create_multi: N[0] of 1100 bits is larger than this build supports"),
])
def test_create_multi_rejects_bad_lists_before_touching_a_device(ns, digitbits, text):
    rc, err, h = _create(ns, digitbits)
    assert rc == -2 and err.startswith(text) and not h.value


def test_multi_calls_refuse_a_null_context():
    import pyecm
    L = pyecm.lib
    sig = (ctypes.c_uint64 * 1)(10)
    idx = (ctypes.c_uint32 * 1)(0)
    assert L.gecm_build_curves_multi(None, sig, idx, 1) == -2
    assert L.gecm_moduli(None) == 0
    assert L.gecm_curve_modulus(None, 0) == -2
    buf = ctypes.create_string_buffer(64)
    assert L.gecm_curve_acc(None, 0, buf, len(buf)) == -2


def test_multi_symbols_are_exported():
    import pyecm
    for s in ("gecm_create_multi", "gecm_build_curves_multi", "gecm_moduli", "gecm_curve_modulus", "gecm_curve_acc"):
        assert s in pyecm.EXPORTS and hasattr(pyecm.lib, s)
    assert hasattr(pyecm, "MultiEngine")
