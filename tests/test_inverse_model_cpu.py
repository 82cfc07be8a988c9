"""CPU: the Python restatement of the device inversion (tests/divsteps_model.py) on the directed inputs that
tests/test_gpu_inverse.py hands to the device: it inverts correctly, converges within the batches the library allots,
stays inside the signed top limb, and the inputs cover what the end game of fe_invert can meet."""
import ctypes
import math
import os
import subprocess

import pytest

import divsteps_model as M
from conftest import ROOT

LIB = os.path.join(ROOT, "avx-ecm_amd", "libgecm.so")

# What the seeded search of divsteps_model.mine() reached (20,100 inputs, 134 on each of the 150 moduli), and the 300
# late-convergence inputs it froze into divsteps_model.MINED:
#   d after the negate: [-N,0) 10,273 times, [0,N) 9,827 times; [-2N,-N) and [N,2N) never.  d was in [-N,0) exactly when
#   the final f was negative, i.e. d stood in [0, N) before the negate every time: one +N step is exercised on half of all
#   inputs, the second +N and the final -N on none.  Cutting the run at the batch g reached 0 (no idle batch after it)
#   still gave only those two ranges.
#   least slack: 1 batch of 28 steps (192-bit moduli, 15 of 16 batches); 4 batches at 416 bits, 10 at 1031.
REACHABLE = {1, 2}


def _cases():
    return [(nl, bits) for nl, bits in M.edge_bits()]


@pytest.mark.parametrize("nl,bits", _cases(), ids=["nl%d_%dbit" % c for c in _cases()])
def test_model_on_the_directed_inputs(nl, bits):
    """Correctness against pow and math.gcd, convergence within inv_iters batches, magnitudes within the signed top limb,
    and both reachable d-ranges and both signs of f, for the five moduli of one bit length.

    Reachable ranges, from the search recorded above: [-N,0) and [0,N).  [-2N,-N) and [N,2N) were never reached, by the
    search or by the directed inputs; nothing here pretends otherwise: the second +N step and the final -N of fe_invert
    stay unexercised by any input known to this suite."""
    assert M.dev_limbs(bits) == nl
    iters = M.inv_iters(bits)
    bound = M.top_limb_bound(nl)
    for kind in M.KINDS:
        n = M.modulus(bits, kind)
        xs = M.operands(n, bits, kind, nl, pow(2, M.ref_maxbits(bits), n))
        res = M.invert_many(n, xs, iters, nl)
        ranges, signs = set(), set()
        for x, r in zip(xs, res):
            g = math.gcd(x, n)
            assert r["gcd"] == g, (bits, kind, x)
            assert r["inv"] == (pow(x, -1, n) if g == 1 else None), (bits, kind, x)
            assert r["converged"] is not None and r["converged"] <= iters, (bits, kind, x, r["converged"], iters)
            assert max(r["maxabs"]) < bound, (bits, kind, x)
            assert r["in_reach"], (bits, kind, x)
            ranges.add(r["d_range"])
            signs.add(r["f_negative"])
        assert ranges >= REACHABLE and signs == {False, True}, (bits, kind, ranges, signs)


def test_the_search_is_reproducible_on_one_modulus():
    """the frozen indices of one modulus are what mine() picks again, and they are its latest convergers"""
    bits, kind = 192, "random"
    n = M.modulus(bits, kind)
    xs = [M.searched(n, bits, kind, i) for i in range(M.SEARCH_PER_MODULUS)]
    res = M.invert_many(n, xs)
    order = sorted(range(len(xs)), key=lambda i: -res[i]["converged"])
    assert tuple(sorted(order[:2])) == M.MINED[(bits, kind)]
    assert M.inv_iters(bits) - res[order[0]]["converged"] == 1          # the least slack met anywhere: one batch
    assert {r["d_range"] for r in res} == REACHABLE


def test_inv_iters_formula_and_library_constants():
    """inv_iters as computed here is what gecm_mod_setup stores, with the other constants the inversion reads"""
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "avx-ecm_amd"), "-j8"])      # as tests/test_abi_cpu.py
    lib = ctypes.CDLL(LIB)
    MAXL = 136

    class Mpl(ctypes.Structure):
        _fields_ = [("n", ctypes.c_int), ("d", ctypes.c_uint32 * MAXL)]

    u32p = ctypes.POINTER(ctypes.c_uint32)

    class Mod(ctypes.Structure):                                        # gecm_mod, host/gecm_mod.h
        _fields_ = [("digitbits", ctypes.c_int), ("nwords", ctypes.c_int), ("maxbits", ctypes.c_int),
                    ("nbits", ctypes.c_int), ("nl", ctypes.c_int), ("N", Mpl), ("N_report", Mpl),
                    ("have_report", ctypes.c_int), ("rref_mod_n", Mpl), ("rint_mod_n", Mpl), ("ref_to_int", Mpl),
                    ("int_to_ref", Mpl), ("rho_ref", ctypes.c_uint64), ("rho28", ctypes.c_uint32), ("n28", u32p),
                    ("kp28", u32p), ("one28", u32p), ("fix28", u32p), ("r3_28", u32p), ("finv28", u32p),
                    ("inv_iters", ctypes.c_uint32)]

    PICK = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_int)
    pick = PICK(lambda b: M.dev_limbs(b) if b <= M.LIMB * M.BUILT[-1] - 5 else 0)
    lib.gecm_mod_setup.argtypes = [ctypes.POINTER(Mod), ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, PICK]
    lib.gecm_mod_free.argtypes = [ctypes.POINTER(Mod)]

    def limbs(p, nl):
        return sum(p[i] << (M.LIMB * i) for i in range(nl))

    for nl, bits in M.edge_bits():
        for kind, digitbits in (("random", 52), ("1mod2^28", 32)):
            n = M.modulus(bits, kind)
            m = Mod()
            assert lib.gecm_mod_setup(ctypes.byref(m), b"test", str(n).encode(), digitbits, 0, pick) == 0
            try:
                assert (m.nbits, m.nl, m.maxbits) == (bits, nl, M.ref_maxbits(bits, digitbits))
                assert m.inv_iters == M.inv_iters(bits)
                assert m.inv_iters * M.LIMB >= (45907 * bits + 26313) // 19929 + 1
                rint, rref = 1 << (M.LIMB * nl), 1 << m.maxbits
                assert (-m.rho28) % (1 << M.LIMB) == pow(n, -1, 1 << M.LIMB)
                assert limbs(m.n28, nl) == n
                assert limbs(m.r3_28, nl) == pow(rint, 3, n)
                assert limbs(m.finv28, nl) == rref * rref * pow(rint, -1, n) % n
            finally:
                lib.gecm_mod_free(ctypes.byref(m))
