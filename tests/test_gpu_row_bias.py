"""The 32-lane stage-1 kernel with the rounding bias of a multiply carried by its last two hand-overs (one limb per lane:
avx-ecm_amd/csrc/gecm_row.hpp; two and three limbs per lane keep the add), against the oracle library.
The fold leans on one fact per shape, that nothing leaves the top lane of a row, so every one-limb-per-lane shape runs at
the shortest and at the longest modulus of its limb class; the other shapes and a batch with two curves per wavefront on the
benchmark's modulus run the same way.  Every case: the 32-lane layout forced, B1 = 2000, the kernel asserted by name, the
save line of every curve (canonical X and Z) equal to the oracle's, byte for byte."""
import ctypes
import os
import random

import pytest

import divsteps_model as M
from conftest import ROOT

pytestmark = pytest.mark.gpu

B1 = 2000
NQ1_EDGES = [(nl, bits) for nl, bits in M.edge_bits() if nl <= 15]       # 9, 11, 13, 15 and 16 rows: both ends of each class


@pytest.fixture(scope="module")
def orc():
    L = ctypes.CDLL(os.path.join(ROOT, "oracle", "libecm_oracle.so"))
    L.orc_create.restype = ctypes.c_void_p
    L.orc_create.argtypes = [ctypes.c_char_p, ctypes.c_int]
    L.orc_destroy.argtypes = [ctypes.c_void_p]
    L.orc_stage1_line.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t,
                                  ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)]
    return L


def _oracle_lines(orc, n, digitbits, sigmas):
    c = orc.orc_create(str(n).encode(), digitbits)
    line = ctypes.create_string_buffer(16384)
    out = []
    for s in sigmas:
        orc.orc_stage1_line(c, s, B1, line, len(line), None, 0, None)
        out.append(line.value.decode())
    orc.orc_destroy(c)
    return out


def _rows_against_the_oracle(orc, n, nl, sig, digitbits=52):
    import pyecm
    want = _oracle_lines(orc, n, digitbits, sig)
    eng = pyecm.Engine(n, digitbits=digitbits)
    assert eng.cfg.dev_limbs == nl
    eng.set_special_form(False)
    eng.set_lanes_per_curve(32)
    eng.build_curves(sig)
    eng.stage1(B1)
    assert eng.lanes_per_curve() == 32 and not eng.special_form_used()
    assert eng.last_kernel_name() == "k_stage1_row<%d, %d, false>" % ((nl + 1 + 15) // 16, nl + 1)
    got = eng.save_lines()
    eng.close()
    assert len(got) == len(sig)
    differ = [k for k in range(len(sig)) if got[k] != want[k]]
    assert not differ, (nl, n.bit_length(), differ[:8])
    assert all("X=0x" in l and "Z=0x" in l for l in got)


@pytest.mark.parametrize("nl,bits", NQ1_EDGES, ids=["nl%d_%dbit" % c for c in NQ1_EDGES])
def test_one_limb_per_lane_at_both_ends_of_the_class(orc, nl, bits):
    n = M.modulus(bits, "random")
    rng = random.Random("row bias:%d" % bits)
    _rows_against_the_oracle(orc, n, nl, [rng.randrange(6, 1 << 63) for _ in range(8)])


@pytest.mark.parametrize("nl,bits", [(30, 831), (37, 1023)], ids=["two_limbs_831bit", "three_limbs_1023bit"])
def test_two_and_three_limbs_per_lane(orc, nl, bits):
    n = M.modulus(bits, "random")
    rng = random.Random("row bias:%d" % bits)
    _rows_against_the_oracle(orc, n, nl, [rng.randrange(6, 1 << 63) for _ in range(8)], 52 if bits < 1000 else 32)


def test_two_curves_per_wavefront_on_the_benchmark_modulus(orc):
    n = random.Random(415).getrandbits(415) | (1 << 414) | 1              # bench.py's N
    _rows_against_the_oracle(orc, n, 15, list(range(1000, 1070)))
