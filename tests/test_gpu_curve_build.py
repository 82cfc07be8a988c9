"""GPU tests of the curve construction on the device (k_build / k_build_multi, gecm_set_curve_build).  The
device build must leave the words the host build uploads — X, Z, s, the stale operands of a failed inversion and the
return value included — on single-N, special-form and multi-modulus contexts, for a fresh build and for a resume, so
that everything downstream (save lines, stage 2) is the same; the directed inputs get their expectation from
tests/suyama_model.py, which tests/test_build_cpu.py checks without a GPU.
The file sorts after tests/test_gpu_cli.py on purpose: test_batch_memory_figure_is_what_a_batch_takes there reads the
device's free memory before and after a small batch and needs a process whose earlier, larger device allocations (the
stage-2 tables made here) have not been freed into the runtime's cache yet."""
import ctypes
import json
import math
import os
import random

import pytest

from conftest import GOLDEN
from suyama_model import N11Q, N40, N65, N415, SIGMA_EDGES, pick_nl, suyama_plain

pytestmark = pytest.mark.gpu

GECM_ERR_ARG, GECM_ERR_STATE = -2, -4
S1 = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "stage1.json")))}
SPECIAL = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "special.json")))}


def _odd_without_small_factors(bits):
    """a fixed odd number of that many bits with no prime factor below 1000: a random sigma meets no failing inversion"""
    small = math.prod(p for p in range(3, 1000, 2) if all(p % q for q in range(3, int(p**0.5) + 1, 2)))
    n = random.Random(bits).getrandbits(bits) | (1 << (bits - 1)) | 1
    while math.gcd(n, small) != 1:
        n += 2
    return n


N600 = _odd_without_small_factors(600)
N1030 = _odd_without_small_factors(1030)
MODULI = {"n40": N40, "n65": N65, "n415": N415, "n1030": N1030}
BATCHES = [1, 63, 64, 65, 200]


def _sigma_list(seed):
    """200 sigmas: random 64-bit values with the edge values among them, one at the head (a batch of 1 meets it), the
    others around the wavefront boundary and in the last, partial wavefront"""
    rnd = random.Random(seed)
    s = [rnd.randrange(6, 1 << 64) for _ in range(200)]
    for pos, edge in zip([0, 31, 62, 63, 64, 130, 199], SIGMA_EDGES[::-1]):
        s[pos] = edge
    return s


def _n_of(case):
    return int(case["save_lines"][0].split("N=0x")[1].split(";")[0], 16)


def _sigmas(case):
    return [int(l.split("SIGMA=")[1].split(";")[0]) for l in case["save_lines"]]


def _build(eng, mode, sigmas, *which):
    eng.set_curve_build(mode)
    rc = eng.build_curves(sigmas, *which)
    assert eng.curve_build() == mode
    return rc


def _words(eng):
    X, Z = eng.download_points()
    return X, Z, eng.download_s()


def _expected(eng, n, sigmas):
    """(X, Z, s, any flag) in the radix of download_points, from the plain Suyama values"""
    r = pow(2, eng.cfg.maxbits, n)
    pl = [suyama_plain(n, s) for s in sigmas]
    return [p[0] * r % n for p in pl], [r] * len(pl), [p[1] * r % n for p in pl], int(any(p[2] for p in pl))


@pytest.fixture(scope="module")
def engines():
    import pyecm
    made = {}

    def get(name, digitbits=52):
        if (name, digitbits) not in made:
            made[name, digitbits] = pyecm.Engine(MODULI[name], digitbits=digitbits)
        return made[name, digitbits]
    yield get
    for e in made.values():
        e.close()


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("name,digitbits", [("n40", 52), ("n65", 52), ("n415", 52), ("n415", 32), ("n1030", 52)])
def test_device_build_leaves_the_words_of_the_host_build(engines, name, digitbits, batch):
    n = MODULI[name]
    eng = engines(name, digitbits)
    assert eng.cfg.dev_limbs == pick_nl(n.bit_length())
    sig = _sigma_list(n % 1000003)[:batch]
    want = _expected(eng, n, sig)
    assert _build(eng, "host", sig) == want[3]
    host = _words(eng)
    assert _build(eng, "device", sig) == want[3]
    dev = _words(eng)
    assert dev == host
    assert dev == want[:3]


@pytest.mark.parametrize("name", ["n40", "n65", "n415", "n1030"])
def test_every_edge_sigma_alone_in_a_batch_of_one(engines, name):
    n = MODULI[name]
    eng = engines(name)
    for s in SIGMA_EDGES:
        want = _expected(eng, n, [s])
        assert _build(eng, "device", [s]) == want[3]
        assert _words(eng) == want[:3], s


def test_failing_inversions_take_the_reference_s_stale_operands():
    """N = 11 q: sigma = 15 loses (16u^3v)^-1 only, sigma = 22 both inverses (test_build_cpu.py checks the gcds)"""
    import pyecm
    sig = [14, 15, 16, 21, 22, 23] + [random.Random(11).randrange(6, 1 << 64) for _ in range(4)]
    assert [suyama_plain(N11Q, s)[2] for s in sig[:6]] == [0, 1, 0, 0, 1, 0]
    eng = pyecm.Engine(N11Q)
    want = _expected(eng, N11Q, sig)
    got = {}
    for mode in ("host", "device"):
        assert _build(eng, mode, sig) == 1
        words = _words(eng)
        assert words == want[:3], mode
        eng.stage1(100)
        got[mode] = (words, eng.save_lines())
    assert got["device"] == got["host"]
    assert _build(eng, "device", [14, 16, 21, 23]) == 0
    eng.close()


@pytest.mark.parametrize("lanes", [1, 8])
@pytest.mark.parametrize("name", ["M251_cofactor_b1_20000_stage2", "M251_cofactor"])
def test_reference_files_of_runs_modulo_a_mersenne_number(name, lanes):
    """Mw = 2^251 - 1 with the report modulus set: the eight save lines of the reference's own runs.  One lane per curve
    runs stage 1 on the special-form twin, which the device build fills from the main context on the device.  The
    reference's own stale operand is in the second case: its sigma 1006 fails on 503 * 54217 (the first case, sigma 7000
    to 7007, meets no failure)"""
    import pyecm
    c = SPECIAL[name]
    sp = c["special"]
    mw = (1 << sp["k"]) + (sp["c"] if sp["sign"] == "+" else -sp["c"])
    eng = pyecm.Engine(mw)
    eng.set_report_modulus(_n_of(c))
    eng.set_lanes_per_curve(lanes)
    sig = _sigmas(c)
    failing = [s for s in sig if suyama_plain(mw, s)[2]]
    assert failing == ([1006] if name == "M251_cofactor" else [])
    assert _build(eng, "device", sig) == (1 if failing else 0)
    eng.stage1(c["B1"])
    assert eng.special_form_used() == (lanes == 1)
    assert [l.rstrip("\n") for l in eng.save_lines()] == c["save_lines"]
    eng.close()


def test_resume_on_a_special_form_context_fills_the_twin_with_the_caller_s_points():
    import pyecm
    c = SPECIAL["M251_cofactor_b1_20000_stage2"]
    mw = (1 << c["special"]["k"]) - 1
    rnd = random.Random(251)
    sig = [1006] + [rnd.randrange(6, 1 << 64) for _ in range(69)]
    xs, zs = [rnd.randrange(mw) for _ in sig], [rnd.randrange(1, mw) for _ in sig]
    eng = pyecm.Engine(mw)
    eng.set_lanes_per_curve(1)
    lines = {}
    for mode in ("host", "device"):
        eng.set_curve_build(mode)
        assert eng.resume(sig, xs, zs) == 1
        assert eng.curve_build() == mode
        s = eng.download_s()
        eng.stage1(500)
        assert eng.special_form_used()
        lines[mode] = (s, eng.save_lines())
    assert lines["device"] == lines["host"]
    eng.close()


@pytest.mark.parametrize("name", ["n415_b1_1000", "n831_b1_1000"])
def test_fixture_save_lines_from_a_device_build(name):
    import pyecm
    case = S1[name]
    eng = pyecm.Engine(_n_of(case), digitbits=int(case["digitbits"]))
    _build(eng, "device", _sigmas(case))
    eng.stage1(case["B1"])
    assert [l.rstrip("\n") for l in eng.save_lines()] == case["save_lines"]
    eng.close()


def _interleave(groups):
    out, i = [], 0
    while any(i < len(g) for g in groups):
        for m, g in enumerate(groups):
            if i < len(g):
                out.append((m, g[i]))
        i += 1
    return out


def _multi_order(with_failure):
    rnd = random.Random(13)
    groups = [[rnd.randrange(6, 1 << 64) for _ in range(k)] for k in (5, 64, 70)]
    groups[0][:3] = [2**64 - 1, 2**63, 6]
    groups[1] = [s if suyama_plain(N11Q, s)[2] == 0 else s + 1 for s in groups[1]]     # sigma = 0, 4, 7 mod 11 fail
    if with_failure:
        groups[1][17] = 15
    order = _interleave(groups)
    return [s for _, s in order], [m for m, _ in order]


def test_multi_modulus_batch_builds_on_the_device():
    """65, 415 (= 11 q) and 600 bits with 5, 64 and 70 curves, interleaved: 59, 0 and 58 padding lanes, which build
    sigma = 0 — no inverse there, and none of the caller's business"""
    import pyecm
    eng = pyecm.MultiEngine([N65, N11Q, N600])
    sig, which = _multi_order(True)
    lines = {}
    for mode in ("host", "device"):
        assert _build(eng, mode, sig, which) == 1
        eng.stage1(1000)
        lines[mode] = eng.save_lines()
    assert len(lines["host"]) == 139 and lines["device"] == lines["host"]
    sig, which = _multi_order(False)
    assert not any(suyama_plain(eng.ns[m], s)[2] for s, m in zip(sig, which))
    for mode in ("host", "device"):
        assert _build(eng, mode, sig, which) == 0
    eng.close()


def test_resume_takes_s_from_the_device_build():
    import pyecm
    sig = [14, 15, 16] + [random.Random(5).randrange(6, 1 << 64) for _ in range(67)]
    eng = pyecm.Engine(N11Q)
    assert _build(eng, "host", sig) == 1
    eng.stage1(1000)
    lines = eng.save_lines()
    eng.stage2(50000)
    straight = eng.download_acc()
    for mode in ("host", "device"):
        eng.set_curve_build(mode)
        assert eng.resume_lines(lines, b1_done=1000) == 1
        assert eng.curve_build() == mode
        assert eng.save_lines() == lines
        eng.stage2(50000)
        assert eng.download_acc() == straight, mode
    eng.close()


def test_multi_modulus_resume_takes_s_from_the_device_build():
    import pyecm
    eng = pyecm.MultiEngine([N65, N11Q, N600])
    sig, which = _multi_order(True)
    assert _build(eng, "host", sig, which) == 1
    eng.stage1(1000)
    lines = eng.save_lines()
    eng.stage2(50000)
    straight = eng.accs()
    for mode in ("host", "device"):
        eng.set_curve_build(mode)
        assert eng.resume_lines(lines, b1_done=1000) == 1
        assert eng.curve_build() == mode
        assert eng.save_lines() == lines
        eng.stage2(50000)
        assert eng.accs() == straight, mode
    eng.close()


def test_mode_and_its_neighbours():
    import pyecm
    eng = pyecm.Engine(N415)
    assert eng.curve_build() == "host"
    eng.set_curve_build("device")
    assert eng.curve_build() == "host"                 # takes effect at the next build
    with pytest.raises(ValueError):
        eng.set_curve_build("gpu")
    assert pyecm.lib.gecm_set_curve_build(eng._h, 2) == GECM_ERR_ARG
    assert pyecm.lib.gecm_download_s(eng._h, eng.empty(1)) == GECM_ERR_ARG      # no batch yet
    sig = _sigma_list(1)[:70]
    words = []
    for mode in ("device", "host", "device", "device", "host"):
        _build(eng, mode, sig)
        words.append(_words(eng))
    assert all(w == words[0] for w in words)
    eng.set_curve_build("device")
    arr = (ctypes.c_uint64 * 2)(7, 5)
    assert pyecm.lib.gecm_build_curves(eng._h, arr, 2) == GECM_ERR_ARG     # the argument checks stay on the host
    assert eng.curve_build() == "host" and _words(eng) == words[0]         # and the batch stays
    eng.close()
    multi = pyecm.MultiEngine([N65, N415])
    multi.set_curve_build("device")
    multi.build_curves([7, 8, 9], [0, 1, 0])
    assert multi.curve_build() == "device"
    buf = (ctypes.c_uint64 * (3 * multi.cfg.nwords))()
    assert pyecm.lib.gecm_download_s(multi._h, buf) == GECM_ERR_STATE
    with pytest.raises(pyecm.GecmError):
        multi.build_curves([7, 8], [0, 2])             # no such modulus
    multi.close()
