"""Wide contexts (gecm_create_wide): ECM stage 1 for numbers of 1032 to 1311 bits on the 32-lane row kernel
at 41, 44 and 48 rows, everything after the kernel on the host.  The expected save lines are the oracle library's
(oracle/libecm_oracle.so: orc_stage1_line), byte for byte; the PARAM 1 and 3 curves are checked against the plain binary
ladder of tests/param_model.py.  Without the feature every case fails at the missing gecm_create_wide."""
import ctypes
import math
import os
import random
from concurrent.futures import ThreadPoolExecutor

import pytest

import wide_row_model as W
from conftest import ROOT
from param_model import param_d
from xladder import ladder_point, stage1_multiplier

pytestmark = pytest.mark.gpu

B1 = 2000
GECM_ERR_ARG, GECM_ERR_STATE = -2, -4
REFUSAL = "not available on a wide context (gecm_create_wide): "


@pytest.fixture(scope="module")
def orc():
    L = ctypes.CDLL(os.path.join(ROOT, "oracle", "libecm_oracle.so"))
    L.orc_create.restype = ctypes.c_void_p
    L.orc_create.argtypes = [ctypes.c_char_p, ctypes.c_int]
    L.orc_destroy.argtypes = [ctypes.c_void_p]
    L.orc_stage1_line.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t,
                                  ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)]
    return L


def _oracle(orc, n, digitbits, sigmas):
    """(save line, decimal factor or "") of every sigma; a curve of this size takes the oracle 0.1 s, so the sigmas are
    shared out over threads, each with a context of its own (the library keeps no state outside a context)"""
    def some(part):
        c = orc.orc_create(str(n).encode(), digitbits)
        line, fac = ctypes.create_string_buffer(16384), ctypes.create_string_buffer(4096)
        out = []
        for s in part:
            orc.orc_stage1_line(c, s, B1, line, len(line), fac, len(fac), None)
            out.append((line.value.decode(), fac.value.decode()))
        orc.orc_destroy(c)
        return out
    workers = max(1, min(8, os.cpu_count() or 1, len(sigmas)))
    parts = [sigmas[w::workers] for w in range(workers)]
    with ThreadPoolExecutor(workers) as pool:
        res = list(pool.map(some, parts))
    out = [None] * len(sigmas)
    for w, r in enumerate(res):
        out[w::workers] = r
    return out


def _sigmas(tag, count=8):
    rng = random.Random("wide:%s" % tag)
    return [rng.randrange(6, 1 << 63) for _ in range(count)]


def _wide_engine(n, digitbits=52):
    import pyecm
    eng = pyecm.Engine(n, digitbits=digitbits, wide=True)
    nl = W.wide_nl(n.bit_length())
    assert eng.is_wide() and eng.cfg.dev_limbs == nl and eng.cfg.nbits == n.bit_length()
    return eng, nl


def _lines_against_the_oracle(orc, n, sig, digitbits=52):
    want = [l for l, _ in _oracle(orc, n, digitbits, sig)]
    eng, nl = _wide_engine(n, digitbits)
    eng.build_curves(sig)
    eng.stage1(B1)
    assert eng.lanes_per_curve() == 32
    assert eng.last_kernel_name() == "k_stage1_row<3, %d, false>" % (nl + 1)
    assert eng.special_form() == (False, 0, 0) and not eng.special_form_used()
    got = eng.save_lines()
    eng.close()
    differ = [k for k in range(len(sig)) if got[k] != want[k]]
    assert len(got) == len(sig) and not differ, (nl, n.bit_length(), differ[:8])
    assert all("X=0x" in l and "Z=0x" in l for l in got)


# ---- 1. both ends of every class ----
ENDS = [(nl, bits) for nl, lo, hi in W.WIDE_CLASSES for bits in (lo, hi)]


@pytest.mark.parametrize("nl,bits", ENDS, ids=["nl%d_%dbit" % c for c in ENDS])
def test_both_ends_of_every_class(orc, nl, bits):
    assert W.wide_nl(bits) == nl
    _lines_against_the_oracle(orc, W.modulus(bits, "random"), _sigmas(bits))


def test_the_largest_number_in_the_32_bit_format(orc):
    _lines_against_the_oracle(orc, W.modulus(1311, "random"), _sigmas("1311/32"), digitbits=32)


# ---- 2. directed moduli on the full 48 rows ----
DIRECTED = {"2^1311-1": (1 << 1311) - 1, "1mod2^28": W.modulus(1311, "1mod2^28"), "2^1310+1": (1 << 1310) + 1,
            "2^1277-1": (1 << 1277) - 1}


@pytest.mark.parametrize("name", sorted(DIRECTED))
def test_directed_moduli_on_48_rows(orc, name):
    n = DIRECTED[name]
    assert W.wide_nl(n.bit_length()) == 47
    _lines_against_the_oracle(orc, n, _sigmas(name))


def test_m1277_opens_no_twin():
    import pyecm
    eng, _ = _wide_engine((1 << 1277) - 1)
    k = ctypes.c_int(-1)
    limbs = ctypes.c_int(-1)
    assert pyecm.lib.gecm_get_special_form(eng._h, ctypes.byref(k), ctypes.byref(limbs)) == 0
    assert (k.value, limbs.value) == (0, 0)
    eng.close()


# ---- 3., 4. two curves per wavefront over more than one block; the same batch on a cut tape ----
N1247 = W.modulus(1247, "random")
SIG70 = _sigmas("70 curves", 70)


@pytest.fixture(scope="module")
def lines70(orc):
    return [l for l, _ in _oracle(orc, N1247, 52, SIG70)]


def test_curve_to_lane_mapping(lines70):
    eng, nl = _wide_engine(N1247)
    assert nl == 47
    eng.build_curves(SIG70)
    eng.stage1(B1)
    done, total = eng.stage1_progress()
    assert (done, total) == (1, 1)
    got = eng.save_lines()
    eng.close()
    assert [k for k in range(70) if got[k] != lines70[k]] == []


def test_cut_tape_chains_lazy_values(lines70, monkeypatch):
    monkeypatch.setenv("GECM_TAPE_CHUNK", "64")
    eng, _ = _wide_engine(N1247)
    eng.build_curves(SIG70)
    eng.stage1(B1)
    done, total = eng.stage1_progress()
    assert total > 1 and done == total
    got = eng.save_lines()
    eng.close()
    assert [k for k in range(70) if got[k] != lines70[k]] == []


# ---- 5. the factor path ----
# N = P * Q of 1250 bits; with these sigmas curves 1, 5, 6 and 13 find P at B1 = 2000 (chosen with the oracle)
P = 1385431279
Q = int("11336616507872388320324536109293682081480499315690090425437690889838648485296953215768288357838614758427079191853705"
        "43716198843419101800668302982587961418076161933898104524539270829342704665377867064664822664655765064118911801209580"
        "68490997627528454476972287610385888041492311636874805969210520950470678525060144592246875605345394094280745772776779"
        "39032482844371254051")
SIG_F = [7310421090297630436, 5652851901138782420, 4296112787267770884, 5128414506321992322, 8317814026605312938,
         977063121815197952, 9024893002221764081, 8901469297606833654, 637436498450426190, 7266672129539821187,
         3004797510859293420, 9205058067026272456, 6659623280115135043, 7075810897278524349, 534083427263368422,
         3593373292793039963]
FINDERS = [1, 5, 6, 13]


def _factor_answers(eng, sig):
    eng.build_curves(sig)
    eng.stage1(B1)
    found, first = eng.scan_factors(1)
    flags = [int(eng.curve_flag(1, k)) for k in range(len(sig))]
    facs = [eng.stage1_factor(k) for k in range(len(sig))]
    return found, first, flags, facs, eng.save_lines()


def test_factor_path(orc):
    n = P * Q
    assert n.bit_length() == 1250
    want = _oracle(orc, n, 52, SIG_F)
    assert [k for k, (_, f) in enumerate(want) if f] == FINDERS and all(want[k][1] == str(P) for k in FINDERS)
    eng, _ = _wide_engine(n)
    found, first, flags, facs, lines = _factor_answers(eng, SIG_F)
    eng.close()
    assert (found, first) == (len(FINDERS), FINDERS[0])
    assert flags == [int(k in FINDERS) for k in range(16)]
    for k in range(16):
        assert (str(facs[k][0]) if facs[k] else "") == want[k][1], k
    assert lines == [l for l, _ in want]


def test_factor_path_with_a_report_modulus(orc):
    f = 1000003                                       # the context works modulo N f, the lines and the factors are N's
    n = P * Q
    want = _oracle(orc, n * f, 52, SIG_F)
    eng, _ = _wide_engine(n * f)
    eng.set_report_modulus(n)
    found, first, flags, facs, lines = _factor_answers(eng, SIG_F)
    eng.close()
    head = "N=0x%x;" % n
    for k in range(16):
        line_nf, g_dec = want[k]
        g = math.gcd(int(g_dec), n) if g_dec else 1    # what the curve found modulo N f, seen from N
        proper = 1 < g < n
        assert flags[k] == int(proper), k
        assert (facs[k][0] if facs[k] else None) == (g if proper else None), k
        assert head in lines[k] and lines[k] == line_nf.replace("N=0x%x;" % (n * f), head), k
    assert found == sum(flags) and first == flags.index(1)
    assert found >= len(FINDERS)


# ---- 6. PARAM 1 and 3 curves ----
def test_param_1_and_3_curves():
    n = N1247
    curves = [(1, 7), (1, (1 << 63) + 12345), (1, (1 << 64) - 1), (3, 7), (3, (1 << 32) - 1), (3, 123456789), (0, 1000),
              (0, 1001)]
    eng, _ = _wide_engine(n)
    eng.build_curves([s for _, s in curves], params=[p for p, _ in curves])
    eng.stage1(B1)
    lines = eng.save_lines()
    eng.close()
    k1 = stage1_multiplier(B1)
    for (param, sigma), line in zip(curves, lines):
        fields = dict(f.strip().split("=", 1) for f in line.strip().rstrip(";").split(";"))
        assert int(fields["SIGMA"]) == sigma and int(fields["B1"]) == B1 and int(fields["N"], 16) == n
        assert ("PARAM" in fields) == (param != 0) and int(fields.get("PARAM", 0)) == param
        if param == 0:
            continue
        X, Z = ladder_point(n, 2, param_d(param, sigma, n), k1)
        gx, gz = int(fields["X"], 16), int(fields["Z"], 16)
        # the same projective point: the PRAC chain and the ladder scale X and Z differently (a Z that shares a factor with n
        # included: this n has small ones)
        assert 0 <= gx < n and 0 <= gz < n and (gx, gz) != (0, 0)
        assert gx * Z % n == X * gz % n, (param, sigma)


# ---- 7. refusals ----
def test_refusals_leave_the_batch_as_it_was():
    import pyecm
    lib = pyecm.lib
    n = W.modulus(1100, "random")
    sig = _sigmas("refusals", 4)
    eng, _ = _wide_engine(n)
    eng.build_curves(sig)
    eng.stage1(B1)
    before = eng.save_lines()
    h = eng._h
    nw = eng.cfg.nwords
    buf = (ctypes.c_uint64 * (nw * 4))()
    u32 = (ctypes.c_uint32 * 64)()
    txt = ctypes.create_string_buffer(8192)
    u64 = (ctypes.c_uint64 * 4)(*sig)
    calls = {
        "gecm_stage2_init": lambda: lib.gecm_stage2_init(h, 0, 0),
        "gecm_stage2": lambda: lib.gecm_stage2(h, 100000, 0, 0),
        "gecm_stage2_prepare": lambda: lib.gecm_stage2_prepare(h, 100000, 0, 0),
        "gecm_stage2_pair": lambda: lib.gecm_stage2_pair(h, 0, None, None, 0),
        "gecm_stage2_factor": lambda: lib.gecm_stage2_factor(h, 0, txt, len(txt), None),
        "gecm_scan_factors(stage 2)": lambda: lib.gecm_scan_factors(h, 2, None),
        "gecm_download_acc": lambda: lib.gecm_download_acc(h, buf),
        "gecm_curve_acc": lambda: lib.gecm_curve_acc(h, 0, txt, len(txt)),
        "the L0 operators": lambda: lib.gecm_vecmulmod(h, buf, buf, buf, 4),
        "gecm_vecinvmod": lambda: lib.gecm_vecinvmod(h, buf, buf, buf, 4),
        "gecm_vecrawop": lambda: lib.gecm_vecrawop(h, 0, 0, u32, u32, u32, 1),
        "gecm_get_one": lambda: lib.gecm_get_one(h, buf),
        "gecm_upload_points": lambda: lib.gecm_upload_points(h, buf, buf, buf, 4),
        "gecm_download_points": lambda: lib.gecm_download_points(h, buf, buf),
        "gecm_download_s": lambda: lib.gecm_download_s(h, buf),
        "gecm_resume_points": lambda: lib.gecm_resume_points(h, u64, buf, buf, 4, B1),
        "gecm_stage1_extend_segment": lambda: lib.gecm_stage1_extend(h, B1, 2 * B1),
        "gecm_normalize_points": lambda: lib.gecm_normalize_points(h),
        "gecm_format_save_line_std": lambda: lib.gecm_format_save_line_std(h, 0, txt, len(txt)),
        "gecm_build_seeds": lambda: lib.gecm_build_seeds(h, 1, buf, buf, 4, 0),
    }
    for name, call in calls.items():
        assert call() == GECM_ERR_STATE, name
        err = lib.gecm_last_error().decode()
        assert err.startswith(name + ": " + REFUSAL), (name, err)
        assert eng.save_lines() == before, name
    # a build on the device
    eng.set_curve_build("device")
    assert lib.gecm_build_curves(h, u64, 4) == GECM_ERR_STATE and REFUSAL in lib.gecm_last_error().decode()
    eng.set_curve_build("host")
    assert eng.save_lines() == before
    # lanes per curve: 1, 2 and 8 make stage 1 answer GECM_ERR_STATE, 0 and 32 run
    for lanes in (1, 2, 8):
        eng.set_lanes_per_curve(lanes)
        assert lib.gecm_stage1(h, B1) == GECM_ERR_STATE and "32 lanes per curve" in lib.gecm_last_error().decode()
        assert eng.save_lines() == before
    eng.set_lanes_per_curve(32)
    eng.build_curves(sig)
    eng.stage1(B1)
    assert eng.save_lines() == before and eng.lanes_per_curve() == 32
    assert eng.batch_bytes(64, with_stage2=True) == 0
    assert eng.batch_bytes(64) == 3 * 64 * 4 * eng.cfg.dev_limbs
    eng.close()


def test_1312_bits_are_refused():
    import pyecm
    assert pyecm.wide_max_bits() == 1311
    h = ctypes.c_void_p()
    n = W.modulus(1312, "random")
    assert pyecm.lib.gecm_create_wide(ctypes.byref(h), 0, str(n).encode(), 52) == GECM_ERR_ARG
    assert "larger than this build supports" in pyecm.lib.gecm_last_error().decode() and not h.value
    assert pyecm.lib.gecm_is_wide(None) == 0


def test_an_ordinary_number_gets_an_ordinary_context():
    import pyecm
    n = random.Random(415).getrandbits(415) | (1 << 414) | 1
    sig = list(range(1000, 1008))
    lines = []
    for wide in (True, False):
        eng = pyecm.Engine(n, wide=wide)
        assert not eng.is_wide() and eng.cfg.dev_limbs == 15
        eng.build_curves(sig)
        eng.stage1(B1)
        lines.append((eng.save_lines(), eng.last_kernel_name(), eng.lanes_per_curve()))
        eng.close()
    assert lines[0] == lines[1]
