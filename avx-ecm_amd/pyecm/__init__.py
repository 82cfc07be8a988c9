"""pyecm — thin ctypes binding of libgecm's C ABI (include/gecm.h) for tests and bench.py.

Plumbing only: every call goes straight to the shared library; there is no Python fallback.
If libgecm.so is missing or fails to load, importing this module raises.
"""
import collections
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GECM_LIB") or os.path.join(os.path.dirname(_HERE), "libgecm.so")

if not os.path.exists(LIB_PATH):
    raise ImportError("libgecm.so not built: run `make -C avx-ecm_amd -j8` (or __graft_entry__.build())")
lib = ctypes.CDLL(LIB_PATH)

c_void_p, c_int, c_size_t, c_char_p, c_u64, c_double = (ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t,
                                                         ctypes.c_char_p, ctypes.c_uint64, ctypes.c_double)


class Config(ctypes.Structure):
    _fields_ = [("digitbits", c_int), ("nwords", c_int), ("maxbits", c_int), ("nbits", c_int),
                ("dev_limbs", c_int), ("device", c_int), ("rho", c_u64)]


class Stage1Stats(ctypes.Structure):
    _fields_ = [("ptadds", c_u64), ("ptdups", c_u64), ("last_prime", c_u64), ("tape_len", c_u64)]


def _sig(name, res, *args):
    f = getattr(lib, name)
    f.restype = res
    f.argtypes = list(args)
    return f


# every symbol include/gecm.h declares
EXPORTS = ["gecm_last_error", "gecm_device_count", "gecm_version", "gecm_create", "gecm_destroy",
           "gecm_get_config", "gecm_device_name", "gecm_get_one", "gecm_vecmulmod", "gecm_vecsqrmod",
           "gecm_vecaddmod", "gecm_vecsubmod", "gecm_vecaddsubmod", "gecm_build_curves",
           "gecm_upload_points", "gecm_stage1", "gecm_sync", "gecm_last_kernel_ms",
           "gecm_get_stage1_stats", "gecm_download_points", "gecm_download_points_plain",
           "gecm_format_save_line", "gecm_stage1_factor", "gecm_set_lanes_per_curve",
           "gecm_get_lanes_per_curve", "gecm_set_special_form", "gecm_get_special_form"]

_sig("gecm_last_error", c_char_p)
_sig("gecm_device_count", c_int)
_sig("gecm_version", c_char_p)
_sig("gecm_create", c_int, ctypes.POINTER(c_void_p), c_int, c_char_p, c_int)
_sig("gecm_destroy", None, c_void_p)
_sig("gecm_get_config", c_int, c_void_p, ctypes.POINTER(Config))
_sig("gecm_device_name", c_int, c_void_p, c_char_p, c_size_t)
_sig("gecm_get_one", c_int, c_void_p, c_void_p)
_sig("gecm_vecmulmod", c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t)
_sig("gecm_vecsqrmod", c_int, c_void_p, c_void_p, c_void_p, c_size_t)
_sig("gecm_vecaddmod", c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t)
_sig("gecm_vecsubmod", c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t)
_sig("gecm_vecaddsubmod", c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t)
_sig("gecm_vecinvmod", c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t)
EXPORTS += ["gecm_vecinvmod"]
# the field functions themselves on raw device limbs (gecm_vecrawop)
RAW_MUL, RAW_SQR, RAW_ADD, RAW_SUB, RAW_CONDSUB = range(5)
RAW_OWN, RAW_TWIN, RAW_BATCH = range(3)
_sig("gecm_vecrawop", c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t)
EXPORTS += ["gecm_vecrawop"]
_sig("gecm_build_curves", c_int, c_void_p, ctypes.POINTER(c_u64), c_size_t)
_sig("gecm_upload_points", c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t)
_sig("gecm_stage1", c_int, c_void_p, c_u64)
_sig("gecm_sync", c_int, c_void_p)
_sig("gecm_set_lanes_per_curve", c_int, c_void_p, c_int)
_sig("gecm_get_lanes_per_curve", c_int, c_void_p)
_sig("gecm_set_special_form", c_int, c_void_p, c_int)
_sig("gecm_get_special_form", c_int, c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int))
_sig("gecm_last_kernel_ms", c_double, c_void_p)
_sig("gecm_get_stage1_stats", c_int, c_void_p, ctypes.POINTER(Stage1Stats))
_sig("gecm_download_points", c_int, c_void_p, c_void_p, c_void_p)
_sig("gecm_download_points_plain", c_int, c_void_p, c_void_p, c_void_p)
_sig("gecm_format_save_line", c_int, c_void_p, c_size_t, c_char_p, c_size_t)
_sig("gecm_stage1_factor", c_int, c_void_p, c_size_t, c_char_p, c_size_t, ctypes.POINTER(c_int))


class Stage2Stats(ctypes.Structure):
    _fields_ = [("ptadds", c_u64), ("numinv", c_u64), ("paired", c_u64), ("device_inversions", c_u64),
                ("D", ctypes.c_uint32), ("U", ctypes.c_uint32), ("L", ctypes.c_uint32), ("amin_last", ctypes.c_uint32)]


class Pairs(ctypes.Structure):
    _fields_ = [("pairmap_v", ctypes.POINTER(ctypes.c_uint32)), ("pairmap_u", ctypes.POINTER(ctypes.c_uint32)),
                ("steps", ctypes.c_uint32), ("amin", ctypes.c_uint32), ("pairs", ctypes.c_uint32),
                ("primes", ctypes.c_uint32)]


_sig("gecm_stage2_init", c_int, c_void_p, ctypes.c_uint32, ctypes.c_uint32)
_sig("gecm_pair_primes", c_int, ctypes.POINTER(Pairs), c_u64, c_u64, ctypes.c_uint32, ctypes.c_uint32)
_sig("gecm_pairmap_release", None, ctypes.POINTER(Pairs))
_sig("gecm_stage2_pair", c_int, c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32),
     ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32)
_sig("gecm_stage2", c_int, c_void_p, c_u64, ctypes.c_uint32, ctypes.c_uint32)
_sig("gecm_stage2_prepare", c_int, c_void_p, c_u64, ctypes.c_uint32, ctypes.c_uint32)
_sig("gecm_stage2_pair_prepare", c_int, c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
     ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32)
_sig("gecm_get_stage2_stats", c_int, c_void_p, ctypes.POINTER(Stage2Stats))
_sig("gecm_download_acc", c_int, c_void_p, c_void_p)
_sig("gecm_stage2_factor", c_int, c_void_p, c_size_t, c_char_p, c_size_t, ctypes.POINTER(c_int))
class RangeDesc(ctypes.Structure):
    _fields_ = [("lo", c_u64), ("hi", c_u64), ("nprimes", c_u64), ("first_prime", c_u64), ("last_prime", c_u64),
                ("checkpoint", c_int)]


_sig("gecm_set_report_modulus", c_int, c_void_p, c_char_p)
_sig("gecm_device_memory", c_int, c_void_p, ctypes.POINTER(c_u64), ctypes.POINTER(c_u64))
_sig("gecm_batch_bytes", c_u64, c_void_p, c_size_t, c_int, c_u64, ctypes.c_uint32, ctypes.c_uint32)
EXPORTS += ["gecm_set_report_modulus", "gecm_device_memory", "gecm_batch_bytes"]
_sig("gecm_last_kernel_name", c_int, c_void_p, c_char_p, c_size_t)
_sig("gecm_stage1_progress", c_int, c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32))
EXPORTS += ["gecm_last_kernel_name", "gecm_stage1_progress"]
_sig("gecm_stage1_ranges", c_int, c_u64)
_sig("gecm_stage1_range", c_int, c_void_p, c_u64, ctypes.c_uint32)
_sig("gecm_stage1_describe_range", c_int, c_u64, c_u64, ctypes.c_uint32, ctypes.POINTER(RangeDesc))
_sig("gecm_format_resume_line", c_int, c_void_p, c_size_t, c_u64, c_char_p, c_size_t)
EXPORTS += ["gecm_stage1_ranges", "gecm_stage1_range", "gecm_stage1_describe_range", "gecm_format_resume_line"]
_sig("gecm_scan_factors", c_int, c_void_p, c_int, ctypes.POINTER(c_size_t))
_sig("gecm_curve_flag", c_int, c_void_p, c_int, c_size_t)
EXPORTS += ["gecm_scan_factors", "gecm_curve_flag", "gecm_prepare_input", "gecm_sizeinbase10"]
_sig("gecm_set_stage2_subseq", c_int, c_void_p, c_int)
_sig("gecm_get_stage2_subseq", c_int, c_void_p, ctypes.POINTER(ctypes.c_uint32))
EXPORTS += ["gecm_set_stage2_subseq", "gecm_get_stage2_subseq"]
S2_SUBSEQ_DEFAULT, S2_SUBSEQ_AUTO = 0, -1
EXPORTS += ["gecm_stage2_init", "gecm_pair_primes", "gecm_pairmap_release", "gecm_stage2_pair", "gecm_stage2", "gecm_stage2_prepare", "gecm_stage2_pair_prepare",
            "gecm_get_stage2_stats", "gecm_download_acc", "gecm_stage2_factor"]


_sig("gecm_create_multi", c_int, ctypes.POINTER(c_void_p), c_int, ctypes.POINTER(c_char_p), c_size_t, c_int)
_sig("gecm_build_curves_multi", c_int, c_void_p, ctypes.POINTER(c_u64), ctypes.POINTER(ctypes.c_uint32), c_size_t)
_sig("gecm_moduli", c_size_t, c_void_p)
_sig("gecm_curve_modulus", c_int, c_void_p, c_size_t)
_sig("gecm_curve_acc", c_int, c_void_p, c_size_t, c_char_p, c_size_t)
EXPORTS += ["gecm_create_multi", "gecm_build_curves_multi", "gecm_moduli", "gecm_curve_modulus", "gecm_curve_acc"]
PACK_WAVE, PACK_LANE = 0, 1
_sig("gecm_set_multi_packing", c_int, c_void_p, c_int)
_sig("gecm_get_multi_packing", c_int, c_void_p)
_sig("gecm_multi_positions", c_size_t, ctypes.POINTER(c_size_t), c_size_t, c_int)
_sig("gecm_multi_packing_max_bits", c_int, c_int)
EXPORTS += ["gecm_set_multi_packing", "gecm_get_multi_packing", "gecm_multi_positions", "gecm_multi_packing_max_bits"]


def multi_positions(counts, packing):
    """padded curve positions of a multi-modulus batch with counts[g] curves on number g; packing is "wave" or "lane" """
    arr = (c_size_t * max(1, len(counts)))(*counts)
    return lib.gecm_multi_positions(arr, len(counts), _PACKINGS[packing])


_PACKINGS = {"wave": PACK_WAVE, "lane": PACK_LANE}


class ResumeNum(ctypes.Structure):
    _fields_ = [("digits", c_void_p), ("len", c_size_t), ("base", c_int)]


class ResumeRec(ctypes.Structure):
    _fields_ = [("sigma", c_u64), ("b1", c_u64), ("n", ResumeNum), ("x", ResumeNum), ("z", ResumeNum)]


_sig("gecm_parse_resume_line", c_int, c_char_p, ctypes.POINTER(ResumeRec))
_sig("gecm_stage1_resume_range", c_int, c_u64, c_u64, ctypes.POINTER(ctypes.c_uint32))
_sig("gecm_resume_points", c_int, c_void_p, ctypes.POINTER(c_u64), c_void_p, c_void_p, c_size_t, c_u64)
_sig("gecm_resume_points_multi", c_int, c_void_p, ctypes.POINTER(c_u64), ctypes.POINTER(ctypes.c_uint32), c_void_p,
     c_void_p, c_size_t, c_u64)
EXPORTS += ["gecm_parse_resume_line", "gecm_stage1_resume_range", "gecm_resume_points", "gecm_resume_points_multi"]
_sig("gecm_set_curve_build", c_int, c_void_p, c_int)
_sig("gecm_get_curve_build", c_int, c_void_p)
_sig("gecm_download_s", c_int, c_void_p, c_void_p)
EXPORTS += ["gecm_set_curve_build", "gecm_get_curve_build", "gecm_download_s"]
CURVE_BUILDS = ("host", "device")      # GECM_BUILD_HOST, GECM_BUILD_DEVICE


class ExtendDesc(ctypes.Structure):
    _fields_ = [("lo", c_u64), ("hi", c_u64), ("nprimes", c_u64), ("power_steps", c_u64), ("last_prime", c_u64)]


_sig("gecm_stage1_extend_segments", c_int, c_u64, c_u64)
_sig("gecm_stage1_describe_extend", c_int, c_u64, c_u64, ctypes.c_uint32, ctypes.POINTER(ExtendDesc))
_sig("gecm_stage1_extend_segment", c_int, c_void_p, c_u64, c_u64, ctypes.c_uint32)
_sig("gecm_stage1_extend", c_int, c_void_p, c_u64, c_u64)
_sig("gecm_normalize_points", c_int, c_void_p)
_sig("gecm_points_normalized", c_int, c_void_p)
_sig("gecm_format_save_line_std", c_int, c_void_p, c_size_t, c_char_p, c_size_t)
_sig("gecm_resume_line_std_bound", c_int, c_char_p, ctypes.POINTER(c_u64))
EXPORTS += ["gecm_stage1_extend_segments", "gecm_stage1_describe_extend", "gecm_stage1_extend_segment", "gecm_stage1_extend",
            "gecm_normalize_points", "gecm_points_normalized", "gecm_format_save_line_std", "gecm_resume_line_std_bound"]


# the parametrisations of a curve: Suyama's sigma, GMP-ECM's batch modes d = sigma^2 / 2^64 and sigma / 2^32
PARAM_SUYAMA, PARAM_BATCH_SQUARE, PARAM_BATCH_32 = 0, 1, 3
_sig("gecm_param_s", c_int, c_int, c_u64, c_char_p, c_char_p, c_size_t)
_sig("gecm_set_next_params", c_int, c_void_p, ctypes.POINTER(ctypes.c_uint8), c_size_t)
_sig("gecm_curve_param", c_int, c_void_p, c_size_t)
_sig("gecm_parse_resume_line_param", c_int, c_char_p, ctypes.POINTER(ResumeRec), ctypes.POINTER(c_int))
_sig("gecm_resume_line_std_bound_param", c_int, c_char_p, ctypes.POINTER(c_u64))
EXPORTS += ["gecm_param_s", "gecm_set_next_params", "gecm_curve_param", "gecm_parse_resume_line_param",
            "gecm_resume_line_std_bound_param"]

# P-1 and P+1 batches: one residue per lane on the stage-1 tape
METHOD_ECM, METHOD_PM1, METHOD_PP1 = 0, 1, 2
_sig("gecm_build_seeds", c_int, c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_u64)
_sig("gecm_build_seeds_multi", c_int, c_void_p, c_int, ctypes.POINTER(ctypes.c_uint32), c_void_p, c_void_p, c_size_t, c_u64)
_sig("gecm_batch_method", c_int, c_void_p)
_sig("gecm_curve_seed", c_int, c_void_p, c_size_t, c_char_p, c_size_t)
_sig("gecm_parse_resume_line_method", c_int, c_char_p, ctypes.POINTER(ResumeRec), ctypes.POINTER(c_int), ctypes.POINTER(c_int),
     ctypes.POINTER(ResumeNum))
_sig("gecm_resume_line_std_bound_method", c_int, c_char_p, ctypes.POINTER(c_u64))
EXPORTS += ["gecm_build_seeds", "gecm_build_seeds_multi", "gecm_batch_method", "gecm_curve_seed",
            "gecm_parse_resume_line_method", "gecm_resume_line_std_bound_method"]

# stage 2 of such batches: opt-in per context
METHOD_S2_OFF, METHOD_S2_ON = 0, 1
_sig("gecm_set_method_stage2", c_int, c_void_p, c_int)
_sig("gecm_get_method_stage2", c_int, c_void_p)
EXPORTS += ["gecm_set_method_stage2", "gecm_get_method_stage2"]

# stage 1 of such batches with a residue per 16-lane DPP row: opt-in per context
METHOD_LANES_AUTO = -1
_sig("gecm_set_method_lanes", c_int, c_void_p, c_int)
_sig("gecm_get_method_lanes", c_int, c_void_p)
_sig("gecm_method_lanes_auto", c_int, c_size_t, c_int, c_int)
EXPORTS += ["gecm_set_method_lanes", "gecm_get_method_lanes", "gecm_method_lanes_auto"]


def method_lanes_auto(positions, limbs, cus):
    """1 or 16: the lanes per residue "auto" gives a method batch of that many (padded) positions"""
    return lib.gecm_method_lanes_auto(positions, limbs, cus)


# stage 1 of the curve batches of a multi-modulus context with 32 lanes per curve: opt-in per context
MULTI_ROWS_OFF, MULTI_ROWS_ON, MULTI_ROWS_AUTO = 0, 1, -1
_MULTI_ROWS = {"off": MULTI_ROWS_OFF, "on": MULTI_ROWS_ON, "auto": MULTI_ROWS_AUTO}
_sig("gecm_set_multi_rows", c_int, c_void_p, c_int)
_sig("gecm_get_multi_rows", c_int, c_void_p)
_sig("gecm_multi_rows_auto", c_int, c_size_t, c_int, c_int)
EXPORTS += ["gecm_set_multi_rows", "gecm_get_multi_rows", "gecm_multi_rows_auto"]


def multi_rows_auto(positions, limbs, cus):
    """0 or 1: whether "auto" runs a multi-modulus curve batch of that many (padded) positions in the row layout"""
    return lib.gecm_multi_rows_auto(positions, limbs, cus)


# wide contexts: stage 1 for numbers of 1032 to 1311 bits
_sig("gecm_create_wide", c_int, ctypes.POINTER(c_void_p), c_int, c_char_p, c_int)
_sig("gecm_is_wide", c_int, c_void_p)
_sig("gecm_wide_max_bits", c_int)
EXPORTS += ["gecm_create_wide", "gecm_is_wide", "gecm_wide_max_bits"]


def wide_max_bits():
    """the largest bit length Engine(n, wide=True) takes (1311)"""
    return lib.gecm_wide_max_bits()


class GecmError(RuntimeError):
    pass


def _chk(rc, what):
    if rc < 0:
        raise GecmError("%s failed (%d): %s" % (what, rc, lib.gecm_last_error().decode()))
    return rc


def pair_primes(b1, b2, D, U):
    p = Pairs()
    _chk(lib.gecm_pair_primes(ctypes.byref(p), b1, b2, D, U), "gecm_pair_primes")
    return p


def device_count():
    return lib.gecm_device_count()


def stage1_ranges(b1):
    return lib.gecm_stage1_ranges(b1)


def describe_range(b1, b2, r):
    d = RangeDesc()
    _chk(lib.gecm_stage1_describe_range(b1, b2, r, ctypes.byref(d)), "gecm_stage1_describe_range")
    return d


# one save_b1.txt / checkpoint.txt / GMP-ECM -save line: b1 is the line's B1 field, z is 1 where the line has no Z
ResumeLine = collections.namedtuple("ResumeLine", "sigma b1 n x z")


# the same with the line's parametrisation (PARAM absent: 0)
ResumeLineParam = collections.namedtuple("ResumeLineParam", "sigma b1 n x z param")


def _parse_line(line, with_param):
    raw = line.encode() if isinstance(line, str) else bytes(line)
    buf = ctypes.create_string_buffer(raw)
    rec = ResumeRec()
    param = c_int(0)
    if with_param:
        rc = _chk(lib.gecm_parse_resume_line_param(buf, ctypes.byref(rec), ctypes.byref(param)), "gecm_parse_resume_line_param")
    else:
        rc = _chk(lib.gecm_parse_resume_line(buf, ctypes.byref(rec)), "gecm_parse_resume_line")
    if rc == 1:
        return None

    def num(f):
        off = f.digits - ctypes.addressof(buf)
        return int(raw[off:off + f.len], f.base)
    fields = (rec.sigma, rec.b1, num(rec.n), num(rec.x), num(rec.z) if rec.z.digits else 1)
    return ResumeLineParam(*fields, param.value) if with_param else ResumeLine(*fields)


def parse_resume_line(line):
    """ResumeLine of one resume line, None for a line to skip (blank or '#'); GecmError names the field that is wrong"""
    return _parse_line(line, False)


def parse_resume_line_param(line):
    """parse_resume_line with PARAM 0, 1 and 3 accepted: ResumeLineParam, the same fields and the parametrisation"""
    return _parse_line(line, True)


# a line of any method: method is METHOD_ECM / _PM1 / _PP1; x0 is the seed of a P-1 / P+1 line, None where it names none
ResumeLineMethod = collections.namedtuple("ResumeLineMethod", "sigma b1 n x z param method x0")


def parse_resume_line_method(line):
    """parse_resume_line_param with METHOD=P-1 and METHOD=P+1 lines accepted: ResumeLineMethod (sigma = 0, param = 0 and
    z = 1 on such a line), None for a line to skip"""
    raw = line.encode() if isinstance(line, str) else bytes(line)
    buf = ctypes.create_string_buffer(raw)
    rec, x0 = ResumeRec(), ResumeNum()
    param, method = c_int(0), c_int(0)
    rc = _chk(lib.gecm_parse_resume_line_method(buf, ctypes.byref(rec), ctypes.byref(param), ctypes.byref(method),
                                                ctypes.byref(x0)), "gecm_parse_resume_line_method")
    if rc == 1:
        return None

    def num(f):
        off = f.digits - ctypes.addressof(buf)
        return int(raw[off:off + f.len], f.base)
    return ResumeLineMethod(rec.sigma, rec.b1, num(rec.n), num(rec.x), num(rec.z) if rec.z.digits else 1, param.value,
                            method.value, num(x0) if x0.digits else None)


def resume_line_std_bound_method(line):
    """resume_line_std_bound for a reader of parse_resume_line_method: the B1 field of a P-1 / P+1 line, and what
    resume_line_std_bound(line, params=True) gives for an ECM line"""
    raw = line.encode() if isinstance(line, str) else bytes(line)
    b = c_u64(0)
    if _chk(lib.gecm_resume_line_std_bound_method(raw, ctypes.byref(b)), "gecm_resume_line_std_bound_method") == 1:
        return None
    return b.value


def param_s(param, sigma, n):
    """s = (A+2)/4 = d of the PARAM 1 (sigma^2 / 2^64) or PARAM 3 (sigma / 2^32) curve of sigma modulo n"""
    buf = ctypes.create_string_buffer(2048)
    _chk(lib.gecm_param_s(param, sigma, str(n).encode(), buf, len(buf)), "gecm_param_s")
    return int(buf.value.decode(), 16)


def stage1_resume_range(b1, field):
    """the range a run to b1 goes on with from lines whose B1 field is `field`; stage1_ranges(b1) = stage 1 is complete"""
    r = ctypes.c_uint32(0)
    _chk(lib.gecm_stage1_resume_range(b1, field, ctypes.byref(r)), "gecm_stage1_resume_range")
    return r.value


def extend_segments(b1_from, b1_to):
    """segments an extension of the standard multiplier from b1_from to b1_to runs in"""
    return _chk(lib.gecm_stage1_extend_segments(b1_from, b1_to), "gecm_stage1_extend_segments")


def describe_extend(b1_from, b1_to, seg):
    d = ExtendDesc()
    _chk(lib.gecm_stage1_describe_extend(b1_from, b1_to, seg, ctypes.byref(d)), "gecm_stage1_describe_extend")
    return d


def resume_line_std_bound(line, params=False):
    """the standard bound the points of a resume line are complete to (None for a line to skip): B1 - 1 for a line of the
    reference semantic (PROGRAM=AVX-ECM) within one prime range, the B1 field for every other line; params=True reads
    the line as parse_resume_line_param does"""
    raw = line.encode() if isinstance(line, str) else bytes(line)
    b = c_u64(0)
    fn = "gecm_resume_line_std_bound_param" if params else "gecm_resume_line_std_bound"
    if _chk(getattr(lib, fn)(raw, ctypes.byref(b)), fn) == 1:
        return None
    return b.value


class Engine:
    """One gecm_ctx: N + limb format + device."""

    def __init__(self, n, digitbits=52, device=0, wide=False):
        """wide: gecm_create_wide, which serves every N gecm_create serves (an ordinary context then) and, from 1032 to
        wide_max_bits() bits, makes a wide context: curve build, stage 1 and its save lines and factors, nothing else."""
        self._h = c_void_p()
        create = "gecm_create_wide" if wide else "gecm_create"
        _chk(getattr(lib, create)(ctypes.byref(self._h), device, str(n).encode(), digitbits), create)
        self.cfg = Config()
        _chk(lib.gecm_get_config(self._h, ctypes.byref(self.cfg)), "gecm_get_config")
        self.n = int(str(n), 0) if isinstance(n, str) else int(n)
        self.batch = 0

    def close(self):
        if self._h:
            lib.gecm_destroy(self._h)
            self._h = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def is_wide(self):
        return bool(lib.gecm_is_wide(self._h))

    # ---- reference vec layout helpers: data[lane + limb*batch] ----
    def _ctype(self):
        return ctypes.c_uint64 if self.cfg.digitbits == 52 else ctypes.c_uint32

    def pack(self, values):
        b, nw, db = len(values), self.cfg.nwords, self.cfg.digitbits
        arr = (self._ctype() * (b * nw))()
        mask = (1 << db) - 1
        for lane, v in enumerate(values):
            for j in range(nw):
                arr[lane + j * b] = (v >> (db * j)) & mask
        return arr

    def unpack(self, arr, b):
        nw, db = self.cfg.nwords, self.cfg.digitbits
        return [sum(int(arr[lane + j * b]) << (db * j) for j in range(nw)) for lane in range(b)]

    def empty(self, b):
        return (self._ctype() * (b * self.cfg.nwords))()

    # ---- L0 ----
    def vecmulmod(self, a, b):
        n = len(a)
        out = self.empty(n)
        _chk(lib.gecm_vecmulmod(self._h, self.pack(a), self.pack(b), out, n), "gecm_vecmulmod")
        return self.unpack(out, n)

    def vecsqrmod(self, a):
        n = len(a)
        out = self.empty(n)
        _chk(lib.gecm_vecsqrmod(self._h, self.pack(a), out, n), "gecm_vecsqrmod")
        return self.unpack(out, n)

    def vecaddmod(self, a, b):
        n = len(a)
        out = self.empty(n)
        _chk(lib.gecm_vecaddmod(self._h, self.pack(a), self.pack(b), out, n), "gecm_vecaddmod")
        return self.unpack(out, n)

    def vecsubmod(self, a, b):
        n = len(a)
        out = self.empty(n)
        _chk(lib.gecm_vecsubmod(self._h, self.pack(a), self.pack(b), out, n), "gecm_vecsubmod")
        return self.unpack(out, n)

    def vecaddsubmod(self, a, b):
        n = len(a)
        s, d = self.empty(n), self.empty(n)
        _chk(lib.gecm_vecaddsubmod(self._h, self.pack(a), self.pack(b), s, d, n), "gecm_vecaddsubmod")
        return self.unpack(s, n), self.unpack(d, n)

    def vecinvmod(self, a):
        """(inv, gcd) of the device inversion: inv[i] = x^-1 R mod N for a[i] = x R mod N (0 where none exists),
        gcd[i] = gcd(a[i], N)"""
        n = len(a)
        inv, g = self.empty(n), self.empty(n)
        _chk(lib.gecm_vecinvmod(self._h, self.pack(a), inv, g, n), "gecm_vecinvmod")
        return self.unpack(inv, n), self.unpack(g, n)

    def vecrawop(self, op, a, b=None, target=RAW_OWN, limbs=None):
        """one field function of the device on raw limbs: a, b lists of residues, each a list of `limbs` 32-bit words
        (default: the context's dev_limbs; the twin's for RAW_TWIN); the result in the same shape, limbs as the function
        left them.  Nothing is checked against N or converted."""
        if limbs is None:
            limbs = self.special_form()[2] if target == RAW_TWIN else self.cfg.dev_limbs
        n = len(a)
        if any(len(v) != limbs for v in a) or (b is not None and (len(b) != n or any(len(v) != limbs for v in b))):
            raise ValueError("vecrawop: every residue has %d limbs, and b as many residues as a" % limbs)

        def planes(vals):
            arr = (ctypes.c_uint32 * max(1, n * limbs))()
            for j in range(limbs):
                arr[j * n:(j + 1) * n] = [v[j] for v in vals]
            return arr
        out = (ctypes.c_uint32 * max(1, n * limbs))()
        _chk(lib.gecm_vecrawop(self._h, target, op, planes(a), None if b is None else planes(b), out, n), "gecm_vecrawop")
        return [[out[i + j * n] for j in range(limbs)] for i in range(n)]

    # ---- L1 ----
    def _next_params(self, params, batch):
        # the parametrisation of every curve of the build that follows (one-shot); None: a build as always
        if params is None:
            return
        if len(params) != batch:
            raise ValueError("params: one parametrisation (0, 1 or 3) per sigma")
        arr = (ctypes.c_uint8 * max(1, batch))(*[p if 0 <= p < 256 else 255 for p in params])
        _chk(lib.gecm_set_next_params(self._h, arr, batch), "gecm_set_next_params")

    def build_curves(self, sigmas, params=None):
        """params: per curve 0 (Suyama, sigma >= 6), 1 (d = sigma^2 / 2^64, 1 <= sigma < 2^64) or 3 (d = sigma / 2^32,
        1 <= sigma < 2^32); None: every curve 0"""
        arr = (c_u64 * len(sigmas))(*sigmas)
        self._next_params(params, len(sigmas))
        self.batch = len(sigmas)
        return _chk(lib.gecm_build_curves(self._h, arr, len(sigmas)), "gecm_build_curves")

    def curve_param(self, k):
        """the parametrisation curve k was built with"""
        return _chk(lib.gecm_curve_param(self._h, k), "gecm_curve_param")

    def set_curve_build(self, where):
        """"host" (default) or "device": where the next build_curves / resume makes the curves; the batch holds the same
        words either way"""
        if where not in CURVE_BUILDS:
            raise ValueError("set_curve_build: 'host' or 'device'")
        _chk(lib.gecm_set_curve_build(self._h, CURVE_BUILDS.index(where)), "gecm_set_curve_build")

    def curve_build(self):
        """what the last build_curves / resume used"""
        return CURVE_BUILDS[_chk(lib.gecm_get_curve_build(self._h), "gecm_get_curve_build")]

    def download_s(self):
        """s = (A+2)/4 of every curve, in the radix download_points uses"""
        s = self.empty(self.batch)
        _chk(lib.gecm_download_s(self._h, s), "gecm_download_s")
        return self.unpack(s, self.batch)

    def upload_points(self, X, Z, s):
        self.batch = len(X)
        _chk(lib.gecm_upload_points(self._h, self.pack(X), self.pack(Z), self.pack(s), len(X)), "gecm_upload_points")

    def resume(self, sigmas, xs, zs, b1_done=0, params=None):
        """start from the plain residues of save or checkpoint lines: mid stage 1 (go on with stage1_range), or with
        b1_done = B1 as after stage1(B1); params as for build_curves"""
        if not len(sigmas) == len(xs) == len(zs):
            raise ValueError("resume: one x and one z per sigma")
        self._fits(xs, zs)
        arr = (c_u64 * len(sigmas))(*sigmas)
        self._next_params(params, len(sigmas))
        self.batch = len(sigmas)
        return _chk(lib.gecm_resume_points(self._h, arr, self.pack(xs), self.pack(zs), len(sigmas), b1_done),
                    "gecm_resume_points")

    def build_seeds(self, method, x0s, xs=None, b1_done=1):
        """a P-1 (METHOD_PM1) or P+1 (METHOD_PP1) batch: one residue per position, seeds x0s; xs = the residues of lines
        complete to b1_done (x0s may then be None: seeds unknown), None = a fresh batch.  Go on with stage1_extend."""
        given = xs if xs is not None else x0s
        if given is None or (x0s is not None and xs is not None and len(x0s) != len(xs)):
            raise ValueError("build_seeds: seeds, residues or one of each per position")
        self._fits(*[v for v in (x0s, xs) if v is not None])
        rc = _chk(lib.gecm_build_seeds(self._h, method, None if x0s is None else self.pack(x0s),
                                       None if xs is None else self.pack(xs), len(given), b1_done), "gecm_build_seeds")
        self.batch = len(given)                   # a refused call leaves the previous batch, and its size
        return rc

    def batch_method(self):
        """METHOD_ECM, METHOD_PM1 or METHOD_PP1: what the batch in the context holds"""
        return lib.gecm_batch_method(self._h)

    def set_method_stage2(self, on):
        """let the stage-2 calls work on P-1 / P+1 batches of this context; holds across builds"""
        return _chk(lib.gecm_set_method_stage2(self._h, METHOD_S2_ON if on else METHOD_S2_OFF), "gecm_set_method_stage2")

    def method_stage2(self):
        return bool(lib.gecm_get_method_stage2(self._h))

    def set_method_lanes(self, lanes):
        """lanes per residue of the P-1 / P+1 batches of this context in stage 1: 1 (the default), 16 or "auto"
        (DESIGN.md §22); holds across builds, takes effect at the next stage1_extend"""
        return _chk(lib.gecm_set_method_lanes(self._h, METHOD_LANES_AUTO if lanes == "auto" else lanes), "gecm_set_method_lanes")

    def method_lanes(self):
        v = lib.gecm_get_method_lanes(self._h)
        return "auto" if v == METHOD_LANES_AUTO else v

    def curve_seed(self, k):
        """x0 of position k of a P-1 / P+1 batch; None where the batch was built without seeds"""
        buf = ctypes.create_string_buffer(2048)
        n = _chk(lib.gecm_curve_seed(self._h, k, buf, len(buf)), "gecm_curve_seed")
        return int(buf.value.decode(), 16) if n else None

    def _fits(self, *vecs):
        # pack() keeps the low MAXBITS bits: what does not fit them is no residue of this context
        if any(v < 0 or v >> self.cfg.maxbits for vec in vecs for v in vec):
            raise ValueError("resume: a residue is negative or longer than the context's %d bits" % self.cfg.maxbits)

    def _line_moduli(self):
        # the N that this context's lines carry: the report modulus, if one is set (read here, not when it is set)
        rep = getattr(self, "_report_modulus", None)
        return [self.n if rep is None else int(rep, 0) if isinstance(rep, str) else int(rep)]

    def _resume_recs(self, recs, ns, b1_done, params=None):
        return self.resume([r.sigma for r in recs], [r.x for r in recs], [r.z for r in recs], b1_done=b1_done, params=params)

    def resume_lines(self, lines, b1_done=0, params=False):
        """resume() from the text of resume lines (skipped lines dropped); every N must be the context's (on a
        MultiEngine: one of its numbers, which decides the curve's modulus).  params=True: lines of PARAM 0, 1 and 3
        are read (parse_resume_line_param) and every curve is built by its line's parametrisation"""
        recs = [r for r in map(parse_resume_line_param if params else parse_resume_line, lines) if r is not None]
        ns = self._line_moduli()
        for k, r in enumerate(recs):
            if r.n not in ns:
                raise ValueError("resume_lines: line %d is on N = %d, not a number of this context" % (k, r.n))
        if params:
            return self._resume_recs(recs, ns, b1_done, [r.param for r in recs])
        return self._resume_recs(recs, ns, b1_done)

    def stage1(self, b1, sync=True):
        _chk(lib.gecm_stage1(self._h, b1), "gecm_stage1")
        if sync:
            self.sync()

    def stage1_range(self, b1, r, sync=True):
        """one ecm_stage1 call of the reference's loop over prime ranges of 1e8 (ecm.c:1209-1234)"""
        _chk(lib.gecm_stage1_range(self._h, b1, r), "gecm_stage1_range")
        if sync:
            self.sync()

    def stage1_extend(self, b1_from, b1_to, sync=True):
        """the points, complete to b1_from with the standard multiplier (1: fresh curves), on to b1_to"""
        _chk(lib.gecm_stage1_extend(self._h, b1_from, b1_to), "gecm_stage1_extend")
        if sync:
            self.sync()

    def stage1_extend_segment(self, b1_from, b1_to, seg, sync=True):
        _chk(lib.gecm_stage1_extend_segment(self._h, b1_from, b1_to, seg), "gecm_stage1_extend_segment")
        if sync:
            self.sync()

    def normalize(self):
        """X <- X/Z, Z <- 1 on the device; 1 if some curve's Z had no inverse and the curve was left as it was, else 0"""
        return _chk(lib.gecm_normalize_points(self._h), "gecm_normalize_points")

    def normalized(self):
        return bool(lib.gecm_points_normalized(self._h))

    def save_line_std(self, k):
        buf = ctypes.create_string_buffer(8192)
        _chk(lib.gecm_format_save_line_std(self._h, k, buf, len(buf)), "gecm_format_save_line_std")
        return buf.value.decode()

    def save_lines_std(self):
        return [self.save_line_std(k) for k in range(self.batch)]

    def resume_line(self, k, b1_field):
        buf = ctypes.create_string_buffer(8192)
        _chk(lib.gecm_format_resume_line(self._h, k, b1_field, buf, len(buf)), "gecm_format_resume_line")
        return buf.value.decode()

    def sync(self):
        _chk(lib.gecm_sync(self._h), "gecm_sync")

    def set_lanes_per_curve(self, lanes):
        """0 = chosen per launch from the batch size, 1 = curve per lane, 2 = X and Z on adjacent lanes,
        8 = X and Z on two quads of lanes with the limbs of each residue spread over the quad"""
        _chk(lib.gecm_set_lanes_per_curve(self._h, lanes), "gecm_set_lanes_per_curve")

    def set_special_form(self, on):
        """use (default) or not the 2^k - 1 multiply for N | 2^k - 1; applies from the next build/upload"""
        _chk(lib.gecm_set_special_form(self._h, 1 if on else 0), "gecm_set_special_form")

    def special_form(self):
        """(enabled, k, limbs)"""
        k, l = c_int(0), c_int(0)
        r = _chk(lib.gecm_get_special_form(self._h, ctypes.byref(k), ctypes.byref(l)), "gecm_get_special_form")
        return bool(r), k.value, l.value

    def special_form_used(self):
        """True if the last stage-1 launch ran with the special multiply"""
        return _chk(lib.gecm_get_special_form(self._h, None, None), "gecm_get_special_form") == 2

    def lanes_per_curve(self):
        """what the last stage-1 launch used"""
        return _chk(lib.gecm_get_lanes_per_curve(self._h), "gecm_get_lanes_per_curve")

    def device_memory(self):
        f, t = c_u64(0), c_u64(0)
        _chk(lib.gecm_device_memory(self._h, ctypes.byref(f), ctypes.byref(t)), "gecm_device_memory")
        return f.value, t.value

    def batch_bytes(self, curves, with_stage2=False, b1=0, D=0, U=0):
        return lib.gecm_batch_bytes(self._h, curves, 1 if with_stage2 else 0, b1, D, U)

    def set_report_modulus(self, n):
        """save lines name n and factors are reported of n (a divisor of the context's modulus): the reference's
        special-form runs, which work modulo 2^k -/+ 1 or 2^k - c and report against the number given"""
        _chk(lib.gecm_set_report_modulus(self._h, None if n is None else str(n).encode()), "gecm_set_report_modulus")
        self._report_modulus = n

    def stage1_progress(self):
        """(launches finished, launches made) of the stage-1 call in flight"""
        d, t = ctypes.c_uint32(0), ctypes.c_uint32(0)
        _chk(lib.gecm_stage1_progress(self._h, ctypes.byref(d), ctypes.byref(t)), "gecm_stage1_progress")
        return d.value, t.value

    def last_kernel_name(self):
        buf = ctypes.create_string_buffer(128)
        _chk(lib.gecm_last_kernel_name(self._h, buf, len(buf)), "gecm_last_kernel_name")
        return buf.value.decode()

    def last_kernel_ms(self):
        return lib.gecm_last_kernel_ms(self._h)

    def stage1_stats(self):
        st = Stage1Stats()
        _chk(lib.gecm_get_stage1_stats(self._h, ctypes.byref(st)), "gecm_get_stage1_stats")
        return st

    def download_points(self):
        X, Z = self.empty(self.batch), self.empty(self.batch)
        _chk(lib.gecm_download_points(self._h, X, Z), "gecm_download_points")
        return self.unpack(X, self.batch), self.unpack(Z, self.batch)

    def download_points_plain(self):
        X, Z = self.empty(self.batch), self.empty(self.batch)
        _chk(lib.gecm_download_points_plain(self._h, X, Z), "gecm_download_points_plain")
        return self.unpack(X, self.batch), self.unpack(Z, self.batch)

    def save_line(self, k):
        buf = ctypes.create_string_buffer(8192)
        _chk(lib.gecm_format_save_line(self._h, k, buf, len(buf)), "gecm_format_save_line")
        return buf.value.decode()

    def save_lines(self):
        return [self.save_line(k) for k in range(self.batch)]

    def stage1_factor(self, k):
        buf = ctypes.create_string_buffer(2048)
        prp = c_int(0)
        rc = _chk(lib.gecm_stage1_factor(self._h, k, buf, len(buf), ctypes.byref(prp)), "gecm_stage1_factor")
        return (int(buf.value.decode()), bool(prp.value)) if rc == 1 else None

    def scan_factors(self, stage=1):
        """device factor scan: (number of curves with a factor, lowest such index or None)"""
        first = c_size_t(0)
        n = _chk(lib.gecm_scan_factors(self._h, stage, ctypes.byref(first)), "gecm_scan_factors")
        return n, (first.value if n else None)

    def curve_flag(self, stage, k):
        return bool(lib.gecm_curve_flag(self._h, stage, k))

    # ---- stage 2 ----
    def stage2(self, b2, D=0, U=0):
        _chk(lib.gecm_stage2(self._h, b2, D, U), "gecm_stage2")

    def stage2_prepare(self, b2, D=0, U=0):
        """host-side pair map for a later stage2(b2, D, U); callable while an asynchronous stage 1 runs"""
        _chk(lib.gecm_stage2_prepare(self._h, b2, D, U), "gecm_stage2_prepare")

    def stage2_init(self, D=0, U=0, sync=True):
        _chk(lib.gecm_stage2_init(self._h, D, U), "gecm_stage2_init")
        if sync:
            self.sync()

    def stage2_pair(self, pairs, sync=True):
        _chk(lib.gecm_stage2_pair(self._h, pairs.steps, pairs.pairmap_v, pairs.pairmap_u, pairs.amin), "gecm_stage2_pair")
        if sync:
            self.sync()

    def stage2_pair_prepare(self, pairs, D, U):
        """host side of stage2_pair(pairs) ahead of time (the launch tape of that pair map); no device work"""
        _chk(lib.gecm_stage2_pair_prepare(self._h, D, U, pairs.steps, pairs.pairmap_v, pairs.pairmap_u, pairs.amin),
             "gecm_stage2_pair_prepare")

    def set_stage2_subseq(self, k):
        """sub-sequences per curve for the table build and the giant steps of stage 2, from the next stage 2 on:
        "default" (single-N: by batch size; multi-modulus: 1), "auto" (by batch size on every context) or 1, 2, .. 32"""
        k = {"default": S2_SUBSEQ_DEFAULT, "auto": S2_SUBSEQ_AUTO}.get(k, k)
        if isinstance(k, bool) or not isinstance(k, int):
            raise ValueError("set_stage2_subseq: 'auto', 'default' or an int")
        _chk(lib.gecm_set_stage2_subseq(self._h, k), "gecm_set_stage2_subseq")

    def stage2_subseq(self):
        """(K of the last stage-2 init, 0 before the first; giant-step chunks made with sub-sequences since)"""
        n = ctypes.c_uint32(0)
        k = _chk(lib.gecm_get_stage2_subseq(self._h, ctypes.byref(n)), "gecm_get_stage2_subseq")
        return k, n.value

    def stage2_stats(self):
        st = Stage2Stats()
        _chk(lib.gecm_get_stage2_stats(self._h, ctypes.byref(st)), "gecm_get_stage2_stats")
        return st

    def download_acc(self):
        A = self.empty(self.batch)
        _chk(lib.gecm_download_acc(self._h, A), "gecm_download_acc")
        return self.unpack(A, self.batch)

    def stage2_factor(self, k):
        buf = ctypes.create_string_buffer(2048)
        prp = c_int(0)
        rc = _chk(lib.gecm_stage2_factor(self._h, k, buf, len(buf), ctypes.byref(prp)), "gecm_stage2_factor")
        return (int(buf.value.decode()), bool(prp.value)) if rc == 1 else None

    def device_name(self):
        buf = ctypes.create_string_buffer(256)
        _chk(lib.gecm_device_name(self._h, buf, len(buf)), "gecm_device_name")
        return buf.value.decode()


class MultiEngine(Engine):
    """One multi-modulus gecm_ctx: curves on many numbers in one batch.  Curve k is the k-th sigma of
    build_curves; every per-curve call works against that curve's own number.  The calls that need one N (L0
    operators, reference-radix uploads and downloads, special forms, report modulus) raise GecmError."""

    def __init__(self, ns, digitbits=52, device=0):
        self._h = c_void_p()
        strs = [str(n).encode() for n in ns]
        arr = (c_char_p * max(1, len(strs)))(*strs)
        _chk(lib.gecm_create_multi(ctypes.byref(self._h), device, arr, len(strs), digitbits), "gecm_create_multi")
        self.cfg = Config()
        _chk(lib.gecm_get_config(self._h, ctypes.byref(self.cfg)), "gecm_get_config")
        self.ns = [int(str(n), 0) if isinstance(n, str) else int(n) for n in ns]
        self.n = max(self.ns)
        self.batch = 0

    def build_curves(self, sigmas, which, params=None):
        """curve k: sigma sigmas[k] on number ns[which[k]]; params as for Engine.build_curves"""
        if len(which) != len(sigmas):
            raise ValueError("build_curves: one modulus index per sigma")
        arr = (c_u64 * len(sigmas))(*sigmas)
        idx = (ctypes.c_uint32 * len(which))(*which)
        self._next_params(params, len(sigmas))
        self.batch = len(sigmas)
        return _chk(lib.gecm_build_curves_multi(self._h, arr, idx, len(sigmas)), "gecm_build_curves_multi")

    def resume(self, sigmas, which, xs, zs, b1_done=0, params=None):
        """Engine.resume with curve k on number ns[which[k]]; xs, zs below that number"""
        if not len(sigmas) == len(which) == len(xs) == len(zs):
            raise ValueError("resume: one modulus index, one x and one z per sigma")
        self._fits(xs, zs)
        arr = (c_u64 * len(sigmas))(*sigmas)
        idx = (ctypes.c_uint32 * len(which))(*which)
        self._next_params(params, len(sigmas))
        self.batch = len(sigmas)
        return _chk(lib.gecm_resume_points_multi(self._h, arr, idx, self.pack(xs), self.pack(zs), len(sigmas), b1_done),
                    "gecm_resume_points_multi")

    def build_seeds(self, method, x0s, which, xs=None, b1_done=1):
        """Engine.build_seeds with position k on number ns[which[k]]"""
        given = xs if xs is not None else x0s
        if given is None or len(which) != len(given) or (x0s is not None and xs is not None and len(x0s) != len(xs)):
            raise ValueError("build_seeds: one modulus index per position, and seeds, residues or one of each")
        self._fits(*[v for v in (x0s, xs) if v is not None])
        idx = (ctypes.c_uint32 * len(which))(*which)
        rc = _chk(lib.gecm_build_seeds_multi(self._h, method, idx, None if x0s is None else self.pack(x0s),
                                             None if xs is None else self.pack(xs), len(given), b1_done),
                  "gecm_build_seeds_multi")
        self.batch = len(given)
        return rc

    def set_packing(self, packing):
        """"wave" (one modulus per wavefront, every number padded to 64 curves) or "lane" (one modulus per lane, only the
        batch's tail padded; numbers up to 415 bits): from the next build_curves or resume on"""
        if packing not in _PACKINGS:
            raise ValueError("set_packing: 'wave' or 'lane'")
        return _chk(lib.gecm_set_multi_packing(self._h, _PACKINGS[packing]), "gecm_set_multi_packing")

    def packing(self):
        """what the last build used"""
        return ["wave", "lane"][_chk(lib.gecm_get_multi_packing(self._h), "gecm_get_multi_packing")]

    def set_rows(self, rows):
        """stage 1 of this context's curve batches with 32 lanes per curve: "off" (the default), "on" or "auto"
        (DESIGN.md §23); holds across builds, takes effect at the next stage-1 launch, and only while
        set_lanes_per_curve is 0"""
        return _chk(lib.gecm_set_multi_rows(self._h, _MULTI_ROWS.get(rows, 2) if isinstance(rows, str) else rows),
                    "gecm_set_multi_rows")

    def rows(self):
        return {v: k for k, v in _MULTI_ROWS.items()}[lib.gecm_get_multi_rows(self._h)]

    def _line_moduli(self):
        return self.ns

    def _resume_recs(self, recs, ns, b1_done, params=None):
        return self.resume([r.sigma for r in recs], [ns.index(r.n) for r in recs], [r.x for r in recs],
                           [r.z for r in recs], b1_done=b1_done, params=params)

    def modulus_of(self, k):
        return _chk(lib.gecm_curve_modulus(self._h, k), "gecm_curve_modulus")

    def acc(self, k):
        """curve k's stage-2 accumulator: the value Engine(ns[modulus_of(k)]).download_acc() gives for it"""
        buf = ctypes.create_string_buffer(1024)
        _chk(lib.gecm_curve_acc(self._h, k, buf, len(buf)), "gecm_curve_acc")
        return int(buf.value.decode(), 16)

    def accs(self):
        return [self.acc(k) for k in range(self.batch)]
