"""CPU tests (no GPU) of the resume front end: gecm_parse_resume_line on every save and checkpoint line the reference wrote
into the fixtures and on the variants a GMP-ECM -save file may hold, its refusals, and gecm_stage1_resume_range against the
reference's checkpoints and the shortened prime ranges the GPU tests use."""
import ctypes
import json
import os
import re

import pytest

from conftest import GOLDEN

GECM_ERR_ARG = -2


@pytest.fixture(scope="module")
def pyecm():
    import pyecm
    return pyecm


@pytest.fixture
def short_ranges(pyecm):
    hook = pyecm.lib.gecm_plan_set_prime_range_for_tests
    hook.argtypes = [ctypes.c_uint64]
    hook.restype = None
    yield hook
    hook(0)


def _fixture_lines():
    out = []
    for f in ("stage1.json", "multirange.json", "batches.json", "special.json"):
        for c in json.load(open(os.path.join(GOLDEN, f))):
            out += c.get("save_lines", []) + c.get("checkpoint_lines", [])
    return out


def _split(line):
    """what a Python split makes of a line of ours"""
    f = dict(p.strip().split("=", 1) for p in line.strip().rstrip(";").split(";"))
    return int(f["SIGMA"]), int(f["B1"]), int(f["N"], 0), int(f["X"], 0), int(f["Z"], 0)


LINES = _fixture_lines()
LINE = LINES[0].rstrip("\n")


def test_every_fixture_line_parses_to_what_split_gives(pyecm):
    assert len(LINES) > 400
    for line in LINES:
        assert tuple(pyecm.parse_resume_line(line)) == _split(line)


def test_variants_of_a_gmp_ecm_save_file(pyecm):
    sigma, b1, n, x, z = want = _split(LINE)
    fields = [p.strip() for p in LINE.rstrip(";").split(";")]
    assert fields[0] == "METHOD=ECM" and fields[-1].startswith("PROGRAM=")
    variants = {
        "reordered": "; ".join(reversed(fields)) + ";",
        "extra fields": "METHOD=ECM; PARAM=0; " + "; ".join(fields[1:]) + "; CHECKSUM=123456789; WHO=someone@host; TIME=Sat Mar  4 "
                        "12:00:00 2023; X0=0x0; Y0=0x0; Y=0x0; COMMENT=2^127-1 = fine, here;",
        "decimal N": LINE.replace("N=0x%x" % n, "N=%d" % n),
        "decimal everything": "METHOD=ECM; SIGMA=%d; B1=%d; N=%d; X=%d; Z=%d;" % want,
        "hex sigma": LINE.replace("SIGMA=%d" % sigma, "SIGMA=0x%x" % sigma),
        "CRLF": LINE + "\r\n",
        "no trailing semicolon": LINE.rstrip(";"),
        "spaces": "  " + LINE.replace("; ", " ;   ").replace("X=", "X = "),
        "upper-case hex": LINE.replace("X=0x%x" % x, "X=0X%X" % x),
    }
    for name, line in variants.items():
        assert tuple(pyecm.parse_resume_line(line)) == want, name
    no_z = "; ".join(f for f in fields if not f.startswith("Z=")) + ";"
    assert tuple(pyecm.parse_resume_line(no_z)) == want[:4] + (1,)
    for skip in ("", "\n", "   \r\n", "# a comment", "  # METHOD=ECM; SIGMA=5;"):
        assert pyecm.parse_resume_line(skip) is None


def test_refusals_name_their_field(pyecm):
    sigma, b1, n, x, z = _split(LINE)
    sub = lambda old, new: LINE.replace(old, new)
    assert "SIGMA=%d;" % sigma in LINE
    cases = [
        (sub("METHOD=ECM", "METHOD=P-1"), "METHOD"),
        (sub("METHOD=ECM;", "METHOD=ECM; PARAM=1;"), "PARAM"),
        (sub("METHOD=ECM;", "METHOD=ECM; PARAM=3;"), "PARAM"),
        (sub("SIGMA=%d; " % sigma, ""), "SIGMA"),
        (sub("B1=%d; " % b1, ""), "B1"),
        (sub("N=0x%x; " % n, ""), "N"),
        (sub("X=0x%x; " % x, ""), "X"),
        (sub("SIGMA=%d;" % sigma, "SIGMA=5;"), "SIGMA"),
        (sub("SIGMA=%d;" % sigma, "SIGMA=%d;" % 2 ** 64), "SIGMA"),
        (sub("SIGMA=%d;" % sigma, "SIGMA=0x1%016x;" % 0), "SIGMA"),
        (sub("N=0x%x" % n, "N=2^127-1"), "N"),
        (sub("N=0x%x" % n, "N=(10^71-1)/9"), "N"),
        (sub("X=0x%x" % x, "X=0x%xg1" % x), "X"),
        (sub("Z=0x%x" % z, "Z=12ab"), "Z"),
        (sub("B1=%d" % b1, "B1=%d.0" % b1), "B1"),
        (sub("X=0x%x" % x, "X="), "X"),
        (sub("X=0x%x" % x, "X=0x"), "X"),
        (sub("X=0x%x" % x, "X=0x" + "f" * 10240), "X"),
        (LINE + " " + LINE, "SIGMA"),                          # two lines run together
        (sub("Z=0x%x;" % z, "Z=0x%x; Z=0x1;" % z), "Z"),
        ("METHOD=ECM; SIGMA=7; B1=100; N=" + "9" * 10240 + "; X=5;", "N"),
    ]
    rec = pyecm.ResumeRec()
    for line, field in cases:
        assert line != LINE
        rc = pyecm.lib.gecm_parse_resume_line(line.encode(), ctypes.byref(rec))
        msg = pyecm.lib.gecm_last_error().decode()
        named = r"\bfield %s\b" % re.escape(field)
        assert rc == GECM_ERR_ARG and re.search(named, msg), (line[:80], rc, msg)
        with pytest.raises(pyecm.GecmError, match=named):
            pyecm.parse_resume_line(line)
    pyecm.lib.gecm_parse_resume_line(sub("N=0x%x" % n, "N=2^127-1").encode(), ctypes.byref(rec))
    assert "expression" in pyecm.lib.gecm_last_error().decode()


def test_resume_range_of_the_reference_s_checkpoints(pyecm):
    mr = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "multirange.json")))}
    field = lambda c: {_split(l)[1] for l in c["checkpoint_lines"]}
    assert field(mr["n204_b1_1.1e8"]) == {99999989} and field(mr["n204_b1_1e8_single_range_checkpoint"]) == {99999989}
    assert pyecm.stage1_resume_range(110000000, 99999989) == 1
    assert pyecm.stage1_resume_range(100000000, 99999989) == 1 == pyecm.stage1_ranges(100000000)   # complete
    assert pyecm.stage1_resume_range(110000000, 110000000) == 2 == pyecm.stage1_ranges(110000000)
    r = ctypes.c_uint32(77)
    assert pyecm.lib.gecm_stage1_resume_range(110000000, 99999971, ctypes.byref(r)) == GECM_ERR_ARG
    assert "not a checkpoint of a run to B1 = 110000000" in pyecm.lib.gecm_last_error().decode()
    with pytest.raises(pyecm.GecmError, match="not a checkpoint"):
        pyecm.stage1_resume_range(110000000, 1000)


def test_resume_range_honours_the_shortened_prime_range(pyecm, short_ranges):
    short_ranges(1000)
    assert pyecm.stage1_resume_range(2500, 997) == 1
    assert pyecm.stage1_resume_range(2500, 1999) == 2
    assert pyecm.stage1_resume_range(2500, 2500) == 3
    for bad in (991, 1009, 2477, 3001):
        with pytest.raises(pyecm.GecmError, match="not a checkpoint"):
            pyecm.stage1_resume_range(2500, bad)


def test_resume_range_with_a_prime_range_length(pyecm, short_ranges):
    """range 503, B1 = 2013: 503 ends the first list and heads the second, and the last range holds no prime — every
    checkpoint field leads to the r + 1 that describe_range implies"""
    short_ranges(503)
    b1 = 2013
    nr = pyecm.stage1_ranges(b1)
    assert nr == 5
    seen = 0
    for r in range(nr):
        d = pyecm.describe_range(b1, b1, r)
        if d.checkpoint and d.nprimes:
            assert pyecm.stage1_resume_range(b1, d.last_prime) == r + 1, (r, d.last_prime)
            seen += 1
    assert seen >= 3
    assert pyecm.describe_range(b1, b1, 0).last_prime == 503
