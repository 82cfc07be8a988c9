"""GPU tests of the command line for P-1 / P+1 stage 2: `avx-ecm -m pm1|pp1 -b B2 input B1` and
`-m ... -b B2 -f FILE B1` find planted factors and write the expected bytes; `-b` with B2 <= B1 writes nothing.  The
expected bytes come from Python integers (tests/unit_model.py, tests/unit_s2_model.py)."""
import math
import os
import random
import subprocess
import tempfile

import pytest

from conftest import ROOT
from suyama_model import is_probable_prime
from unit_model import METHOD_PM1, METHOD_PP1, OFFSET, expected, exponent, method_line, random_modulus
from unit_s2_model import CLI, pair_map, plain_acc, planted_case

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "avx-ecm_amd", "avx-ecm")
FILES = ("save_b1.txt", "checkpoint.txt", "ecm_results.txt")
FLAG = {METHOD_PM1: "pm1", METHOD_PP1: "pp1"}
NAME = {METHOD_PM1: "P-1", METHOD_PP1: "P+1"}
B1, B2, D, U = CLI


@pytest.fixture(scope="module")
def pyecm():
    import pyecm
    return pyecm


def _run(args, files=None, rc=0):
    """one driver run in a fresh directory: (stdout, {file: text or None}); `files`: what to put there first"""
    with tempfile.TemporaryDirectory() as d:
        for name, content in (files or {}).items():
            open(os.path.join(d, name), "w").write(content)
        p = subprocess.run([EXE] + [str(a) for a in args], cwd=d, capture_output=True, text=True, timeout=300)
        assert p.returncode == rc, p.stdout + p.stderr
        rd = lambda f: open(os.path.join(d, f)).read() if os.path.exists(os.path.join(d, f)) else None
        return p.stdout, {f: rd(f) for f in FILES}


def size10(f):
    """mpz_sizeinbase(f, 10): the digit count or one more"""
    return int(f.bit_length() * math.log10(2)) + 1


def label(g):
    return "PRP" if is_probable_prime(g) else "C"


def default_seeds(method, n):
    return [3] if method == METHOD_PM1 else [2 * pow(7, -1, n) % n, 6 * pow(5, -1, n) % n]


def expect(pyecm, method, inputs):
    """(save_b1.txt, ecm_results.txt) of a run on `inputs` with the driver's own seeds: the stage-1 lines of every pass,
    its stage-1 factor lines, then a stage-2 line for every position stage 2 flags and stage 1 did not"""
    save, s1, s2 = "", "", ""
    e = exponent(1, B1)
    for i, n in enumerate(inputs):
        for s in default_seeds(method, n):
            x = expected(method, s, e, n)
            save += method_line(method, B1, n, x, s)
            g = math.gcd((x - OFFSET[method]) % n, n)
            if 1 < g < n:
                s1 += "\nfound %s%d factor %d by %s (B1 = %d): input %d, x0 0x%x\n" % (label(g), size10(g), g, NAME[method], B1, i, s)
                continue
            g = math.gcd(plain_acc(method, x, n, [pair_map(pyecm, CLI)], D, U), n)
            if 1 < g < n:
                s2 += "\nfound %s%d factor %d by %s (B1 = %d, B2 = %d): input %d, x0 0x%x\n" % (label(g), size10(g), g, NAME[method], B1,
                                                                                              B2, i, s)
    return save, s1 + s2


def test_pm1_one_number(pyecm):
    n, p, r, seed = planted_case(METHOD_PM1, B1, B2)
    assert seed == 3
    save, results = expect(pyecm, METHOD_PM1, [n])
    assert results == "\nfound PRP%d factor %d by P-1 (B1 = %d, B2 = %d): input 0, x0 0x3\n" % (size10(p), p, B1, B2)
    out, got = _run(["-m", "pm1", "-b", B2, n, B1])
    assert got["save_b1.txt"] == save and got["checkpoint.txt"] is None
    assert got["ecm_results.txt"] == results and results in out
    assert "P-1 stage 2: B2 %d, D %d, U %d" % (B2, D, U) in out


def test_pp1_list_of_inputs(pyecm):
    n, p, r, seed = planted_case(METHOD_PP1, B1, B2, frac=(2, 7))
    other = random_modulus(200, random.Random(83))
    assert seed == default_seeds(METHOD_PP1, n)[0]
    save, results = expect(pyecm, METHOD_PP1, [other, n])
    assert "factor %d by P+1 (B1 = %d, B2 = %d): input 1, x0 0x%x\n" % (p, B1, B2, seed) in results
    out, got = _run(["-m", "pp1", "-b", B2, "-f", "in.txt", B1], files={"in.txt": "%d\n%d\n" % (other, n)})
    assert got["save_b1.txt"] == save and got["checkpoint.txt"] is None
    assert got["ecm_results.txt"] == results and results in out


def test_b2_not_above_b1_writes_nothing():
    n = random_modulus(200, random.Random(79))
    nothing = {f: None for f in FILES}
    for args, files in ((["-m", "pm1", "-b", 1000, n, 1000], None),
                        (["-m", "pp1", "-b", 500, "-f", "in.txt", 1000], {"in.txt": "%d\n" % n}),
                        (["-m", "pm1", "-b", 999, "-x", "in.txt", 1000], {"in.txt": method_line(METHOD_PM1, 500, n, 5, 3)})):
        out, got = _run(args, files=dict(files or {}), rc=1)
        assert "B2 must be above B1" in out, out
        assert got == nothing
