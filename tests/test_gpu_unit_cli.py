"""GPU tests of the command line for P-1 and P+1: `avx-ecm -m pm1|pp1 input B1 [x0]`, `-m ... -f FILE B1`
under both packings, `-m ... -x FILE B1`, and the refusals, which leave the directory as it was.  The expected bytes come
from Python integers (tests/unit_model.py)."""
import math
import os
import random
import subprocess
import tempfile

import pytest

from conftest import ROOT
from unit_model import METHOD_PM1, METHOD_PP1, expected, exponent, factor_case, method_line, py_gcd_flag, random_modulus

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "avx-ecm_amd", "avx-ecm")
FILES = ("save_b1.txt", "checkpoint.txt", "ecm_results.txt")
FLAG = {METHOD_PM1: "pm1", METHOD_PP1: "pp1"}
NAME = {METHOD_PM1: "P-1", METHOD_PP1: "P+1"}


def _run(args, env=None, files=None, rc=0):
    """one driver run in a fresh directory: (stdout, {file: text or None}); `files`: what to put there first"""
    with tempfile.TemporaryDirectory() as d:
        for name, content in (files or {}).items():
            open(os.path.join(d, name), "w").write(content)
        p = subprocess.run([EXE] + [str(a) for a in args], cwd=d, capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, **(env or {})))
        assert p.returncode == rc, p.stdout + p.stderr
        rd = lambda f: open(os.path.join(d, f)).read() if os.path.exists(os.path.join(d, f)) else None
        return p.stdout, {f: rd(f) for f in FILES}


def size10(f):
    """mpz_sizeinbase(f, 10): the digit count or one more"""
    return int(f.bit_length() * math.log10(2)) + 1


def default_seeds(method, n):
    return [3] if method == METHOD_PM1 else [2 * pow(7, -1, n) % n, 6 * pow(5, -1, n) % n]


def lines_of(method, n, seeds, lo, hi, known=True, start=None):
    e = exponent(lo, hi)
    return "".join(method_line(method, hi, n, expected(method, x, e, n), s if known else None)
                   for s, x in zip(seeds, start or seeds))


@pytest.mark.parametrize("method", [METHOD_PM1, METHOD_PP1])
def test_one_number_finds_its_factor(method):
    # a constructed N = p q whose factor p the driver's own seeds find: the first of a seeded sequence of candidates
    for seed in range(40, 60):
        n, p, q = factor_case(method, random.Random(seed))
        seeds = default_seeds(method, n)
        hits = [s for s in seeds if py_gcd_flag(method, expected(method, s, exponent(1, 1000), n), n) == (p, 1)]
        if hits:
            break
    assert hits, "setup: the default seeds find the factor of none of the candidates"
    out, got = _run(["-m", FLAG[method], n, 1000])
    assert got["save_b1.txt"] == lines_of(method, n, seeds, 1, 1000) and got["checkpoint.txt"] is None
    want = "".join("\nfound PRP%d factor %d by %s (B1 = 1000): input 0, x0 0x%x\n" % (size10(p), p, NAME[method], s) for s in hits)
    assert got["ecm_results.txt"] == want and want in out
    assert "k_unit<" in out
    # a seed of the caller's
    out, got = _run(["-m", FLAG[method], n, 1000, 5])
    assert got["save_b1.txt"] == lines_of(method, n, [5], 1, 1000)


@pytest.mark.parametrize("method", [METHOD_PP1, METHOD_PM1])
def test_list_of_inputs_under_both_packings(method):
    rng = random.Random(77)
    ns = [random_modulus(b, rng) for b in (200, 64, 412)]
    text = "# three inputs\n" + "".join("%d\n" % n for n in ns[:2]) + "\n  %d+0  \n" % ns[2]
    want = "".join(lines_of(method, n, default_seeds(method, n), 1, 1000) for n in ns)
    runs = {}
    for packing in ("wave", "lane"):
        out, got = _run(["-m", FLAG[method], "-f", "in.txt", 1000], env={"GECM_PACKING": packing}, files={"in.txt": text})
        assert got["save_b1.txt"] == want and got["checkpoint.txt"] is None
        assert ("k_unit_lane<" if packing == "lane" else "k_unit_multi<") in out
        runs[packing] = got
    assert runs["wave"] == runs["lane"]
    # a number 7 divides: P+1's first seed does not exist, the gcd is reported, the second seed runs
    if method == METHOD_PP1:
        out, got = _run(["-m", "pp1", "-f", "in.txt", 1000], files={"in.txt": "%d\n%d\n" % (7 * ns[0], ns[1])})
        n7 = 7 * ns[0]
        assert got["ecm_results.txt"].startswith("\nfound PRP1 factor 7 by P+1 (B1 = 1000): input 0, x0 2/7 has no inverse\n")
        assert got["save_b1.txt"] == lines_of(method, n7, [6 * pow(5, -1, n7) % n7], 1, 1000) + \
            lines_of(method, ns[1], default_seeds(method, ns[1]), 1, 1000)


@pytest.mark.parametrize("method", [METHOD_PM1, METHOD_PP1])
def test_lines_taken_to_a_higher_b1(method):
    rng = random.Random(78)
    ns = [random_modulus(b, rng) for b in (200, 297)]
    out, first = _run(["-m", FLAG[method], "-f", "in.txt", 1000], files={"in.txt": "".join("%d\n" % n for n in ns)})
    saved = first["save_b1.txt"]
    out, got = _run(["-m", FLAG[method], "-x", "save_b1.txt", 3000], files={"save_b1.txt": saved})
    want = "".join(lines_of(method, n, default_seeds(method, n), 1, 3000) for n in ns)
    assert got["save_b1.txt"] == saved + want                       # appended to the file it read
    # lines without their seed, one number: the single-N kernel, no X0 in what is written
    n = ns[0]
    bare = "".join(l.replace("X0=0x%x; " % s, "") for l, s in zip(saved.splitlines(True), default_seeds(method, n)))
    out, got = _run(["-m", FLAG[method], "-x", "in.txt", 3000], files={"in.txt": bare})
    assert got["save_b1.txt"] == lines_of(method, n, default_seeds(method, n), 1, 3000, known=False) and "k_unit<" in out


def test_refusals_write_nothing():
    n = random_modulus(200, random.Random(79))
    nothing = {f: None for f in FILES}
    pm1 = method_line(METHOD_PM1, 1000, n, 5, 3)
    ecm = "METHOD=ECM; PARAM=0; SIGMA=7; B1=1000; N=0x%x; X=0x5; PROGRAM=AVX-ECM-STD;\n" % n
    for args, files, text in (
            (["-m", "ecm", n, 1000], None, "pm1 (P-1) and pp1 (P+1)"),
            (["-m", "pm1", "-f", "in.txt", 1000, 100000], {"in.txt": "%d\n" % n}, "no stage 2"),
            (["-m", "pp1", "-x", "in.txt", 1000, 100000], {"in.txt": pm1}, "no stage 2"),
            (["-m", "pm1", n, 1000, 3, 100000], None, "no stage 2"),
            (["-m", "pm1", "-x", "in.txt", 3000], {"in.txt": ecm}, "METHOD=ECM line"),
            (["-m", "pp1", "-x", "in.txt", 3000], {"in.txt": pm1}, "METHOD=P-1 line"),
            (["-m", "pm1", "-x", "in.txt", 500], {"in.txt": pm1}, "extended upwards only"),
            (["-m", "pm1", "-x", "in.txt", 3000], {"in.txt": pm1 + pm1.replace("B1=1000", "B1=2000")}, "not complete to the bound"),
            (["-m", "pm1", "-x", "in.txt", 3000], {"in.txt": pm1 + method_line(METHOD_PM1, 1000, n + 2, 5, 3) + pm1}, "stand further up"),
            (["-m", "pm1", "-x", "in.txt", 3000], {"in.txt": pm1.replace("X=0x5", "X=0x%x" % (n + 1))}, "not below N"),
            (["-m", "pm1", n, 1000, n], None, "x0 must be a number below"),
            (["-m", "pm1", n, 1], None, "B1 must be"),
            (["-m", "pm1", n + 1, 1000], None, "odd integer")):
        out, got = _run(args, files=dict(files or {}), rc=1)
        assert text in out, out
        assert got == nothing
