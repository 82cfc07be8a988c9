"""GPU tests of `avx-ecm -x FILE B1 [B2]`: the save file of a reference-semantic run taken to a higher B1
in one segment and in several, a file on two numbers in one multi-modulus pass, and the refusals, each of which leaves the
directory as it was.  The expected lines come from Python integers (tests/xladder.py), as in tests/test_gpu_extend.py."""
import json
import os
import subprocess
import tempfile

import pytest

from conftest import GOLDEN, ROOT
from xladder import _primes, ladder_point, stage1_multiplier

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "avx-ecm_amd", "avx-ecm")
S1 = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "stage1.json")))}
FILES = ("save_b1.txt", "checkpoint.txt", "ecm_results.txt")
N412 = int(S1["K1"]["N"])               # no small factor: every Z met here has an inverse
N297 = int(S1["T35_46"]["N"])
SIG = list(range(1000, 1008))


def std_line(n, sigma, b):
    u, v = (sigma * sigma - 5) % n, 4 * sigma % n
    x = pow(u, 3, n) * pow(pow(v, 3, n), -1, n) % n
    a24 = pow(v - u, 3, n) * (3 * u + v) % n * pow(16 * pow(u, 3, n) * v % n, -1, n) % n
    X, Z = ladder_point(n, x, a24, stage1_multiplier(b + 1))
    return "METHOD=ECM; PARAM=0; SIGMA=%d; B1=%d; N=0x%x; X=0x%x; PROGRAM=AVX-ECM-STD;\n" % (sigma, b, n, X * pow(Z, -1, n) % n)


def std_text(n, b):
    return "".join(std_line(n, s, b) for s in SIG)


def _described(lo, hi):
    """(primes of (lo, hi], prime powers beyond the first in (lo, hi]) as the driver's segment line states them"""
    primes = _primes(hi)
    powers = sum(1 for p in primes for e in range(2, 41) if lo < p ** e <= hi)
    return sum(1 for p in primes if p > lo), powers


def _run(args, env=None, files=None, rc=0):
    """one driver run in a fresh directory: (stdout, {file: text or None}); `files`: what to put there first"""
    with tempfile.TemporaryDirectory() as d:
        for name, text in (files or {}).items():
            open(os.path.join(d, name), "w").write(text)
        p = subprocess.run([EXE] + [str(a) for a in args], cwd=d, capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, **(env or {})))
        assert p.returncode == rc, p.stdout + p.stderr
        rd = lambda f: open(os.path.join(d, f)).read() if os.path.exists(os.path.join(d, f)) else None
        return p.stdout, {f: rd(f) for f in FILES}


@pytest.fixture(scope="module")
def reference_save():
    """save_b1.txt of `avx-ecm N 8 1000 1` (stage 1 only, sigmas 1000..1007): reference lines, B1 field 1000"""
    _, got = _run([N412, 8, 1000, 1, 1000, 1000])
    assert got["save_b1.txt"].count("PROGRAM=AVX-ECM;\n") == 8 and "; B1=1000; " in got["save_b1.txt"]
    return got["save_b1.txt"]


def test_single_n(reference_save):
    want = std_text(N412, 3000)
    out, got = _run(["-x", "save_b1.txt", 3000, 3000], files={"save_b1.txt": reference_save})
    # the run appends to the save_b1.txt it finds, as every run does
    assert got["save_b1.txt"] == reference_save + want
    assert got["checkpoint.txt"] is None and not got["ecm_results.txt"]
    assert "extending 8 curves on N = %d from B1 = 999 to 3000\n" % N412 in out
    assert _described(999, 3000) == (262, 11)           # 2^10, 2^11, 3^7, 7^4, 11^3, 13^3 and the squares of 37 .. 53
    assert "Extending Stage 1 over (999 : 3000]: 262 primes and 11 further prime-power steps\n" in out
    assert "Stage 1 complete to 3000 at prime 2999 with " in out and "commencing stage 2" not in out
    # the same in short segments: the same save lines, and standard lines at every cut in checkpoint.txt
    env = {"GECM_TEST_PRIME_RANGE": "1024"}
    out, got = _run(["-x", "in.txt", 3000, 3000], env, {"in.txt": reference_save})
    assert got["save_b1.txt"] == want
    assert got["checkpoint.txt"] == std_text(N412, 1024) + std_text(N412, 2048)
    assert out.count("Extending Stage 1 over (") == 3
    assert "Extending Stage 1 over (1024 : 2048]: %d primes and %d further prime-power steps\n" % _described(1024, 2048) in out
    assert "Saving checkpoint after p=1024" in out and "Saving checkpoint after p=2048" in out
    # standard lines go on from their own field, and a bound equal to B1 launches nothing: normalise, write, stage 2
    out, got = _run(["-x", "in.txt", 3000, 3000], files={"in.txt": std_text(N412, 1024)})
    assert got["save_b1.txt"] == want and "from B1 = 1024 to 3000" in out
    out, got = _run(["-x", "in.txt", 3000, 20000], files={"in.txt": want})
    assert got["save_b1.txt"] == want and "commencing stage 2" in out
    assert "Extending Stage 1 over (3000 : 3000]: 0 primes and 0 further prime-power steps\n" in out


def test_two_n(reference_save):
    _, other = _run([N297, 8, 1000, 1, 1000, 1000])
    out, got = _run(["-x", "in.txt", 3000, 3000], files={"in.txt": reference_save + other["save_b1.txt"]})
    assert out.count("multi-modulus pass:") == 1 and "stage 1 extended" in out
    assert got["save_b1.txt"] == std_text(N412, 3000) + std_text(N297, 3000)
    assert got["checkpoint.txt"] is None and not got["ecm_results.txt"]


def test_refusals_write_nothing(reference_save):
    lines = reference_save.splitlines(keepends=True)
    std = std_text(N412, 1024).splitlines(keepends=True)

    def refused(args, text, *words, env=None):
        out, got = _run(args, env, {"in.txt": text}, rc=1)
        assert all(v is None for v in got.values()), got
        assert len(out.strip().splitlines()) <= 3
        for w in words:
            assert w in out, (w, out)

    # lines of one group complete to different bounds: a reference line (999) and a standard line (1024) of one N
    refused(["-x", "in.txt", 3000], lines[0] + std[1], "line 2", "not complete to the bound 999")
    # a bound above B1
    refused(["-x", "in.txt", 900], reference_save, "line 1", "complete to B1 = 999", "upwards")
    # a reference-semantic line above one prime range
    refused(["-x", "in.txt", 3000], reference_save, "line 1", "several prime ranges", "no standard multiplier",
            env={"GECM_TEST_PRIME_RANGE": "512"})
    # several N and more than one segment
    other = std_text(N297, 1024).splitlines(keepends=True)
    two = "".join(std) + "".join(other)
    refused(["-x", "in.txt", 3000], two, "2 numbers", "several segments", "one file per number",
            env={"GECM_TEST_PRIME_RANGE": "1024"})
    # what -r refuses: a line that does not parse, X not below N, one N in two places
    refused(["-x", "in.txt", 3000], lines[0].replace("SIGMA=", "PARAM=1; SIGMA="), "line 1", "PARAM")
    refused(["-x", "in.txt", 3000], lines[0].replace("X=0x", "X=0xfffffffffffffffffffffffffffffffffffffffffffffff"), "not below N")
    split = "".join(std[:4]) + "".join(other[:2]) + "".join(std[4:])
    refused(["-x", "in.txt", 3000], split, "line 7", "put the lines on one number together")
    out, _ = _run(["-x", "in.txt"], rc=1)
    assert out.startswith("usage: avx-ecm -x $file $B1 [$B2]\n")
