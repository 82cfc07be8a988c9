"""GPU tests of the command line for GMP-ECM's PARAM 1 and PARAM 3 curves: `avx-ecm -p PARAM ...`, a fresh
run in standard mode, and `avx-ecm -g -r / -g -x FILE B1 [B2]`, which read save files holding such lines; the refusals
leave the directory as it was.  The expected lines come from Python integers (tests/param_model.py, tests/xladder.py)."""
import json
import os
import subprocess
import tempfile

import pytest

from conftest import GOLDEN, ROOT
from param_model import param_line, param_point
from xladder import ladder_point, stage1_multiplier

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "avx-ecm_amd", "avx-ecm")
S1 = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "stage1.json")))}
FILES = ("save_b1.txt", "checkpoint.txt", "ecm_results.txt")
N412 = int(S1["K1"]["N"])               # no small factor: every Z met here has an inverse
SIG = list(range(1000, 1008))


def suyama_line(n, sigma, b):
    u, v = (sigma * sigma - 5) % n, 4 * sigma % n
    x = pow(u, 3, n) * pow(pow(v, 3, n), -1, n) % n
    a24 = pow(v - u, 3, n) * (3 * u + v) % n * pow(16 * pow(u, 3, n) * v % n, -1, n) % n
    X, Z = ladder_point(n, x, a24, stage1_multiplier(b + 1))
    return "METHOD=ECM; PARAM=0; SIGMA=%d; B1=%d; N=0x%x; X=0x%x; PROGRAM=AVX-ECM-STD;\n" % (sigma, b, n, X * pow(Z, -1, n) % n)


def text(param, b, sig=SIG):
    return "".join(suyama_line(N412, s, b) if param == 0 else param_line(N412, param, s, b) for s in sig)


def gmp_ecm_text(param, b, sig=SIG):
    """the same curves as a GMP-ECM -save file holds them: x alone, CHECKSUM, its own PROGRAM"""
    out = ""
    for s in sig:
        X, Z = param_point(N412, param, s, b)
        out += ("METHOD=ECM; PARAM=%d; SIGMA=%d; B1=%d; N=%d; X=0x%x; CHECKSUM=%d; PROGRAM=GMP-ECM 7.0.5; X0=0x0; Y0=0x0; "
                "WHO=someone@host; TIME=Mon Jan  1 00:00:00 2024;\n" % (param, s, b, N412, X * pow(Z, -1, N412) % N412, 1234567 + s))
    return out


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


@pytest.mark.parametrize("param", [1, 3, 0])
def test_fresh_run_in_standard_mode(param):
    out, got = _run(["-p", param, N412, 8, 1000, 1000, 1000])
    assert got["save_b1.txt"] == text(param, 1000)
    assert got["checkpoint.txt"] is None and not got["ecm_results.txt"]
    assert "Extending Stage 1 over (1 : 1000]: 168 primes and " in out and "commencing stage 2" not in out


def test_fresh_run_in_segments_with_stage_2_and_its_own_sigmas():
    env = {"GECM_TEST_PRIME_RANGE": "512"}
    out, got = _run(["-p", 3, N412, 8, 1000, 1000, 1000], env)
    assert got["save_b1.txt"] == text(3, 1000) and got["checkpoint.txt"] == text(3, 512)
    assert out.count("Extending Stage 1 over (") == 2 and "Saving checkpoint after p=512" in out
    # no sigma given: the driver's generator, reduced into [2, 2^32); B2 left out is 100 B1
    out, got = _run(["-p", 1, N412, 8, 300])
    lines = got["save_b1.txt"].splitlines()
    assert len(lines) == 8 and "commencing stage 2" in out
    for l in lines:
        sigma = int(l.split("SIGMA=")[1].split(";")[0])
        assert l.startswith("METHOD=ECM; PARAM=1; SIGMA=") and 2 <= sigma < 2**32
        assert l + "\n" == param_line(N412, 1, sigma, 300)


def test_a_gmp_ecm_file_is_extended_with_g_and_refused_without():
    save = gmp_ecm_text(1, 1000)
    out, got = _run(["-g", "-x", "gmp.txt", 3000, 3000], files={"gmp.txt": save})
    assert got["save_b1.txt"] == text(1, 3000)
    assert got["checkpoint.txt"] is None and not got["ecm_results.txt"]
    assert "extending 8 curves on N = %d from B1 = 1000 to 3000\n" % N412 in out
    for opt in ("-x", "-r"):
        out, got = _run([opt, "gmp.txt", 3000, 30000], files={"gmp.txt": save}, rc=1)
        assert all(got[f] is None for f in FILES), got
        assert len(out.strip().splitlines()) <= 3 and "line 1" in out and "PARAM" in out


def test_resume_of_a_param_3_file_runs_stage_2():
    save = gmp_ecm_text(3, 1000)
    out, got = _run(["-g", "-r", "gmp.txt", 1000, 20000], files={"gmp.txt": save})
    assert "resuming 8 curves on N = %d after stage 1" % N412 in out and "commencing stage 2" in out
    assert got["save_b1.txt"] is None and got["checkpoint.txt"] is None and not got["ecm_results.txt"]


def test_a_file_mixing_the_parametrisations_goes_through_in_one_group():
    lines = []
    for k, s in enumerate(SIG):
        param = (0, 1, 3)[k % 3]
        lines.append((suyama_line(N412, s, 1000) if param == 0 else gmp_ecm_text(param, 1000, [s]), param, s))
    out, got = _run(["-g", "-x", "mixed.txt", 3000, 3000], files={"mixed.txt": "".join(l for l, _, _ in lines)})
    assert "extending 8 curves on N = %d from B1 = 1000 to 3000\n" % N412 in out and out.count("extending ") == 1
    assert got["save_b1.txt"] == "".join(suyama_line(N412, s, 3000) if p == 0 else param_line(N412, p, s, 3000) for _, p, s in lines)


def test_refusals_write_nothing():
    out, got = _run(["-p", 2, N412, 8, 1000, 1000, 1000], rc=1)
    assert all(v is None for v in got.values()) and "usage: avx-ecm -p $param $input $numcurves $B1 [$B2] [$sigma]\n" in out
    bad = gmp_ecm_text(1, 1000).replace("PARAM=1;", "PARAM=2;", 1)
    out, got = _run(["-g", "-x", "in.txt", 3000], files={"in.txt": bad}, rc=1)
    assert all(v is None for v in got.values()) and "line 1" in out and "PARAM" in out and len(out.strip().splitlines()) <= 3
    zero = gmp_ecm_text(3, 1000).replace("SIGMA=1003;", "SIGMA=0;")
    out, got = _run(["-g", "-r", "in.txt", 1000, 20000], files={"in.txt": zero}, rc=1)
    assert all(v is None for v in got.values()) and "line 4" in out and "SIGMA" in out


def test_usage_lines():
    out, _ = _run(["-p"], rc=1)
    assert out.startswith("usage: avx-ecm -p $param $input $numcurves $B1 [$B2] [$sigma]\n")
    out, _ = _run(["-g", "-r", "x.txt"], rc=1)
    assert out.startswith("usage: avx-ecm -g -r $file $B1 [$B2]\n")
    out, _ = _run(["-g", "-x", "x.txt"], rc=1)
    assert out.startswith("usage: avx-ecm -g -x $file $B1 [$B2]\n")
    out, _ = _run(["-g"], rc=1)
    assert "usage: avx-ecm -g -r $file" in out and "usage: avx-ecm -g -x $file" in out
    # the older entries keep theirs
    out, _ = _run(["-x", "x.txt"], rc=1)
    assert out.startswith("usage: avx-ecm -x $file $B1 [$B2]\n") and "-g" not in out
    out, _ = _run(["-r", "x.txt"], rc=1)
    assert out.startswith("usage: avx-ecm -r $file $B1 [$B2]\n") and "-g" not in out
