"""GPU tests of GECM_METHOD_LANES on the command line: `avx-ecm -m pm1 input B1` and
`avx-ecm -m pp1 -f FILE B1` with 16 lanes per residue and with auto write the files byte for byte as with the variable
unset; a bad value exits 1 and writes nothing."""
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


def _run(args, env=None, files=None, rc=0):
    """one driver run in a fresh directory: (stdout, {file: text or None}); `files`: what to put there first"""
    with tempfile.TemporaryDirectory() as d:
        for name, content in (files or {}).items():
            open(os.path.join(d, name), "w").write(content)
        base = {k: v for k, v in os.environ.items() if k != "GECM_METHOD_LANES"}
        p = subprocess.run([EXE] + [str(a) for a in args], cwd=d, capture_output=True, text=True, timeout=300,
                           env=dict(base, **(env or {})))
        assert p.returncode == rc, p.stdout + p.stderr
        rd = lambda f: open(os.path.join(d, f)).read() if os.path.exists(os.path.join(d, f)) else None
        return p.stdout, {f: rd(f) for f in FILES}


def test_pm1_one_number_with_a_factor():
    # a constructed N = p q whose factor p the driver's own seed 3 finds: the first of a seeded sequence of candidates
    for seed in range(40, 60):
        n, p, q = factor_case(METHOD_PM1, random.Random(seed))
        x = expected(METHOD_PM1, 3, exponent(1, 1000), n)
        if py_gcd_flag(METHOD_PM1, x, n) == (p, 1):
            break
    else:
        pytest.fail("setup: seed 3 finds the factor of none of the candidates")
    out, unset = _run(["-m", "pm1", n, 1000])
    assert "k_unit<" in out and unset["save_b1.txt"] == method_line(METHOD_PM1, 1000, n, x, 3)
    assert unset["ecm_results.txt"] and " factor %d by P-1" % p in unset["ecm_results.txt"]
    for value in ("16", "auto"):
        out, got = _run(["-m", "pm1", n, 1000], env={"GECM_METHOD_LANES": value})
        assert "k_unit_row<" in out and got == unset


@pytest.mark.parametrize("packing", ["wave", "lane"])
def test_pp1_list_of_inputs(packing):
    rng = random.Random(78)
    ns = [random_modulus(b, rng) for b in (200, 64, 412)]
    text = "".join("%d\n" % n for n in ns)
    e = exponent(1, 1000)
    want = "".join(method_line(METHOD_PP1, 1000, n, expected(METHOD_PP1, s, e, n), s)
                   for n in ns for s in (2 * pow(7, -1, n) % n, 6 * pow(5, -1, n) % n))
    out, unset = _run(["-m", "pp1", "-f", "in.txt", 1000], env={"GECM_PACKING": packing}, files={"in.txt": text})
    assert unset["save_b1.txt"] == want and "k_unit_row<" not in out
    for value in ("16", "auto") if packing == "wave" else ("16",):
        out, got = _run(["-m", "pp1", "-f", "in.txt", 1000], env={"GECM_PACKING": packing, "GECM_METHOD_LANES": value},
                        files={"in.txt": text})
        assert "k_unit_row<1, 16>" in out and got == unset


def test_a_bad_value_writes_nothing():
    n = random_modulus(200, random.Random(79))
    for value in ("8", "32", "", "AUTO", "0"):
        for args, files in ((["-m", "pm1", n, 1000], None), (["-m", "pp1", "-f", "in.txt", 1000], {"in.txt": "%d\n" % n})):
            out, got = _run(args, env={"GECM_METHOD_LANES": value}, files=files, rc=1)
            assert out == "GECM_METHOD_LANES must be 1, 16 or auto\n"
            assert got == {f: None for f in FILES}
