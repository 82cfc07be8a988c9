"""The avx-ecm command line on inputs of 1032 to 1311 bits (wide contexts): the plain run writes
save_b1.txt and the stage-1 factor lines of ecm_results.txt byte for byte as the REFERENCE wrote them
(tests/golden/wide.json, made by tests/golden/make_golden_wide.py from oracle/_ref/avx-ecm-52 and -32), skips stage 2 with
one line that names `ecm -resume save_b1.txt`, and the other modes refuse such an input in one line."""
import json
import os
import subprocess
import tempfile

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
EXE = {52: os.path.join(ROOT, "avx-ecm_amd", "avx-ecm"), 32: os.path.join(ROOT, "avx-ecm_amd", "avx-ecm-32")}
WIDE = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "wide.json")))}
NOTICE = "ecm -resume save_b1.txt"


def _lines(text):
    return [l for l in text.splitlines() if l.strip()]


def _run(digitbits, args, ok=True):
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run([EXE[digitbits]] + [str(a) for a in args], cwd=d, capture_output=True, text=True, timeout=300)
        if ok:
            assert p.returncode == 0, p.stdout + p.stderr
        read = lambda f: open(os.path.join(d, f)).read() if os.path.exists(os.path.join(d, f)) else ""
        return p, read("save_b1.txt"), [l for l in read("ecm_results.txt").splitlines() if l.strip()]


@pytest.mark.parametrize("name", sorted(WIDE))
def test_plain_run_writes_the_references_files(name):
    c = WIDE[name]
    p, save, res = _run(c["digitbits"], [c["input"], c["curves"], c["B1"], 1, c["B2"], c["sigma0"]])
    assert save == c["save"]
    assert res == _lines(c["results"])
    for line in c["banner"]:
        assert line in p.stdout.splitlines(), line
    assert "x 28 bits on the device" in p.stdout and NOTICE not in p.stdout


def test_m1277_in_the_32_bit_format_writes_the_52_bit_lines():
    """the residues do not depend on the limb format: the first eight of avx-ecm-32's sixteen lines are avx-ecm-52's (the
    reference's own 32-bit build is no yardstick on this input, tests/golden/make_golden_wide.py)"""
    c = WIDE["m1277_d52"]
    p, save, res = _run(32, [c["input"], 16, c["B1"], 1, c["B2"], c["sigma0"]])
    assert len(save.splitlines()) == 16 and save.splitlines()[:8] == c["save"].splitlines() and res == []
    assert "Choosing MAXBITS = 1280, NWORDS = 40, NBLOCKS = 10 based on input size 1277" in p.stdout


@pytest.mark.parametrize("name", ["random_1247_d52", "m1277_d52"])
def test_stage_2_is_skipped_with_one_line(name):
    c = WIDE[name]
    p, save, res = _run(c["digitbits"], [c["input"], c["curves"], c["B1"], 1, 100 * c["B1"], c["sigma0"]])   # the default B2
    assert save == c["save"] and res == _lines(c["results"])
    assert [NOTICE in l for l in p.stdout.splitlines()].count(True) == 1
    assert "pair-muls in stage 2" not in p.stdout


@pytest.mark.parametrize("mode", [["-m", "pm1", "%s", 1000], ["-p", 1, "%s", 8, 1000]], ids=["pm1", "param"])
def test_other_modes_refuse_a_wide_input(mode):
    n = WIDE["random_1247_d52"]["input"]
    p, save, res = _run(52, [a % n if a == "%s" else a for a in mode], ok=False)
    text = p.stdout + p.stderr
    assert p.returncode != 0 and "larger than this build supports" in text
    assert len([l for l in text.splitlines() if "larger than this build supports" in l]) == 1
    assert save == "" and res == []
