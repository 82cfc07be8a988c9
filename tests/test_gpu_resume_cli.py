"""GPU tests of `avx-ecm -r FILE B1 [B2]`: a checkpoint file resumed through the remaining prime ranges, a
save file taken to stage 2, a file on two numbers in one multi-modulus pass, the three refusals, and the usage texts of
the two older entries, which stay what they were."""
import json
import os
import subprocess
import tempfile

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "avx-ecm_amd", "avx-ecm")
S1 = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "stage1.json")))}
SPECIAL = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "special.json")))}
FILES = ("save_b1.txt", "checkpoint.txt", "ecm_results.txt")


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


def test_checkpoint_file_goes_through_the_remaining_ranges():
    c = S1["K1N_two_full_batches_b1_500"]                      # no small factor: nothing stops the run
    env = {"GECM_TEST_PRIME_RANGE": "1000"}
    _, full = _run([c["N"], 16, 2500, 1, 2500, 300], env)
    ck = full["checkpoint.txt"].splitlines(keepends=True)
    first = [l for l in ck if "; B1=997; " in l]
    second = [l for l in ck if "; B1=1999; " in l]
    assert len(first) == len(second) == 16 and len(ck) == 32
    # (B2 left out is 100 B1, as on the other command lines: a stage 2 follows, which finds nothing in this N)
    out, got = _run(["-r", "in.txt", 2500], env, {"in.txt": "".join(first)})
    assert got["save_b1.txt"] == full["save_b1.txt"]
    assert got["checkpoint.txt"].splitlines() == [l.rstrip("\n") for l in second]
    assert not got["ecm_results.txt"]
    assert "Saving checkpoint after p=1999" in out and "p=997" not in out and "commencing stage 2" in out
    # stage 1 alone, from a file with a comment and a blank line
    out, got = _run(["-r", "in.txt", 2500, 2500], env, {"in.txt": "# a comment\n\n" + "".join(first)})
    assert got["save_b1.txt"] == full["save_b1.txt"] and "commencing stage 2" not in out
    assert got["checkpoint.txt"].splitlines() == [l.rstrip("\n") for l in second] and not got["ecm_results.txt"]


def _stage2_lines(text):
    return [l for l in (text or "").splitlines() if "in stage 2" in l]


def test_save_file_goes_to_stage_2():
    c = S1["n415_b1_1000"]                                      # small factors
    b1, b2 = 1000, 50000
    _, full = _run([c["N"], 8, b1, 1, b2, c["sigma0"]])
    _, s1only = _run([c["N"], 8, b1, 1, b1, c["sigma0"]])
    assert s1only["save_b1.txt"] == full["save_b1.txt"]
    want = _stage2_lines(full["ecm_results.txt"])
    assert want
    out, got = _run(["-r", "save.txt", b1, b2], files={"save.txt": s1only["save_b1.txt"]})
    assert _stage2_lines(got["ecm_results.txt"]) == want
    assert got["ecm_results.txt"].replace("\n", "") == "".join(want)      # and nothing of stage 1 again
    assert got["save_b1.txt"] is None and got["checkpoint.txt"] is None


def test_file_on_two_numbers_takes_a_multi_modulus_pass():
    b1, b2 = 1000, 50000
    saves = []
    for name in ("n415_b1_1000", "n415_two_batches_b1_1000"):
        c = S1[name]
        _, r = _run([c["N"], 8, b1, 1, b1, c["sigma0"]])
        saves.append(r["save_b1.txt"])
    assert saves[0].split("N=")[1].split(";")[0] != saves[1].split("N=")[1].split(";")[0]
    singles = [_run(["-r", "save.txt", b1, b2], files={"save.txt": s})[1]["ecm_results.txt"] or "" for s in saves]
    assert any(singles)
    out, got = _run(["-r", "save.txt", b1, b2], files={"save.txt": saves[0] + saves[1]})
    assert out.count("multi-modulus pass:") == 1
    assert (got["ecm_results.txt"] or "") == singles[0] + singles[1]
    assert got["save_b1.txt"] is None


def test_refusals_write_nothing():
    c = S1["K1N_two_full_batches_b1_500"]
    lines = [l + "\n" for l in c["save_lines"]]                 # B1 field 500
    other = [l + "\n" for l in S1["n415_b1_1000"]["save_lines"]]   # another N, B1 field 1000
    env = {"GECM_TEST_PRIME_RANGE": "1000"}

    def refused(args, text, *words, env=None):
        out, got = _run(args, env, {"in.txt": text}, rc=1)
        assert all(v is None for v in got.values()), got
        assert len(out.strip().splitlines()) <= 3
        for w in words:
            assert w in out, (w, out)

    # neither B1 nor a checkpoint of a run to it
    refused(["-r", "in.txt", 2500], "".join(lines), "B1 field 500", "checkpoint", "extended", env=env)
    # two numbers with ranges left (the B1 = 997 field is a checkpoint of a run to 2500 under the shortened range)
    two = "".join(l.replace("B1=500;", "B1=997;") for l in lines[:8]) + "".join(l.replace("B1=1000;", "B1=997;") for l in other)
    refused(["-r", "in.txt", 2500], two, "2 numbers", "prime range", env=env)
    # X >= N: what a special-form run of the reference leaves next to N=
    sp = SPECIAL["M251_cofactor"]
    assert any(int(l.split("X=")[1].split(";")[0], 16) >= int(l.split("N=")[1].split(";")[0], 16) for l in sp["save_lines"])
    refused(["-r", "in.txt", sp["B1"], sp["B2"]], "\n".join(sp["save_lines"]), "not below N", "special-form", "2^k", "gecm_set_report_modulus")
    # stage 1 complete and no B2 above B1
    refused(["-r", "in.txt", 500, 500], "".join(lines), "usage: avx-ecm -r")
    # lines on one N in two places, another N between them: they would be two moduli of one multi pass
    split = "".join(lines[:8]) + "".join(l.replace("B1=1000;", "B1=500;") for l in other) + "".join(lines[8:16])
    refused(["-r", "in.txt", 500, 5000], split, "line %d" % (8 + len(other) + 1), "put the lines on one number together")
    # a line that does not parse
    refused(["-r", "in.txt", 500, 5000], lines[0].replace("SIGMA=", "PARAM=1; SIGMA="), "line 1", "PARAM")


def test_the_older_entries_keep_their_usage_text():
    out, _ = _run([], rc=1)
    assert out == "usage: avx-ecm $input $numcurves $B1 [$threads] [$B2] [$sigma]\n"
    out, _ = _run(["-f", "x.txt", 8], rc=1)
    assert out == ("usage: avx-ecm -f $file $numcurves $B1 [$threads] [$B2] [$sigma]\n"
                   "       (one input expression per line; blank lines and lines starting with # are skipped)\n")
    out, _ = _run(["-r", "x.txt"], rc=1)
    assert out.startswith("usage: avx-ecm -r $file $B1 [$B2]\n")
