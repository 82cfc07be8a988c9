"""GPU: `avx-ecm -f FILE curves B1 [threads] [B2] [sigma]` (host/avx_ecm_main.c).  The inputs of the file
run in multi-modulus passes, except the ones the reference folds modulo 2^k -/+ c, which take the one-input path in their
place; save_b1.txt and ecm_results.txt must be byte for byte what running `avx-ecm <input> ...` for every line in turn
writes in the same directory — each input's stopping rule included (lines up to its first batch with a factor)."""
import json
import os
import subprocess
import tempfile

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
S1 = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "stage1.json")))}
SPECIAL = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "special.json")))}
S2 = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "stage2_acc.json")))}


def _files(d):
    out = []
    for f in ("save_b1.txt", "ecm_results.txt"):
        p = os.path.join(d, f)
        out.append(open(p, "rb").read() if os.path.exists(p) else b"")
    return out


def _compare(exe, inputs, args, env=None):
    env = dict(os.environ, **(env or {}))
    with tempfile.TemporaryDirectory() as d1, tempfile.TemporaryDirectory() as d2:
        for x in inputs:
            p = subprocess.run([exe, x] + [str(a) for a in args], cwd=d1, capture_output=True, text=True, timeout=300, env=env)
            assert p.returncode == 0, p.stdout + p.stderr
        with open(os.path.join(d2, "inputs.txt"), "w") as f:
            f.write("# a list\n\n" + "\n".join(inputs[:2]) + "\n   \n" + "\n".join(inputs[2:]) + "\n")
        p = subprocess.run([exe, "-f", "inputs.txt"] + [str(a) for a in args], cwd=d2, capture_output=True, text=True,
                           timeout=300, env=env)
        assert p.returncode == 0, p.stdout + p.stderr
        single, multi = _files(d1), _files(d2)
    return single, multi, p.stdout


INPUTS = ["fib(401)",                                   # an expression
          S1["n415_b1_1000"]["N"],                      # a factor in the first batch: the stop rule
          SPECIAL["M251_cofactor"]["N"],                # folded by the reference: the one-input path, in its place
          S2["K1N_b1_2000_b2_1e5"]["N"],
          S1["n831_b1_1000"]["N"]]                      # another size


@pytest.mark.parametrize("env, passes", [({}, 2), ({"GECM_PASS_CURVES": "64"}, 4)], ids=["full_passes", "one_input_per_pass"])
def test_file_of_inputs_writes_what_single_runs_write(env, passes):
    """the folded input splits the others into two passes (two inputs each), or four when a pass takes one input"""
    single, multi, out = _compare(os.path.join(ROOT, "avx-ecm_amd", "avx-ecm"), INPUTS, [32, 1000, 2, 50000, 1000], env)
    assert multi[0] == single[0]
    assert multi[1] == single[1]
    assert single[1] and single[0].count(b"\n") > 0
    assert out.count("multi-modulus pass:") == passes
    assert out.count("commencing parallel ecm on") == len(INPUTS)


def test_file_of_inputs_32_bit_build():
    single, multi, _ = _compare(os.path.join(ROOT, "avx-ecm_amd", "avx-ecm-32"), INPUTS[:2] + INPUTS[3:4],
                                [16, 1000, 2, 50000, 1000])
    assert multi == single
