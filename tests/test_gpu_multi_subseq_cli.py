"""GPU: `GECM_MULTI_SUBSEQ=auto avx-ecm -f FILE ...` (host/avx_ecm_main.c): stage 2 of the multi-modulus
passes runs with sub-sequences per curve chosen by batch size; save_b1.txt and ecm_results.txt are byte for byte what the
default writes, and the "multi-modulus pass:" line names the K that ran."""
import json
import os
import re
import subprocess
import tempfile

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
S1 = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "stage1.json")))}
S2 = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "stage2_acc.json")))}
EXE = os.path.join(ROOT, "avx-ecm_amd", "avx-ecm")
INPUTS = [S1["n415_b1_1000"]["N"], S2["K1N_b1_2000_b2_1e5"]["N"], S1["n200_b1_1000"]["N"]]
ARGS = ["8", "1000", "1", "50000", "1000"]


def _run(env):
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "inputs.txt"), "w") as f:
            f.write("\n".join(INPUTS) + "\n")
        p = subprocess.run([EXE, "-f", "inputs.txt"] + ARGS, cwd=d, capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, **env))
        assert p.returncode == 0, p.stdout + p.stderr
        files = []
        for name in ("save_b1.txt", "ecm_results.txt"):
            path = os.path.join(d, name)
            files.append(open(path, "rb").read() if os.path.exists(path) else b"")
    return files, p.stdout


def _pass_ks(out):
    lines = [l for l in out.splitlines() if l.startswith("multi-modulus pass:")]
    return [int(re.search(r"and stage 2 \(K = (\d+)\)", l).group(1)) for l in lines]


def test_sub_sequences_by_batch_size_write_the_files_of_the_default():
    """three inputs, 8 curves each, B1 = 1000 and B2 = 50000, under both packings"""
    for packing in ("wave", "lane"):
        auto, out_auto = _run({"GECM_MULTI_SUBSEQ": "auto", "GECM_PACKING": packing})
        # the yardstick: the switch unset, or set to what unset means
        plain, out_plain = _run(dict({"GECM_PACKING": packing}, **({"GECM_MULTI_SUBSEQ": "default"} if packing == "lane" else {})))
        assert auto[0] == plain[0] and auto[1] == plain[1], packing
        assert plain[0].count(b"\n") > 0 and plain[1]
        ks = _pass_ks(out_auto)
        assert len(ks) == 1 and ks[0] > 1, out_auto
        assert _pass_ks(out_plain) == [1], out_plain


def test_a_bad_value_is_refused_before_anything_runs():
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "inputs.txt"), "w") as f:
            f.write(INPUTS[0] + "\n")
        p = subprocess.run([EXE, "-f", "inputs.txt"] + ARGS, cwd=d, capture_output=True, text=True, timeout=60,
                           env=dict(os.environ, GECM_MULTI_SUBSEQ="8"))
        assert p.returncode == 1 and "GECM_MULTI_SUBSEQ must be auto or default" in p.stdout, p.stdout + p.stderr
        assert not os.path.exists(os.path.join(d, "save_b1.txt"))
