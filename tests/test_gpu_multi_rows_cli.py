"""GPU: `GECM_MULTI_ROWS=on avx-ecm -f FILE ...` (host/avx_ecm_main.c): stage 1 of the multi-modulus pass
runs with 32 lanes per curve under both packings; save_b1.txt and ecm_results.txt are byte for byte what `off` writes,
and a bad value is refused before anything is written."""
import json
import os
import subprocess
import tempfile

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
S1 = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "stage1.json")))}
S2 = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "stage2_acc.json")))}
EXE = os.path.join(ROOT, "avx-ecm_amd", "avx-ecm")
INPUTS = [S1["n415_b1_1000"]["N"], S2["K1N_b1_2000_b2_1e5"]["N"], S1["n200_b1_1000"]["N"]]
ARGS = ["8", "1000", "1", "1000", "1000"]      # curves B1 threads B2 sigma: stage 1 only, and the sigmas of every run the same


def _run(env, check=True):
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "inputs.txt"), "w") as f:
            f.write("\n".join(INPUTS) + "\n")
        p = subprocess.run([EXE, "-f", "inputs.txt"] + ARGS, cwd=d, capture_output=True, text=True, timeout=120,
                           env=dict(os.environ, **env))
        if check:
            assert p.returncode == 0, p.stdout + p.stderr
        files = []
        for name in ("save_b1.txt", "ecm_results.txt"):
            path = os.path.join(d, name)
            files.append(open(path, "rb").read() if os.path.exists(path) else None)
    return files, p


@pytest.mark.parametrize("packing", ["wave", "lane"])
def test_rows_write_the_files_of_off(packing):
    """three inputs, 8 curves each, B1 = 1000 (n415_b1_1000 finds factors in stage 1)"""
    on, p_on = _run({"GECM_MULTI_ROWS": "on", "GECM_PACKING": packing})
    off, p_off = _run({"GECM_MULTI_ROWS": "off", "GECM_PACKING": packing})
    assert on[0] is not None and on[0].count(b"\n") > 0 and on[1]
    assert on[0] == off[0] and on[1] == off[1]
    passes = [l for l in p_on.stdout.splitlines() if l.startswith("multi-modulus pass:")]
    assert len(passes) == 1 and "%s-packed" % packing in passes[0] and "with 32 lanes per curve" in passes[0], p_on.stdout
    assert "32 lanes per curve" not in p_off.stdout and p_off.stdout.count("multi-modulus pass:") == 1


def test_a_bad_value_is_refused_before_anything_is_written():
    files, p = _run({"GECM_MULTI_ROWS": "yes"}, check=False)
    assert p.returncode == 1 and "GECM_MULTI_ROWS must be on, auto or off" in p.stdout, p.stdout + p.stderr
    assert files == [None, None]
