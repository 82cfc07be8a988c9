"""GPU: `GECM_PACKING=lane avx-ecm -f FILE ...` (host/avx_ecm_main.c).  The passes whose inputs all have at
most 415 bits are lane-packed, larger inputs close the pass and run wave-packed; save_b1.txt and ecm_results.txt are byte
for byte what the default writes."""
import json
import os
import random
import subprocess
import tempfile

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
S1 = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "stage1.json")))}
S2 = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "stage2_acc.json")))}


def _odd(rnd, bits):
    return str(rnd.getrandbits(bits) | (1 << (bits - 1)) | 1)


def _run(inputs, args, env):
    exe = os.path.join(ROOT, "avx-ecm_amd", "avx-ecm")
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "inputs.txt"), "w") as f:
            f.write("\n".join(inputs) + "\n")
        p = subprocess.run([exe, "-f", "inputs.txt"] + [str(a) for a in args], cwd=d, capture_output=True, text=True,
                           timeout=300, env=dict(os.environ, **env))
        assert p.returncode == 0, p.stdout + p.stderr
        files = []
        for name in ("save_b1.txt", "ecm_results.txt"):
            path = os.path.join(d, name)
            files.append(open(path, "rb").read() if os.path.exists(path) else b"")
    return files, p.stdout


def test_lane_packed_passes_write_the_files_of_the_default():
    """six inputs, 8 curves each, B1 = 1000 with stage 2: four of at most 415 bits, two of 623 bits in the middle — a
    lane-packed pass, a wave-packed one, and a lane-packed one again"""
    rnd = random.Random(623)
    inputs = [S1["n415_b1_1000"]["N"], S1["n200_b1_1000"]["N"], S1["n623_b1_1000"]["N"], _odd(rnd, 623),
              S2["K1N_b1_2000_b2_1e5"]["N"], S1["n64_b1_500"]["N"]]
    args = [8, 1000, 1, 50000, 1000]
    plain, out_plain = _run(inputs, args, {})
    lane, out_lane = _run(inputs, args, {"GECM_PACKING": "lane"})
    assert lane[0] == plain[0] and lane[1] == plain[1]
    assert plain[0].count(b"\n") > 0 and plain[1]
    assert out_plain.count("multi-modulus pass:") == 1 and out_plain.count("wave-packed") == 1 and "lane-packed" not in out_plain
    assert out_lane.count("multi-modulus pass:") == 3
    packings = [l.split("-packed")[0].split()[-1] for l in out_lane.splitlines() if l.startswith("multi-modulus pass:")]
    assert packings == ["lane", "wave", "lane"]
    assert out_lane.count("commencing parallel ecm on") == len(inputs)


def test_lane_packing_with_the_device_curve_build_is_refused_before_anything_runs():
    exe = os.path.join(ROOT, "avx-ecm_amd", "avx-ecm")
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "inputs.txt"), "w") as f:
            f.write(S1["n200_b1_1000"]["N"] + "\n")
        for env, text in (({"GECM_PACKING": "lane", "GECM_CURVE_BUILD": "device"}, "cannot be combined with GECM_CURVE_BUILD=device"),
                          ({"GECM_PACKING": "dense"}, "GECM_PACKING must be lane or wave")):
            p = subprocess.run([exe, "-f", "inputs.txt", "8", "1000", "1", "50000", "1000"], cwd=d, capture_output=True,
                               text=True, timeout=60, env=dict(os.environ, **env))
            assert p.returncode == 1 and text in p.stdout, p.stdout + p.stderr
            assert not os.path.exists(os.path.join(d, "save_b1.txt"))
