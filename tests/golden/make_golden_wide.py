#!/usr/bin/env python3
"""Generate tests/golden/wide.json by RUNNING THE REFERENCE ITSELF (oracle/_ref/avx-ecm-52 and avx-ecm-32, built from the
reference's sources by `make -C oracle ref`; build container only).  The fixture is data: inputs, and the save_b1.txt and
ecm_results.txt the reference wrote for them.  Numbers of 1032 to 1311 bits, the sizes a wide context serves
(DESIGN.md §24): B1 = B2 = 1000, which turns stage 2 off in the reference (main.c:548-552), and a fixed sigma.

usage: python tests/golden/make_golden_wide.py
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFDIR = os.path.join(ROOT, "oracle", "_ref")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import wide_row_model as W  # noqa: E402

B1 = 1000
CASES = [
    # name, input expression, digitbits, curves, sigma
    ("random_1247_d52", str(W.modulus(1247, "random")), 52, 8, 1000),
    ("random_1247_d32", str(W.modulus(1247, "random")), 32, 16, 1000),
    ("random_1039_d52", str(W.modulus(1039, "random")), 52, 16, 77777),
    ("random_1039_d32", str(W.modulus(1039, "random")), 32, 16, 77777),
    ("m1277_d52", "2^1277-1", 52, 8, 1234567),
    # (no 2^1277-1 from avx-ecm-32: on this input the reference's DIGITBITS = 32 build writes, for every second curve, a point
    # that is not proportional to the one its DIGITBITS = 52 build writes for the same sigma — its special reduction at a
    # k that is no multiple of 32 — so that output is no yardstick; tests/test_gpu_wide_cli.py holds avx-ecm-32 to the
    # 52-bit fixture instead, whose lines do not depend on the limb format)
]


def run_ref(expr, digitbits, curves, sigma):
    exe = os.path.join(REFDIR, "avx-ecm-%d" % digitbits)
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run([exe, expr, str(curves), str(B1), "1", str(B1), str(sigma)], cwd=d, capture_output=True, text=True,
                           timeout=600)
        assert p.returncode == 0, p.stdout + p.stderr
        read = lambda f: open(os.path.join(d, f)).read() if os.path.exists(os.path.join(d, f)) else ""
        return p.stdout, read("save_b1.txt"), read("ecm_results.txt")


def main():
    out = []
    for name, expr, digitbits, curves, sigma in CASES:
        stdout, save, res = run_ref(expr, digitbits, curves, sigma)
        banner = [l for l in stdout.splitlines() if l.startswith(("Choosing MAXBITS", "Input has", "Using special"))]
        assert save.count("\n") >= 8, name            # a batch that finds a factor is the reference's last
        out.append({"name": name, "input": expr, "digitbits": digitbits, "curves": curves, "B1": B1, "B2": B1, "sigma0": sigma,
                    "save": save, "results": res, "banner": banner})
        print(name, len(save.splitlines()), "lines,", len(res.splitlines()), "result lines")
    with open(os.path.join(HERE, "wide.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
