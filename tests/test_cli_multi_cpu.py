"""CPU: `avx-ecm -f` with a file it cannot read or that holds no input stops with the usage text and exit status 1
before it looks for a device."""
import os
import subprocess
import tempfile

import pytest

from conftest import ROOT

EXE = os.path.join(ROOT, "avx-ecm_amd", "avx-ecm")


@pytest.mark.parametrize("content", [None, "", "# only a comment\n\n   \n"], ids=["missing", "empty", "comments_only"])
def test_file_without_inputs_is_a_usage_error(content):
    with tempfile.TemporaryDirectory() as d:
        if content is not None:
            open(os.path.join(d, "list.txt"), "w").write(content)
        p = subprocess.run([EXE, "-f", "list.txt", "8", "1000"], cwd=d, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1, p.stdout + p.stderr
        assert "usage: avx-ecm -f $file $numcurves $B1" in p.stdout
        assert not os.path.exists(os.path.join(d, "save_b1.txt"))


def test_file_option_without_its_arguments_is_a_usage_error():
    p = subprocess.run([EXE, "-f", "list.txt", "8"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "usage: avx-ecm -f $file" in p.stdout
