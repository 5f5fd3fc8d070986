"""The coefficient table's layout (csrc/svr_coeff.h CoeffLayout), built with g++ through tests/coeff_layout_check.cpp: no engine, no GPU.

For support 16 and 12 over three pixels the program enumerates (pixel id, plane, quad, row) and checks that the index is a layout -- no two
tuples share a float4, none lies beyond the pixels' bytes, support 16 fills them and support 12 leaves exactly rows 12 .. 15 of every quad --
that the 16 rows of a quad are 256 contiguous bytes, that a pixel takes 16384 / 9216 bytes, and that the index is the expression the
kernels carried by hand before the header existed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no C++ compiler in this image")
    exe = str(tmp_path_factory.mktemp("coeff_layout") / "coeff_layout_check")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "coeff_layout_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_the_coefficient_table_index_is_a_layout(driver):
    r = subprocess.run([driver], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
