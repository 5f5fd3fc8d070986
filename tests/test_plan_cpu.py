"""The two decisions of a PSF pass (csrc/svr_plan.h), built with g++ through tests/plan_check.cpp: no engine, no GPU.

pass_path: the kernel family, the scatter level and the two table flags of the five passes under the SVR and PVR defaults, on either side of
the density 0.65 and of a gather cell of 96 pixels, with the tile kernels asked for, with fwd_mode set by the caller and under every legacy mode.
table_plan: build first? evaluate, stream or store? over every combination of pass, may_stream_table, table_on_cells, wanted, state, lazy_ok,
usable cells and empty pixel lists, against one literal row per outcome; never a store together with a build."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no C++ compiler in this image")
    exe = str(tmp_path_factory.mktemp("plan") / "plan_check")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "plan_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_every_pass_path_and_table_plan_is_the_listed_one(driver):
    r = subprocess.run([driver], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
