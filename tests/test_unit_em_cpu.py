"""The host two-class EM over units (csrc/svr_unit_em.h unit_em), built with g++ through tests/unit_em_check.cpp: no engine, no GPU.

The slice form must give the CPU oracle's bits (oracle.pyoracle.host_estep: potentials with the exclusions applied, weights, the five
scalars); the patch form, with its potentials read through the stacks' offset-less copy, a direct evaluation here to the tolerance of
glibc's expf against numpy's float32 exp."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.unit_em_cases import SLICE_CASES, STEP, _case   # the builders live with the device tests' cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no C++ compiler in this image")
    exe = str(tmp_path_factory.mktemp("unit_em") / "unit_em_check")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Werror",
           "-o", exe, os.path.join(ROOT, "tests", "unit_em_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_unit_em(exe, tmp_path, form, pot, w, scale, excluded, var_floor, classes, counts=()):
    n = len(pot)
    blob = b"".join([np.array([form, n], np.int32).tobytes(), np.array([var_floor, STEP], np.float64).tobytes(),
                     np.asarray(classes, np.float32).tobytes(), np.asarray(pot, np.float32).tobytes(),
                     np.asarray(w, np.float32).tobytes(), np.asarray(scale, np.float32).tobytes(),
                     np.asarray(excluded, np.uint8).tobytes(), np.array([len(counts)], np.int32).tobytes(),
                     np.asarray(counts, np.int32).tobytes()])
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(blob)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    out = np.frombuffer(dst.read_bytes(), np.float32)
    return out[:n].copy(), out[n:2 * n].copy(), out[2 * n:].copy()


@pytest.mark.parametrize("name", list(SLICE_CASES))
def test_slice_form_is_the_oracle_bit_for_bit(driver, oracle_mod, tmp_path, name):
    pot, w, scale, fe, small, st = SLICE_CASES[name]
    excl = np.zeros(len(pot), np.uint8)
    excl[fe] = 1
    excl[small] = 1
    p, wt, c = run_unit_em(driver, tmp_path, 0, pot, w, scale, excl, STEP * STEP / 6.28, st)
    op, ow, ost = oracle_mod.host_estep(pot, w, scale, fe, small, STEP, np.float32(st))
    assert np.array_equal(p.view(np.uint32), op.view(np.uint32)), name
    assert np.array_equal(wt.view(np.uint32), ow.view(np.uint32)), name
    assert np.array_equal(c.view(np.uint32), ost.view(np.uint32)), (name, c, ost)
    if name == "likelihood == 0":
        mean, mean2, var, var2, _ = (float(x) for x in c)
        g = lambda x, s: STEP * np.exp(-x * x / (2 * s)) / np.sqrt(6.28 * s)   # noqa: E731
        tail = p[-4:].astype(np.float64)
        assert mean < mean2
        assert all(g(x - mean, var) == 0 and g(x - mean2, var2) == 0 for x in tail[:3]), (tail, c)
        assert wt[-4] == 1 and wt[-3] == 1 and wt[-2] == 0   # the two between the classes, the one above the outliers
    if name == "all units excluded":
        assert np.all(p == -1) and np.all(wt == 0) and c[4] == np.float32(0.9)


def _patch_direct(pot, w, scale, counts, st):
    """The patch-based E-step's host half restated: the potentials of stack k at the patch indices 0 .. counts[k]-1 (no stack offset,
    the later stacks win), the float Gaussian, sums in double."""
    n = len(pot)
    pp = np.zeros(n, np.float32)
    ofs = 0
    for c in counts:
        pp[:c] = pot[ofs:ofs + c]
        ofs += c
    pp[(scale < 0.2) | (scale > 5)] = -1
    w = w.copy()
    m = pp >= 0
    pw, p = w[m].astype(np.float64), pp[m].astype(np.float64)
    mean = np.float32(np.sum(p * pw) / np.sum(pw))
    mean2 = np.float32(np.sum(p * (1 - pw)) / np.sum(1 - pw))
    var = np.float32(np.sum(((p - mean) ** 2) * pw) / np.sum(pw))
    var2 = np.float32(np.sum(((p - mean2) ** 2) * (1 - pw)) / np.sum(1 - pw))
    floor = np.float64(np.float32(0.0001) * np.float32(0.0001)) / 6.28
    var, var2 = max(var, np.float32(floor)), max(var2, np.float32(floor))
    mix = np.float32(st[4])
    g = lambda x, s: np.float32(0.00001) * np.exp(-x * x / (np.float32(2) * s)) / np.sqrt(np.float32(6.28) * s)   # noqa: E731
    for i in range(n):
        x = pp[i]
        if x == -1:
            w[i] = 0
            continue
        g1 = float(g(np.float32(x - mean), var)) if x < mean2 else 0.0
        g2 = float(g(np.float32(x - mean2), var2)) if x > mean else 0.0
        lik = g1 * mix + g2 * (1 - mix)
        w[i] = g1 * mix / lik if lik > 0 else (0 if x >= mean2 else 1)
    return pp, w, np.float32([mean, mean2, var, var2, np.mean(w[pp >= 0].astype(np.float64))])


def test_patch_form_with_the_offset_less_copy(driver, tmp_path):
    rng = np.random.default_rng(7)
    counts = [9, 4, 13, 6]                                           # stacks of different sizes: most patches read another's potential
    n = sum(counts)
    pot, w, scale = _case(rng, n, 0.15)
    scale[[0, 12, 13]] = 1
    st = [0, 0, 0.02, 0.03, 0.8]
    p, wt, c = run_unit_em(driver, tmp_path, 1, pot, w, scale, np.zeros(n, np.uint8), np.float32(0.0001) * np.float32(0.0001) / 6.28, st, counts)
    dp, dw, dc = _patch_direct(pot, w, scale, counts, st)
    assert np.array_equal(p, dp)
    assert p[0] == pot[9 + 4 + 13] and p[12] == pot[9 + 4 + 12] and p[13] == 0     # the last stack to reach an index wins; none reaches 13
    assert np.allclose(wt, dw, atol=1e-4)                          # expf of glibc vs numpy's float32 exp
    assert np.allclose(c, dc, rtol=1e-5)
