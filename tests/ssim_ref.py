"""Shared by tests/test_structural.py and tests/test_structural_gpu.py: the numpy float64 restatement of svr_slice_ssim
(csrc/svr_ssim.inc, stated in include/svr_hip.h), of the decision rule svr_structural_decide (include/svr_host.h), and the tiny phantom
with one slice shifted inside its own plane -- the case --structural is for: such a slice keeps a fair global correlation and loses its
local structure.  The operands and the pixel set are those of tests/slice_quality_ref.py (imported, not restated)."""
import math

import numpy as np

from tests import slice_quality_ref as qref
from tests.slice_quality_ref import CORRUPT_SLICE, CORRUPT_STACK, read_report  # noqa: F401  (the tests take them from here)

HEADER_EX = qref.HEADER + ["ssim", "n_ssim", "structural"]
ROLL = (6, 5)                                          # the shift of the corrupted slice, pixels along (rows, columns)
DEFAULTS = dict(radius=3, k_mad=3.0, min_drop=0.1, min_pixels=25)
# Largest per-pixel |ssim(exactly rounded window sums) - ssim(window sums added left to right in raster order)| on the inputs of
# general_case below, measured by tests/test_structural.py::test_the_order_of_the_window_sums_shows_this_much (which asserts that what
# it measures is no larger, so a changed input or formula shows).  The device adds in a third order (rows, then columns) and is allowed
# 4 x this per pixel.
MEASURED = {"general": 6.4e-15, "general_bias": 5.3e-15}         # measured 6.328e-15 and 5.218e-15 (bias: with the float64 exponential rounded to float32)


def operands(slices, simslices, simweights, scales, bias=None, exp64=False):
    """-> x float32 [ns][sy][sx], y float32, V bool: qual_pixel's operands and set (slice_quality_ref.terms forms them)"""
    shp = np.asarray(slices).shape
    _, inset, t = qref.terms(slices, simslices, simweights, np.ones(shp, np.float32), scales, bias, exp64)
    x, y = t[..., 0].astype(np.float32), t[..., 1].astype(np.float32)
    assert np.array_equal(x.astype(np.float64), t[..., 0]) and np.array_equal(y.astype(np.float64), t[..., 1])    # float32 values, widened
    return x.reshape(shp), y.reshape(shp), inset.reshape(shp)


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def window_sums(x, y, V, R, mode="ltr"):
    """The window's count m (int64) and {Sx, Sy, Sxx, Syy, Sxy} (float64 [5][ns][sy][sx]) over the pixels of V in the (2R+1)^2 box
    clipped to the grid.  mode "ltr": the terms added one by one in raster order of the window (rows top to bottom, left to right in a
    row); "fsum": every sum exactly rounded (math.fsum, pixel by pixel: slow); "dd": the terms added error-free (TwoSum) with the errors
    collected apart and added once at the end -- twice the working precision, fast, and bit-equal to "fsum" on every input of these tests
    (test_structural.py asserts it where it measures)."""
    ns, sy, sx = x.shape
    x64, y64 = np.where(V, x, 0).astype(np.float64), np.where(V, y, 0).astype(np.float64)
    terms = np.stack([x64, y64, x64 * x64, y64 * y64, x64 * y64])
    pad = np.pad(terms, ((0, 0), (0, 0), (R, R), (R, R)))
    vpad = np.pad(V.astype(np.int64), ((0, 0), (R, R), (R, R)))
    m = np.zeros((ns, sy, sx), np.int64)
    offs = [(dy, dx) for dy in range(2 * R + 1) for dx in range(2 * R + 1)]
    for dy, dx in offs:
        m += vpad[:, dy:dy + sy, dx:dx + sx]
    if mode == "fsum":
        S = np.zeros((5, ns, sy, sx))
        cols = np.stack([pad[:, :, dy:dy + sy, dx:dx + sx] for dy, dx in offs], -1).reshape(-1, len(offs))
        S.reshape(-1)[:] = [math.fsum(r) for r in cols.tolist()]
        return m, S
    hi, lo = np.zeros((5, ns, sy, sx)), np.zeros((5, ns, sy, sx))
    for dy, dx in offs:
        t = pad[:, :, dy:dy + sy, dx:dx + sx]
        if mode == "ltr":
            hi = hi + t
        else:
            hi, e = _two_sum(hi, t)
            lo = lo + e
    return m, (hi + lo if mode == "dd" else hi)


def ssim_from_sums(m, S, V, R, c1, c2):
    """-> (counted bool, ssim float64, nan where not counted), the expressions in the order include/svr_hip.h writes them"""
    counted = V & (m >= ((2 * R + 1) ** 2 + 1) // 2)
    md = np.where(counted, m, 1).astype(np.float64)
    sx, sy, sxx, syy, sxy = S
    with np.errstate(invalid="ignore", divide="ignore"):
        mx, my = sx / md, sy / md
        vx, vy, cxy = sxx / md - mx * mx, syy / md - my * my, sxy / md - mx * my
        num = ((2.0 * mx) * my + c1) * (2.0 * cxy + c2)
        den = ((mx * mx + my * my) + c1) * ((vx + vy) + c2)
        val = num / den
    return counted, np.where(counted, val, np.nan)


def ssim_map(slices, simslices, simweights, scales, R, c1, c2, bias=None, exp64=False, mode="ltr"):
    """-> (counted bool [ns][sy][sx], ssim float64 with nan where not counted, m int64)"""
    x, y, V = operands(slices, simslices, simweights, scales, bias, exp64)
    m, S = window_sums(x, y, V, R, mode)
    counted, val = ssim_from_sums(m, S, V, R, c1, c2)
    return counted, val, m


def slice_sums(counted, val):
    """float64 [ns][2] = {n_ssim, S ssim}, the sum exactly rounded"""
    ns = counted.shape[0]
    out = np.zeros((ns, 2))
    for i in range(ns):
        out[i] = [counted[i].sum(), math.fsum(val[i][counted[i]].tolist())]
    return out


def decide(stack_index, sums, eligible, min_pixels=25, k_mad=3.0, min_drop=0.1):
    """svr_structural_decide -> (q float64 [ns], nan = not judged; excluded bool [ns])"""
    si = np.asarray(stack_index)
    n = len(si)
    sums = np.asarray(sums, np.float64).reshape(n, 2)
    q = np.full(n, np.nan)
    for i in range(n):
        if eligible[i] and sums[i, 0] > 0 and sums[i, 0] >= min_pixels:
            q[i] = sums[i, 1] / sums[i, 0]
    ex = np.zeros(n, bool)

    def median(v):
        v = sorted(v)
        k = len(v)
        return v[k // 2] if k % 2 else (v[k // 2 - 1] + v[k // 2]) / 2.0

    for st in sorted(set(si.tolist())):
        idx = [i for i in range(n) if si[i] == st and not math.isnan(q[i])]
        if len(idx) < 4:
            continue
        med = median([q[i] for i in idx])
        mad = median([abs(q[i] - med) for i in idx])
        threshold = med - max(k_mad * 1.4826 * mad, min_drop)
        for i in idx:
            ex[i] = q[i] < threshold
    return q, ex


def constants(max_intensity, min_intensity):
    """c1, c2 as svrh_structural_evaluate forms them"""
    L = float(max_intensity) - float(min_intensity)
    return (0.01 * L) * (0.01 * L), (0.03 * L) * (0.03 * L)


def general_case(seed=11, ns=40, sx=96, sy=80):
    """random floats (the general case of tests/test_slice_quality_gpu.py with more of the simulated weights above 0.99) -> s, y, simw, scales"""
    rng = np.random.default_rng(seed)
    shp = (ns, sy, sx)
    s = rng.uniform(1.0, 1000.0, shp).astype(np.float32)
    s[rng.random(shp) < 0.1] = -1.0
    scales = rng.uniform(0.8, 1.2, ns).astype(np.float32)
    y = (np.abs(s) * scales[:, None, None] + rng.normal(0.0, 30.0, shp)).astype(np.float32)
    simw = rng.uniform(0.985, 1.0, shp).astype(np.float32)   # two pixels in three above 0.99: windows on both sides of the half-window threshold
    return s, y, simw, scales


GENERAL_C = constants(1000.0, 0.0)


def general_bias(shape):
    return np.random.default_rng(13).uniform(-0.3, 0.3, shape).astype(np.float32)


def rolled_stacks():
    """slice_quality_ref.corrupted_stacks with another corruption: the slice shifted by ROLL inside its own plane (np.roll)"""
    from fetalreconstruction_amd import phantom
    stacks, mask, mattr, rattr, rmask = phantom.make_stacks(3, (32, 32, 8), 1.1, 2.2, None, 1.0, 14.0, seed=1, orientations=("ax", "cor", "sag"),
                                                            stack_motion_mm=0.0, stack_motion_deg=0.0)
    d = stacks[CORRUPT_STACK].data
    d[CORRUPT_SLICE] = np.roll(d[CORRUPT_SLICE].copy(), ROLL, (0, 1)).astype(d.dtype)
    return stacks, rattr, rmask


SCHEDULE = dict(qref.SCHEDULE)


def write_cli_case(d, iterations=1):
    """the stacks and the mask as files -> the common arguments of the command line (slice_quality_ref.write_cli_case's, on the rolled slice)"""
    from fetalreconstruction_amd import nifti
    stacks, rattr, rmask = rolled_stacks()
    paths = []
    for k, st in enumerate(stacks):
        nifti.write(d / f"stack{k}.nii.gz", st.data, st.attr)
        paths.append(str(d / f"stack{k}.nii.gz"))
    nifti.write(d / "mask.nii.gz", rmask, rattr)
    return ["-i", *paths, "-m", str(d / "mask.nii.gz"), "--thickness", "2.2", "2.2", "2.2", "--resolution", "1.0", "--no_registration",
            "--iterations", str(iterations), "--rec_iterations_last", str(SCHEDULE["rec_last"]), "--smooth_mask", "0"]
