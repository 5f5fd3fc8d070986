"""Shared by tests/test_slice_quality.py and tests/test_slice_quality_gpu.py: the numpy restatement of svr_slice_quality's ten sums
(csrc/svr_quality.inc) and of the derived values (csrc/svr_io.cpp), and the corrupted tiny phantom of the command-line tests."""
import math

import numpy as np

HEADER = ("stack_index included excluded outside weight scale TranslationX TranslationY TranslationZ RotationX RotationY RotationZ "
          "n_px n ncc rmse mae mean_weight").split()
CORRUPT_STACK, CORRUPT_SLICE = 1, 4                    # the slice of the tiny phantom that is replaced


def terms(slices, simslices, simweights, weights, scales, bias=None, exp64=False):
    """Per slice (n_px, the M-step set as a mask, the eight summands in float64).  x and e are formed in float32 first, as the kernel
    forms them (k_mstep's expressions); exp64: expf replaced by the float64 exponential rounded to float32."""
    ns = slices.shape[0]
    s, y, sw, w = (np.ascontiguousarray(a, np.float32).reshape(ns, -1) for a in (slices, simslices, simweights, weights))
    scale = np.asarray(scales, np.float32).reshape(ns, 1)
    if bias is None:
        x = s * scale
        inset = (s != -1) & (sw > np.float32(0.99))
    else:
        b = np.ascontiguousarray(bias, np.float32).reshape(ns, -1)
        eb = np.exp(-b.astype(np.float64)).astype(np.float32) if exp64 else np.exp(-b)
        assert eb.dtype == np.float32
        x = (s * eb) * scale
        inset = (s != -1) & (sw.astype(np.float64) > 0.99)
    assert x.dtype == np.float32
    e = x - y
    x64, y64, e64 = x.astype(np.float64), y.astype(np.float64), e.astype(np.float64)
    t = np.stack([x64, y64, x64 * x64, y64 * y64, x64 * y64, e64 * e64, np.abs(e64), w.astype(np.float64)], -1)
    return (s != -1).sum(1), inset, t


def sums(slices, simslices, simweights, weights, scales, bias=None, exp64=False):
    """float64 [ns][10]; every sum exactly rounded (math.fsum), so the restatement itself adds no summation error"""
    n_px, inset, t = terms(slices, simslices, simweights, weights, scales, bias, exp64)
    out = np.zeros((len(n_px), 10))
    out[:, 0] = n_px
    out[:, 1] = inset.sum(1)
    for i in range(len(n_px)):
        sel = t[i][inset[i]]
        out[i, 2:] = [math.fsum(sel[:, k]) for k in range(8)]
    return out


def abs_sums(slices, simslices, simweights, weights, scales, bias=None):
    """sum |term| of the eight sums: the scale of a double summation's worst-case error"""
    n_px, inset, t = terms(slices, simslices, simweights, weights, scales, bias)
    return np.stack([np.abs(t[i][inset[i]]).sum(0) for i in range(len(n_px))])


def derive(s):
    """{ncc, rmse, mae, mean_weight} of one row, as include/svr_host.h states them"""
    n, sx, sy, sxx, syy, sxy, see, sae, swt = (float(v) for v in s[1:])
    ncc = rmse = mae = mw = math.nan
    if n >= 2:
        under = (sxx - sx * sx / n) * (syy - sy * sy / n)
        if under > 0:
            ncc = (sxy - sx * sy / n) / math.sqrt(under)
    if n > 0:
        rmse, mae, mw = math.sqrt(see / n), sae / n, swt / n
    return np.array([ncc, rmse, mae, mw])


def read_report(path):
    """-> (header names, float64 [rows][18])"""
    lines = open(path).read().splitlines()
    return lines[0].split("\t"), np.array([[float(v) for v in ln.split("\t")] for ln in lines[1:]], np.float64).reshape(len(lines) - 1, -1)


def corrupted_stacks():
    """The tiny phantom as stacks (three of 32 x 32 x 8, as phantom.problem_tiny) with one slice of one stack replaced by its transpose with
    reversed intensities: a slice that fits the volume nowhere."""
    from fetalreconstruction_amd import phantom
    stacks, mask, mattr, rattr, rmask = phantom.make_stacks(3, (32, 32, 8), 1.1, 2.2, None, 1.0, 14.0, seed=1, orientations=("ax", "cor", "sag"),
                                                            stack_motion_mm=0.0, stack_motion_deg=0.0)
    d = stacks[CORRUPT_STACK].data
    sl = d[CORRUPT_SLICE].copy()
    d[CORRUPT_SLICE] = (sl.max() - sl.T).astype(d.dtype)
    return stacks, rattr, rmask


SCHEDULE = dict(iterations=1, rec_last=5, delta=150.0, last_lambda=0.01)


def write_cli_case(d):
    """the stacks and the mask as files -> the common arguments of the command line"""
    from fetalreconstruction_amd import nifti
    stacks, rattr, rmask = corrupted_stacks()
    paths = []
    for k, st in enumerate(stacks):
        nifti.write(d / f"stack{k}.nii.gz", st.data, st.attr)
        paths.append(str(d / f"stack{k}.nii.gz"))
    nifti.write(d / "mask.nii.gz", rmask, rattr)
    return ["-i", *paths, "-m", str(d / "mask.nii.gz"), "--thickness", "2.2", "2.2", "2.2", "--resolution", "1.0", "--no_registration",
            "--iterations", str(SCHEDULE["iterations"]), "--rec_iterations_last", str(SCHEDULE["rec_last"]), "--smooth_mask", "0"]
