"""Who holds device memory, measured from outside (csrc/svr_devbuf.h, DESIGN.md "Who owns device memory").

A context gives everything back when it is destroyed, and the entry points whose buffers live for one call only -- svr_stack_motion,
svr_slice_quality, svr_slice_ssim, svr_resample_to_reconstruction, svr_channel_scatter -- leave the device's free memory where they
found it.  Two refused calls are measured too: both fail an argument check before anything is allocated, so they show that a refusal takes
nothing, not that an error path after the allocations gives it back -- that is the destructors' work, checked without a device by
tests/devbuf_check.cpp.  Free memory is the driver's own figure (torch.cuda.mem_get_info); every entry point runs once before it is
measured, so that what a kernel's first launch makes the runtime keep (code, scratch) is not counted.

The two big grids take what their arrays hold and no more: reserve() counts elements where hipMalloc counted bytes, and a byte count
handed to it would quadruple a float buffer without any result changing.  A slice grid of 512 x 512 x 16 pixels asks for 33 bytes per
pixel in the per-pixel arrays (five float images 20, a byte image 1, three 32-bit arrays 12) and under 1 more in the three tile lists
(12 bytes per 4 x 4 tile) and the partial sums; a volume of 128^3 voxels for 20 per voxel (recon | volw, addon | cmap, the second volume)
and the mask for 4.  The bounds are 34 bytes per pixel and 24 per voxel plus 32 MiB for the allocator's rounding (about 25 and 4
allocations): one float image taken for bytes adds 12 bytes per element, 50 MB and 25 MB at these sizes, and does not fit under them.
(Measured, before and after the buffers changed their owner: 142606336 and 50331648 bytes, 34 and 24 per element.)

The measurements run in one child process (this file as a script): torch carries its own copy of the HIP runtime and has to come up before
the engine's library does, which no test process that ran another engine test first can promise."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


def _run(prob):
    """a context after one Gaussian reconstruction and one SR iteration on the tiny phantom"""
    from fetalreconstruction_amd import engine as E
    from tests.twins.reconstruction import irtkReconstruction
    rec = E.Reconstruction(0)
    E.sync_gpu(rec, prob)
    d = irtkReconstruction(rec, prob.ns, max_intensity=prob.max_intensity, min_intensity=prob.min_intensity)
    d.SetSmoothingParameters(150, 0.02)
    d.reconstruct_iteration(1)
    rec.syncCPU()
    return rec


def _after_destroy(prob):
    after = []
    for _ in range(3):
        rec = _run(prob)
        rec.close()
        after.append(_free())
    return after


def _around_calls(prob):
    rec = _run(prob)
    rng = np.random.default_rng(2)
    windows = rng.uniform(0.0, 1.0, (4, 96)).astype(np.float32)
    chan = rng.integers(0, 256, prob.slices.shape).astype(np.float32)
    src = rng.uniform(0.0, 100.0, tuple(rec.vsize[::-1])).astype(np.float32)
    ident = np.eye(4)[:3]
    calls = {
        "svr_stack_motion": lambda: rec.stack_motion(windows),
        "svr_slice_quality": lambda: rec.slice_quality(),
        "svr_slice_ssim": lambda: rec.slice_ssim(2, 6.5, 58.5),
        "svr_slice_ssim with the map": lambda: rec.slice_ssim(2, 6.5, 58.5, want_map=True),
        "svr_resample_to_reconstruction": lambda: rec.resample_to_reconstruction(src, ident),
        "svr_channel_scatter": lambda: rec.channel_scatter(chan),
        # argument checks that fail after the context is set up and before anything is allocated: no array to write to, more slices than pixels
        "refused: svr_slice_quality": lambda: rec._lib.svr_slice_quality(rec._h, None),
        "refused: svr_stack_motion": lambda: rec._lib.svr_stack_motion(rec._h, windows.ctypes.data_as(C.c_void_p), 2, 4, None, None, None, None),
    }
    diffs = {}
    for name, call in calls.items():
        call()                                              # (see the module's docstring)
        before = _free()
        r = call()
        diffs[name] = _free() - before
        assert not name.startswith("refused") or r != 0, name
    rec.close()
    return diffs


GRID = (512, 512, 16)          # slice grid (sx, sy, ns)
VOL = (128, 128, 128)
SLACK = 32 << 20


def _grids_take():
    """free memory taken by svr_init_storage_volumes and by svr_init_reconstruction_volume + svr_set_mask on a fresh context"""
    from fetalreconstruction_amd import engine as E
    rec = E.Reconstruction(0)
    f0 = _free()
    rec.initStorageVolumes(GRID, (1.0, 1.0, 2.0))
    f1 = _free()
    rec.InitReconstructionVolume(VOL, (1.0, 1.0, 1.0))
    rec.setMask(VOL, (1.0, 1.0, 1.0), np.ones(VOL[::-1], np.float32))
    f2 = _free()
    rec.close()
    return {"slice_grid": f0 - f1, "volume": f1 - f2}


@pytest.fixture(scope="module")
def measured():
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    print(got)
    return got


def test_destroying_a_context_returns_its_memory(measured):
    after = measured["after_destroy"]
    assert len(after) == 3 and after[1] >= after[0] and after[2] >= after[0], after


def test_per_call_scratch_is_returned(measured):
    diffs = measured["around_calls"]
    assert len(diffs) == 8 and all(d == 0 for d in diffs.values()), diffs


def test_the_grids_take_what_their_arrays_hold(measured):
    took = measured["grids_take"]
    npx, nv = int(np.prod(GRID)), int(np.prod(VOL))
    assert 33 * npx <= took["slice_grid"] <= 34 * npx + SLACK, (took, npx)
    assert 24 * nv <= took["volume"] <= 24 * nv + SLACK, (took, nv)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import torch
    torch.cuda.init()
    from fetalreconstruction_amd import phantom
    tiny = phantom.problem_tiny()
    after = _after_destroy(tiny)                            # (first: the runtime has loaded the engine's code before anything is measured)
    print(json.dumps({"after_destroy": after, "grids_take": _grids_take(), "around_calls": _around_calls(tiny)}), flush=True)
