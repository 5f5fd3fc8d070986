"""Bias correction on the device at size (svr_bias.inc, bias_mode 1) and from the command line (--enableBiasCorrection):
the LDS kernels against the stencils bit for bit on P4, against the oracle on a phantom the oracle can afford, the C++ host
object's SR iterations with bias on, the command line end to end, one rank against two."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests.twins.reconstruction import irtkReconstruction
from tests.util import rel_err, run_to_state

pytestmark = pytest.mark.gpu


def _biased(P, seed=0):
    """P with a smooth multiplicative bias field on every slice (as tests/test_bias.py's _biased)."""
    import copy
    Q = copy.copy(P)
    ns, sy, sx = P.slices.shape
    yy, xx = np.meshgrid(np.linspace(-1, 1, sy), np.linspace(-1, 1, sx), indexing="ij")
    field = np.exp(0.25 * xx - 0.15 * yy)[None] * (1 + 0.05 * np.sin(np.arange(ns) + seed)[:, None, None])
    Q.slices = np.where(P.slices > 0, P.slices * field, P.slices).astype(np.float32)
    return Q


def _gpu_at_estep0(P):
    from fetalreconstruction_amd import engine as E
    rec = E.Reconstruction(0)
    rec.set_flags(disable_bias_correction=False)
    E.sync_gpu(rec, P)
    d = irtkReconstruction(rec, P.ns, max_intensity=P.max_intensity, min_intensity=P.min_intensity)
    d.SetSmoothingParameters(150, 0.02)
    d._disableBiasC = False
    run_to_state(d, "estep0")
    return rec, d


def _finish(rec, sigma):
    assert rec._lib.svr_normalise_bias_finish(rec._h, C.c_float(sigma)) == 0


def test_lds_kernels_are_the_stencils_bit_for_bit_on_p4():
    from fetalreconstruction_amd import engine as E, workloads
    P = _biased(workloads.get("P4"))
    rec, _ = _gpu_at_estep0(P)
    assert rec.get_option("bias_mode") == 1
    sims = rec.debug_get(E.BUF_SIMSLICES).reshape(P.slices.shape)
    sims[:5] = 0.5                                 # residual wr = 0 on whole slices: the wr pass gives 0, the wb pass's value stays
    rec.debug_set(E.BUF_SIMSLICES, sims)
    bias0 = rec.debug_get(E.BUF_BIAS)
    out = {}
    for mode in (1, 0):
        rec.set_option("bias_mode", mode)
        rec.debug_set(E.BUF_BIAS, bias0)
        rec.CorrectBias(12.0, True)                # global: no per-slice mean, so the quirk's +1 shows
        first = rec.debug_get(E.BUF_BIAS)
        rec.CorrectBias(12.0, False)               # a second pass from a non-zero field
        out[mode] = (first, rec.debug_get(E.BUF_BIAS))
    act = (P.slices[:5] != -1) & (out[1][0][:5] != 0)
    assert act.any() and np.allclose(out[1][0][:5][act], 1.0)    # wr / wb = the wb pass's value / itself on the quirk slices
    assert np.array_equal(out[1][0], out[0][0]) and np.array_equal(out[1][1], out[0][1])
    # the NormaliseBias tail on a scattered field, with a voxel of zero weight and a NaN, against k_gauss_conv3d + divS + divexp
    rec.NormaliseBias(0, 12.0)
    bv = rec.debug_get(E.BUF_BIAS_VOLUME)
    rng = np.random.default_rng(1)
    field = (0.2 * rng.standard_normal(bv.shape)).astype(np.float32)
    field[len(field) // 3] = np.nan
    recon = rec.debug_get(E.BUF_RECONSTRUCTED)
    res = {}
    for mode in (2, 0):                            # 2: the LDS tail at every size (bias_mode 1 keeps the stencils below 4.2 M voxels)
        rec.set_option("bias_mode", mode)
        rec.debug_set(E.BUF_BIAS_VOLUME, field)
        rec.debug_set(E.BUF_RECONSTRUCTED, recon)
        _finish(rec, 12.0)
        res[mode] = (rec.debug_get(E.BUF_BIAS_VOLUME), rec.debug_get(E.BUF_RECONSTRUCTED))
    for a, b in zip(res[2], res[0]):
        assert np.array_equal(a, b, equal_nan=True)
    assert rec.get_option("bias_corrections") == 4 and rec.get_option("bias_normalisations") == 3


def test_normalise_bias_scatter_on_the_cell_kernels_repeats_bit_for_bit():
    """The NormaliseBias scatter on the SR scatter's cell kernels: the same bias_vol from two runs and with the coefficient table on
    and off; against round 1's wave-per-pixel kernel with float atomics (bias_mode 0) to float round-off."""
    from fetalreconstruction_amd import engine as E, workloads
    P = _biased(workloads.get("P4"))
    rec, d = _gpu_at_estep0(P)
    d.BiasGPU()
    d.ScaleGPU()
    d.SuperresolutionGPU(1)
    assert rec.get_option("coeff_table") == 1 and rec.get_option("coeff_valid") == 1

    def scatter():
        assert rec._lib.svr_normalise_bias_local(rec._h) == 0
        return rec.debug_get(E.BUF_BIAS_VOLUME)
    table1, table2 = scatter(), scatter()
    assert rec.get_option("bias_scatters_on_cells") == 2
    rec.set_option("coeff_table", 0)
    fly = scatter()
    assert rec.get_option("bias_scatters_on_cells") == 3
    assert np.abs(table1).max() > 0 and np.array_equal(table1, table2) and np.array_equal(table1, fly)
    rec.set_option("bias_mode", 0)
    atomics = scatter()
    assert rec.get_option("bias_scatters_on_cells") == 3 and rel_err(atomics, table1) < 1e-5


def test_bias_steps_against_the_oracle():
    from fetalreconstruction_amd import engine as E, phantom
    from oracle import pyoracle as po
    P = _biased(phantom.make_problem(3, (40, 36, 10), 1.1, 2.2, None, 1.0, 15.0, seed=11, orientations=("ax", "cor", "sag"), name="bias-mid"))
    rec, dg = _gpu_at_estep0(P)
    orc = po.OracleReconstruction(P, po.CANON, bias_correction=True)
    do = irtkReconstruction(orc, P.ns, max_intensity=P.max_intensity, min_intensity=P.min_intensity)
    do.SetSmoothingParameters(150, 0.02)
    do._disableBiasC = False
    run_to_state(do, "estep0")
    for b, a in ((E.BUF_WEIGHTS, orc.weights), (E.BUF_SIMSLICES, orc.simslices), (E.BUF_SIMWEIGHTS, orc.simweights)):
        rec.debug_set(b, a)
    rec.CorrectBias(12.0, False)
    orc.CorrectBias(12.0, False)
    assert rel_err(rec.debug_get(E.BUF_BIAS), orc.bias, floor=1.0) < 2e-5
    # NormaliseBias on identical inputs
    rec.debug_set(E.BUF_BIAS, orc.bias)
    rec.debug_set(E.BUF_WEIGHTS, orc.weights)
    rec.SuperresolutionBackproject(orc.slice_weights)
    orc.SuperresolutionBackproject(orc.slice_weights)
    orc.SuperresolutionUpdate(do._adaptive, do._alpha, do._min_intensity, do._max_intensity, do._delta, do._lambda)
    rec.debug_set(E.BUF_RECONSTRUCTED, orc.recon)
    rec.NormaliseBias(0, 12.0)
    orc.NormaliseBias(0, 12.0)
    assert rel_err(rec.debug_get(E.BUF_BIAS_VOLUME), orc.bias_vol, floor=1.0) < 2e-5
    assert rel_err(rec.syncCPU(), orc.recon) < 2e-5


def test_host_object_sr_iterations_with_bias_track_the_oracle():
    from fetalreconstruction_amd import engine as E, host, phantom
    from oracle import pyoracle as po
    P = _biased(phantom.make_problem(3, (40, 36, 10), 1.1, 2.2, None, 1.0, 15.0, seed=11, orientations=("ax", "cor", "sag"), name="bias-mid"))
    rec = E.Reconstruction(0)
    rec.set_flags(disable_bias_correction=False)
    E.sync_gpu(rec, P)
    orc = po.OracleReconstruction(P, po.CANON, bias_correction=True)
    kw = dict(max_intensity=P.max_intensity, min_intensity=P.min_intensity)
    hc = host.irtkReconstruction(rec, P.ns, **kw)
    hc.set_bias_correction(True, 12.0)
    hc.set_bias_options(False, 0.01)
    do = irtkReconstruction(orc, P.ns, **kw)
    do._disableBiasC = False
    for d in (hc, do):
        d.SetSmoothingParameters(150, 0.02)
        d.reconstruct_iteration(2)
    st = hc.state()
    assert np.allclose(st["scale"], do._scale_gpu, rtol=2e-4)
    assert rel_err(rec.debug_get(E.BUF_BIAS), orc.bias, floor=1.0) < 2e-4
    assert rel_err(rec.syncCPU(), orc.recon) < 2e-4
    assert rec.get_option("bias_corrections") == 2 and rec.get_option("bias_normalisations") == 2


def test_coefficient_table_stays_on_with_bias_at_p4():
    from fetalreconstruction_amd import engine as E, host, workloads
    P = _biased(workloads.get("P4"))
    rec = E.Reconstruction(0)
    rec.set_flags(disable_bias_correction=False)
    E.sync_gpu(rec, P)
    hc = host.irtkReconstruction(rec, P.ns, max_intensity=P.max_intensity, min_intensity=P.min_intensity)
    hc.set_bias_correction(True, 12.0)
    hc.SetSmoothingParameters(150, 0.02)
    hc.reconstruct_iteration(1)
    assert rec.get_option("coeff_table") == 1 and rec.get_option("bias_normalisations") == 1
    assert np.isfinite(rec.syncCPU()).all() and np.isfinite(rec.debug_get(E.BUF_BIAS)).all()


def _write_biased_case(tmp_path):
    from fetalreconstruction_amd import nifti, phantom
    stacks, mask, mattr, rattr, rmask = phantom.make_stacks(3, (40, 40, 12), 1.1, 2.2, None, 1.0, 16.0, seed=2,
                                                            stack_motion_mm=0.0, stack_motion_deg=0.0)
    paths = []
    for k, st in enumerate(stacks):
        nz, ny, nx = st.data.shape
        yy, xx = np.meshgrid(np.linspace(-1, 1, ny), np.linspace(-1, 1, nx), indexing="ij")
        field = np.exp(0.3 * xx - 0.2 * yy)[None] * (1 + 0.05 * np.sin(np.arange(nz) + k)[:, None, None])
        p = tmp_path / f"stack{k}.nii.gz"
        nifti.write(p, st.data * field, st.attr)
        paths.append(str(p))
    nifti.write(tmp_path / "mask.nii.gz", rmask, rattr)
    return paths, str(tmp_path / "mask.nii.gz")


def _correlation(path, radius):
    from fetalreconstruction_amd import geometry as geo, nifti, phantom
    vol, va = nifti.read(path)
    kk, jj, ii = np.meshgrid(np.arange(va.nz), np.arange(va.ny), np.arange(va.nx), indexing="ij")
    w = np.stack([ii, jj, kk, np.ones_like(ii)], -1).astype(float) @ geo.image_to_world(va).T
    truth = phantom.phantom_intensity(w[..., :3], radius)
    inside = (np.sum(w[..., :3] ** 2, -1) < (radius - 3.0) ** 2) & (vol > 0)
    return vol, float(np.corrcoef(vol[inside], truth[inside])[0, 1])


def test_command_line_with_bias_correction(tmp_path):
    import os
    from fetalreconstruction_amd import build
    build.build()
    paths, mpath = _write_biased_case(tmp_path)
    common = ["-i", *paths, "-m", mpath, "--thickness", "2.2", "2.2", "2.2", "--resolution", "1.0", "--no_registration",
              "--iterations", "2", "--rec_iterations_first", "3", "--rec_iterations_last", "4", "--smooth_mask", "0"]
    env = dict(os.environ, SVR_CLI_TIMING="1")
    run = lambda out, *extra: subprocess.run([build.CLI, "-o", str(tmp_path / out), *common, *extra], capture_output=True, text=True,
                                             timeout=240, env=env)
    off = run("off.nii.gz")
    assert off.returncode == 0, off.stderr
    assert "bias correction:" not in off.stderr
    on = run("on.nii.gz", "--enableBiasCorrection", "--sigma", "12")
    assert on.returncode == 0, on.stderr
    assert "[timing] bias correction: 7 CorrectBias, 7 NormaliseBias" in on.stderr, on.stderr
    two = run("two.nii.gz", "--enableBiasCorrection", "--sigma", "12", "-d", "0", "0")          # two ranks, one device (test mode)
    assert two.returncode == 0, two.stderr
    glob = run("glob.nii.gz", "--enableBiasCorrection", "--global_bias_correction", "1")
    assert glob.returncode == 0 and "[timing] bias correction: 7 CorrectBias, 0 NormaliseBias" in glob.stderr, glob.stderr
    assert "not implemented" in glob.stdout
    v_off, c_off = _correlation(tmp_path / "off.nii.gz", 16.0)
    v_on, c_on = _correlation(tmp_path / "on.nii.gz", 16.0)
    v_two, _ = _correlation(tmp_path / "two.nii.gz", 16.0)
    print(f"correlation with the unbiased phantom: bias off {c_off:.4f}, bias on {c_on:.4f}")
    assert not np.array_equal(v_off, v_on) and c_on > c_off     # (recorded: 0.7869 -> 0.7908)
    assert np.abs(v_two - v_on).max() <= 2e-4 * np.abs(v_on).max()                             # sharded NormaliseBias = one rank
