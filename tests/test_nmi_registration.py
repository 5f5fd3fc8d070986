"""Normalised mutual information in the IRTK registration schedule (the reference's --useNMI; csrc/irtk_reg.cpp with SVRH_SIM_NMI,
csrc/svr_nmi.inc on the device).  No GPU here: the binning of irtkCalculateNumberOfBins, the entropy sums of irtkHistogram_2D restated
serially in Python (math.log is the C library's log) against the schedule's, the C++ schedule over a numpy joint-histogram evaluator,
the contrast case NMI exists for, and the command line."""
import math
import subprocess

import numpy as np
import pytest

from fetalreconstruction_amd import build, geometry as geo, host, nifti, phantom


# ---- restatements -------------------------------------------------------------------------------------------------------------
def number_of_bins(mn, mx, maxbin=64):
    """irtkCalculateNumberOfBins (irtkUtil.cc:438-474) -> (nbins, width)"""
    rng, width = mx - mn + 1, 1
    while int(math.ceil(rng / float(width))) > maxbin:
        width += 1
    return int(math.ceil(rng / float(width))), width


def entropy_sums(h, nbt, nbs):
    """irtkHistogram_2D::JointEntropy / EntropyX / EntropyY (H2D.cc:443-523): the sums of c log c, serially in the reference's order
    (_bins[source][target], source-major) -> ((n, S_xy, S_x, S_y), NMI)"""
    h = np.asarray(h)
    term = lambda c: float(c) * math.log(float(c))
    n = int(h[:nbs, :nbt].sum())
    sxy = sx = sy = 0.0
    for j in range(nbs):
        for i in range(nbt):
            if h[j, i] > 0:
                sxy += term(int(h[j, i]))
    for i in range(nbt):
        m = int(h[:nbs, i].sum())
        if m > 0:
            sx += term(m)
    for j in range(nbs):
        m = int(h[j, :nbt].sum())
        if m > 0:
            sy += term(m)
    if n == 0:
        return (0.0, sxy, sx, sy), 0.0
    ex, ey, exy = -sx / n + math.log(n), -sy / n + math.log(n), -sxy / n + math.log(n)
    return (float(n), sxy, sx, sy), (ex + ey) / exy


def joint_histogram(planes, mats, source, width, nbt, nbs):
    """irtkImageRigidRegistrationWithPadding::Evaluate (IRRWP.cc:534-610) with the NMI metric, one histogram over all planes: the
    sampling of k_ncc (double trilinear in EvaluateInside's order, round(), value >= 0); target bin v // width, source already binned"""
    src = np.asarray(source).astype(np.float64)
    vz, vy, vx = src.shape
    h = np.zeros((64, 64), np.uint32)
    for t, M in zip(planes, mats):
        jj, ii = np.nonzero(np.asarray(t) >= 0)
        tv = np.asarray(t)[jj, ii].astype(np.int64)
        i, j = ii.astype(np.float64), jj.astype(np.float64)
        X = M[0, 0] * i + M[0, 1] * j + M[0, 3]
        Y = M[1, 0] * i + M[1, 1] * j + M[1, 3]
        Z = M[2, 0] * i + M[2, 1] * j + M[2, 3]
        ok = (X > 0) & (X < vx - 1) & (Y > 0) & (Y < vy - 1) & (Z > 0) & (Z < vz - 1)
        X, Y, Z, tv = X[ok], Y[ok], Z[ok], tv[ok]
        a, b, c = X.astype(np.int64), Y.astype(np.int64), Z.astype(np.int64)
        t1, u1, v1 = X - a, Y - b, Z - c
        t2, u2, v2 = 1 - t1, 1 - u1, 1 - v1

        def q(dz, dy, dx):
            return src[c + dz, b + dy, a + dx]
        value = (t1 * (u2 * (v2 * q(0, 0, 1) + v1 * q(1, 0, 1)) + u1 * (v2 * q(0, 1, 1) + v1 * q(1, 1, 1))) +
                 t2 * (u2 * (v2 * q(0, 0, 0) + v1 * q(1, 0, 0)) + u1 * (v2 * q(0, 1, 0) + v1 * q(1, 1, 0))))
        keep = value >= 0
        sb, tb = (value[keep] + 0.5).astype(np.int64), tv[keep] // width
        assert (sb < nbs).all() and (tb < nbt).all(), "a sample outside the bins"
        np.add.at(h, (sb, tb), 1)
    return h


def _max_error_mm(a, b, radius=12.0, n=200, seed=0):
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(n, 3))
    p = p / np.linalg.norm(p, axis=1, keepdims=True) * rng.uniform(0, radius, (n, 1))
    p = np.concatenate([p, np.ones((n, 1))], 1)
    return float(np.linalg.norm((p @ np.asarray(a).T - p @ np.asarray(b).T)[:, :3], axis=1).max())


# ---- binning and entropies ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rng_", [1, 64, 65, 128, 129, 32767])
def test_bin_widths_follow_irtk_calculate_number_of_bins(rng_):
    mn = 37
    mx = mn + rng_ - 1
    want_nb, want_w = number_of_bins(mn, mx)
    data = np.concatenate([np.arange(-1, rng_, dtype=np.int64), [0, -1, rng_ - 1]]).astype(np.int16)   # the shifted level: -1 padding, 0 .. range-1
    nb, w, binned = host.irtk_number_of_bins(mn, mx, data)
    assert (nb, w) == (want_nb, want_w)
    assert nb <= 64 and (binned[data > 0] == data[data > 0] // w).all()
    assert (binned[data <= 0] == data[data <= 0]).all()                                  # zeros and padding stay
    assert binned.max() < nb
    assert {1: (1, 1), 64: (64, 1), 65: (33, 2), 128: (64, 2), 129: (43, 3), 32767: (64, 512)}[rng_] == (nb, w)


def test_no_voxel_above_the_padding_gives_one_bin():
    assert host.irtk_number_of_bins(32767, -32768)[:2] == (1, 1)


def test_entropy_sums_are_the_serial_restatement_bit_for_bit():
    rng = np.random.default_rng(7)
    for k in range(60):
        nbt, nbs = int(rng.integers(1, 65)), int(rng.integers(1, 65))
        h = np.zeros((64, 64), np.uint32)
        dense = rng.random() < 0.5
        vals = rng.integers(0, 5000 if dense else 3, (nbs, nbt)) * (rng.random((nbs, nbt)) < (0.9 if dense else 0.2))
        h[:nbs, :nbt] = vals
        s, v = host.nmi_sums(h, nbt, nbs)
        ws, wv = entropy_sums(h, nbt, nbs)
        assert tuple(s) == ws and (v == wv or (math.isnan(v) and math.isnan(wv))), (k, s, ws, v, wv)
    s, v = host.nmi_sums(np.zeros((64, 64), np.uint32), 5, 5)
    assert v == 0.0 and s[0] == 0


# ---- the schedule over the numpy evaluator --------------------------------------------------------------------------------------------
def _numpy_backend(keep=True):
    return host.NmiBackend(joint_histogram, keep=keep)


def _slice_case(tiny, oracle_mod, sel=(4, 9, 12, 20), mm=1.5, deg=2.5, seed=2, knock=(0, 2)):
    o = oracle_mod.OracleReconstruction(tiny, oracle_mod.CANON)
    o.InitializeEMValues()
    o.GaussianReconstruction()
    vol = o.recon.reshape(tiny.vsize[::-1]).astype(np.float32)
    vol = np.where(tiny.mask.reshape(vol.shape) > 0, vol, -1).astype(np.float32)
    rattr = geo.ImageAttributes(*tiny.vsize, *tiny.vdim)
    sel = list(sel)
    T = np.stack([tiny.slice_t[k].reshape(4, 4).astype(np.float64) for k in sel])
    rng = np.random.default_rng(seed)
    P = T.copy()
    for k in knock:
        P[k] = geo.rigid_matrix(*rng.uniform(-mm, mm, 3), *rng.uniform(-deg, deg, 3)) @ T[k]
    return vol, rattr, sel, T, P


def test_schedule_over_the_numpy_evaluator_sees_the_restated_values(tiny, oracle_mod):
    vol, rattr, sel, T, P = _slice_case(tiny, oracle_mod)
    be = _numpy_backend()
    args = (tiny.slices[sel], [tiny.slice_attr[k] for k in sel], P, rattr, vol)
    out, nev = host.SliceToVolumeRegistration(None, *args, backend=be, similarity="nmi")
    assert nev > 100 and len(be.log) == nev and be.calls < nev / 3 and not np.array_equal(out, P)
    # every histogram the schedule turned into a similarity: its sums and NMI are the serial restatement's, bit for bit
    for h, nbt, nbs in be.log[::7]:
        s, v = host.nmi_sums(h, nbt, nbs)
        ws, wv = entropy_sums(h, nbt, nbs)
        assert tuple(s) == ws and v == wv
    assert max(nbs for _, _, nbs in be.log) > 8 and max(nbt for _, nbt, _ in be.log) > 8
    # (no accuracy asserted here: 32 x 32 slices are 8 x 8 at the coarsest level, too few samples for a 64-bin metric, which then
    # prefers less overlap -- NMI's known small-sample bias, the reference's too; the accuracy case is the contrast test below)
    out2, nev2 = host.SliceToVolumeRegistration(None, *args, backend=_numpy_backend(False), similarity="nmi")
    assert np.array_equal(out, out2) and nev == nev2                                  # deterministic
    cc, _ = host.SliceToVolumeRegistration(None, *args, backend=host.NccBackend(lambda t, M, s: oracle_mod.ncc_evaluate(t, M, s)[1]))
    assert not np.array_equal(cc, out)                                                # a different metric


def _package_case():
    R = 13.0
    a = geo.ImageAttributes(30, 30, 10, 1.1, 1.1, 2.2)
    t_pack = [geo.rigid_matrix(1.0, -0.8, 0.5, 1.5, -2.0, 1.0), geo.rigid_matrix(-0.9, 0.8, -0.6, -1.0, 1.5, -2.0)]
    kk, jj, ii = np.meshgrid(np.arange(a.nz), np.arange(a.ny), np.arange(a.nx), indexing="ij")
    pix = np.stack([ii, jj, kk, np.ones_like(ii)], -1).astype(np.float64)
    data = np.zeros((a.nz, a.ny, a.nx))
    for k in range(a.nz):
        w = (pix[k] @ geo.image_to_world(a).T) @ t_pack[k % 2].T
        data[k] = phantom.phantom_intensity(w[..., :3], R) * 700 / 0.55
    ra = geo.ImageAttributes(30, 30, 30, 1.0, 1.0, 1.0)
    kk, jj, ii = np.meshgrid(np.arange(30), np.arange(30), np.arange(30), indexing="ij")
    w = np.stack([ii, jj, kk, np.ones_like(ii)], -1).astype(np.float64) @ geo.image_to_world(ra).T
    vol = (phantom.phantom_intensity(w[..., :3], R) * 700 / 0.55).astype(np.float32)
    return a, data, t_pack, ra, vol


def test_package_to_volume_runs_the_schedule_with_nmi():
    a, data, t_pack, ra, vol = _package_case()
    start = np.tile(np.eye(4), (a.nz, 1, 1))
    be = _numpy_backend()
    t, nev = host.PackageToVolume(None, [data], [a], [2], start, ra, vol, backend=be, similarity="nmi")
    err = [_max_error_mm(t[k], t_pack[k % 2], 10.0) for k in range(a.nz)]
    before = [_max_error_mm(np.eye(4), t_pack[k % 2], 10.0) for k in range(a.nz)]
    print("NMI package registration: error before", np.round(before[:2], 2), "after", np.round(err[:2], 2), "evaluations", nev)
    assert nev > 50 and be.calls < nev and max(err) < 0.6 * min(before)
    for k in range(2, a.nz):
        assert np.allclose(t[k], t[k % 2], atol=1e-12)
    for h, nbt, nbs in be.log[::11]:
        assert tuple(host.nmi_sums(h, nbt, nbs)[0]) == entropy_sums(h, nbt, nbs)[0]


def test_similarity_is_checked():
    with pytest.raises(ValueError):
        host.SliceToVolumeRegistration(None, np.zeros((1, 2, 2), np.float32), [geo.ImageAttributes(2, 2, 1, 1, 1, 1)], np.eye(4)[None],
                                       geo.ImageAttributes(2, 2, 2, 1, 1, 1), np.zeros((2, 2, 2), np.float32), similarity="mi")
    with pytest.raises(ValueError):           # an NCC evaluator for an NMI registration
        host.SliceToVolumeRegistration(None, np.zeros((1, 2, 2), np.float32), [geo.ImageAttributes(2, 2, 1, 1, 1, 1)], np.eye(4)[None],
                                       geo.ImageAttributes(2, 2, 2, 1, 1, 1), np.zeros((2, 2, 2), np.float32),
                                       backend=host.NccBackend(lambda t, M, s: np.zeros(6)), similarity="nmi")


# ---- the case NMI exists for: a non-monotonic intensity relation ------------------------------------------------------------------
def remap_contrast(slices):
    """v -> |v - median of the foreground| rescaled to the old maximum, on the pixels that are not padding: a non-monotonic map, the
    contrast of another weighting"""
    s = np.asarray(slices, np.float32).copy()
    m = s >= 0
    med = float(np.median(s[m & (s > s[m].min())]))                                   # the median of the foreground
    d = np.abs(s[m] - med)
    s[m] = d * (float(s[m].max()) / float(d.max()))
    return s


def _analytic_slice_case(seed=11, mm=3.0, deg=4.0):
    """six axial 48 x 48 slices through the analytic phantom (R = 24 mm) on a 60^3 volume of 1 mm voxels (background 100, a little noise
    in the volume so that no corner padding is guessed), each started from a random rigid misalignment; the truth is the identity"""
    R, n = 24.0, 60
    ra = geo.ImageAttributes(n, n, n, 1.0, 1.0, 1.0)
    kk, jj, ii = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    w = np.stack([ii, jj, kk, np.ones_like(ii)], -1).astype(np.float64) @ geo.image_to_world(ra).T
    rng = np.random.default_rng(0)
    vol = (phantom.phantom_intensity(w[..., :3], R) * 700 / 0.55 + 100 + rng.normal(0, 5, w.shape[:-1])).astype(np.float32)
    attrs, slices = [], []
    for z in (-9.0, -5.0, -1.0, 3.0, 7.0, 10.0):
        a = geo.ImageAttributes(48, 48, 1, 1.0, 1.0, 1.0, origin=(0.3, -0.2, z))
        jj, ii = np.meshgrid(np.arange(48), np.arange(48), indexing="ij")
        pw = np.stack([ii, jj, np.zeros_like(ii), np.ones_like(ii)], -1).astype(np.float64) @ geo.image_to_world(a).T
        slices.append(phantom.phantom_intensity(pw[..., :3], R) * 700 / 0.55 + 100)
        attrs.append(a)
    rng = np.random.default_rng(seed)
    P = np.stack([geo.rigid_matrix(*rng.uniform(-mm, mm, 3), *rng.uniform(-deg, deg, 3)) for _ in attrs])
    return np.stack(slices).astype(np.float32), attrs, P, ra, vol


def test_nmi_registers_slices_of_another_contrast_where_cc_does_not(oracle_mod):
    slices, attrs, P, ra, vol = _analytic_slice_case()
    args = (remap_contrast(slices), attrs, P, ra, vol)
    nmi, _ = host.SliceToVolumeRegistration(None, *args, backend=_numpy_backend(False), similarity="nmi")
    cc, _ = host.SliceToVolumeRegistration(None, *args, backend=host.NccBackend(lambda t, M, s: oracle_mod.ncc_evaluate(t, M, s)[1]))
    before = np.array([_max_error_mm(p, np.eye(4)) for p in P])
    e_nmi = np.array([_max_error_mm(m, np.eye(4)) for m in nmi])
    e_cc = np.array([_max_error_mm(m, np.eye(4)) for m in cc])
    print("contrast-remapped slices: error before", np.round(before, 2), "NMI", np.round(e_nmi, 2), "CC", np.round(e_cc, 2))
    # NMI brings most slices back (median under 1.5 mm, four of six under 2 mm); CC, which assumes a linear relation, loses them all
    assert np.median(e_nmi) < 1.5 and (e_nmi < 2.0).sum() >= 4 and np.median(e_nmi) < 0.6 * np.median(before)
    assert e_cc.min() > 10.0 and np.median(e_cc) > 10 * np.median(e_nmi)
    # the same slices with their own contrast: both metrics register them
    same = (slices, attrs, P, ra, vol)
    nmi2, _ = host.SliceToVolumeRegistration(None, *same, backend=_numpy_backend(False), similarity="nmi")
    cc2, _ = host.SliceToVolumeRegistration(None, *same, backend=host.NccBackend(lambda t, M, s: oracle_mod.ncc_evaluate(t, M, s)[1]))
    assert max(_max_error_mm(m, np.eye(4)) for m in nmi2) < 1.6 and max(_max_error_mm(m, np.eye(4)) for m in cc2) < 1.6


# ---- the command line -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli_case(tmp_path_factory):
    build.build()
    d = tmp_path_factory.mktemp("nmi_cli")
    stacks, mask, mattr, rattr, rmask = phantom.make_stacks(2, (24, 24, 6), 1.1, 2.2, None, 1.0, 10.0, seed=4,
                                                            stack_motion_mm=0.0, stack_motion_deg=0.0)
    paths = []
    for k, st in enumerate(stacks):
        p = d / f"stack{k}.nii.gz"
        nifti.write(p, st.data, st.attr)
        paths.append(str(p))
    nifti.write(d / "mask.nii.gz", rmask, rattr)
    return d, ["-i", *paths, "-m", str(d / "mask.nii.gz"), "--resolution", "1.0"]


def _run(args):
    return subprocess.run([build.CLI, *args], capture_output=True, text=True, timeout=120)


def test_help_lists_use_nmi_as_a_deviation():
    r = _run(["--help"])
    assert r.returncode == 0 and "--useNMI" in r.stdout and "never takes effect" in r.stdout


def test_use_nmi_does_not_change_the_problem(cli_case):
    d, common = cli_case
    a, b = d / "plain.bin", d / "nmi.bin"
    assert _run(["-o", str(d / "x.nii.gz"), *common, "--no_registration", "--dumpProblem", str(a), "--dryRun"]).returncode == 0
    r = _run(["-o", str(d / "x.nii.gz"), *common, "--no_registration", "--useNMI", "--dumpProblem", str(b), "--dryRun"])
    assert r.returncode == 0, r.stderr
    assert a.read_bytes() == b.read_bytes()


def test_use_nmi_with_gpu_registration_is_refused(cli_case):
    d, common = cli_case
    r = _run(["-o", str(d / "x.nii.gz"), *common, "--useNMI", "--useGPUReg"])
    assert r.returncode != 0 and "--useGPUReg" in r.stderr and "cross-correlation only" in r.stderr
