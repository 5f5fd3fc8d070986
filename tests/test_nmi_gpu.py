"""The engine's NMI (csrc/svr_nmi.inc) against the numpy restatement of tests/test_nmi_registration.py: joint histograms equal and the
four sums {n, S_xy, S_x, S_y} and the NMI bit for bit, on random geometry at the sizes of the three levels with 1-plane and multi-plane
evaluations (split over workgroups and merged in global memory); the same optimiser trajectory from the engine and from the numpy
evaluator; the command line end to end on P4 with one stack of another contrast."""
import subprocess
import tempfile
import pathlib

import numpy as np
import pytest

from fetalreconstruction_amd import build, geometry as geo, host, nifti, phantom
from tests.test_nmi_registration import (_analytic_slice_case, _numpy_backend, _package_case, _slice_case, entropy_sums, joint_histogram,
                                         number_of_bins, remap_contrast)


def _plane_matrices(rng, tsize, ssize, nz):
    """per-plane source-from-target matrices of one evaluation: a random rotation and scale around the centres, plane k one NextZ on"""
    ang = rng.uniform(-25, 25, 3)
    R = geo.rigid_matrix(0, 0, 0, *ang)[:3, :3] @ np.diag(rng.uniform(0.6, 1.4, 3))
    ct, cs = (np.array(tsize, float) - 1) / 2, (np.array(ssize, float) - 1) / 2
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = cs - R @ ct + rng.uniform(-3, 3, 3)
    out = []
    for k in range(nz):
        q = M.copy()
        q[:3, 3] = M[:3, 3] + k * M[:3, 2]
        out.append(q)
    return np.stack(out)


@pytest.mark.gpu
def test_device_histograms_and_sums_are_the_restatement():
    from fetalreconstruction_amd import engine as E
    rec = E.Reconstruction(0)
    rng = np.random.default_rng(3)
    # (target grid, planes of the evaluations, source grid): the sizes of a P4 slice's three levels, 3-D targets of one workgroup
    # and of several (64 x 64 planes: 4 per workgroup, so 12 planes = 3 workgroups merged in global memory)
    cases = [((100, 93), [1, 1, 1, 1], (60, 64, 58)), ((50, 47), [1, 3, 1, 7], (30, 32, 29)), ((25, 24), [1, 1, 9, 2], (15, 16, 15)),
             ((64, 64), [12, 1, 5, 4, 13], (40, 44, 38))]
    for (tx, ty), ppe, (sx, sy, sz) in cases:
        for rng_s, rng_t in ((3000, 200), (40, 5000), (700, 64)):
            src = rng.integers(-1, rng_s, (sz, sy, sx)).astype(np.int16)
            src[:, :, :2] = -1
            nbs, ws = number_of_bins(0, rng_s - 1)
            n_planes = int(sum(ppe))
            tg = rng.integers(-1, rng_t, (n_planes, ty, tx)).astype(np.int16)
            tg[:, :3] = -1
            if len(ppe) > 3:
                tg[int(np.cumsum(ppe)[2]):int(np.cumsum(ppe)[3])] = -1                    # an evaluation without a sample
            nbt, wt = number_of_bins(0, rng_t - 1)
            rec.ncc_set_targets(tg)
            rec.ncc_set_source(src)
            rec.nmi_bin_source(ws)
            src_b = np.where(src > 0, src // ws, src).astype(np.int16)
            idx = np.arange(n_planes)
            mats = np.concatenate([_plane_matrices(rng, (tx, ty, k), (sx, sy, sz), k) for k in ppe])
            widths, nbts = np.full(len(ppe), wt), np.full(len(ppe), nbt)
            out, hist = rec.nmi_evaluate(ppe, idx, mats, widths, nbts, nbs, histograms=True)
            at = 0
            for e, k in enumerate(ppe):
                h = joint_histogram(tg[at:at + k], mats[at:at + k], src_b, wt, nbt, nbs)
                assert np.array_equal(hist[e], h), (tx, e)
                s, v = entropy_sums(h, nbt, nbs)
                assert tuple(out[e]) == s, (tx, e, out[e], s)
                assert host.nmi_sums(hist[e], nbt, nbs)[1] == v or np.isnan(v)
                at += k
            assert out[:, 0].max() > 1000 and (out[:, 0] == 0).any() == (len(ppe) > 3)
            # again, without the histograms and in another order: the merge slots were left zero
            perm = rng.permutation(len(ppe))
            starts = np.concatenate([[0], np.cumsum(ppe)[:-1]])
            idx2 = np.concatenate([np.arange(starts[e], starts[e] + ppe[e]) for e in perm])
            out2, _ = rec.nmi_evaluate(np.array(ppe)[perm], idx2, mats[idx2], widths[perm], nbts[perm], nbs)
            assert np.array_equal(out2, out[perm])
    with pytest.raises(E.SvrError):                                                       # bins that do not fit the images
        rec.nmi_evaluate([1], [0], _plane_matrices(rng, (64, 64, 1), (40, 44, 38), 1), [1], [2], 64)


def _moved(a, G):
    import copy
    r = copy.copy(a)
    r.xaxis, r.yaxis, r.zaxis = G[:3, :3] @ np.asarray(a.xaxis, float), G[:3, :3] @ np.asarray(a.yaxis, float), G[:3, :3] @ np.asarray(a.zaxis, float)
    r.origin = (G @ np.array([*np.asarray(a.origin, float), 1.0]))[:3]
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("frame", ["phantom", "bundled mask"])
def test_engine_and_numpy_evaluators_give_the_same_nmi_trajectory(tiny, oracle_mod, frame):
    """the decisions of the optimiser coincide between the device and the numpy NMI, also in the oblique frame of the reference's
    bundled mask 475 mm from the world origin (tests/real_mask.py)"""
    from fetalreconstruction_amd import engine as E
    rec = E.Reconstruction(0)
    vol, rattr, sel, T, P = _slice_case(tiny, oracle_mod)
    sattr = [tiny.slice_attr[k] for k in sel]
    slices, aattr, AP, ara, avol = _analytic_slice_case()
    aslices = remap_contrast(slices)
    if frame != "phantom":
        import real_mask as rm
        m, a, _ = rm.load()
        G = np.eye(4)
        G[:3, 0], G[:3, 1], G[:3, 2] = a.xaxis, a.yaxis, a.zaxis
        G[:3, 3] = rm.centre(m, a)
        Gi = np.linalg.inv(G)
        sattr, rattr, P = [_moved(x, G) for x in sattr], _moved(rattr, G), np.stack([G @ p @ Gi for p in P])
        aattr, ara, AP = [_moved(x, G) for x in aattr], _moved(ara, G), np.stack([G @ p @ Gi for p in AP])
    for args in ((tiny.slices[sel], sattr, P, rattr, vol), (aslices, aattr, AP, ara, avol)):
        dev, nev_d = host.SliceToVolumeRegistration(rec, *args, similarity="nmi")
        cpu, nev_c = host.SliceToVolumeRegistration(None, *args, backend=_numpy_backend(False), similarity="nmi")
        assert nev_d == nev_c and nev_d > 100 and np.array_equal(dev, cpu)
        assert not np.array_equal(dev, args[2])
    if frame != "phantom":
        return
    a, data, t_pack, ra, pvol = _package_case()
    start = np.tile(np.eye(4), (a.nz, 1, 1))
    for evenodd in (False, True):
        dev, nev_d = host.PackageToVolume(rec, [data], [a], [2], start, ra, pvol, evenodd=evenodd, similarity="nmi")
        cpu, nev_c = host.PackageToVolume(None, [data], [a], [2], start, ra, pvol, evenodd=evenodd, backend=_numpy_backend(False),
                                          similarity="nmi")
        assert nev_d == nev_c and nev_d > 50 and np.array_equal(dev, cpu)


def p4_cli_case(tmp):
    """the P4 stacks of tools/run_cli_p4.py written as NIfTI, stack 1 through a non-monotonic intensity map"""
    R = 50.0
    stacks, mask, mattr, rattr, rmask = phantom.make_stacks(4, (100, 93, 70), 1.17647, 1.25, 2.5, 1.0, R, seed=1,
                                                            orientations=("ax", "cor", "sag", "ax"), stack_motion_mm=2.0, stack_motion_deg=3.0)
    paths = []
    for k, st in enumerate(stacks):
        data = remap_contrast(st.data) if k == 1 else st.data
        nifti.write(tmp / f"s{k}.nii.gz", data, st.attr)
        paths.append(str(tmp / f"s{k}.nii.gz"))
    nifti.write(tmp / "mask.nii.gz", rmask, rattr)
    return stacks, R, ["-i", *paths, "-m", str(tmp / "mask.nii.gz"), "--resolution", "1.0"]


def phantom_correlation(path, stacks, R):
    vol, va = nifti.read(path)
    kk, jj, ii = np.meshgrid(np.arange(va.nz), np.arange(va.ny), np.arange(va.nx), indexing="ij")
    w = np.stack([ii, jj, kk, np.ones_like(ii)], -1).astype(float) @ (stacks[0].transformation @ geo.image_to_world(va)).T
    inside = (np.sum(w[..., :3] ** 2, -1) < (R - 6) ** 2) & (vol > 0)
    return float(np.corrcoef(vol[inside], phantom.phantom_intensity(w[..., :3], R)[inside])[0, 1])


@pytest.mark.gpu
def test_command_line_use_nmi_on_p4_with_a_stack_of_another_contrast():
    tmp = pathlib.Path(tempfile.mkdtemp())
    stacks, R, common = p4_cli_case(tmp)
    corr = {}
    for name, extra in (("cc", []), ("nmi", ["--useNMI"]), ("nmi2", ["--useNMI"])):
        r = subprocess.run([build.CLI, "-o", str(tmp / f"{name}.nii.gz"), *common, *extra], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        corr[name] = phantom_correlation(tmp / f"{name}.nii.gz", stacks, R)
    print("correlation with the phantom:", {k: round(v, 4) for k, v in corr.items()})
    assert (tmp / "nmi.nii.gz").read_bytes() == (tmp / "nmi2.nii.gz").read_bytes()
    assert corr["nmi"] >= corr["cc"]
