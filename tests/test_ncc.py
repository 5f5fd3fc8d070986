"""Slice-to-volume NCC cost: the oracle's literal restatement of
irtkImageRigidRegistrationWithPadding::Evaluate against an independent numpy evaluation (CPU),
and the HIP kernel against the oracle (GPU; the six integer moments must be identical)."""
import numpy as np
import pytest

from fetalreconstruction_amd import geometry as geo
from fetalreconstruction_amd import host


def _case(tiny, oracle_mod, n_eval=24, seed=0):
    o = oracle_mod.OracleReconstruction(tiny, oracle_mod.CANON)
    o.GaussianReconstruction()
    vol = o.recon.reshape(tiny.vsize[::-1])
    source = vol.astype(np.int16)                         # static_cast<short>
    targets = np.where(tiny.slices >= 0, tiny.slices, -1).astype(np.int16)
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, tiny.ns, n_eval).astype(np.int32)
    mats = np.zeros((n_eval, 4, 4))
    w2i = tiny.recon_w2i.reshape(4, 4).astype(np.float64)
    for e, k in enumerate(idx):
        t = tiny.slice_t[k].reshape(4, 4).astype(np.float64)
        pert = geo.rigid_matrix(*rng.uniform(-3, 3, 3), *rng.uniform(-4, 4, 3))
        mats[e] = w2i @ (pert @ t) @ tiny.slice_i2w[k].reshape(4, 4).astype(np.float64)
    return source, targets, idx, mats


def _numpy_ncc(target, M, source):
    """Independent evaluation: direct positions M @ (i, j, 0, 1), vectorised trilinear, IRTK round."""
    ty, tx = target.shape
    vz, vy, vx = source.shape
    jj, ii = np.meshgrid(np.arange(ty), np.arange(tx), indexing="ij")
    X = M[0, 0] * ii + M[0, 1] * jj + M[0, 3]
    Y = M[1, 0] * ii + M[1, 1] * jj + M[1, 3]
    Z = M[2, 0] * ii + M[2, 1] * jj + M[2, 3]
    ok = (target >= 0) & (X > 0) & (X < vx - 1) & (Y > 0) & (Y < vy - 1) & (Z > 0) & (Z < vz - 1)
    a, b, c = X[ok].astype(int), Y[ok].astype(int), Z[ok].astype(int)
    t1, u1, v1 = X[ok] - a, Y[ok] - b, Z[ok] - c
    t2, u2, v2 = 1 - t1, 1 - u1, 1 - v1
    s = source.astype(np.float64)
    val = (t1 * (u2 * (v2 * s[c, b, a + 1] + v1 * s[c + 1, b, a + 1]) + u1 * (v2 * s[c, b + 1, a + 1] + v1 * s[c + 1, b + 1, a + 1])) +
           t2 * (u2 * (v2 * s[c, b, a] + v1 * s[c + 1, b, a]) + u1 * (v2 * s[c, b + 1, a] + v1 * s[c + 1, b + 1, a])))
    keep = val >= 0
    sv = np.where(val > 0, (val + 0.5).astype(np.int64), (val - 0.5).astype(np.int64))[keep]
    tv = target[ok][keep].astype(np.int64)
    return np.array([len(tv), tv.sum(), sv.sum(), (tv * tv).sum(), (sv * sv).sum(), (tv * sv).sum()], np.int64)


def test_oracle_ncc_matches_independent_numpy(tiny, oracle_mod):
    source, targets, idx, mats = _case(tiny, oracle_mod)
    nonzero = 0
    for k, M in zip(idx, mats):
        v, sums = oracle_mod.ncc_evaluate(targets[k], M, source)
        ref = _numpy_ncc(targets[k], M, source)
        assert np.array_equal(sums.astype(np.int64), ref)
        if ref[0] > 0:
            nonzero += 1
            n, x, y, x2, y2, xy = ref.astype(np.float64)
            assert v == pytest.approx((xy - x * y / n) / (np.sqrt(x2 - x * x / n) * np.sqrt(y2 - y * y / n)), rel=1e-12)
    assert nonzero >= len(idx) // 2


def test_oracle_ncc_prefers_the_true_alignment(tiny, oracle_mod):
    source, targets, _, _ = _case(tiny, oracle_mod)
    k = int(np.argmax((targets >= 0).reshape(tiny.ns, -1).sum(1)))
    w2i = tiny.recon_w2i.reshape(4, 4).astype(np.float64)
    i2w = tiny.slice_i2w[k].reshape(4, 4).astype(np.float64)
    t = tiny.slice_t[k].reshape(4, 4).astype(np.float64)
    good, _ = oracle_mod.ncc_evaluate(targets[k], w2i @ t @ i2w, source)
    bad, _ = oracle_mod.ncc_evaluate(targets[k], w2i @ (geo.rigid_matrix(tx=4.0, rz=12.0) @ t) @ i2w, source)
    assert good > 0.9 and good > bad + 0.05


@pytest.mark.gpu
def test_device_ncc_moments_equal_the_oracle(tiny, oracle_mod):
    from fetalreconstruction_amd import engine
    source, targets, idx, mats = _case(tiny, oracle_mod, n_eval=64, seed=3)
    rec = engine.Reconstruction(0)
    rec.ncc_set_targets(targets)
    rec.ncc_set_source(source)
    ncc, sums = rec.ncc_evaluate(idx, mats)
    for e, (k, M) in enumerate(zip(idx, mats)):
        v, s = oracle_mod.ncc_evaluate(targets[k], M, source)
        assert np.array_equal(sums[e], s.astype(np.int64))            # integer moments: exact
        assert ncc[e] == pytest.approx(v, rel=1e-12, abs=1e-15)


@pytest.mark.gpu
def test_device_ncc_source_from_reconstruction(tiny, oracle_mod):
    """source = NULL takes static_cast<short> of the engine's current volume (RG.cc:2031)."""
    from fetalreconstruction_amd import engine
    source, targets, idx, mats = _case(tiny, oracle_mod, n_eval=8, seed=5)
    rec = engine.Reconstruction(0)
    engine.sync_gpu(rec, tiny)
    vol = np.random.default_rng(1).uniform(-5, 900, tiny.nvox).astype(np.float32)
    rec.debug_set(engine.BUF_RECONSTRUCTED, vol)
    rec.ncc_set_targets(targets)
    rec.ncc_set_source(None)
    ncc, sums = rec.ncc_evaluate(idx, mats)
    src = vol.reshape(tiny.vsize[::-1]).astype(np.int16)
    for e, (k, M) in enumerate(zip(idx, mats)):
        _, s = oracle_mod.ncc_evaluate(targets[k], M, src)
        assert np.array_equal(sums[e], s.astype(np.int64))


# ---- k_ncc and k_nmi_bin at their edges ---------------------------------------------------------------------------------------
# The independent reference is _numpy_ncc above, the oracle the second opinion; the six moments are integers and must be equal.
def _shift(tx=0.0, ty=0.0, tz=0.0, m=None):
    M = np.eye(4)
    if m is not None:
        M[:3, :3] = m
    M[:3, 3] = (tx, ty, tz)
    return M


_DYADIC = np.array([[0.5, 0.25, 0.0], [-0.25, 0.75, 0.0], [0.25, 0.25, 1.0]])      # every entry a multiple of 1/4


def _edge_cases():
    """name -> (targets int16 [n][ty][tx], source int16 [vz][vy][vx], target index [e], matrices [e][4][4])"""
    rng = np.random.default_rng(17)
    out = {}
    src = rng.integers(-60, 900, (17, 31, 23)).astype(np.int16)                    # negative voxels: value < 0 is dropped
    thin = rng.integers(-60, 900, (2, 31, 23)).astype(np.int16)                     # vz = 2: only 0 < Z < 1 is inside
    small = rng.integers(-3, 4, (17, 31, 23)).astype(np.int16)                      # -0.5 < value < 0 and 0 < value < 0.5 occur
    for tx, ty in ((7, 5), (37, 29), (256, 256)):
        t = rng.integers(-1, 3000, (3, ty, tx)).astype(np.int16)
        t[:, :, -1] = -1
        mats = [
            # multiples of 1/4 throughout: every product and sum is exact in double, the interpolated values are multiples of
            # 1/64 and many are x.5 exactly -- any correct implementation agrees whatever its order of operations, so this
            # checks IRTK's rounding rule (half away from zero) itself
            _shift(1.25, 3.5, 2.75, _DYADIC), _shift(0.75, 8.25, 4.5, _DYADIC * 0.5), _shift(2.5, 2.5, 0.25, _DYADIC.T * 0.25),
            # samples exactly on X = 0 (i = 0) and X = vx - 1 (i = 22), on Y = 0 and on Z = vz - 1: all excluded
            _shift(0.0, 1.0, 1.0), _shift(3.0, 0.0, 2.5), _shift(1.0, 2.0, 16.0),
            # every sample outside: n = 0, ncc = 0
            _shift(1000.0, 1.0, 1.0), _shift(1.0, 1.0, -3.0),
        ]
        idx = np.arange(len(mats)) % 3
        out[f"{tx}x{ty} on 23x31x17"] = (t, src, idx, np.stack(mats))
        out[f"{tx}x{ty} on 23x31x17, values -3..3"] = (t, small, idx[:3], np.stack(mats[:3]))
        flat = [_shift(1.25, 3.5, 0.5, _DYADIC * np.array([[1], [1], [0]])), _shift(0.5, 0.75, 0.25, _DYADIC * 0.5 * np.array([[1], [1], [0]])),
                _shift(0.0, 1.0, 0.5), _shift(1.0, 1.0, 1.0), _shift(1.0, 1.0, 0.0)]
        out[f"{tx}x{ty} on 23x31x2"] = (t, thin, np.arange(len(flat)) % 3, np.stack(flat))
    # the largest sums: 65536 pixels of 32767 against 32767 -- sum t s = 2^16 32767^2 = 7.04e13, far beyond int32 and float
    big = np.full((1, 256, 256), 32767, np.int16)
    out["256x256 at 32767 on 258x258x3 at 32767"] = (big, np.full((3, 258, 258), 32767, np.int16), np.zeros(2, int),
                                                     np.stack([_shift(1.0, 1.0, 1.0), _shift(0.5, 0.75, 0.25)]))
    return out


_EDGE = _edge_cases()
_EDGE_REF = {}


def _edge_ref(name):
    """the numpy moments of a case, computed once"""
    if name not in _EDGE_REF:
        t, s, idx, mats = _EDGE[name]
        _EDGE_REF[name] = np.stack([_numpy_ncc(t[k], M, s) for k, M in zip(idx, mats)])
    return _EDGE_REF[name]


def test_edge_cases_reach_their_edges():
    r = _edge_ref("37x29 on 23x31x17")
    assert (r[:5, 0] > 0).all() and (r[5:, 0] == 0).all()                          # (Z = vz - 1 for every sample: nothing is inside)
    t, s, idx, mats = _EDGE["37x29 on 23x31x17"]
    # X = i, Y = j + 1, Z = 1: the samples are the voxels themselves; i = 0 (X = 0) and i = 22 (X = vx - 1) are out, negative voxels dropped
    assert r[3, 0] == ((t[idx[3]] >= 0)[:, 1:22] & (s[1, 1:30, 1:22] >= 0)).sum()
    assert _edge_ref("7x5 on 23x31x2")[2:, 0].tolist() == [(_EDGE["7x5 on 23x31x2"][0][2] >= 0)[:, 1:].sum(), 0, 0]     # Z = 1 = vz - 1 and Z = 0: out
    big = _edge_ref("256x256 at 32767 on 258x258x3 at 32767")
    assert (big[:, 0] == 65536).all() and (big[:, 5] == 65536 * 32767 ** 2).all() and big[0, 5] > 7e13


@pytest.mark.parametrize("name", sorted(_EDGE))
def test_oracle_ncc_at_the_edges(oracle_mod, name):
    t, s, idx, mats = _EDGE[name]
    for e, (k, M) in enumerate(zip(idx, mats)):
        v, sums = oracle_mod.ncc_evaluate(t[k], M, s)
        assert np.array_equal(sums.astype(np.int64), _edge_ref(name)[e]), (name, e)
        if _edge_ref(name)[e][0] == 0:
            assert v == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(_EDGE))
def test_device_ncc_at_the_edges(name):
    from fetalreconstruction_amd import engine
    t, s, idx, mats = _EDGE[name]
    rec = engine.Reconstruction(0)
    rec.ncc_set_targets(t)
    rec.ncc_set_source(s)
    ncc, sums = rec.ncc_evaluate(idx, mats)
    want = _edge_ref(name)
    assert np.array_equal(sums, want), (name, np.argwhere(sums != want)[:4].tolist())
    assert (ncc[want[:, 0] == 0] == 0).all()
    rec.close()


@pytest.mark.gpu
def test_device_ncc_scratch_growth():
    """svr_ncc_evaluate's device scratch grows past 256 evaluations (200 fit the first allocation, 300 and 700 each replace
    it): every call equals the per-evaluation reference, with repeated and permuted target indices, and the first call's
    results come out again afterwards."""
    from fetalreconstruction_amd import engine
    rng = np.random.default_rng(23)
    t = rng.integers(-1, 3000, (6, 29, 37)).astype(np.int16)
    s = rng.integers(0, 900, (17, 31, 23)).astype(np.int16)
    n = 700
    idx = rng.integers(0, 6, n)
    mats = np.stack([_shift(*rng.uniform(-2, 6, 3), geo.rigid_matrix(0, 0, 0, *rng.uniform(-8, 8, 3))[:3, :3] * rng.uniform(0.4, 0.7)) for _ in range(n)])
    want = np.stack([_numpy_ncc(t[k], M, s) for k, M in zip(idx, mats)])
    assert (want[:, 0] > 0).mean() > 0.8 and (want[:, 0] == 0).any()            # (the inputs: most evaluations overlap the source, some do not)
    rec = engine.Reconstruction(0)
    rec.ncc_set_targets(t)
    rec.ncc_set_source(s)
    first = rng.permutation(n)[:200]
    calls = [first, rng.permutation(n)[:300], rng.permutation(n), first]
    for sel in calls:
        ncc, sums = rec.ncc_evaluate(idx[sel], mats[sel])
        assert np.array_equal(sums, want[sel]), len(sel)
    rec.close()


_NMI_WIDTHS = (1, 2, 3, 7, 64, 511, 512)


def _every_short():
    return np.arange(-1, 32767, dtype=np.int16).reshape(32, 32, 32)          # every value a level can hold: -1 (padding) .. 32766


@pytest.mark.parametrize("width", _NMI_WIDTHS)
def test_host_nmi_bin_is_the_integer_quotient(width):
    """irtkCalculateNumberOfBins' rescaling int(v / (double)width) of every v > 0 is v // width; -1 and 0 stay"""
    v = _every_short()
    nb, w, binned = host.irtk_number_of_bins(0, 64 * width - 1, v)             # a range of 64 width values: the smallest width that fits is `width`
    assert (nb, w) == (64, width)
    assert np.array_equal(binned, np.where(v > 0, v // width, v))


@pytest.mark.gpu
@pytest.mark.parametrize("width", _NMI_WIDTHS)
def test_device_nmi_bin_is_the_host_s(width):
    from fetalreconstruction_amd import engine
    v = _every_short()
    rec = engine.Reconstruction(0)
    rec.ncc_set_source(v)
    rec.nmi_bin_source(width)
    got = rec.ncc_get_source()
    assert np.array_equal(got, host.irtk_number_of_bins(0, 64 * width - 1, v)[2])
    assert np.array_equal(got, np.where(v > 0, v // width, v))
    rec.close()


# ---- CC and NMI see the same samples ------------------------------------------------------------------------------------------------
# With bins of width 1 the joint histogram h[source bin][target bin] of an evaluation determines all six moments of the cross
# correlation over the same planes, so the two metrics can be checked against each other exactly: they share V and the rounded
# source values (csrc/svr_sim.inc: one sampler for both), or these sums differ.
def _same_samples_case():
    """-> (source int16 [7][11][12], targets int16 [4][9][20], evaluations: list of (target planes, matrices [planes][4][4]))"""
    rng = np.random.default_rng(41)
    src = rng.integers(0, 64, (7, 11, 12)).astype(np.int16)
    src[1, 2, 3] = src[3, 5, 6] = src[4, 4, 9] = src[2, 8, 2] = src[5, 6, 5] = -1      # an interpolated value below 0 is dropped
    t = rng.integers(0, 64, (4, 9, 20)).astype(np.int16)
    t[rng.random(t.shape) < 0.08] = -1                                                # scattered padding
    rot = geo.rigid_matrix(0, 0, 0, 9.0, -14.0, 6.0)[:3, :3]
    base = [
        _shift(1.3, 0.9, 1.7, rot * 0.47),                                             # oblique
        _shift(0.0, 0.5, 2.25, np.array([[0.5, 0.0, 0.0], [0.0, 1.0, 0.125], [0.0625, 0.0, 0.75]])),    # column 0 on X = 0
        _shift(1.5, 0.5, 2.25, np.array([[0.5, 0.0, 0.0], [0.0, 1.0, 0.125], [0.0625, 0.0, 0.75]])),    # column 19 on X = 11 = vx - 1
        _shift(1000.0, 1.0, 1.0),                                                      # wholly outside: N = 0
    ]
    evals = []
    for M in base:
        for planes in ([0], [1, 2, 3]):                                                # a slice, and a package of three planes
            mats = np.stack([M.copy() for _ in planes])
            for k in range(len(planes)):
                mats[k, :3, 3] += k * M[:3, 2]                                         # plane k of a 3-D target starts at M (0, 0, k, 1)
            evals.append((planes, mats))
    return src, t, evals


def _moments_of_histogram(h):
    h = np.asarray(h).astype(np.int64)
    sb, tb = np.meshgrid(np.arange(64, dtype=np.int64), np.arange(64, dtype=np.int64), indexing="ij")
    return np.array([h.sum(), (tb * h).sum(), (sb * h).sum(), (tb * tb * h).sum(), (sb * sb * h).sum(), (tb * sb * h).sum()], np.int64)


def test_histogram_moments_equal_the_cc_moments(oracle_mod):
    """the identity on the CPU evaluators: the C oracle's NCC against the numpy joint histogram (and the inputs reach their edges)"""
    from tests.test_nmi_registration import joint_histogram
    src, t, evals = _same_samples_case()
    assert src.min() == -1 and src.max() == 63 and t.min() == -1 and t.max() == 63
    i = np.arange(20)
    assert (evals[2][1][0] @ [0, 3, 0, 1])[0] == 0.0 and (evals[4][1][0] @ [19, 3, 0, 1])[0] == 11.0    # X = 0 and X = vx - 1 exactly
    assert ((evals[3][1][2] @ np.stack([i, 0 * i + 3, 0 * i, 0 * i + 1]))[0] == 0.5 * i).all()        # ... on every plane of a package
    n_seen = []
    for planes, mats in evals:
        cc = sum(oracle_mod.ncc_evaluate(t[p], M, src)[1].astype(np.int64) for p, M in zip(planes, mats))
        got = _moments_of_histogram(joint_histogram([t[p] for p in planes], mats, src, 1, 64, 64))
        assert np.array_equal(got, cc), (planes, got, cc)
        n_seen.append(int(cc[0]))
    assert all(n > 0 for n in n_seen[:6]) and n_seen[6:] == [0, 0]


@pytest.mark.gpu
def test_device_histogram_moments_equal_the_device_cc_moments():
    """the identity on svr_ncc_evaluate and svr_nmi_evaluate(..., hist): both take their samples from the one device sampler"""
    from fetalreconstruction_amd import engine
    src, t, evals = _same_samples_case()
    rec = engine.Reconstruction(0)
    rec.ncc_set_targets(t)
    rec.ncc_set_source(src)
    idx = np.concatenate([planes for planes, _ in evals])
    mats = np.concatenate([m for _, m in evals])
    ppe = [len(planes) for planes, _ in evals]
    _, sums = rec.ncc_evaluate(idx, mats)
    out4, hist = rec.nmi_evaluate(ppe, idx, mats, [1] * len(ppe), [64] * len(ppe), 64, histograms=True)
    at = 0
    for e, n in enumerate(ppe):
        cc = sums[at:at + n].sum(0)
        got = _moments_of_histogram(hist[e])
        assert np.array_equal(got, cc), (e, got, cc)
        assert out4[e, 0] == cc[0]
        at += n
    assert (sums[:-4, 0] > 0).all() and (sums[-4:, 0] == 0).all()
    rec.close()
