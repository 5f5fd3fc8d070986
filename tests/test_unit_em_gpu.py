"""The device's unit-level EM (csrc/svr_em.inc) checked directly, kernel by kernel, against the numpy restatement of the same arithmetic
(tests/unit_em_ref.py) on the cases of tests/unit_em_cases.py.  The tests play the launcher: they fill the all-gather's buffer
themselves -- one context at a time, no processes, no communicator.

  A  k_slice_em<false / true> on crafted vectors: the unpack, the exclusions, the five scalars BIT FOR BIT in the 256-thread order,
     the weights to one float ulp (slices) or four times the measured float-Gaussian gap (patches), numberings, shardings
  B  k_mstep_finish, k_potential_pack and k_mstep_scalars_dev against the separate calls, bit for bit, at the shape sweep's grids
  C  refusals are errors with a message, and leave the context usable
"""
import numpy as np
import pytest

from tests import shape_select as S
from tests import unit_em_cases as K
from tests import unit_em_ref as R
from tests.test_shape_sweep_gpu import _ctx, _em_ctx, _em_inputs

pytestmark = pytest.mark.gpu

STEP = K.STEP
EM3 = np.float32([150.0, 0.85, 1.0 / 160.0])
F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class _Pool:
    """contexts of n slices of 2 x 2 pixels, one per slice count (svr_slice_em_setup may be called again on a context)"""

    def __init__(self):
        self.recs = {}

    def get(self, n_local):
        if n_local not in self.recs:
            self.recs[n_local] = _ctx((4, 4, 4), sgrid=(2, 2, n_local), slices=np.ones((n_local, 2, 2), np.float32))
        return self.recs[n_local]

    def close(self):
        for r in self.recs.values():
            r.close()
        self.recs = {}


@pytest.fixture(scope="module")
def pool():
    p = _Pool()
    yield p
    p.close()


@pytest.fixture(scope="module")
def gap():
    return K.patch_gauss_gap()


def _load(rec, c, rank=None, w=None, state5=None):
    """setup, state, the E-step's own launch (for the buffers), then every rank's packed vectors over what it left"""
    rank = c["rank"] if rank is None else rank
    ident = np.array_equal(c["by_ref"], np.arange(c["n"]))
    rec.slice_em_setup(c["n"], c["world"], rank, c["rlo"], None if ident else R.order_of(c["by_ref"]), STEP)
    if c["form"] == "patch":
        rec.slice_em_set_patch_form(c["src_ref"])
    rec.slice_em_set_state(c["w"] if w is None else w, c["excl"], np.float64(c["state5"] if state5 is None else state5), EM3)
    send, recv, nf = rec.mstep_estep_device(0, STEP)
    maxn = R.max_count(c["rlo"])
    assert nf == 3 * maxn and (recv == send) == (c["world"] == 1)
    rec.device_write(recv, R.pack(c["pot"], c["scale"], c["inside"], c["world"], c["rlo"], maxn))
    return recv


def _local(c, rank=None):
    rank = c["rank"] if rank is None else rank
    return c["rlo"][rank], c["rlo"][rank + 1]


def _check(c, out, w_in, mix_in, gap, tag=""):
    """one run's fetched state against the restatement: w_in, mix_in = the weights and mix_s the run started from"""
    name = c["name"] + tag
    src = None if c["src_ref"] is None else R.src_host(c["src_ref"], c["by_ref"])
    p = R.apply_exclusions(c["pot"], c["scale"], c["excl"], src)
    assert np.array_equal(_bits(out["scale"]), _bits(c["scale"])), name
    assert np.array_equal(out["inside"], c["inside"] > 0.5), name
    assert np.array_equal(_bits(out["potential"]), _bits(p)), name
    m1, m2, s1, s2, den, _ = R.class_scalars(p, w_in, c["by_ref"], c["form"], STEP, "tree256")
    dev = out["scalars5"].astype(F32)
    assert np.array_equal(dev.astype(np.float64), out["scalars5"]), name              # floats held in doubles
    print(name, "device scalars", dev, "tree256", [m1, m2, s1, s2])
    assert np.array_equal(_bits(dev[:4]), _bits([m1, m2, s1, s2])), (name, dev, [m1, m2, s1, s2])
    ser = R.class_scalars(p, w_in, c["by_ref"], c["form"], STEP, "serial")[:4]
    assert R.ulp_diff(dev[:4], np.array(ser, F32)).max() <= 1, (name, dev, ser)
    wd = out["weight"]
    if c["form"] == "slice":
        wr, _, exact = R.unit_weights(p, w_in, dev[0], dev[1], dev[2], dev[3], mix_in, den, "slice", STEP)
        d = R.ulp_diff(wd, wr)
        print(name, "weights, largest ulp distance", int(d.max()))
        assert d.max() <= 1, (name, int(d.max()), int(d.argmax()))
        assert np.array_equal(_bits(wd[exact]), _bits(wr[exact])), name
    else:
        wr, _, exact = R.unit_weights(p, w_in, dev[0], dev[1], dev[2], dev[3], mix_in, den, "patch", STEP, "f64")
        d = np.abs(wd.astype(np.float64) - wr.astype(np.float64))
        w32 = R.unit_weights(p, w_in, dev[0], dev[1], dev[2], dev[3], mix_in, den, "patch", STEP, "f32")[0]
        print(name, "patch weights, largest gap to the float64 Gaussian %.3e (CPU float32 gap %.3e); to numpy's float32 Gaussian %d ulp"
              % (d.max(), gap, int(R.ulp_diff(wd, w32).max())))
        assert (d <= 4 * gap + np.spacing(np.abs(wr)).astype(np.float64)).all(), (name, d.max(), gap)
        assert np.array_equal(_bits(wd[exact]), _bits(wr[exact])), name
    mix = R.unit_mix(p, wd, c["by_ref"], "tree256")
    assert _bits(dev[4])[0] == _bits(mix)[0], (name, dev[4], mix)
    if not (p >= 0).any():
        assert dev[4] == F32(0.9)
    assert np.array_equal(_bits(out["em3"]), _bits(EM3)), name                          # iter 0: the M-step's scalars stay
    return wd, dev[4]


# ================================ A. k_slice_em on crafted vectors ================================
@pytest.mark.parametrize("name", list(K.CASES))
def test_slice_em_against_the_restatement(pool, gap, name):
    """every case: one run, then a second from the first's weights and mix_s (the restatement applied to the device's own state)"""
    c = K.CASES[name]
    lo, hi = _local(c)
    rec = pool.get(hi - lo)
    _load(rec, c)
    rec.slice_em_run()
    w1, mix1 = _check(c, rec.slice_em_fetch(), c["w"], c["state5"][4], gap)
    rec.slice_em_run()
    _check(c, rec.slice_em_fetch(), w1, mix1, gap, " (second run)")


@pytest.mark.parametrize("name", ["mixed 255", "mixed 513", "mixed 257", "patch [130, 127, 256] permuted world 4"])
def test_every_rank_of_a_sharding_gives_the_same_bits(pool, name):
    """the same gathered vectors with rank = 0 .. world - 1, each in a context of its own slice count (an empty rank holds no context)"""
    c = K.CASES[name]
    first = None
    for rank in range(c["world"]):
        lo, hi = _local(c, rank)
        if hi == lo:
            continue
        rec = pool.get(hi - lo)
        _load(rec, c, rank)
        rec.slice_em_run()
        out = rec.slice_em_fetch()
        if first is None:
            first = out
            continue
        for k in ("scale", "weight", "potential", "inside", "scalars5", "em3"):
            assert out[k].tobytes() == first[k].tobytes(), (name, rank, k)


@pytest.mark.parametrize("name", ["mixed 255", "mixed 513", "mixed 1120"])
def test_the_ranks_part_reaches_the_scatters_vector(name):
    """ScaleVolumeSums reads the vector the scatter reads: after a run it must hold w_global[rlo[rank] : rlo[rank + 1]] -- and again
    after other weights were sent in between and svr_slice_em_apply_weights put the EM's back"""
    from fetalreconstruction_amd import engine as E
    c = K.CASES[name]
    lo, hi = _local(c)
    ns = hi - lo
    sgrid = (5, 7, ns)
    ins = _em_inputs(sgrid, 11 + ns)
    slices, sims, simw, weights, inside, scales, slicew = ins
    rec = _em_ctx(ins, sgrid)
    _load(rec, c)
    rec.debug_set(E.BUF_WEIGHTS, weights)                  # (the E-step's own launch in _load moved the per-pixel weights)
    rec.slice_em_run()
    wg = rec.slice_em_fetch()["weight"]
    want = S.scalevol_sums(slices, weights, sims, simw, wg[lo:hi])
    # the weights tell the windows apart: the global vector read at offset 0 or one unit off gives other sums, far outside the bound
    for off in {0, lo - 1, lo + 1} - {lo}:
        if 0 <= off <= c["n"] - ns:
            assert not np.allclose(S.scalevol_sums(slices, weights, sims, simw, wg[off:off + ns]), want, rtol=1e-6, atol=0), (name, off)
    assert np.allclose(rec.ScaleVolumeSums(), want, rtol=1e-10, atol=0), (name, want)
    rec.UpdateSliceWeights(slicew)
    assert np.allclose(rec.ScaleVolumeSums(), S.scalevol_sums(slices, weights, sims, simw, slicew), rtol=1e-10, atol=0)
    rec.slice_em_apply_weights()
    assert np.allclose(rec.ScaleVolumeSums(), want, rtol=1e-10, atol=0), name
    rec.close()


# ================================ B. the fused tails at the sweep's shapes ================================
TAIL_GRIDS = [((23, 89), 1), ((683, 3), 256), ((63, 65), 257), ((17, 241), 513), ((2049, 1), 257)]


def _tail_inputs(grid, ns):
    sx, sy = grid
    sgrid = (sx, sy, ns)
    ins = list(_em_inputs(sgrid, sx * 7 + ns))
    ins[4][2::5] = 0                                       # slices without an inside pixel: their flag is 0
    return sgrid, tuple(ins)


def _twin(ins, sgrid, pvr):
    rec = _em_ctx(ins, sgrid)
    rec.set_option("pvr", pvr)
    return rec


@pytest.mark.parametrize("pvr", [0, 1])
@pytest.mark.parametrize("grid,ns", TAIL_GRIDS)
def test_fused_tails_are_the_separate_calls_bit_for_bit(grid, ns, pvr):
    """svr_mstep_estep_device (k_mstep + k_mstep_finish, k_estep + k_potential_pack) for iter 0, 1, 2 on one context against MStep and
    EStep called separately on its twin, and against mstep_scalars restated on the twin's five sums.  The per-slice inside flags are
    k_slice_inside's of the SIMINSIDE buffer the contexts were given (these contexts hold no PSF to simulate slices with)."""
    from fetalreconstruction_amd import engine as E
    sgrid, ins = _tail_inputs(grid, ns)
    a, b = _twin(ins, sgrid, pvr), _twin(ins, sgrid, pvr)
    flags = a.GetSliceInside()
    assert np.array_equal(flags, ins[4].reshape(ns, -1).any(axis=1)) and (ns < 3 or not flags.all())
    b.slice_em_setup(ns, 1, 0, [0, ns], None, STEP)
    sigma, mix, m = EM3
    for it in (0, 1, 2):
        b.slice_em_set_state(np.ones(ns, F32), np.zeros(ns, np.uint8), np.zeros(5), np.float32([sigma, mix, m]))
        send, recv, nf = b.mstep_estep_device(it, STEP)
        assert nf == 3 * ns and send == recv
        if it > 0:
            s5 = a.MStepSums()
            sigma, mix, m = (F32(x) for x in a.MStep(it, STEP, sigma, mix))
            want = R.mstep_scalars(s5, it, STEP, pvr, *em_before[:2])
            assert np.array_equal(_bits([sigma, mix, m]), _bits(want)), (it, sigma, mix, m, want)
        pot = a.EStep(m, sigma, mix)
        got = b.device_read(send, nf)
        em3 = b.slice_em_fetch()["em3"]
        assert np.array_equal(_bits(em3), _bits([sigma, mix, m])), (it, em3, sigma, mix, m)
        assert np.array_equal(_bits(got[:ns]), _bits(pot)), it
        assert np.array_equal(_bits(got[ns:2 * ns]), _bits(a.GetScaleVector())), it
        assert np.array_equal(got[2 * ns:], flags.astype(F32)), it
        assert np.array_equal(_bits(a.debug_get(E.BUF_WEIGHTS)), _bits(b.debug_get(E.BUF_WEIGHTS))), it
        em_before = (sigma, mix, m)
    # a sharding whose largest rank holds more than this one: k_potential_pack pads with zeros up to maxn
    maxn = ns + 7
    b.slice_em_setup(ns + maxn, 2, 0, [0, ns, ns + maxn], None, STEP)
    b.slice_em_set_state(np.ones(ns + maxn, F32), np.zeros(ns + maxn, np.uint8), np.zeros(5), np.float32([sigma, mix, m]))
    send, recv, nf = b.mstep_estep_device(0, STEP)
    assert nf == 3 * maxn and send != recv
    got = b.device_read(send, nf).reshape(3, maxn)
    pot = a.EStep(m, sigma, mix)
    assert np.array_equal(_bits(got[0, :ns]), _bits(pot)) and np.array_equal(_bits(got[1, :ns]), _bits(a.GetScaleVector()))
    assert np.array_equal(got[2, :ns], flags.astype(F32))
    assert np.array_equal(_bits(got[:, ns:]), np.zeros((3, maxn - ns), np.uint32))
    a.close()
    b.close()


def test_the_packed_inside_flags_are_simulate_slices_own():
    """a phantom with a PSF, its mask cut down to a small box off the centre: SimulateSlices raises the per-slice flags itself (some
    slices keep none), and k_potential_pack's third vector, the scale vector and the potentials are what the separate calls return"""
    from fetalreconstruction_amd import engine as E, phantom
    P = phantom.problem_tiny()
    vx, vy, vz = P.vsize
    mask = np.zeros((vz, vy, vx), np.float32)                # a small box off the centre: slices of any orientation miss it or meet it
    mask[22:28, 22:28, 22:28] = np.array(P.mask, np.float32).reshape(vz, vy, vx)[22:28, 22:28, 22:28]
    assert mask.any()
    P.mask = mask
    recs = []
    for _ in range(2):
        rec = E.Reconstruction(0)
        E.sync_gpu(rec, P)
        ones = np.ones(P.ns, F32)
        rec.UpdateScaleVector(ones, ones)
        rec.InitializeEMValues()
        rec.GaussianReconstruction()
        recs.append(rec)
    a, b = recs
    flags = a.SimulateSlices()
    assert np.array_equal(b.SimulateSlices(), flags) and np.array_equal(a.GetSliceInside(), flags)
    print("slices inside:", int(flags.sum()), "of", P.ns)
    assert flags.any() and not flags.all()
    ns, maxn = P.ns, P.ns + 5
    sigma, mix, m = EM3
    b.slice_em_setup(ns + maxn, 2, 0, [0, ns, ns + maxn], None, STEP)
    b.slice_em_set_state(np.ones(ns + maxn, F32), np.zeros(ns + maxn, np.uint8), np.zeros(5), EM3)
    send, recv, nf = b.mstep_estep_device(0, STEP)
    got = b.device_read(send, nf).reshape(3, maxn)
    pot = a.EStep(m, sigma, mix)
    assert np.array_equal(_bits(got[0, :ns]), _bits(pot)) and np.array_equal(_bits(got[1, :ns]), _bits(a.GetScaleVector()))
    assert np.array_equal(got[2, :ns], flags.astype(F32))
    assert np.array_equal(_bits(got[:, ns:]), np.zeros((3, maxn - ns), np.uint32))
    # ... and through the EM: the unpacked flags of this rank are the same ones
    b.device_write(recv, np.concatenate([got.reshape(-1), np.zeros(3 * maxn, F32)]))
    b.slice_em_run()
    assert np.array_equal(b.slice_em_fetch()["inside"][:ns], flags)
    a.close()
    b.close()


@pytest.mark.parametrize("pvr", [0, 1])
def test_the_ranks_sums_meet_on_the_device(pvr):
    """world 3, iter 2: this rank's five sums (svr_mstep_partial) at its index of the gathered buffer, crafted sums for the others -- a
    rank whose minimum is +inf and whose maximum is -inf; for slices a largest maximum below FLT_MIN, so that both clamps are on the
    path -- then k_mstep_scalars_dev (svr_mstep_estep_device) and k_mstep_scalars_ranks (svr_mstep_estep_ranks) on a twin"""
    sgrid, ins = _tail_inputs((63, 65), 257)
    ns, world, rank = 257, 3, 2
    a, b = _twin(ins, sgrid, pvr), _twin(ins, sgrid, pvr)
    n = 5 + 9 + ns
    b.slice_em_setup(n, world, rank, [0, 5, 14, n], None, STEP)
    sigma, mix = F32(150.0), F32(0.85)
    for clamp in (False, True):
        b.slice_em_set_state(np.ones(n, F32), np.zeros(n, np.uint8), np.zeros(5), np.float32([sigma, mix, 0.0]))
        send, recv = b.mstep_partial(world)
        mine = b.device_read(send, 8, np.float64)
        assert np.array_equal(mine[:5], a.MStepSums())
        all8 = np.zeros((world, 8))
        all8[rank] = mine
        # the first sums cancel only when they are added in rank order: (2^100 - 2^100) + mine, not (mine - 2^100) + 2^100
        all8[0, :5] = [2.0 ** 100, 77.25, 300.0, np.inf, -np.inf]
        all8[1, :5] = [-2.0 ** 100, 1e-3, 7.0, -12.5, 40.0]
        if clamp:                                           # the extremes of every rank: min +inf -> FLT_MAX, max < FLT_MIN -> FLT_MIN (slices)
            all8[:, 3] = np.inf
            all8[1, 4], all8[rank, 4] = 1e-39, 3e-39
        b.device_write(recv, all8)
        s2, r2 = a.mstep_partial(world)
        a.device_write(r2, all8)
        s5 = R.combine_ranks(all8, world)
        assert s5[0] == mine[0] and s5[1] == (77.25 + 1e-3) + mine[1]
        want = R.mstep_scalars(s5, 2, STEP, pvr, sigma, mix)
        sd, rv, nf = b.mstep_estep_device(2, STEP)
        em3 = b.slice_em_fetch()["em3"]
        assert np.array_equal(_bits(em3), _bits(want)), (clamp, em3, want)
        if clamp and not pvr:
            assert em3[2] == F32(1) / (R.FLT_MIN - R.FLT_MAX)
        em_a, pot_a = a.mstep_estep_ranks(world, 2, STEP, sigma, mix)
        assert np.array_equal(_bits(em_a), _bits(em3)), (clamp, em_a, em3)
        assert np.array_equal(_bits(b.device_read(sd, ns)), _bits(pot_a)), clamp
    a.close()
    b.close()


# ================================ C. refusals are errors, not faults ================================
def _refused(call, *words):
    from fetalreconstruction_amd import engine as E
    with pytest.raises(E.SvrError) as e:
        call()
    assert all(w in str(e.value) for w in words), str(e.value)


def test_refusals_leave_the_context_usable(gap):
    c = K.CASES["mixed 257"]
    lo, hi = _local(c)
    ns = hi - lo

    def valid(rec):
        _load(rec, c)
        rec.slice_em_run()
        _check(c, rec.slice_em_fetch(), c["w"], c["state5"][4], gap, " (after a refusal)")

    rec = _ctx((4, 4, 4), sgrid=(2, 2, ns), slices=np.ones((ns, 2, 2), np.float32))
    for call in (rec.slice_em_run, rec.slice_em_fetch, lambda: rec.mstep_estep_device(0, STEP), rec.slice_em_apply_weights,
                 lambda: rec.slice_em_set_patch_form(None)):
        _refused(call, "svr_slice_em_setup first")
    valid(rec)
    n, world, rlo = c["n"], c["world"], c["rlo"]
    bad = list(rlo)
    bad[c["rank"]] -= 1                                      # this rank's range one longer than the context's slice count
    _refused(lambda: rec.slice_em_setup(n, world, c["rank"], bad, None, STEP), "do not match")
    valid(rec)
    _refused(lambda: rec.slice_em_setup(n, 3, 2, [0, n - ns + 5, n - ns, n], None, STEP), "out of order")
    _refused(rec.slice_em_run, "svr_slice_em_setup first")  # (a refused setup leaves none)
    valid(rec)
    order = R.order_of(c["by_ref"]).copy()
    order[3] = order[4]
    _refused(lambda: rec.slice_em_setup(n, world, c["rank"], rlo, order, STEP), "not a permutation")
    order[3] = n
    _refused(lambda: rec.slice_em_setup(n, world, c["rank"], rlo, order, STEP), "not a permutation")
    valid(rec)
    src = np.arange(n, dtype=np.int32)
    src[7] = n
    _refused(lambda: rec.slice_em_set_patch_form(src), "out of range")
    valid(rec)
    # world > 1 and iter > 0: the ranks' sums must have met (svr_mstep_partial) before the fused step
    _refused(lambda: rec.mstep_estep_device(1, STEP), "svr_mstep_partial")
    valid(rec)
    # a new slice grid invalidates the setup
    rec.initStorageVolumes((2, 2, ns), (1.0, 1.0, 1.0))
    _refused(rec.slice_em_run, "svr_slice_em_setup first")
    _refused(rec.slice_em_fetch, "svr_slice_em_setup first")
    rec.FillSlices(np.ones((ns, 2, 2), np.float32), np.full(ns, 2, np.int32), np.full(ns, 2, np.int32))
    rec.setSliceDims(np.ones((ns, 3), np.float32), 2.0)
    m = np.broadcast_to(np.eye(4, dtype=np.float32), (ns, 4, 4)).copy()
    rec.SetSliceMatrices(m, m, m, m, m, m, np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32))
    rec.UpdateScaleVector(np.ones(ns, np.float32), np.ones(ns, np.float32))
    _refused(rec.slice_em_run, "svr_slice_em_setup first")  # (the slices are back, the setup is not)
    valid(rec)
    rec.close()
