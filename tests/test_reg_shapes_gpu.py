"""The device's float slice-to-volume registration (csrc/svr_reg.inc) stage by stage at the shapes of tests/reg_cases.py, against
the C oracle (bit for bit where that is the contract) and the float64 numpy reference of tests/reg_ref.py (within the
tolerances reg_cases derives from the oracle's own measured distance), device against device over the launch options, whole
runs against the oracle where tests/test_reg_ref.py has shown them well-conditioned, the refusals of the test hooks, and the
patch cost of the patch-based path at awkward patch shapes.  The device-only intermediates come back through svr_reg_get."""
import ctypes
import math

import numpy as np
import pytest

from fetalreconstruction_amd import engine as E

import reg_cases as cases
import reg_ref as ref

pytestmark = pytest.mark.gpu

EYE = np.eye(4, dtype=np.float32).reshape(1, 16)
_ctx = {}


def _engine(c):
    """the smallest context the registration needs: a volume, the world-to-image matrix, the registration slices"""
    rec = E.Reconstruction(0)
    rec.InitReconstructionVolume((c.vx, c.vy, c.vz), (c.vdim,) * 3, None, 12.0)
    rec.initStorageVolumes((1, 1, 1), (1.0, 1.0, 1.0))
    rec.SetSliceMatrices(EYE, EYE, EYE, EYE, EYE, EYE, EYE[0], c.w2i)
    rec.UpdateReconstructed((c.vx, c.vy, c.vz), c.vol)
    rec.initRegStorageVolumes(c.W, c.H, c.ns)
    rec.FillRegSlices(c.targets)
    rec.updateResampledSlicesI2W(c.ofs)
    rec.prepareSliceToVolumeReg()
    return rec


@pytest.fixture(scope="module", autouse=True)
def _close_contexts(oracle_mod):
    yield
    for rec, _ in _ctx.values():
        rec.close()
    _ctx.clear()


def _get(name):
    """(engine, oracle) of a case, made once"""
    if name not in _ctx:
        c = cases.get(name)
        _ctx[name] = (_engine(c), cases.oracle_for(c))
    return _ctx[name]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _f32_sum(layer):
    """the float nearest to the exact sum of the values > -1 of a float layer"""
    v = layer[layer > -1]
    return np.float32(math.fsum(float(x) for x in v))


def _check_stage(name, rec, o, level, k, act, widths_note=""):
    """one evaluation at the case's start matrices: every stage of the device against the oracle and the reference"""
    c = cases.get(name)
    r = cases.reference(name, level, k)
    what = (name, "level", level, "list", k, widths_note)
    idx = np.arange(c.ns) if act is None else np.asarray(act)
    a = len(idx)
    scale = float(c.vol.max())
    so, do_ = o.evaluate_costs(c.start, level, act)
    sg, dg = rec.evaluate_costs(c.start, level, act)
    tg, to = rec.reg_get(E.REG_TARGETS), o._resampled_float.reshape(c.ns, c.H, c.W)
    # blurred sampled slices and blurred targets: the oracle's bits, the reference's padding
    assert np.array_equal(_bits(dg), _bits(do_)), (*what, "sampled slices", int((_bits(dg) != _bits(do_)).sum()))
    assert np.array_equal(_bits(tg), _bits(to)), (*what, "targets", int((_bits(tg) != _bits(to)).sum()))
    assert np.array_equal(dg == -1, r["blurred"] == -1) and np.array_equal(tg == -1, r["targets"] == -1), what
    # counts: exact
    cnt_a, cnt_b = rec.reg_get(E.REG_CNT_A), rec.reg_get(E.REG_CNT_B)[:, :a]
    assert np.array_equal(cnt_a, r["cntA"]) and np.array_equal(cnt_b, r["cntB"]), what
    # sums: within tol_rel of count x largest sample (every element is within MEASURED["slices"] of the reference's)
    tol = cases.tol_rel(name)
    sum_a, sum_b = rec.reg_get(E.REG_SUM_A), rec.reg_get(E.REG_SUM_B)[:, :a]
    ea, eb = np.abs(sum_a - r["sumA"]) / (np.maximum(r["cntA"], 1) * scale), np.abs(sum_b - r["sumB"]) / (np.maximum(r["cntB"], 1) * scale)
    print(*what, f"sumA {ea.max():.2e} sumB {eb.max():.2e} of {tol:.2e}", end=" ")
    assert ea.max() <= tol and eb.max() <= tol, (*what, ea.max(), eb.max(), tol)
    assert (sum_a[r["cntA"] == 0] == 0).all() and (sum_b[r["cntB"] == 0] == 0).all(), what
    # that the accumulation is double: the float stored is the float nearest to the exact sum of the float layer.  This does not need
    # integer voxels (a blurred layer holds none); it is asserted on the two cases whose layers are small and whose samples are integers
    # times 8-bit fractions, where every partial sum fits a double and the equality is therefore certain rather than likely
    if c.integer:
        assert all(sum_a[s] == _f32_sum(tg[s]) for s in range(c.ns)), what
        assert all(sum_b[o_, s] == _f32_sum(dg[o_, s]) for o_ in range(3) for s in range(a)), what
    # moments: the same tol_rel, of pairs x (largest sample)^2
    mom = rec.reg_get(E.REG_MOMENTS)[:, :a]
    em = np.abs(mom - r["mom"]) / (np.maximum(r["pairs"], 1)[..., None] * scale * scale)
    print(f"moments {em.max():.2e} of {tol:.2e}", end=" ")
    assert em.max() <= tol, (*what, em.max(), tol)
    assert (mom[r["pairs"] == 0] == 0).all(), what
    # ... and at their own magnitude against the oracle, which adds the same float terms in double in another order: the stored
    # floats can differ by the one final rounding (2^-23 of the value); the signed sum m0 also by the order of fewer than 2^13
    # double additions of terms whose absolute values sum to at most sqrt(m1 m2) (2^-40 of that)
    sb_o, mom_o = o.last_stages()
    ulp = 2.0 ** -23
    assert (np.abs(sum_b - sb_o) <= ulp * np.abs(sb_o)).all(), (*what, "sumB against the oracle", np.abs(sum_b - sb_o).max())
    slack = 2.0 ** -40 * np.sqrt(mom_o[..., 1].astype(np.float64) * mom_o[..., 2])
    assert (np.abs(mom[..., 1:] - mom_o[..., 1:]) <= ulp * np.abs(mom_o[..., 1:])).all(), (*what, "m1, m2 against the oracle")
    assert (np.abs(mom[..., 0] - mom_o[..., 0]) <= ulp * np.abs(mom_o[..., 0]) + slack).all(), (*what, "m0 against the oracle")
    # similarities: the reference within tol_sim, the oracle within the project's 2e-6, zeros where they belong
    es = np.abs(sg - r["sim"]).max()
    print(f"sim {es:.2e} of {cases.tol_sim(name):.2e}")
    assert es <= cases.tol_sim(name), (*what, es)
    assert np.abs(sg - so).max() <= 2e-6, (*what, np.abs(sg - so).max())
    live = r["sim"] != 0                                     # the active slices that have data
    assert np.array_equal(sg != 0, live) and (sg != 0).sum() == live.sum() <= a, what
    inactive = np.setdiff1d(np.arange(c.ns), idx)
    assert (sg[inactive] == 0).all(), what
    if name != "dead_slices":
        assert live.sum() == a, what
    table = rec.reg_get(E.REG_SIMILARITIES)
    assert np.array_equal(_bits(table[0]), _bits(sg)) and (table[1:] == 0).all(), what
    got_act, _, width = rec.reg_get(E.REG_ACTIVE)
    assert np.array_equal(got_act, idx), what
    return sg, mom, sum_b, width


@pytest.mark.parametrize("name", cases.NAMES)
def test_stages_are_the_oracle_and_the_reference(name):
    rec, o = _get(name)
    c = cases.get(name)
    for level in (1, 0):
        for k, act in enumerate(cases.active_lists(c)):
            _check_stage(name, rec, o, level, k, act)
    if name == "dead_slices":
        sg, _ = rec.evaluate_costs(c.start, 0)
        assert sg[1] == 0 and sg[3] == 0 and (sg[[0, 2, 4]] != 0).all()
        assert rec.reg_get(E.REG_CNT_A)[1] == 0 and rec.reg_get(E.REG_SUM_A)[1] == 0                         # no target data
        assert (rec.reg_get(E.REG_CNT_B)[:, 3] == c.W * c.H).all() and (rec.reg_get(E.REG_SUM_B)[:, 3] == 0).all()   # all zeros


@pytest.mark.parametrize("name,auto", [("red_4096", 256), ("red_4270", 1024)])
def test_reduction_width_follows_the_image_size(name, auto):
    """4096 pixels stay on 256 lanes, 4270 take 1024 on their own.  The two widths give the same float bits here (the double sums
    differ far below a float rounding), so the results cannot show which one ran: the width the reductions were launched with is
    read back (svr_reg_get).  The automatic choice is then the forced width it should equal, bit for bit, and the other width
    stays within the tolerances (inside _check_stage)."""
    rec, o = _get(name)
    try:
        for level in (1, 0):
            out = {}
            for width in (0, 256, 1024):
                rec.set_option("reg_red_threads", width)
                out[width] = _check_stage(name, rec, o, level, 0, None, f"width {width}")
                assert out[width][3] == (width or auto), (name, level, "asked for", width, "ran with", out[width][3])
            for x, y in zip(out[0][:3], out[auto][:3]):
                assert np.array_equal(_bits(x), _bits(y)), (name, level, "automatic is not", auto)
    finally:
        rec.set_option("reg_red_threads", 0)


def _device_run(rec, c, schedule, batch, blind):
    rec.set_option("reg_batch", batch)
    rec.set_option("reg_blind", blind)
    rec.prepareSliceToVolumeReg()                            # (back to the default schedule)
    if schedule:
        rec.set_schedule(*schedule)
    t = rec.registerSlicesToVolume(c.start)
    act, ls_max, _ = rec.reg_get(E.REG_ACTIVE)
    return t, rec.reg_counters(), act, ls_max


@pytest.mark.parametrize("name", cases.NAMES)
def test_whole_runs_device_against_device(name):
    """the literal launch sequence (reg_batch 0, reg_blind 0) against the batched gradient and the blind line search: matrices,
    counters and the active list left behind, bit for bit.  Default schedule; (2, 1, 2) from 1024 slices on, which is what takes
    the blind line search's compaction and its tail loop past 1024 active slices."""
    rec, _ = _get(name)
    c = cases.get(name)
    schedule = (2, 1, 2) if c.ns >= 1024 else None
    try:
        t0, c0, a0, m0 = _device_run(rec, c, schedule, 0, 0)
        assert c0[1] > 0 and np.abs(t0 - c.start.reshape(-1, 4, 4)).max() > 0.01
        for batch, blind in ((1, 4), (1, 0), (0, 1), (1, 7)):
            t, cn, a, m = _device_run(rec, c, schedule, batch, blind)
            key = (name, batch, blind)
            assert np.array_equal(cn, c0), (*key, cn, c0)
            assert np.array_equal(_bits(t), _bits(t0)), (*key, int((_bits(t) != _bits(t0)).any(axis=(1, 2)).sum()), "slices differ")
            assert np.array_equal(a, a0) and m == m0, key
        if name == "ns_1100":
            assert m0 > 1024                                 # a line-search step kept more than one chunk of slices
    finally:
        rec.set_option("reg_batch", 1)
        rec.set_option("reg_blind", 4)


@pytest.mark.parametrize("name", [n for n in cases.NAMES if cases.TRAJECTORY[n]])
def test_whole_runs_are_the_oracle_s(name):
    """only where tests/test_reg_ref.py shows the run well-conditioned: equal counters, every matrix within 1e-5, the same active
    list left behind, in order"""
    rec, _ = _get(name)
    c = cases.get(name)
    schedule = cases.TRAJECTORY[name]
    to, co, ao, mo = cases.oracle_run(c, schedule)
    try:
        for batch, blind in ((1, 4), (0, 0)):
            tg, cg, ag, mg = _device_run(rec, c, schedule, batch, blind)
            assert np.array_equal(cg, co), (name, batch, blind, cg, co)
            d = np.abs(tg - to).reshape(c.ns, -1).max(1)
            assert (d <= 1e-5).all(), (name, batch, blind, int((d > 1e-5).sum()), "slices differ, the worst by", d.max())
            assert np.array_equal(ag, ao) and mg == mo, (name, batch, blind, len(ag), len(ao), mg, mo)
        assert np.abs(tg - c.start.reshape(-1, 4, 4)).max() > 0.01
        if name == "ns_1100":
            assert mg > 1024 and len(ag) > 1024              # the first line-search step left more than 1024 slices: the second chunk ran
    finally:
        rec.set_option("reg_batch", 1)
        rec.set_option("reg_blind", 4)


def _raw(rec, fn, *args):
    """a library entry called with the arguments as given (the binding would refuse some of them itself) -> (status, message)"""
    rc = getattr(rec._lib, fn)(rec._h, *args)
    msg = rec._lib.svr_last_error(rec._h)
    return rc, (msg.decode() if msg else "")


def test_refusals_leave_the_state_alone():
    """every refused call is an error code with a message, and the next valid call gives the answer it gave before"""
    c = cases.get("wide_37x5")
    rec = E.Reconstruction(0)
    rec.InitReconstructionVolume((c.vx, c.vy, c.vz), (c.vdim,) * 3, None, 12.0)
    rec.initStorageVolumes((1, 1, 1), (1.0, 1.0, 1.0))
    rec.SetSliceMatrices(EYE, EYE, EYE, EYE, EYE, EYE, EYE[0], c.w2i)
    rec.UpdateReconstructed((c.vx, c.vy, c.vz), c.vol)
    t = np.ascontiguousarray(c.start, np.float32).copy()
    sim, buf = np.zeros(c.ns, np.float32), np.zeros(c.ns * c.W * c.H + 8, np.float32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    evaluate = lambda: _raw(rec, "svr_reg_evaluate_costs", P(t), 0, None, 0, P(sim), None)
    register = lambda: _raw(rec, "svr_register_slices_to_volume", P(t.copy()))
    get = lambda which, nbytes: _raw(rec, "svr_reg_get", int(which), P(buf), ctypes.c_size_t(nbytes))
    for call, msg in ((evaluate, "FillRegSlices"), (register, "FillRegSlices"), (lambda: get(E.REG_SUM_A, 4 * c.ns), "no registration state"),
                      (lambda: _raw(rec, "svr_prepare_slice_to_volume_reg"), "svr_init_reg_storage_volumes first")):
        rc, text = call()                                    # before svr_init_reg_storage_volumes
        assert rc != 0 and msg in text, (rc, text)
    rec.initRegStorageVolumes(c.W, c.H, c.ns)
    for step in (lambda: rec.FillRegSlices(c.targets), lambda: rec.updateResampledSlicesI2W(c.ofs), lambda: rec.prepareSliceToVolumeReg()):
        with pytest.raises(E.SvrError, match="FillRegSlices / updateResampledSlicesI2W / prepareSliceToVolumeReg first"):
            rec.evaluate_costs(c.start, 0)
        with pytest.raises(E.SvrError, match="FillRegSlices / updateResampledSlicesI2W / prepareSliceToVolumeReg first"):
            rec.registerSlicesToVolume(c.start)
        with pytest.raises(E.SvrError, match="no registration state"):
            rec.reg_get(E.REG_SUM_A)
        step()
    o = cases.oracle_for(c)
    good = rec.evaluate_costs(c.start, 1, [2, 0])
    state = [rec.reg_get(w) for w in range(8)]
    assert np.abs(good[0] - o.evaluate_costs(c.start, 1, [2, 0])[0]).max() <= 2e-6 and (good[0][[0, 2]] != 0).all()
    other = c.ident                                          # (refused evaluations come with other matrices: none of them may be taken)
    refused = ((lambda: rec.evaluate_costs(other, 2), "level out of range"), (lambda: rec.evaluate_costs(other, -1), "level out of range"),
               (lambda: rec.evaluate_costs(other, 0, [0, c.ns]), "active slice out of range"),
               (lambda: rec.evaluate_costs(other, 0, [-1]), "active slice out of range"),
               (lambda: rec.evaluate_costs(other, 0, [0] * (c.ns + 1)), "active list too long"),
               (lambda: get(E.REG_TARGETS, 4 * c.ns * c.W * c.H - 4), "svr_reg_get: size mismatch"),
               (lambda: get(E.REG_ACTIVE, 4 * c.ns), "svr_reg_get: size mismatch"),
               (lambda: get(E.REG_SUM_B, 0), "svr_reg_get: size mismatch"),
               (lambda: get(9, 4), "svr_reg_get: unknown array"), (lambda: get(-1, 4), "svr_reg_get: unknown array"),
               (lambda: rec.set_schedule(3, 0, 0), "at most 2 levels"))
    for call, msg in refused:
        try:
            out = call()
            rc, text = out if isinstance(out[0], int) else (0, "accepted")
        except E.SvrError as e:
            rc, text = 1, str(e)
        assert rc != 0 and msg in text, (msg, rc, text)
        for w in range(8):                                   # reading is repeatable and a refusal changes nothing it reads
            assert np.array_equal(rec.reg_get(w), state[w]), (msg, w)
        again = rec.evaluate_costs(c.start, 1, [2, 0])
        assert np.array_equal(_bits(again[0]), _bits(good[0])) and np.array_equal(_bits(again[1]), _bits(good[1])), msg
        assert np.array_equal(rec.reg_get(E.REG_ACTIVE)[0], [2, 0])
    rec.close()


# ---- the patch cost ---------------------------------------------------------------------------------------------------------------
def _patch_engine(c):
    rec = E.Reconstruction(0)
    rec.set_option("pvr", 1)
    rec.InitReconstructionVolume(c.vsize, (c.vdim,) * 3, None, 12.0)
    rec.initStorageVolumes((c.px, c.py, c.n), (1.0, 1.0, 1.0))
    rec.FillSlices(c.patches, [c.px] * c.n, [c.py] * c.n)
    eye = np.tile(EYE, (c.n, 1))
    rec.SetSliceMatrices(eye, eye, eye, eye, eye, eye, EYE[0], c.w2i)
    rec.UpdateReconstructed(c.vsize, c.vol)
    return rec


@pytest.mark.parametrize("name", cases.PATCH_NAMES)
def test_patch_cost_at_awkward_patch_shapes(name, oracle_mod):
    """px != py, fewer samples than a workgroup, sizes no multiple of level + 1, levels 0-2: integer data gives the reference's six
    sums exactly; generic data the exact counts, sums within twice the oracle's measured distance, and the oracle's NCC"""
    for integer in (True, False):
        c = cases.patch_case(name, integer)
        rec = _patch_engine(c)
        for level in range(3):
            ng, sg = rec.cc_patches(c.ri2w, c.tm, level)
            no, so = oracle_mod.cc_patches(c.patches, c.ri2w, c.tm, c.w2i, c.vol, level)
            want = [ref.cc_patch(c.patches[k], c.ri2w[k], c.tm[k], c.w2i, c.vol, level) for k in range(c.n)]
            sr = np.stack([w[1] for w in want])
            what = (name, integer, level)
            assert np.array_equal(sg[:, 0], sr[:, 0]) and (sr[:, 0] > 0).all(), what
            if integer:
                assert np.array_equal(sg, sr), (*what, np.abs(sg - sr).max())
            else:
                e = (np.abs(sg[:, 1:] - sr[:, 1:]) / np.maximum(np.abs(sr[:, 1:]), 1)).max()
                print(*what, f"sums {e:.2e} of {2 * cases.PATCH_MEASURED[name]:.2e}")
                assert e <= 2 * cases.PATCH_MEASURED[name], (*what, e)
            many = sr[:, 0] > 2
            assert np.allclose(ng[many], no[many], rtol=0, atol=2e-4, equal_nan=True), (*what, np.abs(ng - no)[many].max())
        if integer:                                          # a buffer instead of the uploaded patches
            buf = np.where(c.patches >= 0, c.patches + 1, c.patches).astype(np.float32)
            want = np.stack([ref.cc_patch(buf[k], c.ri2w[k], c.tm[k], c.w2i, c.vol, 1)[1] for k in range(c.n)])
            assert np.array_equal(rec.cc_patches(c.ri2w, c.tm, 1, buf)[1], want), name
        rec.close()


def test_patch_registration_on_a_non_square_patch(oracle_mod):
    """19 x 13 patches at 2.7 mm: level 1 blurs with 13 taps and the second pass with 14 (svr_pvr_register_patches).  The acceptance
    rule of test_pvr_patch_registration_parity -- equal launch count, the evaluation-count band -- with the share of identical patches
    the oracle itself keeps under a last-bit perturbation of the volume (reg_cases.PATCH_REG_SHARE, 11 of 24) less one patch."""
    c = cases.patch_reg_case()
    rec = _patch_engine(c)
    for k, v in zip(("pvr_reg_levels", "pvr_reg_steps", "pvr_reg_iterations"), c.schedule):
        rec.set_option(k, v)
    tg, tig, cg = rec.register_patches(c.ri2w, c.mo, c.invmo, c.T)
    to, tio, co = cases.oracle_patch_run(c)
    same = np.abs(tg - to).max(axis=1) < 1e-4
    print("evaluations", cg, co, "max |dT|", np.abs(tg - to).max(), "identical patches", same.mean())
    assert cg[0] == co[0] == c.schedule[0] * c.schedule[1] * c.schedule[2] and cg[2] == co[2] == c.n
    assert abs(int(cg[1]) - int(co[1])) <= max(10, int(co[1]) // 1000)
    assert same.mean() >= cases.PATCH_REG_SHARE - cases.PATCH_REG_MARGIN
    assert np.allclose(tig[same], tio[same], atol=1e-3)
    rec.close()
