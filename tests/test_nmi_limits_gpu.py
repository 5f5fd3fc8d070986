"""The device NMI (csrc/svr_nmi.inc) where its schedule splits, merges and regrows, on the cases of tests/nmi_cases.py (which
tests/test_nmi_cases.py shows to reach those edges): bins per evaluation mixed in one call, the compaction and the serial sums from no
bin to all 4096, plane sizes around the planes a workgroup takes, 70 chunks per evaluation, 150 merge slots per call across two
regrowths, 3000 workgroups, the term table's last entry, refused calls that leave every slot zero, and the evaluation arena shared with
NCC and LNCC.  Everything is compared exactly: histograms with array_equal, {n, S_xy, S_x, S_y} as tuples, repeated calls by their bytes."""
import math

import numpy as np
import pytest

from fetalreconstruction_amd import host
from tests import lncc_ref, nmi_cases as nc
from tests.test_ncc import _numpy_ncc
from tests.test_nmi_registration import entropy_sums, joint_histogram


def _load(rec, setup):
    rec.ncc_set_targets(setup.targets)
    rec.ncc_set_source(setup.source)
    rec.nmi_bin_source(setup.ws)
    assert np.array_equal(rec.ncc_get_source(), setup.binned)
    return rec


def _context(setup):
    from fetalreconstruction_amd import engine as E
    return _load(E.Reconstruction(0), setup)


def _run(rec, call):
    return rec.nmi_evaluate(*call.args(), histograms=call.hist)


def _same_bits(a, b):
    return a[0].tobytes() == b[0].tobytes() and (a[1] is None) == (b[1] is None) and (a[1] is None or np.array_equal(a[1], b[1]))


def _check(rec, setup, call, what):
    """one call against the restatement, then the same call again at once: the same bits (slots and counters were left zero)"""
    got = _run(rec, call)
    out, hist = got
    want_out, want_hist, want_nmi = nc.restate(setup, call, joint_histogram, entropy_sums)
    for e in range(len(call)):
        if call.hist:
            assert np.array_equal(hist[e], want_hist[e]), (what, e, np.argwhere(hist[e] != want_hist[e])[:5])
            v = host.nmi_sums(hist[e], int(call.nbts[e]), call.nbs)[1]
            assert v == want_nmi[e] or (math.isnan(v) and math.isnan(want_nmi[e])), (what, e, v, want_nmi[e])
        assert tuple(out[e]) == tuple(want_out[e]), (what, e, out[e], want_out[e])
    assert _same_bits(_run(rec, call), got), what
    return got


@pytest.mark.gpu
def test_bins_per_evaluation_mixed_in_one_call():
    wide, flat, call64, call1 = nc.case1()
    rec = _context(wide)
    with_h = _check(rec, wide, call64, "64 source bins")
    order = [3, 9, 0, 6, 2, 8, 1, 5, 7, 4]                               # another order, no histograms: other slots, the same sums
    without = _check(rec, wide, call64.take(order, hist=False), "64 source bins, reordered")
    assert without[0].tobytes() == with_h[0][order].tobytes()
    _load(rec, flat)
    _check(rec, flat, call1, "1 source bin")


@pytest.mark.gpu
def test_compaction_and_serial_sums_from_no_bin_to_all_of_them():
    setup, call = nc.case2_full()
    out, hist = _check(_context(setup), setup, call, "4096 bins")
    assert np.count_nonzero(hist[0]) == 4096 and out[0, 0] == 131072
    setup, call = nc.case2_sparse()
    rec = _context(setup)
    out, hist = _check(rec, setup, call, "sparse")
    assert [int(np.count_nonzero(h)) for h in hist] == nc.CASE2_NNZ
    assert (out[3] == 0).all() and (out[4] == 0).all()
    _check(rec, setup, call.take(range(len(call)), hist=False), "sparse, no histograms")


@pytest.mark.gpu
@pytest.mark.parametrize("tx,ty", nc.CASE3_SIZES)
def test_plane_sizes_around_the_planes_a_workgroup_takes(tx, ty):
    setup, call = nc.case3(tx, ty)
    rec = _context(setup)
    with_h = _check(rec, setup, call, (tx, ty))
    without = _check(rec, setup, call.take([2, 1, 3, 0], hist=False), (tx, ty, "reordered"))
    assert without[0].tobytes() == with_h[0][[2, 1, 3, 0]].tobytes()


@pytest.mark.gpu
def test_many_chunks_many_slots_and_two_regrowths_on_one_context():
    setup, a, b = nc.case4()
    rec = _context(setup)
    _check(rec, setup, a, "70 and 33 chunks")
    got = [_check(rec, setup, c, f"{len(c)} split evaluations") for c in b]
    assert _same_bits(got[3], got[0])                                    # after 150 slots and two new layouts: the first call's bits
    assert got[2][0][:3].tobytes() == got[0][0].tobytes()
    _check(rec, setup, a.take(range(len(a)), hist=False), "70 and 33 chunks, after the regrowths")


@pytest.mark.gpu
def test_three_thousand_single_plane_evaluations_in_one_call():
    setup, batch = nc.case4_batch()
    out, _ = _check(_context(setup), setup, batch, "3000 workgroups")
    assert out[:61].tobytes() == out[61:122].tobytes()


@pytest.mark.gpu
def test_term_table_entry_one_past_the_first_upload():
    (first, call1), (second, call2) = nc.case5()
    rec = _context(first)
    _check(rec, first, call1, "35 pixels")
    _load(rec, second)
    out, hist = _check(rec, second, call2, "36 samples in one bin")
    t = 36 * math.log(36)
    assert tuple(out[0]) == (36.0, t, t, t) and hist[0][5, 3] == 36


@pytest.mark.gpu
def test_refused_calls_leave_nothing_behind():
    from fetalreconstruction_amd import engine as E
    setup, refused, mended, valid = nc.case6()
    fresh = _run(_context(setup), valid)                                 # on a context that ran nothing else
    rec = _context(setup)
    for name in ("first chunk", "last chunk", "single block"):
        with pytest.raises(E.SvrError, match="outside the bins"):
            _run(rec, refused[name])
        assert _same_bits(_check(rec, setup, valid, f"after {name}"), fresh)
        _check(rec, setup, mended[name], f"{name}, mended")
    with pytest.raises(E.SvrError, match="target index out of range"):  # refused before any launch
        _run(rec, refused["index"])
    assert _same_bits(_check(rec, setup, valid, "after the index"), fresh)


def _evaluate(rec, setup, metric, args):
    """one call of the sequence checked against its restatement on the binned source -> what it returned, as bytes"""
    if metric == "nmi":
        out, hist = _check(rec, setup, args, metric)
        return out.tobytes() + (hist.tobytes() if hist is not None else b"")
    idx, mats = args
    if metric == "ncc":
        ncc, sums = rec.ncc_evaluate(idx, mats)
        for e, (i, M) in enumerate(zip(idx, mats)):
            assert np.array_equal(sums[e], _numpy_ncc(setup.targets[i], M, setup.binned)), (metric, e)
        return ncc.tobytes() + sums.tobytes()
    sums, kmap = rec.lncc_evaluate(idx, mats, 3, maps=metric == "lncc maps")
    for e, (i, M) in enumerate(zip(idx, mats)):
        key = ("lncc", int(i), M.tobytes())
        if key not in setup.cache:
            setup.cache[key] = lncc_ref.lncc_plane(setup.targets[i], M, setup.binned, 3)
        N, S, k = setup.cache[key]
        assert (int(sums[e, 0]), int(sums[e, 1])) == (N, S), (metric, e)
        assert kmap is None or np.array_equal(kmap[e], k), (metric, e)
    return sums.tobytes() + (kmap.tobytes() if kmap is not None else b"")


@pytest.mark.gpu
def test_ncc_nmi_and_lncc_share_one_growing_arena():
    setup, seq = nc.case7()
    rec = _context(setup)
    for step, (metric, args) in enumerate(seq):
        shared = _evaluate(rec, setup, metric, args)
        assert shared == _evaluate(_context(setup), setup, metric, args), (step, metric)   # a context that ran nothing else
