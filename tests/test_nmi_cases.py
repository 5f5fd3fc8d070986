"""Every case of tests/nmi_cases.py reaches the edge it is there for.  No GPU: the chunk, slot, capacity and term-table arithmetic comes
from the schedule restated in nmi_cases.py, the counts and bins from joint_histogram / entropy_sums of tests/test_nmi_registration.py.
tests/test_nmi_limits_gpu.py runs the same cases on the device and has nothing left to decide but equality; a case that stops reaching
its edge fails here."""
import math

import numpy as np
import pytest

from tests import lncc_ref, nmi_cases as nc
from tests.test_ncc import _numpy_ncc
from tests.test_nmi_registration import entropy_sums, joint_histogram, number_of_bins


def _restate(setup, call):
    return nc.restate(setup, call, joint_histogram, entropy_sums)


def test_the_schedule_restated():
    assert [nc.per_block(*s) for s in [(64, 64), (100, 93), (8, 8), (61, 67), (37, 33)]] == [4, 1, 256, 4, 13]
    assert [nc.per_block(*s) for s in nc.CASE3_SIZES] == nc.CASE3_PER_BLOCK
    assert nc.chunks(70, 100, 93) == 70 and nc.chunks(13, 64, 64) == 4 and nc.chunks(4, 64, 64) == 1
    t = nc.Tables()
    first = t.call([12, 1, 5, 4, 13], 64, 64)                           # the largest call of tests/test_nmi_gpu.py
    assert first["chunks"] == [3, 1, 2, 1, 4] and first["slots"] == 3 and (first["slots_before"], first["slots_after"]) == (0, 64)
    assert first["terms_after"] == 13 * 4096 + 1
    five_stacks = t.call([70] * 65, 100, 93)                             # five P4 stacks at a gradient step
    assert five_stacks["slots"] == 65 and five_stacks["slots_after"] == 97 and five_stacks["workgroups"] == 65 * 70


def test_case_1_mixes_bin_layouts_in_one_call():
    wide, flat, call64, call1 = nc.case1()
    assert nc.per_block(wide.tx, wide.ty) == 4
    info = nc.Tables().call(call64.ppe, wide.tx, wide.ty)
    assert info["chunks"] == nc.CASE1_CHUNKS and info["slots"] == 5 and {1, 2, 3} == set(info["chunks"])
    assert sorted(set(nc.CASE1_KINDS)) == sorted({(7, 1), (5, 2), (2, 33), (1, 64), (512, 64)})
    assert number_of_bins(0, 64) == (33, 2) and number_of_bins(0, 63) == (64, 1) and number_of_bins(0, 32766) == (64, 512)
    assert wide.targets.max() == 32766 and (wide.ws, wide.nbs) == number_of_bins(0, 3007)[::-1]
    assert flat.binned.max() == 0 and flat.source.max() > 400 and flat.nbs == 1  # one source bin, from positive values
    assert np.array_equal(wide.targets, flat.targets)
    for setup, call in ((wide, call64), (flat, call1)):
        out, hist, nmi = _restate(setup, call)
        rows = np.zeros(64, np.int64)
        for e, (kind, planes) in enumerate(nc.CASE1_EVALS):
            w, nbt = nc.CASE1_KINDS[kind]
            assert (call.widths[e], call.nbts[e], call.ppe[e]) == (w, nbt, planes)
            t = setup.targets[call.idx[call.planes(e)]]
            assert t.max() == nc.CASE1_TOPS[kind] and t.max() // w == nbt - 1          # the targets have the range of their bins
            assert out[e, 0] > 200 * planes and hist[e][:, nbt - 1].sum() > 0, (e, out[e])   # and the last target bin is used
            assert hist[e][:, nbt:].sum() == 0 and hist[e][call.nbs:].sum() == 0
            rows += hist[e].sum(1).astype(np.int64)
        assert (rows[:call.nbs] > 0).all()                               # every source bin, the last one too
    assert math.isnan(_restate(flat, call1)[2][0]) and _restate(flat, call1)[0][0, 1] > 0   # nbt = nbs = 1: one joint bin, NMI 0 / 0


def test_case_2_full_histogram():
    setup, call = nc.case2_full()
    info = nc.Tables().call(call.ppe, setup.tx, setup.ty)
    assert info["chunks"] == [8] and info["max_count"] == 131072
    out, hist, _ = _restate(setup, call)
    assert out[0, 0] == 131072 and np.count_nonzero(hist[0]) == 4096
    assert (hist[0].min(), hist[0].max()) == (3, 60)                     # the smallest and the largest count


def test_case_2_sparse_histograms_and_no_sample():
    setup, call = nc.case2_sparse()
    out, hist, _ = _restate(setup, call)
    nnz = [int(np.count_nonzero(h)) for h in hist]
    assert nnz == nc.CASE2_NNZ == [5, 27, 16, 0, 0, 32]                  # below 8; 3 x 8 + 3; 2 x 8 and no tail; none; 4 x 8
    assert [int(v) for v in out[:, 0]] == nnz                            # one sample per non-zero bin
    assert (out[3] == 0).all() and (out[4] == 0).all()
    assert (setup.targets[3] == -1).all() and (setup.targets[4] >= 0).all()   # (d) by padding, and by a matrix outside the source
    (_, _), (one, call_one) = nc.case5()                                 # (b) one non-zero bin
    assert np.count_nonzero(_restate(one, call_one)[1][0]) == 1


@pytest.mark.parametrize("tx,ty", nc.CASE3_SIZES)
def test_case_3_plane_sizes_around_per_block(tx, ty):
    setup, call = nc.case3(tx, ty)
    pb = nc.per_block(tx, ty)
    assert list(call.ppe) == [pb, pb + 1, 2 * pb, 1]
    info = nc.Tables().call(call.ppe, tx, ty)
    assert info["chunks"] == [1, 2, 2, 1] and info["slots"] == 2          # unsplit, a last chunk of one plane, two full chunks
    assert (pb + 1) - pb == 1 and 2 * pb - pb == pb
    if (tx, ty) == (5, 7):
        assert tx * ty < 256 and call.ppe[1] == 469 and setup.targets.shape[0] == 3
    out, _, _ = _restate(setup, call)
    assert (out[:, 0] > 0.25 * call.ppe * tx * ty).all(), out[:, 0]


def test_case_4_many_chunks_slots_and_regrowth():
    setup, a, b = nc.case4()
    assert nc.per_block(setup.tx, setup.ty) == 1
    t = nc.Tables()
    info = t.call(a.ppe, 129, 64)
    assert info["chunks"] == [70, 1, 1, 1, 33] and info["slots"] == 2 and info["slots_after"] == 64
    out, _, _ = _restate(setup, a)
    assert (out[:, 0] > 0.25 * a.ppe * 129 * 64).all()
    assert [len(c) for c in b] == nc.CASE4_CALLS
    caps = []
    for c in b:
        assert (c.ppe == 2).all()
        info = t.call(c.ppe, 129, 64)
        assert info["slots"] == len(c) and set(info["chunks"]) == {2}
        assert (info["slots"] > info["slots_before"]) == (len(c) > 3)    # the 65 and the 150 are the first calls beyond the capacity
        caps.append(info["slots_after"])
    assert caps == nc.CASE4_CAPS == [64, 97, 225, 225]
    assert all(np.array_equal(x, y) for x, y in zip(b[0].args()[:5], b[3].args()[:5]))
    assert (_restate(setup, b[0])[0][:, 0] > 4000).all()
    small, batch = nc.case4_batch()
    info = nc.Tables().call(batch.ppe, small.tx, small.ty)
    assert info["workgroups"] == 3000 and info["slots"] == 0 and info["slots_after"] == 0 and not batch.hist
    out, _, _ = _restate(small, batch)
    assert len(small.cache) == 61 and (out[:, 0] > 0).sum() > 2500 and len({tuple(r) for r in out}) > 50


def test_case_5_needs_the_entry_one_past_the_first_table():
    (first, call1), (second, call2) = nc.case5()
    t = nc.Tables()
    info = t.call(call1.ppe, first.tx, first.ty)
    assert (first.tx, first.ty) == (5, 7) and info["terms_after"] == 36   # entries 0 .. 35
    info = t.call(call2.ppe, second.tx, second.ty)
    assert info["max_count"] == 36 == info["terms_before"] and info["terms_after"] == 72
    assert _restate(first, call1)[0][0, 0] == 35
    out, hist, nmi = _restate(second, call2)
    assert hist[0][5, 3] == 36 and hist[0].sum() == 36                   # all 36 pixels, one joint bin
    want = 36 * math.log(36)
    assert tuple(out[0]) == (36.0, want, want, want)


def test_case_6_refusals_are_one_value_at_the_end_of_the_bins():
    setup, refused, mended, valid = nc.case6()
    row, col = nc.CASE6_BAD_AT
    assert setup.targets[2, row, col] == 192 == 64 * 3 and setup.targets[:2].max() == 191
    diff = setup.targets[2] != setup.targets[0]
    assert diff.sum() == 1 and diff[row, col]
    where = {"first chunk": (0, 0), "last chunk": (1, 4), "single block": (1, 0)}   # (evaluation, plane of it)
    for name, (e, k) in where.items():
        bad, good = refused[name], mended[name]
        info = nc.Tables().call(bad.ppe, 129, 64)
        assert info["chunks"][e] == (1 if name == "single block" else 5) and info["slots"] == 2
        at = bad.starts[e] + k
        assert np.flatnonzero(bad.idx != good.idx).tolist() == [at] and bad.idx[at] == 2 and good.idx[at] == 0
        with pytest.raises(AssertionError, match="outside the bins"):
            _restate(setup, bad)
        out, _, _ = _restate(setup, good)
        assert (out[:, 0] > 1000).all()
        # the restatement samples that pixel of that plane
        plane = setup.targets[0].copy()
        n_with = joint_histogram([plane], good.mats[at:at + 1], setup.binned, 3, 64, 64).sum()
        plane[row, col] = -1
        assert n_with - joint_histogram([plane], good.mats[at:at + 1], setup.binned, 3, 64, 64).sum() == 1
    assert refused["index"].idx.max() == 3 == setup.targets.shape[0] and (refused["index"].idx != mended["first chunk"].idx).sum() == 1
    info = nc.Tables().call(valid.ppe, 129, 64)
    assert info["slots"] == 3 and info["chunks"] == [5, 5, 5, 1]          # at least as many split evaluations as any refused call
    assert (_restate(setup, valid)[0][:, 0] > 1000).all()


def test_case_7_every_metric_grows_the_arena_once():
    setup, seq = nc.case7()
    assert [m for m, _ in seq] == ["ncc", "nmi", "lncc maps", "ncc", "nmi", "lncc"]
    assert nc.CASE7_TARGET_BINS == number_of_bins(0, 1799) and nc.CASE7_SOURCE_BINS == number_of_bins(0, 2499)
    assert setup.targets.max() == 1799 and setup.source.max() < 2500 and setup.binned.max() == 62
    assert len(seq[0][1][0]) == 10 and len(seq[1][1]) == 40 and seq[1][1].hist and len(seq[3][1][0]) == 300 and not seq[4][1].hist
    assert set(nc.Tables().call(seq[1][1].ppe, setup.tx, setup.ty)["chunks"]) == {1, 2, 3}
    arena, grew = nc.Arena(), []
    for metric, args in seq:
        if metric == "ncc":
            grew.append(arena.ncc(len(args[0]))[1])
        elif metric == "nmi":
            grew.append(arena.nmi(args, setup.tx, setup.ty)[1])
        else:
            grew.append(arena.lncc(len(args[0]), setup.tx, setup.ty, metric == "lncc maps")[1])
    assert grew == [True, True, True, False, False, False]              # NCC's floor, NMI's histograms, LNCC's maps; then all fit
    assert nc.Arena().ncc(300)[0] > 256 * 180                            # alone, the 300 would have grown it themselves
    out, _, _ = _restate(setup, seq[1][1])
    assert (out[:, 0] > 100).all()
    idx, mats = seq[2][1]                                                # the other two metrics have something to sum on the binned source
    assert len(idx) == nc.CASE7_LNCC and all(lncc_ref.lncc_plane(setup.targets[i], M, setup.binned, 3)[0] > 100 for i, M in zip(idx[:8], mats))
    assert all(_numpy_ncc(setup.targets[i], M, setup.binned)[0] > 100 for i, M in zip(*seq[0][1]))
