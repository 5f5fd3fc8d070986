"""The coefficient table written by one kernel family and read by the other (csrc/svr_coeff.h: the one layout every writer and reader uses).

The other table tests pair a writer with the readers of its own family; a site with a different idea of the layout would pass them.  Here
every writer (k_coeff_build, the cell scatter's store, the cell gather's store) feeds every reader (cell scatter, cell gather by LDS-DMA, tile
scatter, tile gather) at support 16, in one context: back_mode, fwd_mode and coeff_lazy raise no change in the invalidation map
(tests/test_invalidation_gpu.py), so the table a writer left stands while the readers take turns and all twelve pairs are reachable."""
import numpy as np
import pytest

from tests.test_parity_gpu import TOL_SUM
from tests.util import rel_err

pytestmark = pytest.mark.gpu

# reader: (option, mode, the pass it is)
READERS = {
    "cell scatter": ("back_mode", 5, "scatter"),
    "cell gather by LDS-DMA": ("fwd_mode", 2, "gather"),
    "tile scatter": ("back_mode", 4, "scatter"),
    "tile gather": ("fwd_mode", 1, "gather"),
}


def test_every_table_writer_feeds_every_table_reader(tiny):
    from fetalreconstruction_amd import engine as E
    rng = np.random.default_rng(23)
    on = tiny.slices != -1
    ones = np.ones(tiny.ns, np.float32)
    psf = np.where(on, rng.uniform(0.5, 1.5, tiny.slices.shape), 0).astype(np.float32)
    vol = rng.uniform(0.5, 1.5, tiny.nvox).astype(np.float32)
    w = np.where(on, rng.uniform(0.2, 1.0, tiny.slices.shape), 0).astype(np.float32)
    sim = np.where(tiny.slices > 0, tiny.slices * rng.uniform(0.8, 1.2, tiny.slices.shape), 0).astype(np.float32)

    def context(table):
        rec = E.Reconstruction(0)
        E.sync_gpu(rec, tiny)
        rec.timer_enable(True)
        rec.set_option("coeff_table", table)
        rec.UpdateScaleVector(ones, ones)
        rec.debug_set(E.BUF_PSF_SUMS, psf)
        rec.debug_set(E.BUF_RECONSTRUCTED, vol)
        return rec

    def run(rec, kind):
        """one pass from the same inputs every time"""
        if kind == "gather":
            for b, dt in ((E.BUF_SIMSLICES, np.float32), (E.BUF_SIMWEIGHTS, np.float32), (E.BUF_SIMINSIDE, np.uint8)):
                rec.debug_set(b, np.zeros(sim.shape, dt))
            rec.SimulateSlices()
            return [rec.debug_get(b).copy() for b in (E.BUF_SIMSLICES, E.BUF_SIMWEIGHTS, E.BUF_SIMINSIDE)]
        rec.debug_set(E.BUF_SIMSLICES, sim)
        rec.debug_set(E.BUF_WEIGHTS, w)
        rec.SuperresolutionBackproject(ones)
        return [rec.debug_get(b).copy() for b in (E.BUF_ADDON, E.BUF_CONFIDENCE_MAP)]

    def counts(rec):
        tm = rec.timers()
        return {k: tm[k][1] for k in ("coeff_build", "backproject_store", "forward_store", "backproject_table", "forward_table")}

    def step(rec, kind, expect):
        """the pass, and which of the table's timers it must have raised (all others stand)"""
        before = counts(rec)
        out = run(rec, kind)
        after = counts(rec)
        assert {k: after[k] - before[k] for k in after} == {k: int(k in expect) for k in after}, (kind, expect, before, after)
        return out

    def same(got, want, what):
        for k, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(a, b, equal_nan=True), (what, k)

    def no_fallback(rec, what):
        assert not any(rec.fallbacks().values()), (what, rec.fallbacks())

    # the reference: the same modes with every tap evaluated in every pass
    rec = context(0)
    ref = {}
    for name, (opt, mode, kind) in READERS.items():
        rec.set_option(opt, mode)
        ref[name] = step(rec, kind, ())
        assert rec.get_option(opt) == mode and rec.get_option("coeff_valid") == 0
        no_fallback(rec, name)
    rec.close()

    rec = context(1)
    for writer in ("k_coeff_build", "cell scatter store", "cell gather store"):
        rec.set_option("back_mode", 5)
        rec.set_option("fwd_mode", 2)
        rec.set_option("coeff_lazy", int(writer != "k_coeff_build"))
        rec.set_option("coeff_invalidate", 1)
        assert rec.get_option("coeff_valid") == 0
        if writer == "k_coeff_build":                        # (ahead of the gather that asks for it, which then reads it)
            same(step(rec, "gather", ("coeff_build", "forward_table")), ref["cell gather by LDS-DMA"], writer)
            assert rec.get_option("coeff_state") == 2
        elif writer == "cell scatter store":
            same(step(rec, "scatter", ("backproject_store",)), ref["cell scatter"], writer)
            assert rec.get_option("coeff_state") == 1
        else:
            same(step(rec, "gather", ("forward_store",)), ref["cell gather by LDS-DMA"], writer)
            assert rec.get_option("coeff_state") == 1
        state = rec.get_option("coeff_state")
        for name, (opt, mode, kind) in READERS.items():
            pair = f"{writer} -> {name}"
            rec.set_option(opt, mode)
            got = step(rec, kind, ("forward_table",) if kind == "gather" else ("backproject_table",))
            assert rec.get_option(opt) == mode and rec.get_option("coeff_state") == state, pair    # the writer's table, still
            no_fallback(rec, pair)
            if name == "tile scatter":                       # float atomics in run-dependent order, in the reference too
                assert np.array_equal(got[1] > 0, ref[name][1] > 0), pair
                for k in (0, 1):
                    err = rel_err(got[k], ref[name][k])
                    print(f"{pair}: rel_err[{k}] = {err:.3e}")
                    assert err < TOL_SUM, (pair, k, err)
            else:                                            # sums in a fixed order: the bits of evaluating every tap
                same(got, ref[name], pair)
    rec.close()
