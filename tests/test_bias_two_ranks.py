"""Bias correction through the C++ sharded host with gloo: two PROCESSES on the one GPU, each with its own engine context and half of
the slices (tests/test_two_ranks_one_gpu.py's set-up), three reconstruction iterations with BiasGPU / NormaliseBiasGPU in every SR
iteration -- the sharded NormaliseBias (each rank scatters its own slices on its own cell lists, the bias volume is all-reduced,
every rank finishes) against the one-rank run."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests.test_two_ranks_one_gpu import _free_port, _problem

pytestmark = pytest.mark.gpu if __name__ != "__main__" else None


def _worker(rank, world, port, outdir):
    import torch                                       # before the engine's library: torch carries its own copy of the HIP runtime
    import torch.distributed as dist
    from fetalreconstruction_amd import engine as E, host, phantom
    from fetalreconstruction_amd.sharding import TorchComm, shard_units, slice_cost_weights
    os.environ["GLOO_SOCKET_IFNAME"] = "lo"
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        P = _problem()
        act = (P.slices != -1).reshape(P.ns, -1).sum(1)
        work = slice_cost_weights(act, P.slice_i2w, P.slice_t, P.recon_w2i, P.slice_dim, P.vdim[0])
        order, ranges = shard_units(work, P.stack_index, world, "spatial")
        lo, hi = ranges[rank]
        rec = E.Reconstruction(0)
        rec.set_flags(disable_bias_correction=False)
        E.sync_gpu(rec, phantom.sub_problem(P, 0, 0, select=order[lo:hi]))
        d = host.irtkReconstruction(rec, P.ns, (lo, hi), TorchComm(device=None, slabs=True), P.max_intensity, P.min_intensity)
        d.set_unit_order(order)
        d.set_bias_correction(True, 12.0)
        d.SetSmoothingParameters(150, 0.02)
        d.reconstruct_iteration(3)
        st = d.state()
        np.savez(os.path.join(outdir, f"rank{rank}.npz"), recon=rec.syncCPU(), scale=st["scale"], order=order,
                 cells=np.array([rec.get_option("bias_scatters"), rec.get_option("bias_scatters_on_cells")]))
        rec.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_bias_two_processes_on_one_gpu_match_one_rank():
    from fetalreconstruction_amd import engine as E, host
    P = _problem()
    rec = E.Reconstruction(0)
    rec.set_flags(disable_bias_correction=False)
    E.sync_gpu(rec, P)
    ref = host.irtkReconstruction(rec, P.ns, max_intensity=P.max_intensity, min_intensity=P.min_intensity)
    ref.set_bias_correction(True, 12.0)
    ref.SetSmoothingParameters(150, 0.02)
    ref.reconstruct_iteration(3)
    v_ref, s_ref = rec.syncCPU().copy(), ref.state()
    rec.close()
    world, port = 2, _free_port()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        # two worker processes of this file, each under its own time limit (coreutils timeout: it ends the child, not just the wait)
        procs = [subprocess.Popen(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), str(r), str(world), str(port), d],
                                  cwd=root, env=dict(os.environ, PYTHONPATH=root), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                 for r in range(world)]
        outs = [p.communicate(timeout=330)[0] for p in procs]
        for p, o in zip(procs, outs):
            assert p.returncode == 0, o[-3000:]
        rr = [dict(np.load(os.path.join(d, f"rank{r}.npz"))) for r in range(world)]
    r0 = rr[0]
    assert np.array_equal(r0["recon"], rr[1]["recon"], equal_nan=True)
    for r in rr:
        assert tuple(r["cells"]) == (3, 3)                 # one NormaliseBias per SR iteration, every one on the cell kernels
    err = np.abs(r0["recon"] - v_ref).max() / np.abs(v_ref).max()
    print(f"two ranks vs one, bias on: max rel diff {err:.2e}")
    assert err <= 1e-4 and np.array_equal(r0["recon"] == -1, v_ref == -1)
    assert np.allclose(r0["scale"], s_ref["scale"][r0["order"]], rtol=1e-4)


if __name__ == "__main__":
    _worker(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
