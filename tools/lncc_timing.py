"""One P4 slice-to-volume pass of the IRTK schedule (280 slices) with CC, with NMI (--useNMI) and with the windowed cross correlation
(--useLNCC) at radius 3 and 7, every similarity on the GPU, in one process: reconstructs once, then registers from the true transformations; prints wall time,
evaluations, the ratio to the CC pass and the schedule's own split (SVR_REG_TIMING=1 on stderr).
usage: lncc_timing.py [p4|s8 ...]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("SVR_REG_TIMING", "1")
import numpy as np  # noqa: E402

from fetalreconstruction_amd import engine, geometry as geo, host, phantom  # noqa: E402
from tests.twins.reconstruction import irtkReconstruction  # noqa: E402

for which in sys.argv[1:] or ["p4"]:
    P = phantom.problem_p4() if which == "p4" else phantom.problem_s8()
    rec = engine.Reconstruction(0)
    engine.sync_gpu(rec, P)
    d = irtkReconstruction(rec, P.ns, max_intensity=P.max_intensity, min_intensity=P.min_intensity)
    d.SetSmoothingParameters(150, 0.02)
    d.reconstruct_iteration(2)
    vol = rec.syncCPU().reshape(P.vsize[::-1])
    rattr = geo.ImageAttributes(*P.vsize, *P.vdim)
    T = P.slice_t.reshape(-1, 4, 4).astype(np.float64)
    cases = (("cc", None), ("nmi", None), ("lncc", 3), ("lncc", 7))
    per_eval = {}
    for rep in range(2):                                  # the second round is the measurement (first calls allocate)
        for sim, radius in cases:
            t0 = time.time()
            Tn, nev = host.SliceToVolumeRegistration(rec, P.slices, P.slice_attr, T, rattr, vol, similarity=sim, radius=radius)
            wall = time.time() - t0
            per_eval[(sim, radius)] = wall / nev
            print(f"{which} {sim}{'' if radius is None else ' R=' + str(radius)}: {P.ns} slices, wall {wall:.3f} s, {nev} similarity evaluations, "
                  f"{1e6 * wall / nev:.2f} us each", flush=True)
    for sim, radius in cases[1:]:
        print(f"{which} {sim}{'' if radius is None else ' R=' + str(radius)} / cc, wall per evaluation: {per_eval[(sim, radius)] / per_eval[('cc', None)]:.2f}x", flush=True)
