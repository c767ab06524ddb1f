"""Times of the boundary integrals on the bench mesh (bowl3D h = 0.02), after a warm-up call, by device events (best / median of
--reps):
  * npg_boundary_compute (k_boundary_faces + k_boundary_fold) with and without the per-face table, and the wall time of
    BoundaryIntegrals.compute() (the launches and the download of 24 doubles per group);
  * next to it, in the same process, npg_integrals_compute: the pass over all the cells - the yardstick.
The workgroup of k_boundary_faces is a compile-time constant (NPG_BND_BLOCK, csrc/boundary_core.h): to compare another width, build
the library with EXTRA=-DNPG_BND_BLOCK=64 under tools/ and run this tool again with NPG_AB_LIB pointing at it.
Usage: python tools/boundary_bench.py [--workload L] [--steps K] [--reps R]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import nupgcm_amd as npg  # noqa: E402
from nupgcm_amd import _lib as L, workloads  # noqa: E402


def timed(ctx, fn, reps):
    fn()
    ctx.sync()
    t = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        t.append(ctx.timer_stop())
    return min(t), float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bowl3D_h0.02")
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    arch = npg.GPU()
    ctx = arch.ctx
    t0 = time.time()
    model = workloads.example_model(arch, a.workload)
    npg.run(model, n_steps=a.steps)
    m = model.fe_data.mesh
    print(f"{ctx.name()}; library {os.path.basename(L.LIB_PATH)}; {a.workload}: {m.ncell} cells, P{model.fe_data.spaces.b_order} buoyancy; "
          f"set-up + {a.steps} steps {time.time() - t0:.1f} s")
    t0 = time.time()
    bi = npg.BoundaryIntegrals(model)
    print(f"BoundaryIntegrals: {len(bi.faces)} faces in groups {dict(zip(bi.groups, np.bincount(bi.face_group).tolist()))}; set-up {time.time() - t0:.2f} s")
    r = bi.compute(faces=True)                                           # warm-up
    ctx.sync()
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        r2 = bi.compute()
        wall.append(time.perf_counter() - t0)
    assert all(np.array_equal(r.raw[g], r2.raw[g], equal_nan=True) for g in r.groups)   # the same bits on every call
    x, b = model.inversion.solver.x, model.b_vec
    lib = L.lib()
    tot = timed(ctx, lambda: L.check(lib.npg_boundary_compute(bi.h, x.h, b.h, int(bi.full_stress), bi._out.h, None)), a.reps)
    fac = timed(ctx, lambda: L.check(lib.npg_boundary_compute(bi.h, x.h, b.h, int(bi.full_stress), bi._out.h, bi._faces_out.h)), a.reps)
    mi = npg.MeshIntegrals(model)
    vol = timed(ctx, lambda: L.check(lib.npg_integrals_compute(mi.h, x.h, b.h, int(mi.full_stress), mi._out.h)), a.reps)
    print(r)
    print(f"npg_boundary_compute by events, totals only: best {tot[0]:.4f} ms, median {tot[1]:.4f} ms of {a.reps} ({len(bi.faces) / tot[0] / 1e3:.2f} Mfaces/s); "
          f"with the per-face table: best {fac[0]:.4f} ms, median {fac[1]:.4f} ms; BoundaryIntegrals.compute() wall: best {min(wall) * 1e3:.3f} ms, "
          f"median {np.median(wall) * 1e3:.3f} ms")
    print(f"npg_integrals_compute by events: best {vol[0]:.4f} ms, median {vol[1]:.4f} ms")
    print(f"ratio npg_boundary_compute / npg_integrals_compute = {tot[0] / vol[0]:.3f} (best), {tot[1] / vol[1]:.3f} (median)")


if __name__ == "__main__":
    main()
