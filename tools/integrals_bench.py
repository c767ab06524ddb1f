"""Times of the mesh integrals on the bench mesh (bowl3D h = 0.02), after a warm-up call:
  * npg_integrals_compute (k_cell_integrals + k_integrals_fold) by device events, and the wall time of MeshIntegrals.compute()
    (the launch, the fold and the download of NPG_NINT doubles);
  * next to it, in the same process, npg_fe_advection_rhs by events: the pass over the same [component][cell] tables that every
    timestep makes - the yardstick.
Usage: python tools/integrals_bench.py [--workload L] [--steps K] [--reps R]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import nupgcm_amd as npg  # noqa: E402
from nupgcm_amd import _lib as L, workloads  # noqa: E402
from nupgcm_amd.architectures import DeviceVector  # noqa: E402


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
    print(f"{ctx.name()}; {a.workload}: {m.ncell} cells, P{model.fe_data.spaces.b_order} buoyancy; set-up + {a.steps} steps {time.time() - t0:.1f} s")
    mi = npg.MeshIntegrals(model)
    r = mi.compute()                                                     # warm-up
    ctx.sync()
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        r2 = mi.compute()
        wall.append(time.perf_counter() - t0)
    assert np.array_equal(r.raw, r2.raw)                                 # the same bits on every call
    x, b = model.inversion.solver.x, model.b_vec
    dev = timed(ctx, lambda: L.check(L.lib().npg_integrals_compute(mi.h, x.h, b.h, int(mi.full_stress), mi._out.h)), a.reps)
    out = DeviceVector(ctx, b.n)
    fe = model.evolution.fe
    adv = timed(ctx, lambda: fe.advection_rhs(L.NPG_BDF2, model.timestepper.dt, model.params.N2, b, b, x, x, out), a.reps)
    print(r)
    print(f"npg_integrals_compute by events: best {dev[0]:.3f} ms, median {dev[1]:.3f} ms of {a.reps} ({m.ncell / dev[0] / 1e3:.1f} Mcells/s); "
          f"MeshIntegrals.compute() wall: best {min(wall) * 1e3:.3f} ms, median {np.median(wall) * 1e3:.3f} ms")
    print(f"npg_fe_advection_rhs by events: best {adv[0]:.3f} ms, median {adv[1]:.3f} ms")
    print(f"ratio npg_integrals_compute / npg_fe_advection_rhs = {dev[0] / adv[0]:.2f} (best), {dev[1] / adv[1]:.2f} (median)")


if __name__ == "__main__":
    main()
