"""Times of the linearised model on the bench mesh (bowl3D h = 0.02) after a few model steps:
  * npg_fe_tangent_rhs (k_tangent_local + the gather) next to npg_fe_advection_rhs (k_advection_local + the same gather) on the same
    engine and state, alternating, by device events - the advection load is the yardstick: both are thread-per-cell, the tangent reads
    twice the nodal data;
  * one LinearizedModel.apply (one inversion from a zero guess at rtol, atol = 0, behind the model's preconditioner), wall time;
  * one implicit_step and one eigenmodes(n = 4) with their counts of applies, inner iterations and inversions, wall time.
Warm-up: every timed shape runs once before its window.  The kernel figures are the best and the median of --reps windows of --inner
calls, and the spread; the solves are the median and the spread of --solve-reps calls.  Lines are written as they come.
Usage: python tools/linearized_bench.py [--workload L] [--preconditioner P] [--steps K] [--reps R] [--inner N] [--solve-reps S] [--dt T]
       [--tol E] [--ncv M] [--maxrestart X] [--out FILE]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import nupgcm_amd as npg  # noqa: E402
from nupgcm_amd import _lib as L, workloads  # noqa: E402


def window(ctx, fn, inner):
    """milliseconds per call over one window of `inner` calls, by device events"""
    ctx.timer_start()
    for _ in range(inner):
        fn()
    return ctx.timer_stop() / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bowl3D_h0.02")
    ap.add_argument("--preconditioner", default="multigrid")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--solve-reps", type=int, default=5)
    ap.add_argument("--dt", type=float, default=100.0)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--ncv", type=int, default=20)
    ap.add_argument("--maxrestart", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    f = open(a.out, "w") if a.out else None

    def say(s):
        print(s, flush=True)
        if f:
            f.write(s + "\n")
            f.flush()
    arch = npg.GPU()
    ctx = arch.ctx
    t0 = time.time()
    model = workloads.example_model(arch, a.workload, preconditioner=a.preconditioner)
    npg.run(model, n_steps=a.steps)
    fed, prm, fe = model.fe_data, model.params, model.evolution.fe
    d, m = fed.dofs, fed.mesh
    say(f"{ctx.name()}; {a.workload}: {m.ncell} cells, P{fed.spaces.b_order} buoyancy, {d.nb} buoyancy rows, {d.nu + d.np} inversion rows; "
        f"preconditioner {a.preconditioner}; set-up + {a.steps} steps {time.time() - t0:.1f} s")
    lin = npg.LinearizedModel(model)
    rng = np.random.default_rng(0)
    db = npg.DeviceVector.from_host(ctx, rng.standard_normal(d.nb))
    dx = lin.invert(db).copy()
    out = npg.DeviceVector(ctx, d.nb)
    b, x = lin.b_base, lin.x_base

    def tangent():
        fe.tangent_rhs(prm.N2, b, x, db, dx, out)

    def advection():
        fe.advection_rhs(L.NPG_BDF2, 1e-3, prm.N2, b, b, x, x, out)
    pieces = [("npg_fe_tangent_rhs", tangent), ("npg_fe_advection_rhs (BDF2, fp64)", advection)]
    for _, fn in pieces:
        fn()
    ctx.sync()
    times = {name: [] for name, _ in pieces}
    for _ in range(a.reps):
        for name, fn in pieces:
            times[name].append(window(ctx, fn, a.inner))
    say(f"kernel windows of {a.inner} calls, {a.reps} windows per figure, alternating")
    for name, _ in pieces:
        t = times[name]
        say(f"{name}: best {min(t):.4f} ms, median {np.median(t):.4f} ms, spread {max(t) - min(t):.4f} ms")
    tt, ta = times[pieces[0][0]], times[pieces[1][0]]
    say(f"tangent load / advection load = {min(tt) / min(ta):.3f} (best), {np.median(tt) / np.median(ta):.3f} (median) - expected within about 2")

    def wall(fn, reps):
        ts = []
        for _ in range(reps):
            ctx.sync()
            t1 = time.perf_counter()
            fn()
            ctx.sync()
            ts.append((time.perf_counter() - t1) * 1e3)
        return ts
    lin.apply(db, out)
    it0 = lin.n_inversion_iterations
    ts = wall(lambda: lin.apply(db, out), a.solve_reps)
    say(f"apply (one inversion at rtol {lin.rtol:g}, atol 0, from a zero guess; {(lin.n_inversion_iterations - it0) // a.solve_reps} Krylov "
        f"iterations): median {np.median(ts):.2f} ms, spread {max(ts) - min(ts):.2f} ms over {a.solve_reps} calls")
    lin.implicit_step(db, a.dt, out)
    ts = wall(lambda: lin.implicit_step(db, a.dt, out), max(2, a.solve_reps // 2))
    say(f"implicit_step dt = {a.dt:g} (rtol {100 * lin.rtol:g}): {lin.last_step['niter']} inner iterations in {lin.last_step['npass']} pass(es): "
        f"median {np.median(ts):.1f} ms, spread {max(ts) - min(ts):.1f} ms")
    t1 = time.perf_counter()
    em = lin.eigenmodes(4, a.dt, ncv=a.ncv, tol=a.tol, maxrestart=a.maxrestart)
    ctx.sync()
    say(f"eigenmodes(n = 4, dt = {a.dt:g}, ncv = {a.ncv}, tol = {a.tol:g}): wall {time.perf_counter() - t1:.1f} s; {em.n_restarts} restart(s), "
        f"{em.n_applies} applies, {em.n_inner} inner iterations, {em.n_inversions} inversions; converged {em.converged.tolist()}")
    say(f"sigma = {em.sigma.tolist()}; residuals = {em.residuals.tolist()}")
    if f:
        f.close()


if __name__ == "__main__":
    main()
