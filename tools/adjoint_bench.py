"""Times of the adjoint of the linearised model on the bench mesh (bowl3D h = 0.02) after a few model steps:
  * npg_fe_tangent_adjoint (k_tangent_adjoint_local + the two gathers) next to npg_fe_tangent_rhs (k_tangent_local + one gather) on the
    same engine and base state, alternating, by device events - the tangent load is the yardstick: the adjoint writes 40 local planes
    where the tangent writes 10, and gathers through two inverted indices;
  * one LinearizedModel.apply_adjoint beside one LinearizedModel.apply behind the same preconditioner (one inversion each from a zero
    guess at rtol, atol = 0), wall time, with their Krylov iteration counts, and the one-off set-up of the transposed inversion.
Warm-up: every timed shape runs once before its window.  The kernel figures are the best and the median of --reps windows of --inner
calls, and the spread; the solves are the median and the spread of --solve-reps calls, alternating.  Lines are written as they come,
one before every solve: behind Diagonal(1 / h^3) a solve from a zero guess is tens of thousands of restarted-GMRES iterations (hence
the default --rtol 1e-6, the model's own, and the cap --itmax: the library's default cap is 2 n iterations, minutes at this size).
Usage: python tools/adjoint_bench.py [--workload L] [--preconditioner P] [--steps K] [--reps R] [--inner N] [--solve-reps S] [--rtol E]
       [--itmax I] [--vector base|random] [--out FILE]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import nupgcm_amd as npg  # noqa: E402
from nupgcm_amd import workloads  # noqa: E402


def window(ctx, fn, inner):
    """milliseconds per call over one window of `inner` calls, by device events"""
    ctx.timer_start()
    for _ in range(inner):
        fn()
    return ctx.timer_stop() / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bowl3D_h0.02")
    ap.add_argument("--preconditioner", default="diagonal")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--solve-reps", type=int, default=3)
    ap.add_argument("--rtol", type=float, default=1e-6)
    ap.add_argument("--itmax", type=int, default=100000)
    ap.add_argument("--vector", default="base", choices=["base", "random"])
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
    lin = npg.LinearizedModel(model, rtol=a.rtol)
    lin.inv_solver.kwargs["itmax"] = a.itmax
    rng = np.random.default_rng(0)
    db = npg.DeviceVector.from_host(ctx, rng.standard_normal(d.nb))
    dx = npg.DeviceVector.from_host(ctx, rng.standard_normal(d.nu + d.np))
    out, out_x = npg.DeviceVector(ctx, d.nb), npg.DeviceVector(ctx, d.nu + d.np)
    b, x = lin.b_base, lin.x_base

    def adjoint():
        fe.tangent_adjoint(prm.N2, b, x, db, out, out_x)

    def tangent():
        fe.tangent_rhs(prm.N2, b, x, db, dx, out)
    pieces = [("npg_fe_tangent_adjoint", adjoint), ("npg_fe_tangent_rhs", tangent)]
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
    ta, tt = times[pieces[0][0]], times[pieces[1][0]]
    say(f"adjoint load / tangent load = {min(ta) / min(tt):.3f} (best), {np.median(ta) / np.median(tt):.3f} (median) - expected about 2-3")

    def wall(fn):
        ctx.sync()
        t1 = time.perf_counter()
        fn()
        ctx.sync()
        return (time.perf_counter() - t1) * 1e3
    t_setup = wall(lin._adjoint)
    say(f"set-up of the transposed inversion (A', B', their solver; once per LinearizedModel): {t_setup:.1f} ms")
    lin.adj_solver.kwargs["itmax"] = a.itmax
    if a.vector == "base":
        # the solves act on the base buoyancy itself: white noise is a right-hand side that Diagonal(1 / h^3) does not bring to
        # rtol 1e-6 in 100 000 iterations on this mesh (measured: 2.2e-6 after 100 000, 20.9 s)
        db.copy_from(b)
    say(f"the solves act on {'the base buoyancy' if a.vector == 'base' else 'white noise'}")
    ts = {"apply": [], "apply_adjoint": []}
    its = {"apply": 0, "apply_adjoint": 0}
    for rep in range(a.solve_reps + 1):                 # the first round is the warm-up
        for name, fn in (("apply", lin.apply), ("apply_adjoint", lin.apply_adjoint)):
            say(f"{'warm-up' if rep == 0 else 'timed'} {name} (rtol {lin.rtol:g}, at most {a.itmax} iterations) ...")
            it0 = lin.n_inversion_iterations
            try:
                t = wall(lambda: fn(db, out))
            except RuntimeError as e:
                say(f"{name}: the inversion did not converge within the cap: {e}")
                if f:
                    f.close()
                return
            if rep:
                ts[name].append(t)
            its[name] = lin.n_inversion_iterations - it0
            say(f"  {t:.1f} ms, {its[name]} Krylov iterations")
    for name in ts:
        say(f"{name} (one inversion at rtol {lin.rtol:g}, atol 0, from a zero guess; {its[name]} Krylov iterations): median "
            f"{np.median(ts[name]):.2f} ms, spread {max(ts[name]) - min(ts[name]):.2f} ms over {a.solve_reps} calls")
    say(f"apply_adjoint / apply = {np.median(ts['apply_adjoint']) / np.median(ts['apply']):.3f} (median); the adjoint load is "
        f"{100 * np.median(ta) / np.median(ts['apply_adjoint']):.3f} % of an apply_adjoint")
    if f:
        f.close()


if __name__ == "__main__":
    main()
