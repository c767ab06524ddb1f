"""Times of the closure derivatives of the linearised model:
  * npg_fe_tangent_diffusion, npg_fe_tangent_eddy and npg_fe_tangent_eddy_adjoint (full stress) on the bench mesh (bowl3D h = 0.02)
    after a few model steps, next to npg_fe_tangent_rhs and npg_fe_tangent_adjoint on the same engine and base state - the two loads of
    the parent commit, whose kernels this commit leaves as they were, are the yardsticks - in alternating windows, by device events;
  * one LinearizedModel.apply with closures="tangent" beside one with closures="frozen" on a model with both closures on (--apply-workload,
    behind --preconditioner; one inversion each from a zero guess at rtol, atol = 0), wall time, with their Krylov iteration counts and
    the set-up each constructor costs (tangent: the own A at nu(b_base), its preconditioner, the base flow solved once more).
Warm-up: every timed shape runs once before its window.  The kernel figures are the best and the median of --reps windows of --inner
calls, and the spread; the applies are the median and the spread of --solve-reps calls, alternating.  No time is a pass condition.
Usage: python tools/closures_bench.py [--workload L] [--apply-workload L] [--preconditioner P] [--steps K] [--reps R] [--inner N]
       [--solve-reps S] [--rtol E] [--out FILE]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import nupgcm_amd as npg  # noqa: E402
from nupgcm_amd import workloads  # noqa: E402

KAPPA_C, N2MIN = 5.0, 1.0


def window(ctx, fn, inner):
    """milliseconds per call over one window of `inner` calls, by device events"""
    ctx.timer_start()
    for _ in range(inner):
        fn()
    return ctx.timer_stop() / inner


def closure_model(arch, label, preconditioner):
    """the example model on the named mesh with both closures on, BDF1"""
    prm, frc = workloads.example_parameters()
    frc.conv_param = npg.ConvectionParameterization(KAPPA_C, N2MIN, True)
    frc.eddy_param = npg.EddyParameterization(prm.f, N2MIN, True)
    fed = workloads.example_fe_data(workloads.bowl_mesh_model(label))
    ts = npg.BDF1(t_start=0.0, t_stop=1e9, dt=1e-3)
    kw = dict(block_nodes=False) if preconditioner == "dense_inverse" else {}
    inv = npg.InversionToolkit(arch, fed, prm, frc, preconditioner=preconditioner, **kw)
    return npg.Model(arch, prm, frc, fed, inv, npg.EvolutionToolkit(arch, fed, prm, frc, ts), ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bowl3D_h0.02")
    ap.add_argument("--apply-workload", default="bowl3D_h0.1")
    ap.add_argument("--preconditioner", default="dense_inverse")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--solve-reps", type=int, default=5)
    ap.add_argument("--rtol", type=float, default=1e-10)
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
    model = workloads.example_model(arch, a.workload)
    npg.run(model, n_steps=a.steps)
    fed, prm, fe = model.fe_data, model.params, model.evolution.fe
    d, m = fed.dofs, fed.mesh
    say(f"{ctx.name()}; {a.workload}: {m.ncell} cells, P{fed.spaces.b_order} buoyancy, {d.nb} buoyancy rows, {d.nu + d.np} inversion rows; "
        f"set-up + {a.steps} steps {time.time() - t0:.1f} s")
    rng = np.random.default_rng(0)
    db = npg.DeviceVector.from_host(ctx, rng.standard_normal(d.nb))
    dx = npg.DeviceVector.from_host(ctx, rng.standard_normal(d.nu + d.np))
    out, out_x = npg.DeviceVector(ctx, d.nb), npg.DeviceVector(ctx, d.nu + d.np)
    b, x = model.b_vec.copy(), model.inversion.solver.x.copy()
    a2e2 = prm.alpha ** 2 * prm.eps ** 2
    pieces = [("npg_fe_tangent_diffusion", lambda: fe.tangent_diffusion(KAPPA_C, N2MIN, prm.alpha, prm.N2, b, db, out)),
              ("npg_fe_tangent_eddy", lambda: fe.tangent_eddy(a2e2, True, N2MIN, prm.alpha, prm.N2, b, x, db, out_x)),
              ("npg_fe_tangent_eddy_adjoint", lambda: fe.tangent_eddy_adjoint(a2e2, True, N2MIN, prm.alpha, prm.N2, b, x, dx, out)),
              ("npg_fe_tangent_rhs", lambda: fe.tangent_rhs(prm.N2, b, x, db, dx, out)),
              ("npg_fe_tangent_adjoint", lambda: fe.tangent_adjoint(prm.N2, b, x, db, out, out_x))]
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
    med = {name: float(np.median(t)) for name, t in times.items()}
    for name in ("npg_fe_tangent_diffusion", "npg_fe_tangent_eddy", "npg_fe_tangent_eddy_adjoint"):
        say(f"{name} / npg_fe_tangent_rhs = {med[name] / med['npg_fe_tangent_rhs']:.3f}, / npg_fe_tangent_adjoint = "
            f"{med[name] / med['npg_fe_tangent_adjoint']:.3f} (medians)")
    del model, db, dx, out, out_x, b, x

    def wall(fn):
        ctx.sync()
        t1 = time.perf_counter()
        r = fn()
        ctx.sync()
        return (time.perf_counter() - t1) * 1e3, r
    t0 = time.time()
    model = closure_model(arch, a.apply_workload, a.preconditioner)
    npg.run(model, n_steps=a.steps)
    d = model.fe_data.dofs
    say(f"{a.apply_workload} with both closures on (kappa_c {KAPPA_C}, N2min {N2MIN}): {model.fe_data.mesh.ncell} cells, {d.nb} buoyancy rows, "
        f"{d.nu + d.np} inversion rows; preconditioner {a.preconditioner}; set-up + {a.steps} steps {time.time() - t0:.1f} s")
    lins = {}
    for mode in ("tangent", "frozen"):
        t, lins[mode] = wall(lambda: npg.LinearizedModel(model, rtol=a.rtol, closures=mode))
        say(f"LinearizedModel(closures={mode!r}): {t:.1f} ms")
    db = npg.DeviceVector.from_host(ctx, np.random.default_rng(0).standard_normal(d.nb))
    out = npg.DeviceVector(ctx, d.nb)
    ts = {mode: [] for mode in lins}
    its = {}
    for rep in range(a.solve_reps + 1):                 # the first round is the warm-up
        for mode, lin in lins.items():
            it0 = lin.n_inversion_iterations
            t, _ = wall(lambda: lin.apply(db, out))
            its[mode] = lin.n_inversion_iterations - it0
            if rep:
                ts[mode].append(t)
    for mode in lins:
        say(f"apply, closures={mode!r} (one inversion at rtol {a.rtol:g}, atol 0, from a zero guess; {its[mode]} Krylov iterations): median "
            f"{np.median(ts[mode]):.2f} ms, spread {max(ts[mode]) - min(ts[mode]):.2f} ms over {a.solve_reps} calls")
    say(f"apply tangent / apply frozen = {np.median(ts['tangent']) / np.median(ts['frozen']):.3f} (median)")
    if f:
        f.close()


if __name__ == "__main__":
    main()
