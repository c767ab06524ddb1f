"""Times of the fused multi-tracer right-hand side on the bench mesh (bowl3D h = 0.02) after a few model steps:
  * one npg_tracers_rhs for K = 1, 2, 4, 8 tracers (k_tracers_local + k_tracers_gather), by device events;
  * next to it, in the same process, on the same flow and alternating with it, K calls of the unchanged npg_fe_evolution_rhs
    (k_advection_local + k_gather_rows each): what K tracers cost without the fusion;
  * the bytes each form has to move at least, counted from the shapes (geometry, DoF tables, scattered velocity and tracer values as if
    each were read once per cell, local vectors written and read once), and the rate that makes over the best time.
Every tracer has a background gradient, a source and a flux, so the fused call does all of its work; in both element modes.
Warm-up: every timed shape is launched once before the window.  Each figure is the best and the median of --reps windows of --inner
calls; fused and unfused windows alternate, so a drift of the machine shows in both.
Usage: python tools/tracers_bench.py [--workload L] [--steps K] [--reps R] [--inner N] [--out FILE]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import nupgcm_amd as npg  # noqa: E402
from nupgcm_amd import _lib as L, workloads  # noqa: E402
from nupgcm_amd.evolution import evolution_parameter  # noqa: E402


def window(ctx, fn, inner):
    """milliseconds per call over one window of `inner` calls, by device events"""
    ctx.timer_start()
    for _ in range(inner):
        fn()
    return ctx.timer_stop() / inner


def min_bytes(ncell, nq, nloc, n_b, n_inv, K, fused):
    """the least traffic of K right-hand sides: per pass-1 launch the geometry (13 doubles), the velocity DoF table (30 int32) and the
    two velocity vectors; per tracer the DoF table (nloc int32), two tracer vectors, the local vector written and read, the inverted
    index (int32) and the row written with rhs_diff and flux read"""
    launches = 1 if fused else K
    per_launch = ncell * (13 * 8 + 30 * 4) + 2 * n_inv * 8
    per_tracer = ncell * nloc * 4 + 2 * n_b * 8 + 2 * ncell * nloc * 8 + ncell * nloc * 4 + 3 * n_b * 8
    return launches * per_launch + K * per_tracer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bowl3D_h0.02")
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    arch = npg.GPU()
    ctx = arch.ctx
    t0 = time.time()
    model = workloads.example_model(arch, a.workload)
    npg.run(model, n_steps=a.steps)
    fed, prm, ts, ev = model.fe_data, model.params, model.timestepper, model.evolution
    m = fed.mesh
    nb, ninv, nloc, nq = fed.dofs.nb, model.inversion.solver.x.n, (10 if fed.spaces.b_order == 2 else 4), len(m.q_w)
    say(f"{ctx.name()}; {a.workload}: {m.ncell} cells, P{fed.spaces.b_order} buoyancy, {nb} rows, nq = {nq}; set-up + {a.steps} steps "
        f"{time.time() - t0:.1f} s; windows of {a.inner} calls, {a.reps} windows per figure, fused and unfused alternating")
    theta = evolution_parameter(prm, ts)
    x, xp = model.inversion.solver.x, model._prev["x_prev"]
    b, bp = model.b_vec, model._prev["b_prev"]
    yb = npg.DeviceVector(ctx, nb)
    scheme = L.NPG_BDF2

    def unfused_one():
        ev.fe.evolution_rhs(scheme, ts.dt, prm.N2, theta, b, bp, x, xp, ev.rhs_diff, ev.rhs_flux, ev.rhs_M, ev.rhs_h, ev.rhs_v, yb)
    rng = np.random.default_rng(20261018)
    for prec in ("fp64", "fp32"):
        ev.fe.set_precision(prec)
        for K in (1, 2, 4, 8):
            specs = [dict(name=f"t{k}", initial=model.state.b * (1.0 + 0.1 * k), dirichlet=0.1 * (k + 1), gamma=prm.N2 * (1.0 + 0.05 * k),
                          source=0.5 * k, flux=1e-3 * (k + 1)) for k in range(K)]
            tr = npg.PassiveTracers(model, specs)
            tr.c_prev.upload(tr.c.to_host() * (1.0 + 1e-3 * rng.standard_normal(tr.c.n)))

            def fused():
                tr.rhs(scheme, ts.dt, theta, x, xp)

            def unfused():
                for _ in range(K):
                    unfused_one()
            fused(), unfused()                                         # warm-up of both shapes
            ctx.sync()
            tf, tu = [], []
            for _ in range(a.reps):
                tf.append(window(ctx, fused, a.inner))
                tu.append(window(ctx, unfused, a.inner))
            bf, bu = min_bytes(m.ncell, nq, nloc, nb, ninv, K, True), min_bytes(m.ncell, nq, nloc, nb, ninv, K, False)
            say(f"{prec} K = {K}: npg_tracers_rhs best {min(tf):.4f} ms, median {np.median(tf):.4f} ms (spread {max(tf) - min(tf):.4f}); "
                f"{K} x npg_fe_evolution_rhs best {min(tu):.4f} ms, median {np.median(tu):.4f} ms (spread {max(tu) - min(tu):.4f}); "
                f"fused / unfused = {min(tf) / min(tu):.3f} (best), {np.median(tf) / np.median(tu):.3f} (median); least traffic "
                f"{bf / 1e6:.1f} MB -> {bf / (min(tf) * 1e-3) / 1e9:.0f} GB/s fused, {bu / 1e6:.1f} MB -> {bu / (min(tu) * 1e-3) / 1e9:.0f} GB/s unfused")
            del tr
    ev.fe.set_precision("fp64")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
