"""Times of the batched CG (npg_cg_multi_solve) on the bench mesh (bowl3D h = 0.02) after a few model steps:
  * one BatchedCgWorkspace.solve of K = 1, 2, 4, 8 right-hand sides against the evolution matrix A = M + theta (Kh + Kv) with its Jacobi P;
  * next to it, in the same process and alternating with it, the parent path: K npg_cg_solve calls on K CgWorkspaces, as
    PassiveTracers makes them - the same right-hand sides, the same warm starts (restored before every solve in both paths, by the
    same stacked copy), the model's tolerances;
  * one PassiveTracers step (fused right-hand side + solves), batched against unbatched, at K = 4 and K = 8.
The results of the two paths are compared bit by bit once per shape.  Warm-up: every timed shape runs once before its windows.  Each
figure is the best and the median of --reps windows of --inner calls, by device events.
Usage: python tools/cg_multi_bench.py [--workload L] [--steps K] [--reps R] [--inner N] [--out FILE]"""
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
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
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
    ev = model.evolution
    A, P, kw = ev.solver.A, ev.solver.P, dict(ev.solver.kwargs)
    n = A.shape[0]
    say(f"{ctx.name()}; {a.workload}: evolution matrix {n} rows, {A.nnz} entries ({A.nnz / n:.1f} per row, {12 * A.nnz / 1e6:.0f} MB of "
        f"(col, val)); P {type(P).__name__}; solver kwargs {kw}; set-up + {a.steps} steps {time.time() - t0:.1f} s; windows of {a.inner} "
        f"solves, {a.reps} windows per figure, batched and single alternating")
    rng = np.random.default_rng(20261018)
    # the buoyancy's own last system: its right-hand side and the warm start it had (the b of the step before), so a column needs
    # the iterations a tracer needs in a model step
    y0, b0 = ev.solver.y.to_host(), model._prev["b_prev"].to_host()
    for K in (1, 2, 4, 8):
        # right-hand sides and warm starts of K tracer-like columns: the buoyancy's own system, scaled and perturbed per column
        Y = np.concatenate([y0 * (1.0 + 0.1 * k) for k in range(K)])
        X0 = np.concatenate([b0 * (1.0 + 0.1 * k) * (1.0 + 1e-6 * rng.standard_normal(n)) for k in range(K)])
        y, x0 = npg.DeviceVector.from_host(ctx, Y), npg.DeviceVector.from_host(ctx, X0)
        xs, xb = npg.DeviceVector(ctx, K * n), npg.DeviceVector(ctx, K * n)
        singles = [npg.CgWorkspace(ctx, n) for _ in range(K)]
        yv, xv = [y.view(k * n, n) for k in range(K)], [xs.view(k * n, n) for k in range(K)]
        wb = npg.BatchedCgWorkspace(ctx, n, K)

        def single():
            xs.copy_from(x0)
            for k in range(K):
                singles[k].solve(A, yv[k], xv[k], P, **kw)

        def batched():
            xb.copy_from(x0)
            wb.solve(A, y, xb, P, **kw)
        single(), batched()                                        # warm-up of both shapes
        ctx.sync()
        same = bool(np.array_equal(xs.to_host().view(np.uint64), xb.to_host().view(np.uint64)))
        it = [s["niter"] for s in wb.stats]
        assert it == [w.stats["niter"] for w in singles]
        tb, tsg = [], []
        for _ in range(a.reps):
            tb.append(window(ctx, batched, a.inner))
            tsg.append(window(ctx, single, a.inner))
        say(f"K = {K}: niter {it}; bits equal: {same}; batched best {min(tb):.3f} ms, median {np.median(tb):.3f} ms; {K} x npg_cg_solve best "
            f"{min(tsg):.3f} ms, median {np.median(tsg):.3f} ms; batched / single = {min(tb) / min(tsg):.3f} (best), "
            f"{np.median(tb) / np.median(tsg):.3f} (median)")
        del singles, wb
    xp = model._prev["x_prev"]
    for K in (4, 8):
        specs = [dict(name=f"t{k}", initial=model.state.b * (1.0 + 0.1 * k), dirichlet=0.1 * (k + 1), gamma=model.params.N2 * (1.0 + 0.05 * k),
                      source=0.5 * k, flux=1e-3 * (k + 1)) for k in range(K)]
        trs = {mode: npg.PassiveTracers(model, specs, batched=mode) for mode in (False, True)}
        for tr in trs.values():
            tr.step(model, xp)                                     # warm-up
        ctx.sync()
        same = bool(np.array_equal(trs[False].c.to_host().view(np.uint64), trs[True].c.to_host().view(np.uint64)))
        t = {False: [], True: []}
        for _ in range(a.reps):
            for mode in (True, False):
                t[mode].append(window(ctx, lambda tr=trs[mode]: tr.step(model, xp), a.inner))
        it = [s["niter"] for s in trs[True].stats[-1]]
        say(f"PassiveTracers.step K = {K}: niter of the last step {it}; bits equal after the first step: {same}; batched best "
            f"{min(t[True]):.3f} ms, median {np.median(t[True]):.3f} ms; unbatched best {min(t[False]):.3f} ms, median "
            f"{np.median(t[False]):.3f} ms; batched / unbatched = {min(t[True]) / min(t[False]):.3f} (best), "
            f"{np.median(t[True]) / np.median(t[False]):.3f} (median)")
        del trs
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
