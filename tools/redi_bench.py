"""Times of the isoneutral mixing of the passive tracers on the bench mesh (bowl3D h = 0.02) after a few model steps, by device events:
  * the per-step pieces: npg_tracers_isoneutral_update (k_redi_update), npg_tracers_isoneutral_matrix (k_redi_matrix), and
    A_c.combine + A_c.inv_diag;
  * the yardsticks, in the same process on the same state and alternating with them: npg_fe_assemble_matrix(NPG_MAT_KH) - the same
    rows and pairs, one product per pair where K_iso evaluates four - and the convection closure's per-step kappa_v refresh
    (npg_fe_update_kappa_convection + the NPG_MAT_KV assembly);
  * the per-timestep slowdown of a 4-tracer isoneutral run against the same run with level mixing: wall time of --run-steps steps of
    run() on two models of their own, after a warm-up step.
Warm-up: every timed shape is launched once before its window.  Each figure is the best and the median of --reps windows of --inner
calls, and the spread; the pieces and their yardsticks alternate, so a drift of the machine shows in both.
Usage: python tools/redi_bench.py [--workload L] [--steps K] [--reps R] [--inner N] [--run-steps S] [--out FILE]"""
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


def specs4(model):
    b = model.state.b
    return [dict(name=f"t{k}", initial=b * (1.0 + 0.1 * k), source=0.1 * k) for k in range(4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bowl3D_h0.02")
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--run-steps", type=int, default=5)
    ap.add_argument("--kappa", type=float, default=1.0)
    ap.add_argument("--slope-max", type=float, default=0.5)
    ap.add_argument("--bz-min", type=float, default=0.1)
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
    fed, prm, ts, ev, frc = model.fe_data, model.params, model.timestepper, model.evolution, model.forcings
    m = fed.mesh
    say(f"{ctx.name()}; {a.workload}: {m.ncell} cells, P{fed.spaces.b_order} buoyancy, {fed.dofs.nb} rows, nq = {len(m.q_w)}; set-up + "
        f"{a.steps} steps {time.time() - t0:.1f} s; windows of {a.inner} calls, {a.reps} windows per figure, alternating")
    iso = npg.Isoneutral(a.kappa, a.slope_max, a.bz_min)
    tr = npg.PassiveTracers(model, specs4(model), isoneutral=iso)
    theta = evolution_parameter(prm, ts)
    lib = L.lib()
    Kh, Kv = ev.fe.new_matrix("b"), ev.fe.new_matrix("b")
    cp = frc.conv_param
    kc, n2min = (cp.kappa_c, cp.N2min) if cp.is_on else (1.0, 0.1)

    def update():
        L.check(lib.npg_tracers_isoneutral_update(tr.h, float(prm.N2), model.b_vec.h))

    def matrix():
        L.check(lib.npg_tracers_isoneutral_matrix(tr.h, tr.Kiso.h))

    def combine():
        tr.A.combine(1.0, ev.M, theta, tr.Kiso, ev.Kv)
        tr.A.inv_diag(tr.P.diag)

    def kh():
        ev.fe.assemble(L.NPG_MAT_KH, Kh)

    def kv_refresh():
        ev.fe.update_kappa_convection(kc, n2min, prm.alpha, prm.N2, model.b_vec)
        ev.fe.assemble(L.NPG_MAT_KV, Kv)
    pieces = [("npg_tracers_isoneutral_update", update), ("npg_tracers_isoneutral_matrix", matrix), ("combine + inv_diag", combine),
              ("npg_fe_assemble_matrix(NPG_MAT_KH)", kh), ("kappa_v refresh (closure + NPG_MAT_KV)", kv_refresh)]
    kv_keep = None
    if not cp.is_on:                                           # the closure's refresh overwrites kappa_v: put the model's table back after
        kv_keep = frc.kappa_v
    for _, fn in pieces:
        fn()
    ctx.sync()
    times = {name: [] for name, _ in pieces}
    for _ in range(a.reps):
        for name, fn in pieces:
            times[name].append(window(ctx, fn, a.inner))
    if kv_keep is not None:
        ev.fe.set_coeff("kappa_v", kv_keep)
    for name, _ in pieces:
        t = times[name]
        say(f"{name}: best {min(t):.4f} ms, median {np.median(t):.4f} ms, spread {max(t) - min(t):.4f} ms")
    i = tr.isoneutral_info()
    say(f"floored {i['floored']} and clipped {i['clipped']} of {i['points']} points (slope_max {a.slope_max}, bz_min {a.bz_min})")
    say(f"K_iso assembly / NPG_MAT_KH assembly = {min(times[pieces[1][0]]) / min(times[pieces[3][0]]):.3f} (best), "
        f"{np.median(times[pieces[1][0]]) / np.median(times[pieces[3][0]]):.3f} (median); per step update + K_iso + combine = "
        f"{sum(min(times[p[0]]) for p in pieces[:3]):.4f} ms against the closure's refresh {min(times[pieces[4][0]]):.4f} ms")
    del tr
    # the slowdown of a 4-tracer run: two models of their own, a warm-up step each, then --run-steps steps timed by the wall clock
    walls = {}
    for mode in ("level", "isoneutral"):
        mm = workloads.example_model(arch, a.workload)
        npg.run(mm, n_steps=1)
        mm.tracers = npg.PassiveTracers(mm, specs4(mm), isoneutral=iso if mode == "isoneutral" else None)
        npg.run(mm, n_steps=1)
        ctx.sync()
        per = []
        for _ in range(a.run_steps):
            t1 = time.perf_counter()
            npg.run(mm, n_steps=1)
            ctx.sync()
            per.append(time.perf_counter() - t1)
        walls[mode] = per
        its = [[s["niter"] for s in st] for st in mm.tracers.stats[-a.run_steps:]]
        say(f"4 tracers, {mode} mixing: per step best {min(per) * 1e3:.2f} ms, median {np.median(per) * 1e3:.2f} ms, spread "
            f"{(max(per) - min(per)) * 1e3:.2f} ms over {a.run_steps} steps; tracer CG iterations per step {its}")
        del mm
    say(f"per-timestep slowdown isoneutral / level = {np.median(walls['isoneutral']) / np.median(walls['level']):.3f} (median), "
        f"{min(walls['isoneutral']) / min(walls['level']):.3f} (best)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
