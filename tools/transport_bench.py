"""Times of the tracers' transport operator on the bench mesh (bowl3D h = 0.02) after a few model steps, by device events:
  * the pieces of TracerTransport.set_flow: npg_tracers_transport_update (k_transport_velocity), npg_tracers_transport_matrix
    (k_transport_matrix), npg_tracers_transport_load for one tracer (k_transport_load + the gather);
  * the yardsticks, in the same process on the same state and alternating with them: npg_tracers_isoneutral_matrix (k_redi_matrix -
    the same rows, pairs, binary searches and row adds, four tables and seven products per pair where C reads three and makes three)
    and npg_fe_assemble_matrix(NPG_MAT_KH);
  * one GMRES iteration on T: a solve cut off at --gmres-its iterations, divided by the iterations it took;
  * the iteration count and wall time of an ideal-age equilibrium (S = 1, Dirichlet 0, lambda = 0, scale 1) at rtol 1e-8.
Warm-up: every timed shape is launched once before its window.  Each figure is the best and the median of --reps windows of --inner
calls, and the spread; the pieces and their yardsticks alternate, so a drift of the machine shows in both.
Usage: python tools/transport_bench.py [--workload L] [--steps K] [--reps R] [--inner N] [--gmres-its I] [--itmax M] [--out FILE]"""
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
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--gmres-its", type=int, default=300)
    ap.add_argument("--itmax", type=int, default=30000)
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
    fed, prm, ev = model.fe_data, model.params, model.evolution
    m = fed.mesh
    say(f"{ctx.name()}; {a.workload}: {m.ncell} cells, P{fed.spaces.b_order} buoyancy, {fed.dofs.nb} rows, nq = {len(m.q_w)}; set-up + "
        f"{a.steps} steps {time.time() - t0:.1f} s; windows of {a.inner} calls, {a.reps} windows per figure, alternating")
    tt = npg.TracerTransport(model, [dict(name="age", source=1.0, dirichlet=0.0)])
    iso = npg.PassiveTracers(model, [dict(name="t")], isoneutral=npg.Isoneutral(1.0, 0.5, 0.1))
    iso.update_isoneutral(model.b_vec)
    lib = L.lib()
    x = model.inversion.solver.x
    Kh = ev.fe.new_matrix("b")
    dec = L.as_f64(tt.decay)

    def update():
        L.check(lib.npg_tracers_transport_update(tt.h, x.h, 1.0))

    def matrix():
        L.check(lib.npg_tracers_transport_matrix(tt.h, tt.C.h))

    def load():
        L.check(lib.npg_tracers_transport_load(tt.h, tt.kappa_hat, L.ptr(dec), None, None, tt.g.h))

    def kiso():
        L.check(lib.npg_tracers_isoneutral_matrix(iso.h, iso.Kiso.h))

    def kh():
        ev.fe.assemble(L.NPG_MAT_KH, Kh)
    pieces = [("npg_tracers_transport_update", update), ("npg_tracers_transport_matrix", matrix), ("npg_tracers_transport_load (K = 1)", load),
              ("npg_tracers_isoneutral_matrix", kiso), ("npg_fe_assemble_matrix(NPG_MAT_KH)", kh)]
    for _, fn in pieces:
        fn()
    ctx.sync()
    times = {name: [] for name, _ in pieces}
    for _ in range(a.reps):
        for name, fn in pieces:
            times[name].append(window(ctx, fn, a.inner))
    for name, _ in pieces:
        t = times[name]
        say(f"{name}: best {min(t):.4f} ms, median {np.median(t):.4f} ms, spread {max(t) - min(t):.4f} ms")
    tm, tk, th = (times[pieces[i][0]] for i in (1, 3, 4))
    say(f"C assembly / K_iso assembly = {min(tm) / min(tk):.3f} (best), {np.median(tm) / np.median(tk):.3f} (median) - expected <= 1.1; "
        f"C assembly / NPG_MAT_KH assembly = {min(tm) / min(th):.3f} (best), {np.median(tm) / np.median(th):.3f} (median)")
    pe = tt.peclet()
    say(f"flow: umax {tt.info()['umax']:.3e}, cell Peclet number median {np.median(pe):.3e}, largest {pe.max():.3e}")
    # one GMRES iteration on T: a solve cut off after --gmres-its iterations (warm-up solve first), from c = 0 each time
    T, P, g, c = tt.operator(0), tt._P[0.0], tt.load(0), tt.view(0)
    per = []
    for rep in range(4):
        c.fill(0.0)
        ctx.sync()
        t1 = time.perf_counter()
        st = tt.ws.solve(T, g, c, P, atol=0.0, rtol=1e-30, itmax=a.gmres_its)
        ctx.sync()
        if rep:
            per.append((time.perf_counter() - t1) * 1e3 / max(1, st["niter"]))
    say(f"one GMRES({tt.memory}) iteration on T (fp64 basis, Jacobi): best {min(per):.4f} ms, median {np.median(per):.4f} ms "
        f"({st['niter']} iterations per solve, 3 solves)")
    c.fill(0.0)
    ctx.sync()
    t1 = time.perf_counter()
    tt.equilibrium(rtol=1e-8, itmax=a.itmax)
    ctx.sync()
    wall = time.perf_counter() - t1
    st, (rn, r0) = tt.stats[0], tt.residual[0]
    v = tt.values(0)
    say(f"ideal-age equilibrium, rtol 1e-8 from c = 0: solved {st['solved']}, {st['niter']} iterations in {st['passes']} pass(es), wall "
        f"{wall:.2f} s; ||P r|| / ||P r0|| = {rn / r0:.3e}; age {v.min():.3f} .. {v.max():.3f}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
