"""Times of the grid diagnostics on the bench mesh (bowl3D h = 0.02) with a 256^3 grid, after a warm-up call:
  * the path through the host: sample_to_grid(n^3, fields=("u", "b", "grad_b")) + the host diagnostics, wall time, and the device
    time of its kernels alone (k_locate + k_sample of u, b, grad b, summed over sample_to_grid's chunks);
  * GridDiagnostics.compute(): wall time, and the device time of npg_fe_grid_integrals (k_grid_integrals + k_grid_fold and the
    download of the axes for their check) by events.  The split between the two kernels comes from a kernel trace of this program.
The two results are compared before anything is printed as a time.  Usage: python tools/diagnostics_bench.py [--workload L] [--grid N]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import nupgcm_amd as npg  # noqa: E402
from nupgcm_amd import _lib as L, sampling, workloads  # noqa: E402
from nupgcm_amd.architectures import DeviceVector  # noqa: E402


def timed(ctx, fn, reps=3):
    fn()
    ctx.sync()
    best = 1e30
    for _ in range(reps):
        ctx.timer_start()
        fn()
        best = min(best, ctx.timer_stop())
    return best


def host_path(model, n):
    g = npg.sample_to_grid(model, n, n, n, fields=("u", "b", "grad_b"))
    Psi, U = npg.barotropic_streamfunction(g)
    psi_bar, v_int, b_bar = npg.overturning_streamfunction(g)
    N2_bar = npg.average_stratification(g, -0.5, 1, alpha=model.params.alpha)
    return dict(Psi=Psi, U=U, psi_bar=psi_bar, v_int=v_int, b_bar=b_bar, N2_bar=N2_bar, H=npg.depth(g), width=npg.zonal_width(g))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bowl3D_h0.02")
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-host-path", action="store_true", help="time GridDiagnostics only (for a kernel trace)")
    a = ap.parse_args()
    arch = npg.GPU()
    ctx = arch.ctx
    n = a.grid
    t0 = time.time()
    model = workloads.example_model(arch, a.workload)
    npg.run(model, n_steps=a.steps)
    m = model.fe_data.mesh
    print(f"{a.workload}: {m.ncell} cells; set-up + {a.steps} steps {time.time() - t0:.1f} s; grid {n}^3 = {n ** 3 / 1e6:.1f} M points")
    gd = npg.GridDiagnostics(model, n, n, n)
    r = gd.compute()                                                     # warm-up
    ctx.sync()
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        r = gd.compute()
        wall.append(time.perf_counter() - t0)
    call = lambda: L.check(L.lib().npg_fe_grid_integrals(gd.fe.h, gd.loc.h, model.inversion.solver.x.h, model.b_vec.h, float(model.params.N2),
                                                         gd._axes.h, n, n, n, gd._col.h, gd._zon.h))
    dev = timed(ctx, call, reps=a.reps)
    print(f"GridDiagnostics.compute(): wall {min(wall) * 1e3:.2f} ms (best of {a.reps}; median {np.median(wall) * 1e3:.2f} ms); "
          f"npg_fe_grid_integrals by events {dev:.3f} ms ({n ** 3 / dev / 1e3:.0f} Mpoints/s); {r.count_z.sum() / n ** 3:.3f} of the points inside; "
          f"|Psi| max {np.nanmax(np.abs(r.Psi)):.6e}, |psi_bar| max {np.nanmax(np.abs(r.psi_bar)):.6e}")
    if a.skip_host_path:
        return
    host_path(model, n)                                                  # warm-up
    t0 = time.perf_counter()
    h = host_path(model, n)
    t_host = time.perf_counter() - t0
    t0 = time.perf_counter()
    npg.sample_to_grid(model, n, n, n, fields=("u", "b", "grad_b"))
    t_grid = time.perf_counter() - t0
    for name, got in (("H", r.H), ("width", r.width), ("U", r.U), ("Psi", r.Psi), ("v_int", r.v_int), ("psi_bar", r.psi_bar), ("b_bar", r.b_bar),
                      ("N2_bar", r.N2_bar(-0.5, 1))):
        assert np.array_equal(np.isnan(got), np.isnan(h[name])), name
        err, scale = np.nanmax(np.abs(got - h[name])), np.nanmax(np.abs(h[name]))
        print(f"  {name}: fused vs host path max difference {err:.2e} of max {scale:.2e}")
        assert err <= 1e-10 * scale, name
    print(f"sample_to_grid({n}^3, u, b, grad_b) + host diagnostics: {t_host:.3f} s wall (sample_to_grid alone {t_grid:.3f} s)")
    # the device time inside that path: its kernels alone, over sample_to_grid's chunks
    loc, fe = gd.loc, gd.fe
    lo, hi = loc.bounding_box
    xs, ys, zs = (np.linspace(lo[d], hi[d], n) for d in range(3))
    Y2, Z2 = np.meshgrid(ys, zs, indexing="ij")
    step = max(1, sampling.CHUNK // (n * n))
    tot = dict(locate=0.0, u=0.0, b=0.0, grad_b=0.0)
    for i0 in range(0, n, step):
        i1 = min(n, i0 + step)
        pts = np.empty((i1 - i0, n * n, 3))
        pts[:, :, 0], pts[:, :, 1], pts[:, :, 2] = xs[i0:i1, None], Y2.ravel(), Z2.ravel()
        pts = pts.reshape(-1, 3)
        pv = DeviceVector.from_host(ctx, pts.ravel())
        out = sampling.Located(ctx, len(pts))
        tot["locate"] += timed(ctx, lambda: L.check(L.lib().npg_locator_find(loc.h, pv.h, len(pts), out.h)), reps=2)
        for f in ("u", "b", "grad_b"):
            code, nc = sampling._FIELDS[f]
            vec = model.b_vec if f in ("b", "grad_b") else model.inversion.solver.x
            o = DeviceVector(ctx, len(pts) * nc)
            tot[f] += timed(ctx, lambda: L.check(L.lib().npg_fe_sample(fe.h, code, vec.h, out.h, o.h)), reps=2)
    ksum = sum(tot.values())
    print("  kernels of that path by events: " + "; ".join(f"{k} {v:.3f} ms" for k, v in tot.items()) + f"; sum {ksum:.3f} ms")
    print(f"ratios: host path wall / compute() wall = {t_host / min(wall):.0f}x; npg_fe_grid_integrals / (k_locate + k_sample) = {dev / ksum:.2f}")


if __name__ == "__main__":
    main()
