"""Times of the point sampler on the bench mesh (bowl3D h = 0.02): locate and each field's evaluation for the 256^2 slice and the 256^3
grid (device events around the library calls, after a warm-up call), the bin statistics, and the wall time of save_vtk on the same
model - the only way to get these fields out without the sampler.  Usage: python tools/sampling_bench.py [--workload L] [--nbins N ...]"""
import argparse
import ctypes as C
import os
import sys
import tempfile
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bowl3D_h0.02")
    ap.add_argument("--nbins", type=int, nargs="*", default=[0])
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--no-vtk", action="store_true")
    ap.add_argument("--grid", type=int, default=256)
    a = ap.parse_args()
    arch = npg.GPU()
    ctx = arch.ctx
    t0 = time.time()
    model = workloads.example_model(arch, a.workload)
    npg.run(model, n_steps=a.steps)
    m = model.fe_data.mesh
    print(f"{a.workload}: {m.ncell} cells, {model.fe_data.dofs.nu + model.fe_data.dofs.np} inversion unknowns; set-up + {a.steps} steps {time.time() - t0:.1f} s")
    fe = sampling.device_fe(arch, model.fe_data)
    n = a.grid
    for nb in a.nbins:
        t0 = time.time()
        loc = npg.PointLocator(model, nbins=nb)
        info = loc.info()
        print(f"nbins={nb or 'auto'}: locator built in {time.time() - t0:.2f} s; bins {info['dims']}, entries {info['entries']}, "
              f"mean {info['mean_per_bin']:.1f} / max {info['max_per_bin']} candidates per bin")
        lo, hi = info["lo"], info["hi"]
        X, Z = np.meshgrid(np.linspace(lo[0], hi[0], n), np.linspace(lo[2], hi[2], n), indexing="ij")
        sets = {f"slice y=0 {n}^2": np.stack([X, 0 * X, Z], -1).reshape(-1, 3)}
        Y2, Z2 = np.meshgrid(np.linspace(lo[1], hi[1], n), np.linspace(lo[2], hi[2], n), indexing="ij")
        step = max(1, sampling.CHUNK // (n * n))
        for name, pts in sets.items():
            pv = DeviceVector.from_host(ctx, pts.ravel())
            out = sampling.Located(ctx, len(pts))
            ms = timed(ctx, lambda: L.check(L.lib().npg_locator_find(loc.h, pv.h, len(pts), out.h)))
            line = f"  {name}: locate {ms:.3f} ms ({len(pts) / ms / 1e3:.1f} Mpoints/s, {out.valid.mean():.3f} inside)"
            for f, (code, nc) in sampling._FIELDS.items():
                vec = model.b_vec if f in ("b", "grad_b") else model.inversion.solver.x
                o = DeviceVector(ctx, len(pts) * nc)
                ms = timed(ctx, lambda: L.check(L.lib().npg_fe_sample(fe.h, code, vec.h, out.h, o.h)))
                line += f"; {f} {ms:.3f} ms"
            print(line)
        # the n^3 grid in chunks of whole x-planes (sample_to_grid's chunks): kernel times summed over the chunks
        xs = np.linspace(lo[0], hi[0], n)
        tot = dict(locate=0.0, u=0.0, p=0.0, b=0.0, grad_b=0.0)
        inside = 0
        for i0 in range(0, n, step):
            i1 = min(n, i0 + step)
            pts = np.empty((i1 - i0, n * n, 3))
            pts[:, :, 0], pts[:, :, 1], pts[:, :, 2] = xs[i0:i1, None], Y2.ravel(), Z2.ravel()
            pts = pts.reshape(-1, 3)
            pv = DeviceVector.from_host(ctx, pts.ravel())
            out = sampling.Located(ctx, len(pts))
            tot["locate"] += timed(ctx, lambda: L.check(L.lib().npg_locator_find(loc.h, pv.h, len(pts), out.h)), reps=2)
            inside += int(out.valid.sum())
            for f, (code, nc) in sampling._FIELDS.items():
                vec = model.b_vec if f in ("b", "grad_b") else model.inversion.solver.x
                o = DeviceVector(ctx, len(pts) * nc)
                tot[f] += timed(ctx, lambda: L.check(L.lib().npg_fe_sample(fe.h, code, vec.h, out.h, o.h)), reps=2)
        print(f"  grid {n}^3 ({n ** 3 / 1e6:.1f} M points, {inside / n ** 3:.3f} inside, chunks of {step * n * n}): "
              + "; ".join(f"{k} {v:.2f} ms" for k, v in tot.items()))
        del loc
    t0 = time.time()
    g = npg.sample_to_grid(model, n, n, n)
    t1 = time.time()
    Psi, U = npg.barotropic_streamfunction(g)
    print(f"sample_to_grid({n}^3, u and b) end to end, host transfers included: {t1 - t0:.2f} s wall; depth max {npg.depth(g).max():.4f}, "
          f"|Psi| max {np.nanmax(np.abs(Psi)):.3e}")
    if not a.no_vtk:
        with tempfile.TemporaryDirectory() as d:
            t0 = time.time()
            npg.save_vtk(model, os.path.join(d, "state.vtu"))
            print(f"save_vtk on the same model: {time.time() - t0:.1f} s wall, {os.path.getsize(os.path.join(d, 'state.vtu')) / 1e6:.0f} MB")


if __name__ == "__main__":
    main()
