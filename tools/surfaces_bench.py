"""Times of the maps on buoyancy surfaces on the bench mesh (bowl3D h = 0.02): 256 x 256 columns, 32 levels, after a warm-up call:
  * the set-up on the host (npg_surfaces_create: the tiling of the columns) and the number of segments;
  * npg_surfaces_compute (k_surfaces_scan + k_surfaces_fields) by device events, and the wall time of BuoyancySurfaces.compute() (the
    launches and the download of the maps);
  * next to it, in the same process and on the same state, the same maps the way they are made today: sample_to_grid on a 256^3 grid
    (u and b), downloaded, and the uppermost crossing of every level found in numpy by linear interpolation between the grid's z
    levels - and how far that z lies from the exact crossing.
Usage: python tools/surfaces_bench.py [--workload L] [--steps K] [--reps R] [--columns N] [--levels N] [--grid N] [--out FILE]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import nupgcm_amd as npg  # noqa: E402
from nupgcm_amd import _lib as L, workloads  # noqa: E402


def timed(ctx, fn, reps):
    fn()
    ctx.sync()
    t = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        t.append(ctx.timer_stop())
    return min(t), float(np.median(t))


def grid_surfaces(g, levels):
    """the uppermost crossing of each level along z of a GridSamples, by linear interpolation between grid points: (nlev, nx, ny)"""
    B = g["b"]
    out = np.full((len(levels),) + B.shape[:2], np.nan)
    for k, Bk in enumerate(levels):
        d = B - Bk
        with np.errstate(invalid="ignore"):
            above = d >= 0.0
        ok = np.isfinite(d[:, :, 1:]) & np.isfinite(d[:, :, :-1])
        flip = ok & (above[:, :, 1:] != above[:, :, :-1])
        any_ = flip.any(axis=2)
        top = flip.shape[2] - 1 - np.argmax(flip[:, :, ::-1], axis=2)           # the uppermost interval with a flip
        i, j = np.nonzero(any_)
        kk = top[i, j]
        d0, d1 = d[i, j, kk], d[i, j, kk + 1]
        out[k, i, j] = g.z[kk] + (g.z[kk + 1] - g.z[kk]) * d0 / (d0 - d1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bowl3D_h0.02")
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--columns", type=int, default=256)
    ap.add_argument("--levels", type=int, default=32)
    ap.add_argument("--grid", type=int, default=256)
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
    m = model.fe_data.mesh
    say(f"{ctx.name()}; {a.workload}: {m.ncell} cells, P{model.fe_data.spaces.b_order} buoyancy; set-up + {a.steps} steps {time.time() - t0:.1f} s")
    npg.sampling.locator(model)
    ends = npg.BuoyancySurfaces(model, [0.0], nx=64, ny=64).compute()
    lo, hi = np.nanmin(np.minimum(ends.B_bot, ends.B_top)), np.nanmax(np.maximum(ends.B_bot, ends.B_top))
    levels = np.linspace(lo, hi, a.levels + 2)[1:-1]
    t0 = time.perf_counter()
    S = npg.BuoyancySurfaces(model, levels, nx=a.columns, ny=a.columns)
    setup = time.perf_counter() - t0
    info = S.info
    say(f"npg_surfaces_create: {info['columns']} columns ({info['dry']} dry) tiled into {info['segments']} segments, at most "
        f"{info['max_per_column']} per column, in {setup * 1e3:.1f} ms on the host (one thread)")
    M = S.compute()                                                      # warm-up
    ctx.sync()
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        M2 = S.compute()
        wall.append(time.perf_counter() - t0)
    assert np.array_equal(M.z, M2.z, equal_nan=True) and np.array_equal(M.u, M2.u, equal_nan=True)      # the same bits on every call
    x, b = model.inversion.solver.x, model.b_vec
    N2 = float(model.params.N2)
    dev = timed(ctx, lambda: L.check(L.lib().npg_surfaces_compute(S.h, x.h, b.h, N2, L.ptr(S.levels), len(S.levels), S._out.h, S._cols.h)),
                a.reps)
    ncross = int((M.ncross > 0).sum())
    say(f"levels {levels[0]:.4e} .. {levels[-1]:.4e}: {ncross} of {M.ncross.size} (level, column) pairs crossed, at most {int(M.ncross.max())} "
        f"crossings of one level in one column; status counts (crossed, outcropped, grounded, dry) {np.bincount(M.status.ravel(), minlength=4).tolist()}")
    say(f"npg_surfaces_compute ({a.columns} x {a.columns} columns, {a.levels} levels) by events: best {dev[0]:.3f} ms, median {dev[1]:.3f} ms of "
        f"{a.reps} ({info['segments'] / dev[0] / 1e3:.1f} Msegments/s); BuoyancySurfaces.compute() wall (launches + download of "
        f"{9 * M.z.size * 8 / 1e6:.1f} MB): best {min(wall) * 1e3:.2f} ms, median {np.median(wall) * 1e3:.2f} ms")
    # the same maps from a sampled grid
    t0 = time.perf_counter()
    g = npg.sample_to_grid(model, a.columns, a.columns, a.grid, fields=("u", "b"))
    t_grid = time.perf_counter() - t0
    t0 = time.perf_counter()
    zg = grid_surfaces(g, levels)
    t_np = time.perf_counter() - t0
    both = np.isfinite(zg) & np.isfinite(M.z)
    dz = np.abs(zg - M.z)[both]
    say(f"sample_to_grid({a.columns} x {a.columns} x {a.grid}; u, b) {t_grid:.2f} s + numpy crossings {t_np:.2f} s = "
        f"{(t_grid + t_np) / min(wall):.0f} x BuoyancySurfaces.compute(); crossed in both {int(both.sum())}, only on the grid "
        f"{int((np.isfinite(zg) & ~np.isfinite(M.z)).sum())}, only exact {int((~np.isfinite(zg) & np.isfinite(M.z)).sum())}; "
        f"|z_grid - z_exact| median {np.median(dz):.2e}, max {dz.max():.2e} (grid spacing {g.z[1] - g.z[0]:.2e})")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
