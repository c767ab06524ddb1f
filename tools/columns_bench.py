"""Times of the column integrals on the bench mesh (bowl3D h = 0.02): 256 x 256 columns, after a warm-up call:
  * the set-up on the host (npg_columns_create: the tiling of the columns) and the number of segments;
  * npg_columns_compute (k_column_segments + k_column_fold) by device events, and the wall time of ColumnIntegrals.compute() (the
    launches and the download of the 31 maps).  The split between the two kernels comes from a kernel trace of this tool
    (rocprofv3 --kernel-trace --stats -- python tools/columns_bench.py --reps 5);
  * (a) GridDiagnostics.compute() over the same columns (256 z levels, a trapezoid per column) in the same process on the same state,
    and how far its H, U, V lie from the exact integrals;
  * (b) what the device path replaces: the download of the state, and - with --host, in a process of its own on the CPU() architecture,
    no toolkits and a zero state (the cost does not depend on the values) - the host library's npg_columns_compute over the same columns.
Usage: python tools/columns_bench.py [--workload L] [--steps K] [--reps R] [--columns N] [--host] [--out FILE]"""
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


def walled(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return min(t) * 1e3, float(np.median(t)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bowl3D_h0.02")
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--columns", type=int, default=256)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    arch = npg.CPU() if a.host else npg.GPU()
    ctx = arch.ctx
    t0 = time.time()
    steps = 0 if a.host else a.steps
    if a.host:                                                           # the mesh, the spaces and zero vectors: no toolkits
        from types import SimpleNamespace
        prm, frc = workloads.example_parameters()
        fed = workloads.example_fe_data(workloads.bowl_mesh_model(a.workload))
        xv = npg.DeviceVector(ctx, fed.dofs.nu + fed.dofs.np)
        model = SimpleNamespace(arch=arch, fe_data=fed, params=prm, forcings=frc, b_vec=npg.DeviceVector(ctx, fed.dofs.nb),
                                inversion=SimpleNamespace(solver=SimpleNamespace(x=xv)), step_index=1)
    else:
        model = workloads.example_model(arch, a.workload)
    if steps:
        npg.run(model, n_steps=steps)
    m = model.fe_data.mesh
    name = f"host library, {os.cpu_count()} CPUs visible, OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')}" if a.host else ctx.name()
    say(f"{name}; {a.workload}: {m.ncell} cells, P{model.fe_data.spaces.b_order} buoyancy; set-up + {steps} steps {time.time() - t0:.1f} s")
    npg.sampling.locator(model)
    t0 = time.perf_counter()
    CI = npg.ColumnIntegrals(model, nx=a.columns, ny=a.columns)
    setup = time.perf_counter() - t0
    info = CI.info
    say(f"npg_columns_create: {info['columns']} columns ({info['dry']} dry) tiled into {info['segments']} segments, at most "
        f"{info['max_per_column']} per column, in {setup * 1e3:.1f} ms on the host")
    out = CI.compute_raw()
    x, b = model.inversion.solver.x, model.b_vec
    call = lambda: L.check(L.lib().npg_columns_compute(CI.h, x.h, b.h, CI._out.h, None))
    if a.host:
        w = walled(call, a.reps)
        say(f"npg_columns_compute on the host ({a.columns} x {a.columns} columns): best {w[0]:.2f} ms, median {w[1]:.2f} ms of {a.reps} "
            f"({info['segments'] / w[0] / 1e3:.1f} Msegments/s)")
    else:
        assert np.array_equal(out, CI.compute_raw(), equal_nan=True)                     # the same bits on every call
        dev = timed(ctx, call, a.reps)
        wall = walled(CI.compute, a.reps)
        say(f"npg_columns_compute ({a.columns} x {a.columns} columns) by events: best {dev[0]:.3f} ms, median {dev[1]:.3f} ms of {a.reps} "
            f"({info['segments'] / dev[0] / 1e3:.1f} Msegments/s); ColumnIntegrals.compute() wall (launches + download of "
            f"{out.size * 8 / 1e6:.1f} MB): best {wall[0]:.2f} ms, median {wall[1]:.2f} ms")
        G = npg.GridDiagnostics(model, x=CI.x, y=CI.y, nz=256)
        g = G.compute()
        gwall = walled(G.compute, a.reps)
        M = CI.compute()
        wet = ~np.isnan(M.H) & (g.H > 0)
        say(f"(a) GridDiagnostics.compute() over the same columns, 256 z levels: wall best {gwall[0]:.2f} ms, median {gwall[1]:.2f} ms; "
            f"against the exact integrals max|dH| = {np.abs(g.H - M.H)[wet].max():.2e} of {np.nanmax(M.H):.3f}, max|dU| = "
            f"{np.abs(g.U - M.U[..., 0])[wet].max():.2e} of {np.nanmax(np.abs(M.U[..., 0])):.2e}, max|dV| = "
            f"{np.abs(g.V - M.U[..., 1])[wet].max():.2e} of {np.nanmax(np.abs(M.U[..., 1])):.2e}")
        down = walled(lambda: (x.to_host(), b.to_host()), a.reps)
        say(f"(b) the download of the state ({(x.n + b.n) * 8 / 1e6:.1f} MB): best {down[0]:.2f} ms, median {down[1]:.2f} ms "
            f"(the host library's npg_columns_compute: this tool with --host)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
