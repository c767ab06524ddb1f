"""Times of InteriorForcing on the bench mesh (bowl3D h = 0.02), after a warm-up call (best / median of --reps), with a sponge over
roughly a tenth of the cells (the northern tenth by centroid) and a three-keyframe periodic source over all cells, evaluated between
two keyframes (both series blend two tables):
  * npg_interior_apply (k_interior_local + k_interior_gather), npg_interior_matrix and npg_interior_budget by device events, the
    extra vector pass of evolve() (rhs_flux + (c / dt) rhs_src), and the constructor (wall);
  * next to it the only alternative without the feature: the load evaluated on the host (numpy over the same points, one keyframe
    blend, the contraction with the shape values and the scatter into the rows) plus the upload of one vector per step (wall);
  * the time step of the same model without the forcing (wall per step of run(), after two warm-up steps), for the ratio.
Usage: python tools/interior_bench.py [--workload L] [--reps R] [--steps S]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bowl3D_h0.02")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    arch = npg.GPU()
    ctx = arch.ctx
    t0 = time.time()
    prm, frc = workloads.example_parameters()
    m = npg.Mesh(workloads.bowl_mesh_model(a.workload))
    fed = npg.FEData(m, npg.Spaces(m, u_diri_tags=["bottom", "coastline", "surface"], u_diri_vals=[(0, 0, 0)] * 3,
                                   u_diri_masks=[(True, True, True), (True, True, True), (False, False, True)],
                                   b_diri_tags=["coastline", "surface"], b_diri_vals=[0.0, 0.0]))
    ts = npg.BDF2(t_start=0.0, t_stop=1e9, dt=1e-3)
    model = npg.Model(arch, prm, frc, fed, npg.InversionToolkit(arch, fed, prm, frc), npg.EvolutionToolkit(arch, fed, prm, frc, ts), ts)
    print(f"{ctx.name()}; library {os.path.basename(L.LIB_PATH)}; {a.workload}: {m.ncell} cells, {fed.dofs.nu + fed.dofs.np} + {fed.dofs.nb} unknowns; "
          f"set-up {time.time() - t0:.1f} s")
    # the time step without the forcing
    npg.run(model, n_steps=2)
    ctx.sync()
    t0 = time.perf_counter()
    npg.run(model, n_steps=a.steps)
    ctx.sync()
    step = (time.perf_counter() - t0) / a.steps
    print(f"time step without the forcing: {step * 1e3:.2f} ms wall per step ({a.steps} steps after 2 warm-up steps)")
    yc = m.geo_coords[m.cell_geo][:, :, 1].mean(axis=1)
    cells = yc > np.quantile(yc, 0.9)
    gamma = lambda x: 5.0 * np.clip((x[..., 1] - np.quantile(yc, 0.9)) / (yc.max() - np.quantile(yc, 0.9)), 0.0, 1.0) ** 2 + 0.1
    qs = [lambda x: 1e-2 * np.cos(np.pi * x[..., 1]), lambda x: 2e-2 * np.sin(np.pi * x[..., 0]) * x[..., 2], lambda x: -1e-2 * np.cos(np.pi * x[..., 1])]
    target = npg.ForcingSeries([0.0, 1.0], [lambda x: x[..., 2], lambda x: 1.2 * x[..., 2]], period=2.0)
    t0 = time.time()
    sponge = np.where(cells[:, None], gamma(m.quad_points()), 0.0)
    f = npg.InteriorForcing(model, source=npg.ForcingSeries([0.0, 0.5, 1.0], qs, period=1.5), restoring=(sponge, target))
    print(f"InteriorForcing: {f.info()}, sponge cells {int(cells.sum())}; constructor {time.time() - t0:.2f} s")
    f.apply(model, 0.3)
    ctx.sync()
    first = f.rhs_src.to_host()
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        f.apply(model, 0.3)
        ctx.sync()
        wall.append(time.perf_counter() - t0)
    assert np.array_equal(first, f.rhs_src.to_host())
    ev = timed(ctx, lambda: f.apply(model, 0.3), a.reps)
    print(f"npg_interior_apply by events: best {ev[0]:.4f} ms, median {ev[1]:.4f} ms of {a.reps}; InteriorForcing.apply() + sync wall: best "
          f"{min(wall) * 1e3:.3f} ms, median {np.median(wall) * 1e3:.3f} ms")
    mix = npg.DeviceVector(ctx, fed.dofs.nb)
    ax = timed(ctx, lambda: mix.lincomb([1.0, 2.0 / 3.0], [model.evolution.rhs_flux, f.rhs_src]), a.reps)
    print(f"evolve()'s extra pass rhs_flux + (c / dt) rhs_src by events: best {ax[0]:.4f} ms, median {ax[1]:.4f} ms")
    print(f"apply + extra pass against the time step: {(ev[1] + ax[1]) / (step * 1e3) * 100:.4f} % (medians)")
    mt = timed(ctx, lambda: L.check(L.lib().npg_interior_matrix(f.h, f.R.h)), a.reps)
    print(f"npg_interior_matrix by events: best {mt[0]:.4f} ms, median {mt[1]:.4f} ms")
    bd = timed(ctx, lambda: L.check(L.lib().npg_interior_budget(f.h, f._key, f._w, model.b_vec.h, f._out.h)), a.reps)
    print(f"npg_interior_budget by events: best {bd[0]:.4f} ms, median {bd[1]:.4f} ms; budget(t = 0.3) = {f.budget(model, 0.3)}")
    # the alternative without the feature: the load on the host over the same points, and one upload per step
    Nb = np.asarray(m.N2 if fed.spaces.b_order == 2 else m.N1)
    rows = fed.tables.b_pos[fed.spaces.cell_b_nodes]
    bdv = np.where(rows < 0, fed.spaces.b_diri_val[fed.spaces.cell_b_nodes], 0.0)
    qt, tt, g, W = f.key_tables["source"], f.key_tables["target"], f.gamma_table, f.weights
    host = []
    for _ in range(max(3, a.reps // 4)):
        t0 = time.perf_counter()
        x = 0.4 * qt[0] + 0.6 * qt[1] + g * ((0.7 * tt[0] + 0.3 * tt[1]) - bdv[f.cells] @ Nb.T)
        loc = (W * x) @ Nb
        vec = np.zeros(fed.dofs.nb)
        r = rows[f.cells]
        np.add.at(vec, r[r >= 0], loc[r >= 0])
        dev = npg.DeviceVector.from_host(ctx, vec)
        ctx.sync()
        host.append(time.perf_counter() - t0)
        del dev
    print(f"host path (numpy load over the same points + one upload) wall: best {min(host) * 1e3:.2f} ms, median {np.median(host) * 1e3:.2f} ms")
    f.detach()


if __name__ == "__main__":
    main()
