"""Times of SurfaceForcing.apply on the bench mesh (bowl3D h = 0.02), after a warm-up call (best / median of --reps):
  * npg_forcing_apply (k_forcing_local + k_forcing_gather) by device events, with a three-keyframe periodic wind series, a flux and a
    restoring target between keyframes (every channel blends two tables), and the wall time of SurfaceForcing.apply();
  * next to it the parent's host path for ONE change of the forcing: Mesh.surface_load of tau_x and of the flux plus the upload of
    the two vectors (wall time) - what a run had to stop for;
  * the set-up: the constructor, and npg_forcing_surface_matrix by events.
Usage: python tools/forcing_bench.py [--workload L] [--reps R]"""
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
    a = ap.parse_args()
    arch = npg.GPU()
    ctx = arch.ctx
    t0 = time.time()
    # the example's mesh, parameters and velocity tags with a surface FLUX condition: no buoyancy Dirichlet tag, so the flux rows and the
    # restoring matrix are exercised (the example itself pins b at the surface - there only the wind rows are recomputed)
    prm, frc = workloads.example_parameters()
    frc = npg.Forcings(frc.nu, frc.kappa_h, frc.kappa_v, 0.0, 0.0, npg.SurfaceFluxBC(0.0))
    m = npg.Mesh(workloads.bowl_mesh_model(a.workload))
    fed = npg.FEData(m, npg.Spaces(m, u_diri_tags=["bottom", "coastline", "surface"], u_diri_vals=[(0, 0, 0)] * 3,
                                   u_diri_masks=[(True, True, True), (True, True, True), (False, False, True)]))
    ts = npg.BDF2(t_start=0.0, t_stop=1e9, dt=1e-3)
    model = npg.Model(arch, prm, frc, fed, npg.InversionToolkit(arch, fed, prm, frc), npg.EvolutionToolkit(arch, fed, prm, frc, ts), ts)
    print(f"{ctx.name()}; library {os.path.basename(L.LIB_PATH)}; {a.workload}: {m.ncell} cells, {fed.dofs.nu + fed.dofs.np} + {fed.dofs.nb} unknowns; "
          f"set-up {time.time() - t0:.1f} s")
    taus = [lambda x: 1e-2 * np.cos(np.pi * x[..., 1]), lambda x: 2e-2 * np.sin(np.pi * x[..., 0]), lambda x: -1e-2 * np.cos(np.pi * x[..., 1])]
    flux = lambda x: 1e-3 * np.sin(np.pi * x[..., 0])
    has_diri = bool((fed.spaces.b_dof < 0).any())
    kw = {} if has_diri else dict(flux=flux, restoring=(lambda x: 1.0 + x[..., 0] ** 2, npg.ForcingSeries([0.0, 1.0], [0.0, lambda x: x[..., 1]], period=2.0)))
    t0 = time.time()
    sf = npg.SurfaceForcing(model, tau_x=npg.ForcingSeries([0.0, 0.5, 1.0], taus, period=1.5), tau_y=taus[1], **kw)
    print(f"SurfaceForcing: {sf.info()}; constructor {time.time() - t0:.2f} s" + (" (buoyancy Dirichlet surface: wind only)" if has_diri else ""))
    sf.apply(model, 0.3)
    ctx.sync()
    first = (model.inversion.b.to_host(), model.evolution.rhs_flux.to_host())
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        sf.apply(model, 0.3)
        ctx.sync()
        wall.append(time.perf_counter() - t0)
    assert np.array_equal(first[0], model.inversion.b.to_host()) and np.array_equal(first[1], model.evolution.rhs_flux.to_host())
    ev = timed(ctx, lambda: sf.apply(model, 0.3), a.reps)
    print(f"npg_forcing_apply by events: best {ev[0]:.4f} ms, median {ev[1]:.4f} ms of {a.reps}; SurfaceForcing.apply() + sync wall: best "
          f"{min(wall) * 1e3:.3f} ms, median {np.median(wall) * 1e3:.3f} ms")
    if sf.S is not None:
        sm = timed(ctx, lambda: L.check(L.lib().npg_forcing_surface_matrix(sf.h, sf.alpha, sf.S.h)), a.reps)
        print(f"npg_forcing_surface_matrix by events: best {sm[0]:.4f} ms, median {sm[1]:.4f} ms")
    sf.detach()
    # the parent's path for one change of the forcing: two host surface integrals, two uploads
    host = []
    prm, t = model.params, fed.tables
    for _ in range(max(3, a.reps // 4)):
        t0 = time.perf_counter()
        vec = np.zeros(fed.dofs.nu + fed.dofs.np)
        load = m.surface_load(lambda x: prm.alpha * taus[0](x))
        pos = t.u_pos[:, 0]
        vec[pos[pos >= 0]] += load[pos >= 0]
        wind = npg.DeviceVector.from_host(ctx, vec)
        fl = np.zeros(fed.dofs.nb)
        load = m.surface_load(lambda x: prm.alpha * flux(x))[:fed.spaces.nb_nodes]
        fl[t.b_pos[t.b_pos >= 0]] = load[t.b_pos >= 0]
        dev = npg.DeviceVector.from_host(ctx, fl)
        ctx.sync()
        host.append(time.perf_counter() - t0)
        del wind, dev
    print(f"host path (surface_load of tau_x and of the flux + two uploads) wall: best {min(host) * 1e3:.2f} ms, median {np.median(host) * 1e3:.2f} ms")


if __name__ == "__main__":
    main()
