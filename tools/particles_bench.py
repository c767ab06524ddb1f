"""Time of one fused particle step on the bench mesh (bowl3D h = 0.02, 2^20 particles seeded inside the mesh, the state after a few
timesteps), after a warm-up call, by device events, best and median of 20:
  * npg_particles_advance(nsub = 1): k_particles_advance, one launch - the calls follow one another, as a run makes them (the particles
    move on; the cells they remember are warm);
  * next to it, in the same process, the unfused path the library already had, on the four stage points of the first step: four times
    (npg_locator_find + npg_fe_sample(NPG_SAMPLE_U)), eight launches.  The host round trips and the formation of the stage points
    between them are NOT counted, which flatters this baseline.
The share of the step's locations (stages 2, 3, 4 and the end point; stage 1 is carried over) that the remembered cell serves without
an election is counted on the host from one download of the located stage points.
--diffusion adds, after the lines above and in the same process, npg_particles_walk(nsub = 1) (k_particles_walk) from the
same seeds and h: with walls only, and with walls and diffusion - the model's kappa forcings at the vertices, c_d h = 1e-4 - next to
the frozen npg_particles_advance timed above.
Usage: python tools/particles_bench.py [--workload L] [--steps K] [--reps R] [--log2n N] [--diffusion]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import nupgcm_amd as npg  # noqa: E402
from nupgcm_amd import _lib as L, workloads  # noqa: E402
from nupgcm_amd.architectures import DeviceVector  # noqa: E402
from nupgcm_amd.sampling import locator  # noqa: E402


def timed(ctx, fn, reps):
    fn()
    ctx.sync()
    t = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        t.append(ctx.timer_stop())
    return min(t), float(np.median(t))


def seeds_inside(model, n, seed=1):
    loc = npg.PointLocator(model)
    lo, hi = loc.bounding_box
    rng = np.random.default_rng(seed)
    out, have = [], 0
    while have < n:
        p = lo + rng.random((1 << 20, 3)) * (hi - lo)
        p = p[loc.locate(p).valid]
        out.append(p)
        have += len(p)
    return np.vstack(out)[:n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bowl3D_h0.02")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--diffusion", action="store_true")
    a = ap.parse_args()
    arch = npg.GPU()
    ctx = arch.ctx
    t0 = time.time()
    model = workloads.example_model(arch, a.workload)
    npg.run(model, n_steps=a.steps)
    m = model.fe_data.mesh
    n = 1 << a.log2n
    x0 = seeds_inside(model, n)
    umax = float(np.abs(model.state.u).max())
    h = 0.5 * 0.02 / umax                                                # h max|u| = half a cell
    print(f"{ctx.name()}; {a.workload}: {m.ncell} cells; {n} particles inside the mesh; set-up + {a.steps} steps {time.time() - t0:.1f} s; "
          f"max|u| = {umax:.3e}, h = {h:.3e}")
    # the unfused path: stage points of the first step through nan_eval, kept on the device
    lib, x = L.lib(), model.inversion.solver.x
    loc = locator(model)
    u = lambda p: npg.nan_eval(model, "u", p)
    k1 = u(x0)
    y2 = x0 + (0.5 * h) * k1
    k2 = u(y2)
    y3 = x0 + (0.5 * h) * k2
    k3 = u(y3)
    y4 = x0 + h * k3
    k4 = u(y4)
    xp = x0 + (h / 6.0) * (((k1 + 2.0 * k2) + 2.0 * k3) + k4)
    stages = [x0, y2, y3, y4]
    found = [loc.locate(p) for p in stages + [xp]]
    cells = [f.cells for f in found]
    served = sum(int(((cells[k] == cells[k - 1]) & (found[k].lambdas.min(axis=1) >= 1e-8)).sum()) for k in range(1, 5))
    located = sum(int((cells[k] >= 0).sum()) for k in range(1, 5))
    print(f"first step: {served} of {4 * n} locations served by the remembered cell ({served / (4 * n):.4f}); {4 * n - located} not located")
    pv = [DeviceVector.from_host(ctx, p.ravel()) for p in stages]
    lc = [npg.Located(ctx, n) for _ in stages]
    uv = [DeviceVector(ctx, 3 * n) for _ in stages]
    fe = loc.fe

    def unfused():
        for k in range(4):
            L.check(lib.npg_locator_find(loc.h, pv[k].h, n, lc[k].h))
            L.check(lib.npg_fe_sample(fe.h, L.NPG_SAMPLE_U, x.h, lc[k].h, uv[k].h))
    base = timed(ctx, unfused, a.reps)
    tr = npg.ParticleTracker(model, x0, nsub=1)

    def fused():
        L.check(lib.npg_particles_advance(tr.h, tr.fe.h, tr.loc.h, x.h, x.h, 0.0, 1.0, h, 1))
    # the first fused step against the numpy restatement through nan_eval, then the timing
    fused()
    got, st = tr.positions, tr.status
    lost = np.isnan(k1 + k2 + k3 + k4).any(axis=1) | (cells[4] < 0)
    print(f"first fused step against the unfused path: max|dx| = {np.abs(got[~lost] - xp[~lost]).max():.3e}, status equal: "
          f"{np.array_equal(st == 1, lost)}, {int(lost.sum())} lost")
    dev = timed(ctx, fused, a.reps)
    xb = x.copy()
    tb = npg.ParticleTracker(model, x0, nsub=1)

    def blended():
        L.check(lib.npg_particles_advance(tb.h, tb.fe.h, tb.loc.h, xb.h, x.h, 0.0, 1.0, h, 1))
    bl = timed(ctx, blended, a.reps)
    print(f"npg_particles_advance(nsub = 1), frozen, by events: best {dev[0]:.3f} ms, median {dev[1]:.3f} ms of {a.reps} "
          f"({n / dev[0] / 1e3:.1f} Mparticle-steps/s); {int((tr.status == 0).sum())} alive after {a.reps + 2} steps")
    print(f"npg_particles_advance(nsub = 1), blended, by events: best {bl[0]:.3f} ms, median {bl[1]:.3f} ms")
    print(f"4 x (npg_locator_find + npg_fe_sample(U)) by events: best {base[0]:.3f} ms, median {base[1]:.3f} ms")
    print(f"ratio fused / unfused = {dev[0] / base[0]:.2f} (best), {dev[1] / base[1]:.2f} (median)")
    if not a.diffusion:
        return
    frc = model.forcings
    for label, dif in (("walls only", None), ("walls and diffusion", (frc.kappa_h, frc.kappa_v, 1e-4 / h))):
        t1 = time.time()
        tw = npg.ParticleTracker(model, x0, nsub=1, walls=True, diffusion=dif, seed=1)
        setup = time.time() - t1

        def walk():
            L.check(lib.npg_particles_walk(tw.h, tw.fe.h, tw.loc.h, x.h, x.h, 0.0, 1.0, h, 1))
        wk = timed(ctx, walk, a.reps)
        st = tw.status
        print(f"npg_particles_walk(nsub = 1), frozen, {label}, by events: best {wk[0]:.3f} ms, median {wk[1]:.3f} ms of {a.reps} "
              f"({n / wk[0] / 1e3:.1f} Mparticle-steps/s; {wk[0] / dev[0]:.2f} x npg_particles_advance); after {a.reps + 1} steps "
              f"{int((st == 0).sum())} alive, {int((st == 1).sum())} lost, {int((st == 2).sum())} stuck, {int(tw.reflections.sum())} "
              f"reflections; tables and seeds set up in {setup:.1f} s")


if __name__ == "__main__":
    main()
