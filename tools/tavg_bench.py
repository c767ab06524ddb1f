"""Times of TimeAverages on the bench mesh (bowl3D h = 0.02), after a warm-up call (device events around 10 calls, per call; best /
median of --reps such windows):
  * npg_tavg_accumulate means only (k_tavg_means alone) and with co-moments (k_tavg_comoments + k_tavg_means); the co-moment launch is
    the difference of the two (the means launch is the same in both), with the bytes each moves and the fraction of the HBM
    specification (8 TB/s) that implies;
  * the same with the node table in MESH order (ordered=False): what ordering the gathers by x_inv position is worth;
  * next to it the parent's only route to the same result: the download of x and b plus the numpy recurrence on the host (wall time);
  * the wall time of run() steps with and without model.averages, in alternating blocks.
Usage: python tools/tavg_bench.py [--workload L] [--reps R] [--steps S]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import nupgcm_amd as npg  # noqa: E402
from nupgcm_amd import _lib as L, workloads  # noqa: E402
from nupgcm_amd.averages import _PA, _PB  # noqa: E402

HBM_SPEC = 8.0e12       # bytes / s


INNER = 10              # calls between one pair of events: the queue stays fed, the launch latency of a single call drops out


def timed(ctx, fn, reps):
    """(best, median) ms per call of `reps` windows of INNER calls each"""
    fn()
    ctx.sync()
    t = []
    for _ in range(reps):
        ctx.timer_start()
        for _ in range(INNER):
            fn()
        t.append(ctx.timer_stop() / INNER)
    return min(t), float(np.median(t))


def bytes_moved(ta):
    """(co-moment launch, means launch): ten doubles read and written per table node, a value and a mean gathered per free position, the
    five table entries; two doubles read and one written per entry of [x_inv | b]"""
    iu, ib = ta._table
    nsel = len(ta.sel)
    gathers = int((iu >= 0).sum() + (ib[0] >= 0).sum() + ((ib[1] >= 0) & (ib[1] != ib[0])).sum())
    return nsel * (20 * 8 + 5 * 4) + 2 * 8 * gathers, 3 * 8 * (ta.n_inv + ta.n_b)


def report(ctx, model, label, reps, **kw):
    x, b = model.inversion.solver.x, model.b_vec
    ta = npg.TimeAverages(model, weight="steps", **kw)
    ta.add_sample(x, b, 1.0)
    both = timed(ctx, lambda: ta.add_sample(x, b, 1.0), reps)
    cb, mb = bytes_moved(ta)
    print(f"{label}: {len(ta.sel)} table nodes, {ta.nbytes / 1e6:.1f} MB held; co-moments + means by events: best {both[0]:.4f} ms, median "
          f"{both[1]:.4f} ms of {reps}; {(cb + mb) / 1e6:.1f} MB per call = {(cb + mb) / (both[0] * 1e-3) / HBM_SPEC:.3f} of the HBM spec")
    ta.detach()
    return both, cb, mb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bowl3D_h0.02")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    arch = npg.GPU()
    ctx = arch.ctx
    t0 = time.time()
    model = workloads.example_model(arch, a.workload)                                      # the headline configuration of bench.py
    fed = model.fe_data
    m = fed.mesh
    n_inv, n_b = fed.dofs.nu + fed.dofs.np, fed.dofs.nb
    print(f"{ctx.name()}; library {os.path.basename(L.LIB_PATH)}; {a.workload}: {m.ncell} cells, {m.nn} P2 nodes, {n_inv} + {n_b} unknowns; "
          f"set-up {time.time() - t0:.1f} s")
    rng = np.random.default_rng(1)
    x, b = model.inversion.solver.x, model.b_vec
    x.upload(rng.standard_normal(n_inv))
    b.upload(rng.standard_normal(n_b))
    # means only
    tm = npg.TimeAverages(model, covariances=False, weight="steps")
    tm.add_sample(x, b, 1.0)
    means = timed(ctx, lambda: tm.add_sample(x, b, 1.0), a.reps)
    mb = 3 * 8 * (n_inv + n_b)
    print(f"means only (k_tavg_means): best {means[0]:.4f} ms, median {means[1]:.4f} ms of {a.reps}; {mb / 1e6:.1f} MB = "
          f"{mb / (means[0] * 1e-3) / HBM_SPEC:.3f} of the HBM spec")
    tm.detach()
    for label, kw in (("table ordered by x_inv position", {}), ("table in mesh order", dict(ordered=False))):
        both, cb, _ = report(ctx, model, label, a.reps, **kw)
        co = both[0] - means[0]
        print(f"    co-moment launch = both - means only: {co:.4f} ms; {cb / 1e6:.1f} MB = {cb / (co * 1e-3) / HBM_SPEC:.3f} of the HBM spec")
    # the parent's route: download, numpy recurrence
    ta = npg.TimeAverages(model, weight="steps")
    iu, ib = (t.astype(np.int64) for t in ta._table)
    mx, mbv, Cm, W = np.zeros(n_inv), np.zeros(n_b), np.zeros((10, len(ta.sel))), 1.0
    host = []
    for _ in range(max(3, a.reps // 4)):
        t0 = time.perf_counter()
        xh, bh = x.to_host(), b.to_host()
        t1 = time.perf_counter()
        W1 = W + 1.0
        r, q = 1.0 / W1, W / W1
        dx, db = xh - mx, bh - mbv
        d = [np.where(iu[c] >= 0, dx[np.maximum(iu[c], 0)], 0.0) for c in range(3)]
        d0, d1 = (np.where(ib[c] >= 0, db[np.maximum(ib[c], 0)], 0.0) for c in range(2))
        d.append(np.where(ib[0] == ib[1], d0, 0.5 * (d0 + d1)))
        for p in range(10):
            Cm[p] = Cm[p] + (q * d[_PA[p]]) * d[_PB[p]]
        mx, mbv, W = mx + r * dx, mbv + r * db, W1
        host.append((time.perf_counter() - t0, t1 - t0))
    ta.detach()
    print(f"host route (download of x and b, numpy recurrence) wall: best {min(h[0] for h in host) * 1e3:.1f} ms, of which the download "
          f"{min(h[1] for h in host) * 1e3:.1f} ms")
    # run() with and without, alternating blocks
    x.fill(0.0)
    b.fill(0.0)
    npg.run(model, n_steps=3)                                                              # warm-up: BDF2's first step, graph captures
    ta = npg.TimeAverages(model)
    ta.detach()
    block = max(1, a.steps // 2)
    for rnd in range(2):
        for with_avg in (False, True):
            model.averages = ta if with_avg else None
            ctx.sync()
            t0 = time.perf_counter()
            npg.run(model, n_steps=block)
            dt = time.perf_counter() - t0
            print(f"run(): {block} steps {'with   ' if with_avg else 'without'} model.averages: {dt / block * 1e3:.1f} ms per step")
    model.averages = None
    print(f"samples taken in the run: {ta.nsamples}, W = {ta.weight():.6g}")


if __name__ == "__main__":
    main()
