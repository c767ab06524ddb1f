"""Times of the (latitude band, buoyancy class) table on the bench mesh (bowl3D h = 0.02), 64 x 64 bins, level = 1, after a warm-up call:
  * npg_classes_compute (memset + k_class_scan + k_classes_fold + k_class_bin + k_classes_convert) by device events, and the wall
    time of BuoyancyClasses.compute() (the launches and the download of the table);
  * next to it, in the same process and on the same state, npg_integrals_compute by events: the yardstick (11 points x 15 channels
    against 8 samples x 8 channels, one pass against two);
  * the same call with ONE bin - the contention case: every lane ends with one run and all of them add to the same 8 slots;
  * the atomics pass 2 sends, counted on the host from the samples' bins in the kernel's own lane order (a lane adds up a run of
    samples that share a bin and sends 8 bytes per non-zero channel when the bin changes), and the bytes per second that makes over the
    WHOLE call - a lower bound of what the atomic units sustain, the other passes are in the same time.
Usage: python tools/classes_bench.py [--workload L] [--steps K] [--reps R] [--bins N] [--level V] [--out FILE]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import nupgcm_amd as npg  # noqa: E402
from nupgcm_amd import _lib as L, fe as F, workloads  # noqa: E402


def timed(ctx, fn, reps):
    fn()
    ctx.sync()
    t = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        t.append(ctx.timer_stop())
    return min(t), float(np.median(t))


def sample_B_y(model, lam):
    """B = N2 z + b' and y of every sample (ncell, ns), from the device vector and the closed-form P2 / P1 shape functions"""
    fed = model.fe_data
    m, t, s = fed.mesh, fed.tables, fed.spaces
    b = model.b_vec.to_host()
    bn = np.where(t.b_pos >= 0, b[np.maximum(t.b_pos, 0)], s.b_diri_val)
    N, _ = F.p2_tables(lam, F._TET_EDGE_A, F._TET_EDGE_B)
    X = m.geo_coords[m.cell_geo]
    bp = np.einsum("si,ci->cs", N, bn[m.cell_nodes]) if s.b_order == 2 else np.einsum("si,ci->cs", lam, bn[m.cells])
    return float(model.params.N2) * np.einsum("sk,ck->cs", lam, X[:, :, 2]) + bp, np.einsum("sk,ck->cs", lam, X[:, :, 1])


def atomics_sent(bins, ncell, block=256, max_blocks=1024):
    """runs of equal bins along every lane's sample sequence (cells c, c + grid, c + 2 grid, ... of lane c mod grid, samples in order)"""
    grid = min((ncell + block - 1) // block, max_blocks) * block
    lane = np.arange(ncell) % grid
    order = np.argsort(lane, kind="stable")                   # per lane ascending cells
    seq, ln = bins[order].ravel(), np.repeat(lane[order], bins.shape[1])
    return 1 + int(((seq[1:] != seq[:-1]) | (ln[1:] != ln[:-1])).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bowl3D_h0.02")
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--level", type=int, default=1)
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
    lam, _ = npg.watermass.default_rule(a.level)
    B, y = sample_B_y(model, lam)
    be = np.linspace(B.min(), B.max(), a.bins + 1)[1:-1]
    ye = np.linspace(y.min(), y.max(), a.bins + 1)[1:-1]
    K = npg.BuoyancyClasses(model, be, ye, level=a.level)
    T = K.compute()                                                      # warm-up
    ctx.sync()
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        T2 = K.compute()
        wall.append(time.perf_counter() - t0)
    assert np.array_equal(T.raw, T2.raw)                                 # the same bits on every call
    x, b = model.inversion.solver.x, model.b_vec
    N2 = float(model.params.N2)
    dev = timed(ctx, lambda: L.check(L.lib().npg_classes_compute(K.h, x.h, b.h, N2, K._table.h, K._info.h)), a.reps)
    # the same two passes with ONE bin, the contention case: one run per lane, 8 atomics per lane, all lanes on the same 8 slots
    K1 = npg.BuoyancyClasses(model, (), (), level=a.level)
    one = timed(ctx, lambda: L.check(L.lib().npg_classes_compute(K1.h, x.h, b.h, N2, K1._table.h, K1._info.h)), a.reps)
    mi = npg.MeshIntegrals(model)
    ref = timed(ctx, lambda: L.check(L.lib().npg_integrals_compute(mi.h, x.h, b.h, int(mi.full_stress), mi._out.h)), a.reps)
    bins = np.searchsorted(ye, y, side="right") * a.bins + np.searchsorted(be, B, side="right")
    runs = atomics_sent(bins, m.ncell)
    nbytes = runs * 8 * npg.watermass.NCLS
    vol = mi.compute_raw()[0]
    say(f"{T}; occupied bins {int((T.volume > 0).sum())} of {T.volume.size}; |sum ch0 - volume| = {abs(T.volume.sum() - vol):.2e}")
    say(f"npg_classes_compute ({a.bins} x {a.bins} bins, {len(lam)} samples per cell) by events: best {dev[0]:.3f} ms, median {dev[1]:.3f} ms of "
        f"{a.reps} ({m.ncell * len(lam) / dev[0] / 1e3:.1f} Msamples/s); BuoyancyClasses.compute() wall: best {min(wall) * 1e3:.3f} ms, "
        f"median {np.median(wall) * 1e3:.3f} ms")
    grid = min((m.ncell + 255) // 256, 1024) * 256
    say(f"npg_classes_compute with ONE bin (the contention case: {min(grid, m.ncell)} lanes x {npg.watermass.NCLS} atomics on the same "
        f"{npg.watermass.NCLS} slots) by events: best {one[0]:.3f} ms, median {one[1]:.3f} ms = at most "
        f"{one[0] * 1e6 / (min(grid, m.ncell) * npg.watermass.NCLS):.1f} ns per same-address atomic")
    say(f"npg_integrals_compute by events: best {ref[0]:.3f} ms, median {ref[1]:.3f} ms")
    say(f"ratio npg_classes_compute / npg_integrals_compute = {dev[0] / ref[0]:.2f} (best), {dev[1] / ref[1]:.2f} (median)")
    say(f"pass 2 sends {runs} runs of {m.ncell * len(lam)} samples = at most {runs * npg.watermass.NCLS} 64-bit atomics, {nbytes / 1e6:.2f} MB: "
        f"{nbytes / (dev[0] * 1e-3) / 1e9:.2f} GB/s of atomic payload over the whole call (best time)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
