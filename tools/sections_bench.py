"""Times of SectionTransports on the bench mesh (bowl3D h = 0.02), after a warm-up call (device events around INNER calls, per call;
best / median of --reps such windows, at least 0.5 s in all):
  * npg_sections_compute (k_section_pieces + k_section_fold) for one meridional section in one bin, for 32 latitudes x 32 depth bins
    (the case DESIGN.md 28 quotes) and for the same latitudes in one bin each, with and without the per-piece output, with the bytes the
    two launches move counted from the shapes and the fraction of the HBM specification (8 TB/s) that implies;
  * the plan's set-up time (host, once) and its size;
  * the whole compute() including the download (wall), and next to it the download of the state alone (wall) - the first step of the
    only other route, a host pass over the downloaded state.
--quick: the device calls only (for a kernel trace, which gives the two launches apart).
Usage: python tools/sections_bench.py [--workload L] [--reps R] [--quick]"""
import argparse
import os
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import nupgcm_amd as npg  # noqa: E402
from nupgcm_amd import _lib as L, workloads  # noqa: E402

HBM_SPEC = 8.0e12       # bytes / s
INNER = 10
NSEC = L.NPG_NSEC


def timed(ctx, fn, reps):
    fn()
    ctx.sync()
    t = []
    while len(t) < reps or sum(t) * INNER < 500.0:
        ctx.timer_start()
        for _ in range(INNER):
            fn()
        t.append(ctx.timer_stop() / INNER)
    return min(t), float(np.median(t)), len(t)


def bytes_moved(st, nb):
    """(pieces launch, fold launch) counted from the shapes: per piece its tables (cell, section, 12 barycentrics, area, 2 x 6
    coefficients), its cell's 12 gradients, 4 z, 34 + nb DoF codes and the values behind them, and its 14 terms written; the fold reads
    every term once and writes 14 doubles per bin.  Pieces of one cell re-read that cell's tables, so the HBM traffic of the pieces
    launch is below this count by what the caches hold."""
    n = st.npiece
    pieces = n * (4 + 1 + 13 * 8 + 12 * 8 + (12 + 4) * 8 + (34 + nb) * (4 + 8) + NSEC * 8)
    fold = n * NSEC * 8 + st.nbin * (NSEC * 8 + 16)
    return pieces, fold


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bowl3D_h0.02")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    arch = npg.GPU()
    ctx = arch.ctx
    t0 = time.time()
    fed = workloads.example_fe_data(workloads.bowl_mesh_model(a.workload))
    prm, frc = workloads.example_parameters()
    m, d = fed.mesh, fed.dofs
    n_inv, n_b = d.nu + d.np, d.nb
    x, b = npg.DeviceVector(ctx, n_inv), npg.DeviceVector(ctx, n_b)
    model = SimpleNamespace(arch=arch, fe_data=fed, params=prm, forcings=frc, b_vec=b, inversion=SimpleNamespace(solver=SimpleNamespace(x=x)))
    rng = np.random.default_rng(1)
    x.upload(rng.standard_normal(n_inv))
    b.upload(rng.standard_normal(n_b))
    nb = 10 if fed.spaces.b_order == 2 else 4
    print(f"{ctx.name()}; library {os.path.basename(L.LIB_PATH)}; {a.workload}: {m.ncell} cells, {n_inv} + {n_b} unknowns; set-up {time.time() - t0:.1f} s")
    ys = np.linspace(-0.93, 0.93, 32)
    zed = np.linspace(-1.0, 0.0, 33)
    cases = {"one section x = 0.1, one bin": [npg.Section.longitude(0.1)],
             "32 latitudes, one bin each": [npg.Section.latitude(y, name=f"y{k}") for k, y in enumerate(ys)],
             "32 latitudes x 32 depth bins": [npg.Section.latitude(y, z_edges=zed, name=f"y{k}") for k, y in enumerate(ys)]}
    sts = {}
    for name, secs in cases.items():
        st = npg.SectionTransports(model, secs)
        sts[name] = st
        i = st.info
        print(f"{name}: plan {i['setup_seconds']:.3f} s on the host; {i['pieces']} pieces, {i['bins']} bins, {i['cut_cells']} cut cells, largest bin "
              f"{i['max_per_bin']}")
        st._pieces_out = npg.DeviceVector(ctx, max(1, NSEC * st.npiece))
        xh, bh, lib = x.h, b.h, L.lib()
        for label, po in (("", None), (" with pieces_out", st._pieces_out.h)):
            best, med, n = timed(ctx, lambda: L.check(lib.npg_sections_compute(st.h, xh, bh, st._out.h, po)), a.reps)
            pb, fb = bytes_moved(st, nb)
            print(f"{name}{label}: both launches by events: best {best:.4f} ms, median {med:.4f} ms of {n} windows of {INNER}; counted bytes: pieces "
                  f"{pb / 1e6:.1f} MB + fold {fb / 1e6:.1f} MB = {(pb + fb) / (best * 1e-3) / HBM_SPEC:.3f} of the HBM spec")
    if a.quick:
        return
    st = sts["32 latitudes x 32 depth bins"]
    for pieces in (False, True):
        wall = []
        for _ in range(5):
            ctx.sync()
            t0 = time.perf_counter()
            st.compute_raw(pieces)
            wall.append(time.perf_counter() - t0)
        print(f"compute_raw(pieces={pieces}) with the download, wall: best {min(wall) * 1e3:.2f} ms")
    wall = []
    for _ in range(5):
        ctx.sync()
        t0 = time.perf_counter()
        x.to_host(), b.to_host()
        wall.append(time.perf_counter() - t0)
    print(f"the download of the state alone (what a host pass starts with), wall: best {min(wall) * 1e3:.2f} ms")
    a1, a2 = st.compute_raw()[0], st.compute_raw()[0]
    print(f"two calls, the same bits: {np.array_equal(a1, a2)}; total area of the 32 sections {a1[:, 0].sum():.9f}")


if __name__ == "__main__":
    main()
