"""Times of NodalFields on the bench mesh (bowl3D h = 0.02), after a warm-up call (device events around INNER calls, per call; best /
median of --reps such windows, at least 0.5 s in all):
  * npg_nodal_compute (k_nodal_cells + k_nodal_nodes) for fields=("b",) and for all fields, both weights, with the bytes the two launches
    move counted from the shapes and the fraction of the HBM specification (8 TB/s) that implies;
  * the whole compute() including the download and the scatter into mesh order (wall);
  * next to it the parent's only route to the three closure fields of save_vtk: the download of the state plus
    io._nodal_closure_fields on the host (wall), in the same process;
  * the valences, and the node launch with the rows in mesh order (the default) against rows sorted by valence.
--quick: the device calls only (for a kernel trace, which gives the two launches apart).
Usage: python tools/nodal_bench.py [--workload L] [--reps R] [--quick]"""
import argparse
import os
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import nupgcm_amd as npg  # noqa: E402
from nupgcm_amd import _lib as L, io as nio, workloads  # noqa: E402
from nupgcm_amd.nodal import channels_of, mask_of  # noqa: E402

HBM_SPEC = 8.0e12       # bytes / s
INNER = 10


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


def bytes_moved(nf, fields, nb):
    """(cells launch, nodes launch) counted from the shapes, every table and every record entry once per USE in the cells launch
    (tables: 12 G, the DoF codes; the state gathered through them) and once per use in the nodes launch (a vertex incidence reads the
    record's channels once, a mid-node incidence twice) - the nodes launch re-reads a record up to ten times, so its HBM traffic is
    below this count by what the caches hold"""
    mask = mask_of(fields)
    ncell, nsel = nf.model.fe_data.mesh.ncell, len(nf.sel)
    nslot = (36 if mask & 1 else 0) + ((12 if nb == 10 else 3) if mask & 2 else 0) + (3 if mask & 4 else 0)
    codes = (30 if mask & 1 else 0) + (nb if mask & 2 else 0) + (4 if mask & 4 else 0)
    cells = ncell * (12 * 8 + codes * (4 + 8) + nslot * 8)
    ptr, inc = nf._table
    local = inc & 15
    nch = len(channels_of(mask)) - 2
    per_vertex = (9 if mask & 1 else 0) + (3 if mask & 2 else 0) + (3 if mask & 4 else 0)
    reads = int((local < 4).sum()) * per_vertex + int((local >= 4).sum()) * 2 * per_vertex
    nodes = reads * 8 + len(inc) * (4 + 8) + nsel * (16 + (nch + 2) * 8)
    return cells, nodes, ncell * nslot * 8


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
    print(f"{ctx.name()}; library {os.path.basename(L.LIB_PATH)}; {a.workload}: {m.ncell} cells, {m.nn} P2 nodes, {n_inv} + {n_b} unknowns; "
          f"set-up {time.time() - t0:.1f} s")
    t0 = time.time()
    nfs = {w: npg.NodalFields(model, weight=w) for w in ("volume", "count")}
    nfs["count, rows sorted by valence"] = npg.NodalFields(model, weight="count", ordered=True)
    val = nfs["count"].valence
    print(f"incidence tables built in {(time.time() - t0) / 2:.2f} s each; {len(nfs['count']._table[1])} incidences; valence min {val.min()} "
          f"median {int(np.median(val))} max {val.max()}")
    for w, nf in nfs.items():
        for fields in (("b",), ("u", "b", "p")):
            best, med, n = timed(ctx, lambda: nf.compute_device(fields), a.reps)
            cb, nbts, scr = bytes_moved(nf, fields, nb)
            print(f"weight={w} fields={','.join(fields)}: both launches by events: best {best:.4f} ms, median {med:.4f} ms of {n} windows of "
                  f"{INNER}; scratch {scr / 1e6:.1f} MB; counted bytes: cells {cb / 1e6:.1f} MB + nodes {nbts / 1e6:.1f} MB = "
                  f"{(cb + nbts) / (best * 1e-3) / HBM_SPEC:.3f} of the HBM spec; device memory held {nf.nbytes / 1e6:.1f} MB")
    if a.quick:
        return
    nf = nfs["count"]
    for fields in (("b",), ("u", "b", "p")):
        wall = []
        for _ in range(5):
            ctx.sync()
            t0 = time.perf_counter()
            g = nf.compute(fields)
            wall.append(time.perf_counter() - t0)
        print(f"compute({fields}) with the download and the scatter into mesh order, wall: best {min(wall) * 1e3:.1f} ms")
    wall = []
    for _ in range(5):
        ctx.sync()
        t0 = time.perf_counter()
        abz, nu, kv = nf.compute(("b",)).closures()
        wall.append(time.perf_counter() - t0)
    new = min(wall)
    print(f"the three closure fields through NodalFields (compute(('b',)).closures()), wall: best {new * 1e3:.1f} ms")
    sp = fed.spaces
    host = []
    for _ in range(3):
        ctx.sync()
        t0 = time.perf_counter()
        xh, bh = x.to_host(d.inv_p_inversion), b.to_host(d.inv_p_b)                          # what model.state downloads
        t1 = time.perf_counter()
        bn = np.where(sp.b_dof >= 0, bh[np.maximum(sp.b_dof, 0)], sp.b_diri_val)
        b_full = prm.N2 * m.node_coords[:, 2] + bn
        abz0, nu0, kv0 = nio._nodal_closure_fields(model, b_full)
        host.append((time.perf_counter() - t0, t1 - t0))
    old = min(h[0] for h in host)
    print(f"the parent's route (download of the state, io._nodal_closure_fields on the host), wall: best {old * 1e3:.1f} ms, of which the "
          f"download {min(h[1] for h in host) * 1e3:.1f} ms; ratio parent / new = {old / new:.1f}")
    print(f"agreement of the two: max |alpha*b_z difference| {np.max(np.abs(abz - abz0)):.3e}, max |alpha*b_z| {np.max(np.abs(abz0)):.3e}")


if __name__ == "__main__":
    main()
