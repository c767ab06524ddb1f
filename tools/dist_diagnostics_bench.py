"""GridDiagnostics on a mesh-partitioned model, timed: per rank the locator's cells (owned, witness) and memory, the
device time of npg_fe_grid_integrals - once with the ranks taking turns (each rank's kernel alone on the device) and once with all
ranks launching together, as compute() does - the cross-rank sum of the 4 nx ny + 6 ny nz doubles, and compute()'s wall time.
The state is the model's initial one unless --steps is given: the pass does the same work whatever the values are.

    NPG_COMM_TRANSPORT=peer python -m torch.distributed.run --nproc-per-node=3 tools/dist_diagnostics_bench.py [--workload L] [--grid N]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch.distributed as dist  # noqa: E402

import nupgcm_amd as npg  # noqa: E402
from nupgcm_amd import _lib as L, partition, sampling  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bowl3D_h0.02")
    ap.add_argument("--steps", type=int, default=0)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    arch = npg.GPU(int(os.environ.get("NPG_FORCE_DEVICE", 0)))
    ctx = arch.ctx
    n = a.grid
    t0 = time.time()
    m = partition.example_model(arch, a.workload, dist)
    if a.steps:
        npg.invert(m)
        npg.run(m, n_steps=a.steps)
    gd = npg.GridDiagnostics(m, n, n, n)
    info = gd.loc.info()
    r = gd.compute()                                                     # warm-up
    call = lambda: L.check(L.lib().npg_fe_grid_integrals(gd.fe.h, gd.loc.h, m.inversion.solver.x.h, m.b_vec.h, float(m.params.N2),
                                                         gd._axes.h, n, n, n, gd._col.h, gd._zon.h))

    def device_ms():
        best = 1e30
        for _ in range(a.reps):
            ctx.timer_start()
            call()
            best = min(best, ctx.timer_stop())
        return best
    alone = 0.0
    for turn in range(world):                                            # one rank at a time: its kernel alone on the device
        dist.barrier()
        if turn == rank:
            alone = device_ms()
    dist.barrier()
    together = device_ms()                                               # all ranks at once, sharing the device
    dist.barrier()
    t_sum = []
    for _ in range(a.reps):
        ctx.sync()
        dist.barrier()
        t1 = time.perf_counter()
        sampling._allreduce(ctx, gd._out)
        ctx.sync()
        t_sum.append(time.perf_counter() - t1)
    wall = []
    for _ in range(a.reps):
        dist.barrier()
        t1 = time.perf_counter()
        r = gd.compute()
        wall.append(time.perf_counter() - t1)
    rows = [None] * world
    dist.all_gather_object(rows, dict(rank=rank, cells=info["cells"], owned=info["owned"], witness=info["witness"], bytes=info["bytes"],
                                      bins=info["dims"], alone=alone, together=together, allreduce=min(t_sum) * 1e3, wall=min(wall) * 1e3,
                                      wall_median=float(np.median(wall)) * 1e3))
    if rank == 0:
        nc = m.fe_data.mesh.ncell
        print(f"{a.workload}: {nc} cells, {world} ranks on one device, transport {ctx.comm_info()['in_cycle_transport']}; set-up "
              f"{time.time() - t0:.1f} s; grid {n}^3; {r.count_z.sum() / n ** 3:.3f} of the points inside; "
              f"|Psi| max {np.nanmax(np.abs(r.Psi)):.6e}")
        for w in rows:
            print(f"  rank {w['rank']}: locator {w['cells']} cells = {w['owned']} owned ({w['owned'] / nc:.3f} of the mesh) + {w['witness']} witness, "
                  f"bins {w['bins']}, {w['bytes'] / 2 ** 20:.1f} MiB; npg_fe_grid_integrals by events: alone {w['alone']:.3f} ms, all ranks "
                  f"at once {w['together']:.3f} ms; sum over ranks of {gd._out.n} doubles {w['allreduce']:.3f} ms wall; compute() "
                  f"{w['wall']:.2f} ms wall (best of {a.reps}; median {w['wall_median']:.2f} ms)")
        print(f"  owned cells in all: {sum(w['owned'] for w in rows)} of {nc}; slowest rank's kernel alone "
              f"{max(w['alone'] for w in rows):.3f} ms, sum of the ranks' kernels alone {sum(w['alone'] for w in rows):.3f} ms")
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
