"""One rank of the partitioned sampling tests (launched by tests/test_gpu_dist_sampling.py through torch.distributed.run; all ranks
share GPU 0 and talk through the transport NPG_COMM_TRANSPORT names, as in tests/dist_rehearsal_worker.py).

  synthetic <out> <points.npz>   the partitioned bowl3D h = 0.1 model is NOT stepped: every rank uploads its slice of one synthetic
                                 global state (synthetic_state - the test process uploads the same vectors to a one-device model, so
                                 the nodal values are bit-identical on both sides) and samples it through every entry point
  stepped <out>                  2 steps of the partitioned example model; GridDiagnostics.compute() runs in an on_plot hook"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import nupgcm_amd as npg                                     # noqa: E402
from nupgcm_amd import sampling, workloads                   # noqa: E402

MESH = "bowl3D_h0.1"
GRID = (48, 40, 56)              # GridDiagnostics of the synthetic state: three different axis lengths
SLICE_N, PROFILE_AT, PROFILE_N = 48, (0.3, 0.2), 32


def synthetic_state(fed):
    """(xg, bg): [u; p] and b' in solver (device) order, smooth functions of the coordinates of each DoF's node"""
    m, t, d = fed.mesh, fed.tables, fed.dofs
    X = m.node_coords
    xg, bg = np.zeros(d.nu + d.np), np.zeros(d.nb)
    f = (lambda x: np.sin(2.1 * x[:, 0] + 0.3) * np.cos(1.7 * x[:, 1]) * (1.0 + x[:, 2]),
         lambda x: np.cos(1.3 * x[:, 0]) * np.sin(2.9 * x[:, 1] - 0.2) * (0.5 - x[:, 2]),
         lambda x: 0.1 * np.sin(3.0 * x[:, 0] * x[:, 1]) * x[:, 2])
    for a in range(3):
        on = t.u_pos[:, a] >= 0
        xg[t.u_pos[on, a]] = f[a](X[on])
    on = t.p_pos >= 0
    xg[t.p_pos[on]] = (X[:m.nv, 0] - 0.4 * X[:m.nv, 1] ** 2 + np.sin(5.0 * X[:m.nv, 2]))[on]
    nbn = len(t.b_pos)
    on = t.b_pos >= 0
    bg[t.b_pos[on]] = (np.sin(2.0 * X[:nbn, 0] - X[:nbn, 1]) * X[:nbn, 2] + 0.2 * X[:nbn, 2] ** 2)[on]
    return xg, bg


def diagnostics_arrays(g, tag):
    return {f"{tag}_col": g.col, f"{tag}_zon": g.zon, f"{tag}_x": g.x, f"{tag}_y": g.y, f"{tag}_z": g.z}


def sample_everything(model, pts):
    """every sampling entry point on `model` - called by the ranks and, on the one-device model, by the test process"""
    out = {}
    loc = sampling.locator(model).locate(pts)
    out["valid"] = loc.valid
    for f in ("u", "p", "b", "grad_b"):
        out[f"pt_{f}"] = npg.nan_eval(model, f, pts, loc)
    lo, hi = sampling.locator(model).bounding_box
    out["box"] = np.concatenate([lo, hi])
    s = npg.sample_slice(model, y=0.0, bbox=(lo[0], lo[2], hi[0], hi[2]), n=SLICE_N)
    out.update(slice_u=s["u"], slice_b=s["b"], slice_valid=s["cache"].valid)
    p = npg.sample_profiles(model, *PROFILE_AT, n=PROFILE_N)
    out.update(prof_H=p["H"], prof_u=p["u"], prof_b=p["b"], prof_valid=p["cache"].valid, dry_H=npg.find_H(model, 0.99, 0.99))
    g = npg.sample_to_grid(model, 32, 32, 32, fields=("u", "b", "grad_b"), chunk=5000)          # several chunks
    out.update(grid_valid=g.valid, grid_u=g["u"], grid_b=g["b"], grid_grad_b=g["grad_b"])
    gd = npg.GridDiagnostics(model, *GRID)
    out.update(diagnostics_arrays(gd.compute(), "gd1"))
    out.update(diagnostics_arrays(gd.compute(), "gd2"))
    dflt = npg.GridDiagnostics(model)                                                            # the default 256^3 axes
    out.update(default_x=dflt.x, default_y=dflt.y, default_z=dflt.z)
    return out


def main():
    import torch.distributed as dist
    from nupgcm_amd import partition
    mode, out = sys.argv[1], sys.argv[2]
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    arch = npg.GPU(int(os.environ.get("NPG_FORCE_DEVICE", 0)))
    m = partition.example_model(arch, workloads.bowl_mesh_model(MESH), dist)
    res = dict(transport=arch.ctx.comm_info()["in_cycle_transport"])
    if mode == "synthetic":
        xg, bg = synthetic_state(m.fe_data)
        m.inversion.solver.x.upload(xg[m.layout.inv.globals()])
        m.b_vec.upload(bg[m.layout.b.globals()])
        res.update(sample_everything(m, np.load(sys.argv[3])["pts"]))
        info = sampling.locator(m).info()
        res.update(loc_cells=np.array([info["cells"], info["owned"], info["witness"], info["bytes"]]))
    else:
        seen = []
        gd = npg.GridDiagnostics(m, *GRID)
        m.on_plot = lambda model, t: seen.append((model.step_index, gd.compute()))
        npg.invert(m)
        npg.run(m, n_steps=2, n_plot=2)
        assert [s[0] for s in seen] == [2]
        res.update(diagnostics_arrays(seen[0][1], "gd1"))
        res.update(u=m.state.u, p=m.state.p, b=m.state.b)                                      # collective gathers
    arch.ctx.sync()
    np.savez(f"{out}.rank{rank}.npz", **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
