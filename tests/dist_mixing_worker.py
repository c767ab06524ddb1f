"""One rank of the partitioned mixing-table tests (launched by tests/test_gpu_dist_mixing.py through torch.distributed.run; all ranks
share GPU 0 and talk through the transport NPG_COMM_TRANSPORT names, as tests/dist_watermass_worker.py).

  <out>   bowl3D h = 0.1 (the example model) and the small channel basin, neither stepped: every rank uploads its slice of one synthetic
          global state (dist_sampling_worker.synthetic_state - the test process uploads the same vectors to the one-device models) and
          bins its mixing table twice, with non-constant diffusivities (mixing_ref.kappa_h_fn / kappa_v_fn), the closure on and the
          edges and closure arguments the test process chose (<out>.edges.npz)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import nupgcm_amd as npg                                     # noqa: E402
from nupgcm_amd import workloads                             # noqa: E402
from tests.dist_integrals_worker import channel_mesh_model   # noqa: E402
from tests.dist_sampling_worker import MESH, synthetic_state  # noqa: E402
from tests.mixing_ref import kappa_h_fn, kappa_v_fn          # noqa: E402


def bin_twice(model, tag, be, ye, closure):
    K = npg.BuoyancyClasses(model, be, ye)
    K.set_diffusivity(kappa_h_fn, kappa_v_fn)
    t1, d1, S1 = K.mixing_raw(closure=closure)
    t2, d2, S2 = K.mixing_raw(closure=closure)
    return {f"{tag}_raw1": t1, f"{tag}_raw2": t2, f"{tag}_info1": np.concatenate([[d1], S1]), f"{tag}_info2": np.concatenate([[d2], S2]),
            f"{tag}_counted": np.int64(K.ncells_counted)}


def main():
    import torch.distributed as dist
    from nupgcm_amd import partition
    out = sys.argv[1]
    edges = np.load(f"{out}.edges.npz")
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    arch = npg.GPU(int(os.environ.get("NPG_FORCE_DEVICE", 0)))
    res = {}
    for tag, m in (("bowl", partition.example_model(arch, workloads.bowl_mesh_model(MESH), dist)),
                   ("channel", partition.channel_basin_model(arch, channel_mesh_model(), dist, invert_now=False))):
        xg, bg = synthetic_state(m.fe_data)
        m.inversion.solver.x.upload(xg[m.layout.inv.globals()])
        m.b_vec.upload(bg[m.layout.b.globals()])
        res.update(bin_twice(m, tag, edges[f"{tag}_b"], edges[f"{tag}_y"], tuple(edges[f"{tag}_closure"])))
    res["transport"] = arch.ctx.comm_info()["in_cycle_transport"]
    arch.ctx.sync()
    np.savez(f"{out}.rank{rank}.npz", **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
