"""One rank of the partitioned mesh-integral tests (launched by tests/test_gpu_dist_integrals.py through torch.distributed.run; all
ranks share GPU 0 and talk through the transport NPG_COMM_TRANSPORT names, as tests/dist_sampling_worker.py).

  <out>   bowl3D h = 0.1 (the example model) and the small channel basin, neither stepped: every rank uploads its slice of one synthetic
          global state (dist_sampling_worker.synthetic_state - the test process uploads the same vectors to the one-device models) and
          integrates it twice"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import nupgcm_amd as npg                                     # noqa: E402
from nupgcm_amd import channel_basin, workloads              # noqa: E402
from tests.dist_sampling_worker import MESH, synthetic_state  # noqa: E402


def channel_mesh_model():
    return channel_basin.channel_basin_model(0.125, workloads.CB_ALPHA, dz=0.125)


def integrate(model, tag):
    mi = npg.MeshIntegrals(model)
    return {f"{tag}_raw1": mi.compute_raw(), f"{tag}_raw2": mi.compute_raw(), f"{tag}_counted": np.int64(mi.ncells_counted)}


def main():
    import torch.distributed as dist
    from nupgcm_amd import partition
    out = sys.argv[1]
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    arch = npg.GPU(int(os.environ.get("NPG_FORCE_DEVICE", 0)))
    res = {}
    for tag, m in (("bowl", partition.example_model(arch, workloads.bowl_mesh_model(MESH), dist)),
                   ("channel", partition.channel_basin_model(arch, channel_mesh_model(), dist, invert_now=False))):
        xg, bg = synthetic_state(m.fe_data)
        m.inversion.solver.x.upload(xg[m.layout.inv.globals()])
        m.b_vec.upload(bg[m.layout.b.globals()])
        res.update(integrate(m, tag))
    res["transport"] = arch.ctx.comm_info()["in_cycle_transport"]
    arch.ctx.sync()
    np.savez(f"{out}.rank{rank}.npz", **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
