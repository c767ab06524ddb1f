"""The mixing table of a mesh-partitioned model (BuoyancyClasses.mixing on a partition.PartitionedModel): 2 and 3 ranks on
one GPU, peer-window and shared-memory transports, bowl3D h = 0.1 and the small channel basin, non-constant diffusivities and the
closure on, against the restatement and the one-device models in this process.  As in tests/test_gpu_dist_watermass.py the models are
not stepped: one synthetic global state is uploaded to the one-device model and, slice by slice, to every rank.  Each configuration is
launched once, in fresh child processes, under its own time limit; a failed launch fails its test and nothing is started after it in
that test."""
import os
import subprocess
import sys

import numpy as np
import pytest

import nupgcm_amd as npg
from nupgcm_amd import workloads

from . import dist_integrals_worker as W
from . import mixing_ref as mr
from .dist_sampling_worker import MESH, synthetic_state
from .test_gpu_distributed import _free_port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _launch(world, transport, out, timeout=300):
    env = dict(os.environ, NPG_COMM_TRANSPORT=transport, NPG_FORCE_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2",
               NPG_PEER_TIMEOUT_S="60")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(HERE, "dist_mixing_worker.py"), out]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)          # one attempt: no retry
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    ranks = [dict(np.load(f"{out}.rank{k}.npz")) for k in range(world)]
    assert all(str(z["transport"]) == transport for z in ranks)
    return ranks


@pytest.fixture(scope="module")
def serial():
    """tag -> (one-device model with the synthetic state, its edges, the closure, the restatement, its table and S)"""
    arch = npg.GPU()
    out = {}
    for tag, model in (("bowl", workloads.example_model(arch, MESH)),
                       ("channel", workloads.channel_basin_model(arch, mesh_model=W.channel_mesh_model()))):
        xg, bg = synthetic_state(model.fe_data)
        model.inversion.solver.x.upload(xg)
        model.b_vec.upload(bg)
        mv = mr.view(model)
        on = mr.choose_closure(mv, mr.rule_of(mv.fe_data.mesh, 1))
        rule, N2, smp, be, ye = mr.model_edges(mv, 1, True, on)
        ref = mr.MixRestated(smp, be, ye)
        assert np.mean((ref.g > 0.05) & (ref.g < 0.95)) >= 0.1
        tab, dropped, S = npg.BuoyancyClasses(mv, be, ye).mixing_raw(closure=on)
        assert dropped == 0
        out[tag] = (model, be, ye, on, ref, tab, S)
    return out


@pytest.mark.parametrize("world,transport", [(2, "peer"), (3, "shm")])
def test_partitioned_mixing_equals_the_one_device_model(serial, tmp_path, world, transport):
    out = str(tmp_path / f"w{world}_{transport}")
    np.savez(f"{out}.edges.npz", **{f"{tag}_{a}": v[i] for tag, v in serial.items() for a, i in (("b", 1), ("y", 2), ("closure", 3))})
    ranks = _launch(world, transport, out)
    for tag, (model, be, ye, on, ref, one, S1) in serial.items():
        nc = model.fe_data.mesh.ncell
        z = ranks[0]
        for other in ranks[1:]:                                              # every rank returns the same bits
            assert np.array_equal(other[f"{tag}_raw1"], z[f"{tag}_raw1"]) and np.array_equal(other[f"{tag}_info1"], z[f"{tag}_info1"]), tag
        for r in ranks:                                                      # two calls give identical bits
            assert np.array_equal(r[f"{tag}_raw1"], r[f"{tag}_raw2"]) and np.array_equal(r[f"{tag}_info1"], r[f"{tag}_info2"]), tag
        counted = [int(r[f"{tag}_counted"]) for r in ranks]
        assert sum(counted) == nc and min(counted) > 0, (tag, counted, nc)   # every cell exactly once
        got, info = z[f"{tag}_raw1"], z[f"{tag}_info1"]
        assert info[0] == 0
        S = info[1:]                                                         # the ranks' S_c added up: each rank's unit is at most 2^-60 of it
        mr.compare(got, S, ref, f"{world} ranks {transport} {tag} (cells per rank {counted})")
        err = np.abs(got - one)                                              # and against the one-device table: two quantisations
        bound = ref.n_total * mr.EPS * ref.S_total + ref.n[:, :, None] * 2.0 ** -61 * (S + S1) + ref.closure_bound
        assert (err <= bound).all(), (tag, err.max())
        assert np.abs(one).max(axis=(0, 1)).min() > 0                        # every channel is exercised, the closure's included
