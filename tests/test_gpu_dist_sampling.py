"""Sampling and GridDiagnostics of a mesh-partitioned model (nupgcm_amd.sampling on a partition.PartitionedModel):
2 and 3 ranks on one GPU, peer-window and shared-memory transports, against the one-device model in this process.

The comparison is about sampling, not about Krylov tolerances: the models are not stepped.  One synthetic global state (smooth
functions of the DoF coordinates, tests/dist_sampling_worker.synthetic_state) is uploaded to the one-device model's vectors and, slice
by slice, to every rank - the nodal values are bit-identical on both sides.  One more launch steps the partitioned model and samples
from an on_plot hook: the ghost values must be current when sampling happens."""
import os
import subprocess
import sys

import numpy as np
import pytest

import nupgcm_amd as npg
from nupgcm_amd import workloads

from . import dist_sampling_worker as W
from .test_gpu_distributed import _free_port
from .test_partition_sampling import adversarial_points

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EPS = np.finfo(np.float64).eps


def _launch(world, transport, mode, out, *extra, timeout=600):
    env = dict(os.environ, NPG_COMM_TRANSPORT=transport, NPG_FORCE_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2",
               NPG_PEER_TIMEOUT_S="60")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(HERE, "dist_sampling_worker.py"), mode, out, *extra]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)          # one attempt: no retry
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    ranks = [dict(np.load(f"{out}.rank{k}.npz")) for k in range(world)]
    assert all(str(z["transport"]) == transport for z in ranks)
    return ranks


@pytest.fixture(scope="module")
def points():
    """the adversarial points of the CPU exactly-once test (rank cuts of 2, 3 and 5 ranks, the row z = 0, the bounding box's corners and
    face centres, a coarse grid) and a 64^3 grid over the bounding box"""
    adv, _ = adversarial_points(W.MESH)
    m = workloads.example_fe_data(workloads.bowl_mesh_model(W.MESH)).mesh
    X = m.geo_coords[m.cell_geo].reshape(-1, 3)
    g = np.meshgrid(*(np.linspace(X[:, a].min(), X[:, a].max(), 64) for a in range(3)), indexing="ij")
    return np.vstack([adv, np.column_stack([v.ravel() for v in g])])


@pytest.fixture(scope="module")
def serial(points):
    """the one-device model with the synthetic state, sampled through the same calls as the ranks"""
    model = workloads.example_model(npg.GPU(), W.MESH)
    xg, bg = W.synthetic_state(model.fe_data)
    model.inversion.solver.x.upload(xg)
    model.b_vec.upload(bg)
    return model, W.sample_everything(model, points)


@pytest.fixture(scope="module")
def launches(points, tmp_path_factory):
    """(world, transport) -> the ranks' results; each configuration is launched once"""
    d = tmp_path_factory.mktemp("dist_sampling")
    np.savez(d / "points.npz", pts=points)
    done = {}

    def get(world, transport):
        if (world, transport) not in done:
            done[world, transport] = _launch(world, transport, "synthetic", str(d / f"w{world}_{transport}"), str(d / "points.npz"))
        return done[world, transport]
    return get


def reassociation_bound(n, channel):
    """a sum of at most n terms re-associated into per-rank partial sums: n eps is the first-order bound of the re-association, 8 the
    margin for the two-level sum (z tiles / x chunks, then ranks) and the wave tree - relative to the channel's largest entry"""
    return 8 * n * EPS * np.abs(channel).max()


def check_integrals(got_col, got_zon, ref_col, ref_zon, label):
    nx, ny, nz = ref_col.shape[1], ref_col.shape[2], ref_zon.shape[2]
    assert np.array_equal(got_col[0], ref_col[0]) and np.array_equal(got_zon[0], ref_zon[0])    # counts: exactly once, on the device
    assert ref_col[0].sum() == ref_zon[0].sum() and ref_col[0].sum() > 0.2 * nx * ny * nz
    for name, got, ref, n in (("col", got_col, ref_col, nz), ("zon", got_zon, ref_zon, nx)):
        for ch in range(1, len(ref)):
            err, bound = np.abs(got[ch] - ref[ch]).max(), reassociation_bound(n, ref[ch])
            print(f"{label} {name}[{ch}]: max |partitioned - serial| {err:.3e}, bound 8 n eps max|channel| = {bound:.3e} (n = {n})")
            assert err <= bound, (label, name, ch, err, bound)


@pytest.mark.parametrize("world,transport", [(2, "peer"), (3, "shm")])
def test_partitioned_sampling_equals_the_one_device_model(serial, launches, points, world, transport):
    model, ref = serial
    ranks = launches(world, transport)
    z = ranks[0]
    for other in ranks[1:]:                                                  # every rank receives the same, complete result
        for k in ref:
            assert np.array_equal(other[k], z[k], equal_nan=True), k
    # the bounding box and with it the default axes are the serial ones, bit for bit
    assert np.array_equal(z["box"], ref["box"])
    for a in "xyz":
        assert np.array_equal(z[f"default_{a}"], ref[f"default_{a}"]) and np.array_equal(z[f"gd1_{a}"], ref[f"gd1_{a}"])
    # point sampling: the same NaN pattern and the same bits - same winner cell, same lambda, same arithmetic (k_sample is the
    # serial instance; the merge adds zeros to one rank's value)
    assert np.array_equal(z["valid"], ref["valid"]) and 0.3 < ref["valid"].mean() < 0.9
    for f in ("u", "p", "b", "grad_b"):
        assert np.array_equal(np.isnan(z[f"pt_{f}"]), np.isnan(ref[f"pt_{f}"])), f
        assert np.array_equal(np.isnan(ref[f"pt_{f}"]).reshape(len(points), -1).all(1), ~ref["valid"]), f
        assert np.array_equal(z[f"pt_{f}"], ref[f"pt_{f}"], equal_nan=True), f
    # grid sampling
    for k in ("slice_u", "slice_b", "slice_valid", "prof_H", "prof_u", "prof_b", "prof_valid", "dry_H", "grid_valid", "grid_u",
              "grid_b", "grid_grad_b"):
        assert np.array_equal(z[k], ref[k], equal_nan=True), k
    assert ref["prof_H"] > 0.1 and ref["prof_valid"].all() and ref["dry_H"] == 0.0 and ref["slice_valid"].any()
    # counts and integrals; two compute() calls give the same bits
    check_integrals(z["gd1_col"], z["gd1_zon"], ref["gd1_col"], ref["gd1_zon"], f"{world} ranks {transport}")
    assert np.array_equal(z["gd1_col"], z["gd2_col"]) and np.array_equal(z["gd1_zon"], z["gd2_zon"])
    # every cell of the mesh is owned once; every rank holds a witness layer
    cells = np.array([r["loc_cells"] for r in ranks])
    print(f"{world} ranks: locator cells per rank {cells[:, 0].tolist()}, owned {cells[:, 1].tolist()}, witness {cells[:, 2].tolist()}, "
          f"bytes {cells[:, 3].tolist()}")
    assert cells[:, 1].sum() == model.fe_data.mesh.ncell and (cells[:, 2] > 0).all()


def test_peer_and_shm_transports_give_the_same_bits(serial, launches):
    _, ref = serial
    a, b = launches(3, "peer"), launches(3, "shm")
    for za, zb in zip(a, b):
        for k in ref:
            assert np.array_equal(za[k], zb[k], equal_nan=True), k
    check_integrals(a[0]["gd1_col"], a[0]["gd1_zon"], ref["gd1_col"], ref["gd1_zon"], "3 ranks peer")


def test_diagnostics_follow_the_stepped_state(tmp_path):
    """2 steps of the partitioned example model, GridDiagnostics.compute() from an on_plot hook: finite where H > 0, and equal - to
    the re-association bound - to the diagnostics of a one-device model loaded with the gathered PartitionedState.  Stale ghost
    values would show as differences of the size of one step's change."""
    ranks = _launch(2, "peer", "stepped", str(tmp_path / "stepped"))
    z = ranks[0]
    for k in ("gd1_col", "gd1_zon"):
        assert np.array_equal(ranks[1][k], z[k])
    model = workloads.example_model(npg.GPU(), W.MESH)
    d = model.fe_data.dofs
    model.inversion.solver.x.upload(np.concatenate([z["u"], z["p"]])[d.p_inversion])
    model.b_vec.upload(z["b"][d.p_b])
    assert np.abs(z["u"]).max() > 0 and np.abs(z["b"]).max() > 0
    g = npg.GridDiagnostics(model, *W.GRID).compute()
    got = npg.sampling.GridIntegrals(z["gd1_x"], z["gd1_y"], z["gd1_z"], z["gd1_col"], z["gd1_zon"], model.params.alpha)
    wet = got.H > 0
    assert wet.any() and np.isfinite(got.Psi[wet]).all() and np.isfinite(got.U[wet]).all() and np.isnan(got.Psi[~wet]).all()
    assert np.isfinite(got.psi_bar[got.width > 0]).all() and np.isfinite(got.b_bar[got.width > 0]).all()
    check_integrals(z["gd1_col"], z["gd1_zon"], g.col, g.zon, "stepped, 2 ranks peer")
