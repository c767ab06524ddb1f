"""Sampling a mesh-partitioned model, host logic on CPU (nupgcm_amd.partition: RankLayout.cell_owner, RankLayout.locator_cells):
every cell has one owner who keeps it, a rank's locator cells contain the witness layer, and - the point of it - every point is
claimed by exactly one rank, the one that owns the cell the one-device locator elects.

The exactly-once check states the product's rule ONCE, in numpy (`elect`): a cell accepts a point when its min lambda >= -1e-10; among
the accepting cells the largest min lambda wins, equal min lambda goes to the lowest global cell id.  It is applied to all cells (the
serial locator) and, per rank, to the rank's locator cells, on the same min-lambda matrix (tests/sampling_ref.Brute.lambdas): both
sides share the arithmetic, so no point is left out as ambiguous."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from nupgcm_amd import channel_basin, workloads
from nupgcm_amd.fe import _TET_EDGE_A as EA, _TET_EDGE_B as EB
from nupgcm_amd.partition import NodePartition, RankLayout

from .sampling_ref import Brute

WORLDS = (2, 3, 5)
MESHES = ("bowl3D_h0.1", "channel")
TOL = -1e-10                 # sample_core.h: kInsideTol


@functools.lru_cache(maxsize=None)
def fe_data(name):
    if name == "channel":       # the smallest channel-basin mesh of the suite (x-periodic: cells on both sides of the seam)
        fed = workloads.channel_basin_fe_data(channel_basin.channel_basin_model(0.125, workloads.CB_ALPHA, dz=0.125))
        assert fed.mesh.periodic
        return fed
    return workloads.example_fe_data(workloads.bowl_mesh_model(name))


@functools.lru_cache(maxsize=None)
def layouts(name, world):
    fed = fe_data(name)
    part = NodePartition(fed, world)
    return [RankLayout(fed, part, r) for r in range(world)]


@functools.lru_cache(maxsize=None)
def vertex_neighbours(name):
    """brute-force adjacency: N[c, d] != 0 where cells c and d share a geometric vertex (incidence matrix times its transpose)"""
    cg = fe_data(name).mesh.cell_geo
    nc = len(cg)
    inc = sp.csr_matrix((np.ones(4 * nc, dtype=np.int32), (np.repeat(np.arange(nc), 4), cg.ravel())), shape=(nc, int(cg.max()) + 1))
    return (inc @ inc.T).tocsr()


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name", MESHES)
def test_every_cell_has_one_owner_who_keeps_it_and_sees_its_neighbours(name, world):
    fed, lays = fe_data(name), layouts(name, world)
    nc = fed.mesh.ncell
    N = vertex_neighbours(name)
    owner = lays[0].cell_owner
    assert owner.shape == (nc,) and owner.min() >= 0 and owner.max() < world
    claimed = np.zeros(nc, dtype=int)
    for r, lay in enumerate(lays):
        assert np.array_equal(lay.cell_owner, owner)                         # every rank derives the same ownership
        cells, owned = lay.locator_cells(fed)
        assert np.array_equal(cells, np.unique(cells)) and owned.dtype == bool and len(owned) == len(cells)
        mine = cells[owned]
        assert np.array_equal(mine, np.nonzero(owner == r)[0])
        assert np.isin(mine, lay.cells).all()                                # the owner keeps the cell: tables and values are there
        claimed[mine] += 1
        want = np.unique(N[mine].indices)                                    # the owned cells and every vertex-neighbour of one
        assert np.array_equal(cells, want)
        assert len(mine) > 0 and len(cells) > len(mine)
    assert (claimed == 1).all()


# ---- exactly once ------------------------------------------------------------------------------------------------------------------
def elect(M, gids):
    """THE RULE.  M (n, k): min lambda of n points in k cells whose global ids `gids` ascend.  Returns the global id of each point's
    cell, -1 where no cell accepts it: accepted = min lambda >= -1e-10; the largest min lambda wins, ties to the lowest global id
    (argmax returns the first maximum, the columns ascend in global id)."""
    assert (np.diff(gids) > 0).all()
    cand = np.where(M >= TOL, M, -np.inf)
    k = cand.argmax(axis=1)
    return np.where(np.isfinite(cand[np.arange(len(M)), k]), gids[k], -1)


def adversarial_points(name):
    """vertices, edge midpoints and face centroids of the cells on both sides of every rank cut (2, 3 and 5 ranks); the top-surface row
    z = 0; the corners and face centres of the bounding box; a coarse regular grid"""
    fed = fe_data(name)
    m = fed.mesh
    N = vertex_neighbours(name)
    cut = np.zeros(m.ncell, dtype=bool)
    for world in WORLDS:
        owner = layouts(name, world)[0].cell_owner
        coo = N.tocoo()
        differ = owner[coo.row] != owner[coo.col]
        cut[coo.row[differ]] = True
    X = m.geo_coords[m.cell_geo[cut]]                                        # (ncut, 4, 3)
    faces = [(1, 2, 3), (0, 2, 3), (0, 1, 3), (0, 1, 2)]
    pts = [X.reshape(-1, 3), (0.5 * (X[:, EA] + X[:, EB])).reshape(-1, 3)] + [X[:, f].mean(axis=1) for f in faces]
    Xall = m.geo_coords[m.cell_geo]
    lo, hi = Xall.reshape(-1, 3).min(0), Xall.reshape(-1, 3).max(0)
    mid = 0.5 * (lo + hi)
    gx, gy = np.meshgrid(np.linspace(lo[0], hi[0], 33), np.linspace(lo[1], hi[1], 33), indexing="ij")
    pts.append(np.column_stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)]))                  # the row z = 0
    pts.append(np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])]))
    fc = []
    for a in range(3):
        for v in (lo[a], hi[a]):
            p = mid.copy()
            p[a] = v
            fc.append(p)
    pts.append(np.array(fc))
    g = np.meshgrid(*(np.linspace(lo[a], hi[a], 13) for a in range(3)), indexing="ij")
    pts.append(np.column_stack([v.ravel() for v in g]))
    return np.unique(np.vstack(pts), axis=0), int(cut.sum())


VARIANTS = ("witness", "owned_only", "kept_cells")


@functools.lru_cache(maxsize=None)
def claims(name):
    """serial winner of every adversarial point and, per world and variant, how many ranks claim it and which cell they claim.
       witness     the product: the rank's locator cells (owned + witness layer), a claim where the winner is owned
       owned_only  the rule the witness layer replaces: the rank's owned cells alone
       kept_cells  the cells the rank keeps anyway (RankLayout.cells), a claim where the winner is owned"""
    fed = fe_data(name)
    pts, ncut = adversarial_points(name)
    br = Brute(fed.mesh)
    allc = np.arange(fed.mesh.ncell)
    subsets = {}
    for world in WORLDS:
        for r, lay in enumerate(layouts(name, world)):
            cells, owned = lay.locator_cells(fed)
            own = np.zeros(fed.mesh.ncell, dtype=bool)
            own[cells[owned]] = True
            subsets[world, r] = dict(witness=cells, owned_only=cells[owned], kept_cells=lay.cells, own=own)
    serial = np.empty(len(pts), dtype=np.int64)
    count = {(w, v): np.zeros(len(pts), dtype=int) for w in WORLDS for v in VARIANTS}
    cell = {(w, v): np.full(len(pts), -1, dtype=np.int64) for w in WORLDS for v in VARIANTS}
    for i in range(0, len(pts), 512):
        sl = slice(i, i + 512)
        M = br.lambdas(pts[sl]).min(-1)                                      # (chunk, ncell): ONE lambda function for both sides
        serial[sl] = elect(M, allc)
        for (world, r), s in subsets.items():
            for v in VARIANTS:
                w = elect(M[:, s[v]], s[v])
                mine = (w >= 0) & s["own"][np.maximum(w, 0)]
                count[world, v][sl] += mine
                cell[world, v][sl] = np.where(mine, w, cell[world, v][sl])
    return pts, ncut, serial, count, cell


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name", MESHES)
def test_every_point_is_claimed_exactly_once_by_the_owner_of_the_serial_winner(name, world):
    pts, ncut, serial, count, cell = claims(name)
    found = serial >= 0
    print(f"{name}, {world} ranks: {len(pts)} points ({ncut} cells at rank cuts), {found.sum()} in the mesh")
    assert ncut > 100 and found.sum() > 1000 and (~found).sum() > 100
    c, w = count[world, "witness"], cell[world, "witness"]
    assert np.array_equal(c, found.astype(int)), (np.nonzero(c != found)[0][:10], c[c != found][:10])
    assert np.array_equal(w, serial)                                         # the claimed global cell is the serial winner


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name", MESHES)
def test_the_points_bite_without_the_witness_layer(name, world, record_property):
    """The same check with the witness layer dropped must fail on these points - a vertex on a rank cut is accepted by owned cells of
    both ranks - or the points would not exercise the rule.  The intermediate variant (the cells a rank keeps anyway) is reported,
    not asserted (DESIGN.md 14 quotes it)."""
    pts, ncut, serial, count, cell = claims(name)
    found = (serial >= 0).astype(int)
    c = count[world, "owned_only"]
    double, missing = int((c > found).sum()), int((c < found).sum())
    k = count[world, "kept_cells"]
    kd, km = int((k > found).sum()), int((k < found).sum())
    kw = int(((k == found) & (cell[world, "kept_cells"] != serial)).sum())
    print(f"{name}, {world} ranks, {len(pts)} points: owned cells only {double} double / {missing} missing claims; "
          f"kept cells {kd} double / {km} missing / {kw} claimed in another cell than the serial winner")
    record_property("owned_only", (double, missing))
    record_property("kept_cells", (kd, km, kw))
    assert double + missing >= 1
    assert double >= 1
