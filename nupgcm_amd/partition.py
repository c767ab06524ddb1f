"""Mesh-partitioned execution of the hot path: every rank holds ITS cells, ITS rows and ITS slice of the state - nothing
global lives on a device (new work; the reference is single-device).  north_star: "the unstructured mesh is partitioned
across the 8 GPUs of one node with RCCL over xGMI carrying the Krylov global inner products and interface halo exchange".

Decomposition (owner computes, one ghost-cell layer):

  * rows     - `distributed.RowPartition`: contiguous blocks of the RCM-ordered inversion rows [u; p] and buoyancy rows;
  * cells    - a rank keeps every cell that touches one of its rows (C = C_inv + C_b).  Row-owner assembly
               (csrc/fe.hip: the lanes that own a CSR row walk the (cell, local DoF) pairs carrying it) then produces the
               owned rows of every matrix and right-hand side completely and touches no other row: no atomics, no
               reduction over ranks, the same bits as the one-GPU assembly for every owned entry;
  * vectors  - a field lives as [ owned | solver ghosts | further ghosts ]: the solver ghosts are the off-rank columns of
               the owned rows (what the Krylov SpMV needs: the solvers work on the leading [owned | solver ghosts] VIEW of
               the state vector, no copy), the further ghosts are the remaining DoFs of the rank's cells (what the element
               kernels read: advection velocity, buoyancy gradient for the closures).  Two halo plans per field fill them -
               the solver's own (every Krylov iteration) and the extra one (once after a solve);
  * state    - never replicated and never all-gathered: after a solve the ghosts are refreshed from their owners
               (two ghost-sized messages) where the replicated design moved 8 N bytes per step;
  * closures - kappa_v (every step) and nu (every 10th step) are re-evaluated and K_v / A re-assembled on the rank's cells
               only, straight into the rank's row block (src/model.jl:160-170,229-261).

Host side: every rank still builds the global FEData (mesh topology, RCM, DoF tables - integer index work at set-up) to
derive its layout; everything that touches values is local and on the device."""
from __future__ import annotations

import os
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

from . import _lib as L
from .architectures import DeviceCSR, DeviceVector
from .assembly import DeviceFE
from .distributed import Halo, RowPartition, halo_plan
from .evolution import collect_evolution_LHS_into, evolution_parameter
from .fe import DeviceTables
from .inputs import SurfaceFluxBC
from .iterative_solvers import CgWorkspace, Diagonal, GmresWorkspace, IterativeSolverToolkit
from .model import Model
from .timesteppers import BDF1


class NodePartition:
    """Ownership by mesh NODE: the P2 nodes are swept in reverse-Cuthill-McKee order of the node graph and cut into
    `nranks` consecutive chunks of equal SpMV work (non-zeros of the inversion rows a node carries); every DoF - velocity
    components, pressure, buoyancy - belongs to the rank of its node.  All fields are therefore cut along the SAME surfaces:
    a rank's pressure rows sit where its velocity rows sit, its buoyancy rows too, and the ghost layer of every matrix is the
    one layer of cells across those surfaces (`distributed.RowPartition` cuts each field's own RCM sequence separately,
    which leaves e.g. all surface nodes with the last rank).  Same interface as RowPartition where partition.py uses it."""

    def __init__(self, fe_data, nranks, node_owner=None):
        """node_owner: an ownership given from outside (a coarser multigrid level inherits the owner of the fine node each of
        its nodes coincides with) instead of the work-balanced cut of this mesh's own RCM sweep"""
        from scipy.sparse.csgraph import reverse_cuthill_mckee
        m, t, d = fe_data.mesh, fe_data.tables, fe_data.dofs
        self.nu, self.np, self.nb, self.nranks = d.nu, d.np, d.nb, int(nranks)
        self.n_full, self.n_surf = d.n_full, d.n_surf
        if node_owner is None:
            order = np.asarray(reverse_cuthill_mckee(sp.csr_matrix(d.adj2), symmetric_mode=True), dtype=np.int64)
            rowlen = np.diff(fe_data.pattern_A()[0]).astype(np.float64)
            w = np.zeros(m.nn)
            for a in range(3):
                on = t.u_pos[:, a] >= 0
                w[on] += rowlen[t.u_pos[on, a]]
            on = t.p_pos >= 0
            w[:m.nv][on] += rowlen[t.p_pos[on]]
            cum = np.cumsum(w[order])
            cuts = np.searchsorted(cum, cum[-1] * np.arange(1, nranks) / nranks, side="left")
            node_owner = np.empty(m.nn, dtype=np.int32)
            node_owner[order] = np.searchsorted(cuts, np.arange(m.nn), side="right").astype(np.int32)
        else:
            node_owner = np.ascontiguousarray(node_owner, dtype=np.int32)
            if node_owner.shape != (m.nn,):
                raise ValueError("NodePartition: one owner per P2 node")
        self.node_owner = node_owner
        self._inv_owner = np.empty(d.nu + d.np, dtype=np.int32)
        for a in range(3):
            on = t.u_pos[:, a] >= 0
            self._inv_owner[t.u_pos[on, a]] = node_owner[on]
        on = t.p_pos >= 0
        self._inv_owner[t.p_pos[on]] = node_owner[:m.nv][on]
        nbn = len(t.b_pos)
        on = t.b_pos >= 0
        self._b_owner = np.empty(d.nb, dtype=np.int32)
        self._b_owner[t.b_pos[on]] = node_owner[:nbn][on]

    def inv_owner(self):
        return self._inv_owner

    def b_owner(self):
        return self._b_owner

    def inv_owned(self, r):
        return np.nonzero(self._inv_owner == r)[0]

    def b_owned(self, r):
        return np.nonzero(self._b_owner == r)[0]

    def n_own_u(self, r):
        return int((self._inv_owner[:self.nu] == r).sum())

    def local_nodes(self, r):
        """(full nodes, surface nodes) whose rows rank r owns: they lead its local numbering in this order (ascending global
        ids keep [x y z of full nodes | x y of surface nodes | other u | p])"""
        own = self._inv_owner[:self.nu] == r
        nf3, nbr = 3 * self.n_full, 3 * self.n_full + 2 * self.n_surf
        a, b = int(own[:nf3].sum()), int(own[nf3:nbr].sum())
        assert a % 3 == 0 and b % 2 == 0
        return a // 3, b // 2


class FieldLayout:
    """Local numbering of one field on one rank: [owned | solver ghosts | further ghosts]."""

    def __init__(self, n_global, owned, g_sol, g_ext):
        self.owned, self.g_sol, self.g_ext = owned, g_sol, g_ext
        self.n_own, self.n_sol, self.n_loc = len(owned), len(owned) + len(g_sol), len(owned) + len(g_sol) + len(g_ext)
        self.lut = np.full(n_global, -1, dtype=np.int64)
        self.lut[owned] = np.arange(self.n_own)
        self.lut[g_sol] = self.n_own + np.arange(len(g_sol))
        self.lut[g_ext] = self.n_sol + np.arange(len(g_ext))

    def globals(self):
        return np.concatenate([self.owned, self.g_sol, self.g_ext])


def _by_owner(ids, owner):
    ids = np.asarray(ids, dtype=np.int64)
    return ids[np.lexsort((ids, owner[ids]))]


class RankLayout:
    """What rank `rank` keeps: its cells and the local numberings of both fields.  Pure host logic (numpy) - exercised on
    CPU by tests/test_partition.py."""

    def __init__(self, fe_data, part, rank):
        t, d = fe_data.tables, fe_data.dofs
        self.rank, self.part = rank, part
        nc = len(t.cell_p)
        inv_ids = np.concatenate([t.cell_u.reshape(nc, 30), t.cell_p], axis=1).astype(np.int64)     # (nc, 34), < 0: constrained
        b_ids = t.cell_b.astype(np.int64)
        own_inv, own_b = part.inv_owner(), part.b_owner()
        self.owner_inv, self.owner_b = own_inv, own_b
        mine_i = np.zeros(d.nu + d.np + 1, dtype=bool)            # (+1: slot for the negative codes)
        mine_i[:-1] = own_inv == rank
        mine_b = np.zeros(d.nb + 1, dtype=bool)
        mine_b[:-1] = own_b == rank
        c_inv = mine_i[np.where(inv_ids >= 0, inv_ids, -1)].any(axis=1)
        c_b = mine_b[np.where(b_ids >= 0, b_ids, -1)].any(axis=1)
        self.cells = np.nonzero(c_inv | c_b)[0]
        self.n_cells_inv, self.n_cells_b = int(c_inv.sum()), int(c_b.sum())
        # owner of a CELL (sampling: which rank reports a point that lies in it): the lowest rank among the owners of its free
        # inversion and buoyancy DoFs - each of those ranks keeps the cell (it touches one of its rows), so the owner always holds the
        # cell's tables and, after refresh_ghosts, its values.  A cell without any free DoF is given to rank 0 (see locator_cells).
        big = np.iinfo(np.int32).max
        o_i = np.where(inv_ids >= 0, own_inv[np.maximum(inv_ids, 0)], big).min(axis=1)
        o_b = np.where(b_ids >= 0, own_b[np.maximum(b_ids, 0)], big).min(axis=1)
        self.cell_owner = np.minimum(o_i, o_b)
        self.cell_owner[self.cell_owner == big] = 0
        self.cell_owner = self.cell_owner.astype(np.int32)

        def layout(ids, c_rows, owned, owner, n):
            sol = np.unique(ids[c_rows][ids[c_rows] >= 0])
            sol = sol[owner[sol] != rank]
            allc = np.unique(ids[self.cells][ids[self.cells] >= 0])
            ext = allc[owner[allc] != rank]
            ext = np.setdiff1d(ext, sol, assume_unique=True)
            return FieldLayout(n, owned, _by_owner(sol, owner), _by_owner(ext, owner))

        self.inv = layout(inv_ids, c_inv, self._interior_first(fe_data, part, rank, part.inv_owned(rank), own_inv), own_inv, d.nu + d.np)
        self.b = layout(b_ids, c_b, part.b_owned(rank), own_b, d.nb)
        self.n_own_u = part.n_own_u(rank) if hasattr(part, "n_own_u") else int(part.u_bounds[rank + 1] - part.u_bounds[rank])

    @staticmethod
    def _interior_first(fe_data, part, rank, owned, owner):
        """Local order of the owned inversion rows: within each class of the node-block numbering - (x, y, z) triples of full nodes,
        (x, y) pairs of surface nodes, the other velocity rows, the pressure rows - the NODES none of whose rows reads an off-rank
        column come first, the nodes on the rank's boundary last, each group in ascending global order.  The SpMV tiles are runs of
        consecutive local rows, and a tile with one ghost column has to wait for the halo exchange: in ascending global order the
        boundary nodes are spread over the whole range whenever the sweep that numbers the DoFs and the sweep that cuts the ranks
        are not the same (they are separate RCM runs: velocity mass graph, pressure mass graph, node graph) - rank 4 of 8 of bowl3D
        h = 0.02 had 106 of 2 606 tiles without a ghost column; with the boundary nodes last the interior tiles are what runs beside
        the exchange.  MEASURED (profiles/r05_dist_cycle.txt, same box): 1 010 of 2 612 tiles interior instead of 106 - but the
        Arnoldi kernel gets SLOWER (35.2 -> 38.5 us: the boundary nodes collected at the end of each class gather from all over the
        range) and the two-launch form costs 9.5 us more than exchanging first (83.6 against 74.1 us per iteration): OFF by
        default, NPG_PART_INTERIOR_FIRST=1 turns it on (for a wire slow enough that hiding it pays for the split)."""
        if os.environ.get("NPG_PART_INTERIOR_FIRST", "0") != "1" or len(owned) == 0 or not isinstance(part, NodePartition):
            return owned
        d = fe_data.dofs
        rp, ci, _ = fe_data.pattern_A()
        rp = np.asarray(rp, dtype=np.int64)
        off = (owner[np.asarray(ci)] != rank).astype(np.int64)
        cs = np.concatenate([[0], np.cumsum(off)])
        row_bnd = (cs[rp[owned + 1]] - cs[rp[owned]]) > 0                      # owned row reads an off-rank column
        nf3, nbr = 3 * int(getattr(d, "n_full", 0)), 3 * int(getattr(d, "n_full", 0)) + 2 * int(getattr(d, "n_surf", 0))
        # node key of every owned row: rows of one node share it (ownership is by node, so a node's rows are all here or none)
        key = np.where(owned < nf3, owned // 3, np.where(owned < nbr, nf3 + (owned - nf3) // 2, nbr + owned))
        cls = np.where(owned < nf3, 0, np.where(owned < nbr, 1, np.where(owned < d.nu, 2, 3)))
        uk, inv = np.unique(key, return_inverse=True)
        node_bnd = np.zeros(len(uk), dtype=bool)
        np.logical_or.at(node_bnd, inv, row_bnd)
        order = np.lexsort((owned, node_bnd[inv], cls))                       # class, then interior before boundary, then global id
        return owned[order]

    def locator_cells(self, fe_data):
        """(cells, owned): the cells of this rank's point locator, ascending global ids, and the mask of the ones it OWNS
        (cell_owner == rank).  The others are the WITNESS layer: every cell that shares at least one geometric vertex
        (mesh.cell_geo - where the cell lies, not the periodic master of its vertices) with an owned cell.  Witness cells carry
        geometry only and are never evaluated; they take part in the election of a point's cell (largest min lambda, ties to the lowest
        global id) so that every rank that could report a point sees every cell that accepts it, and a point is reported only where
        the winner is owned - exactly once over the ranks.
        Cells without a free DoF belong to rank 0.  No rank keeps such a cell (RankLayout.cells lists cells that touch an owned row),
        so it could not be evaluated; the choice made here is to ASSERT that every owned cell is kept - true of every mesh of this
        project, whose pressure space pins one vertex at most - rather than to add Dirichlet-only cells to rank 0's engine."""
        cg = fe_data.mesh.cell_geo
        own = self.cell_owner == self.rank
        assert np.isin(np.nonzero(own)[0], self.cells, assume_unique=True).all(), \
            "a cell without free DoFs is owned by rank 0 but kept by no rank: sampling cannot evaluate it"
        touched = np.zeros(int(cg.max()) + 1, dtype=bool)
        touched[cg[own].ravel()] = True
        cells = np.nonzero(touched[cg].any(axis=1))[0]
        return cells, own[cells]

    def ghost_nodes(self, fe_data):
        """(first local column, components) of every velocity NODE among this rank's solver ghosts whose components are all ghosts
        here: in the node-block numbering a full node's DoFs are 3c, 3c + 1, 3c + 2 and a surface node's 3 n_full + 2c, + 1, and the
        ghosts are ordered by (owner, global id) - ownership is by node - so the components of a ghost node are adjacent columns.
        What npg_csr_set_ghost_nodes takes (the windowed tiles then keep owned-ghost couplings as node records)."""
        d = fe_data.dofs
        g = np.asarray(self.inv.g_sol, dtype=np.int64)
        nf3, nbr = 3 * int(getattr(d, "n_full", 0)), 3 * int(getattr(d, "n_full", 0)) + 2 * int(getattr(d, "n_surf", 0))
        first, ncomp = [], []
        if len(g) >= 3:
            k = np.nonzero((g[:-2] < nf3) & (g[:-2] % 3 == 0) & (g[1:-1] == g[:-2] + 1) & (g[2:] == g[:-2] + 2))[0]
            first.append(self.inv.n_own + k)
            ncomp.append(np.full(len(k), 3))
        if len(g) >= 2:
            k = np.nonzero((g[:-1] >= nf3) & (g[:-1] < nbr) & ((g[:-1] - nf3) % 2 == 0) & (g[1:] == g[:-1] + 1))[0]
            first.append(self.inv.n_own + k)
            ncomp.append(np.full(len(k), 2))
        if not first:
            return np.zeros(0, np.int32), np.zeros(0, np.int32)
        first, ncomp = np.concatenate(first), np.concatenate(ncomp)
        o = np.argsort(first, kind="stable")
        return first[o].astype(np.int32), ncomp[o].astype(np.int32)

    def local_tables(self, fe_data) -> DeviceTables:
        t = fe_data.tables
        cu, cp, cb = t.cell_u[self.cells], t.cell_p[self.cells], t.cell_b[self.cells]
        lu = np.where(cu >= 0, self.inv.lut[np.maximum(cu, 0)], cu)
        lp = np.where(cp >= 0, self.inv.lut[np.maximum(cp, 0)], cp)
        lb = np.where(cb >= 0, self.b.lut[np.maximum(cb, 0)], cb)
        assert (lu[cu >= 0] >= 0).all() and (lp[cp >= 0] >= 0).all() and (lb[cb >= 0] >= 0).all()
        return DeviceTables(cell_u=np.ascontiguousarray(lu, dtype=np.int32), cell_p=np.ascontiguousarray(lp, dtype=np.int32),
                            cell_b=np.ascontiguousarray(lb, dtype=np.int32), u_diri=t.u_diri, b_diri=t.b_diri,
                            u_pos=None, p_pos=None, b_pos=None)

    def local_pattern(self, pattern, rows: FieldLayout, cols: FieldLayout, solver_cols=True):
        """rows `rows.owned` of a global CSR pattern in local numbering; solver_cols: the column space is the solver's
        [owned | solver ghosts] (square systems), else the full local numbering (B: inversion rows x buoyancy columns)."""
        rp, ci, shape = pattern
        P = sp.csr_matrix((np.ones(len(ci), dtype=np.int8), ci, rp), shape=shape)[rows.owned]
        lc = cols.lut[P.indices]
        ncol = cols.n_sol if solver_cols else cols.n_loc
        assert (lc >= 0).all() and (lc < ncol).all()
        Q = sp.csr_matrix((P.data, lc, P.indptr), shape=(rows.n_own, ncol))
        Q.sort_indices()
        return Q.indptr.astype(np.int64), Q.indices.astype(np.int32), Q.shape


class _LocalMesh:
    """The slice of fe.Mesh that assembly.DeviceFE and the coefficient evaluation read, restricted to a rank's cells."""

    def __init__(self, mesh, cells):
        self.cells_global = cells
        self.grad_lambda = np.ascontiguousarray(mesh.grad_lambda[cells])
        self.detJ = np.ascontiguousarray(mesh.detJ[cells])
        self.q_w, self.q_lam = mesh.q_w, mesh.q_lam
        self.N2, self.dN2, self.N1, self.dN1 = mesh.N2, mesh.dN2, mesh.N1, mesh.dN1
        self._X = mesh.geo_coords[mesh.cell_geo[cells]]            # (ncell, 4, 3) every cell's own vertex coordinates
        self.ncell = len(cells)

    def quad_points(self):
        return np.einsum("qk,cki->cqi", self.q_lam, self._X)

    def h_cells(self):
        X = self._X
        return np.linalg.norm(X[:, :, None, :] - X[:, None, :, :], axis=-1).max(axis=(1, 2))


class LocalFEData:
    """Quacks like fe.FEData for assembly.DeviceFE: a rank's cells with DoF tables in the rank's local numbering."""

    def __init__(self, fe_data, lay: RankLayout):
        self.mesh = _LocalMesh(fe_data.mesh, lay.cells)
        self.spaces = SimpleNamespace(b_order=fe_data.spaces.b_order)
        self.tables = lay.local_tables(fe_data)
        self.dofs = SimpleNamespace(nu=lay.inv.n_loc, np=0, nb=lay.b.n_loc)


class _Comm:
    """The few host-level reductions a timestep needs beside the solvers' own (blow-up guard, CFL step)."""

    def __init__(self, ctx):
        self.ctx = ctx

    def any(self, flag):
        return self.ctx.allreduce_sum([1.0 if flag else 0.0])[0] > 0.0

    def min(self, value):
        v = np.zeros(self.ctx.nranks)
        v[self.ctx.rank] = value
        return float(self.ctx.allreduce_sum(v).min())

    def max(self, value):
        v = np.zeros(self.ctx.nranks)
        v[self.ctx.rank] = value
        return float(self.ctx.allreduce_sum(v).max())


class PartitionedSolverToolkit:
    """IterativeSolverToolkit of a rank's row block.  `x` is the rank's state vector [owned | solver ghosts | further
    ghosts]; the Krylov solver works on its leading view `x_sol` (warm start included) and the ghosts are refreshed from
    their owners when it returns."""

    def __init__(self, A, P, y, workspace, kwargs, label, x, lay: FieldLayout, halo_sol, halo_ext):
        self.A, self.P, self.y, self.workspace, self.kwargs, self.label = A, P, y, workspace, dict(kwargs), label
        self.x, self.lay, self.halo, self.halo_ext = x, lay, halo_sol, halo_ext
        self.x_sol = x.view(0, lay.n_sol)
        self.x_own = x.view(0, lay.n_own)

    def refresh_ghosts(self):
        self.halo.exchange(self.x_sol)
        if self.halo_ext is not None:
            self.halo_ext.exchange(self.x)

    def solve(self):
        self.workspace.solve(self.A, self.y, self.x_sol, self.P, **self.kwargs)
        self.refresh_ghosts()


class PartitionedState:
    """model.state of a partitioned model: u, p, b in the native (Gridap) DoF order, gathered from the ranks' owned
    slices.  COLLECTIVE - every rank must read the same attribute (diagnostics, checkpoints, tests)."""

    def __init__(self, model):
        self._m = model

    def _gather(self, x, lay, n):
        m = self._m
        parts = [None] * m.dist.get_world_size()
        m.dist.all_gather_object(parts, (lay.owned, x.view(0, lay.n_own).to_host()))
        full = np.empty(n)
        for ids, vals in parts:
            full[ids] = vals
        return full

    def _inv(self):
        d = self._m.fe_data.dofs
        full = self._gather(self._m.inversion.solver.x, self._m.layout.inv, d.nu + d.np)
        return full[d.inv_p_inversion]

    @property
    def u(self):
        return self._inv()[:self._m.fe_data.dofs.nu]

    @property
    def p(self):
        return self._inv()[self._m.fe_data.dofs.nu:]

    @property
    def b(self):
        d = self._m.fe_data.dofs
        return self._gather(self._m.b_vec, self._m.layout.b, d.nb)[d.inv_p_b]


def halo_plans(dist, rank, lay: FieldLayout, owner):
    """(solver plan, extra plan) of one field - host logic, collective over `dist` (any backend; exercised with gloo on CPU).
    The extra ghosts sit behind [owned | solver ghosts]: for their plan that whole leading part is the "owned" segment
    (send indices only ever name truly owned entries)."""
    allg = [None] * dist.get_world_size()
    dist.all_gather_object(allg, (lay.g_sol, lay.g_ext))
    return (halo_plan(rank, lay.owned, owner, [a[0] for a in allg]), halo_plan(rank, lay.owned, owner, [a[1] for a in allg]))


def _make_halos(ctx, dist, rank, lay: FieldLayout, owner):
    plan_s, plan_e = halo_plans(dist, rank, lay, owner)
    return Halo(ctx, lay.n_own, len(lay.g_sol), plan_s), Halo(ctx, lay.n_sol, len(lay.g_ext), plan_e)


def partitioned_model(arch, fe_data, params, forcings, ts, dist, atol=1e-6, rtol=1e-6, itmax=0, memory=20, reorth_eta=0.1,
                      block_nodes=None, first_step_lhs="bdf1", element_precision=None, b0=None, partition="node"):
    """Model(arch, params, forcings, fe_data, InversionToolkit(...), EvolutionToolkit(...), ts) with the mesh, the matrices
    and the state partitioned over the ranks of `dist` (torch.distributed, initialised).  Call on every rank.  Mirrors
    src/inversion.jl:20-94 and src/evolution.jl:62-126 on the rank's cells and rows; the reference's GPU preconditioner
    Diagonal(1/h^dim) uses the GLOBAL median edge length (src/inversion.jl:42-54)."""
    from .architectures import comm_unique_id
    if getattr(fe_data.mesh, "dim", 3) != 3:
        raise NotImplementedError("partitioned_model: tetrahedral meshes only (the embedded 2-D meshes run on one GPU)")
    ctx = arch.ctx
    rank, world = dist.get_rank(), dist.get_world_size()
    if ctx.nranks != world:
        ids = [comm_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(ids, src=0)
        ctx.comm_init(ids[0], rank, world)
    d = fe_data.dofs
    part = (NodePartition(fe_data, world) if partition == "node" else
            RowPartition(d.nu, d.np, d.nb, world, d.n_full, d.n_surf))
    # every rank must own rows of both systems: a rank left empty (tiny mesh, many ranks) would fail alone in npg_gmres_create
    # while the others wait in a collective - all ranks see the same partition, so all of them raise together here
    counts_i = np.bincount(part.inv_owner(), minlength=world)
    counts_b = np.bincount(part.b_owner(), minlength=world)
    if counts_i.min() == 0 or counts_b.min() == 0:
        raise ValueError(f"partitioned_model: {world} ranks leave a rank without rows (inversion rows per rank {counts_i.tolist()}, "
                         f"buoyancy rows {counts_b.tolist()}): use fewer ranks for this mesh")
    lay = RankLayout(fe_data, part, rank)
    lfd = LocalFEData(fe_data, lay)
    fe = DeviceFE(ctx, lfd)
    if element_precision is not None:
        fe.set_precision(element_precision)
    full_stress = callable(forcings.nu) or forcings.eddy_param.is_on
    # ---- inversion (src/inversion.jl:20-94) --------------------------------------------------------------------------
    fe.set_coeff("nu", forcings.nu)
    fe.set_coeff("f", params.f)
    a2e2 = params.alpha ** 2 * params.eps ** 2
    rp, ci, shp = lay.local_pattern(fe_data.pattern_A(structural=full_stress), lay.inv, lay.inv)
    A = DeviceCSR.from_pattern(ctx, shp[0], shp[1], rp, ci)
    fe.assemble(L.NPG_MAT_A, A, scale=a2e2, full_stress=full_stress)
    if block_nodes is None and os.environ.get("NPG_BLOCK_NODES"):
        block_nodes = os.environ["NPG_BLOCK_NODES"] != "0"          # tuning / debugging override
    if block_nodes is None:
        block_nodes = d.nu + d.np >= 100000
    if block_nodes and not full_stress:
        if hasattr(lay, "ghost_nodes") and isinstance(part, NodePartition) and os.environ.get("NPG_GHOST_NODES", "1") != "0":
            A.set_ghost_nodes(*lay.ghost_nodes(fe_data))   # (round 5) ghost nodes as record columns of the windowed tiles
        A.block_nodes(*part.local_nodes(rank))             # owned nodes lead the local numbering
    elif block_nodes and sum(part.local_nodes(rank)) > 0 and os.environ.get("NPG_PACK_NODES", "1") != "0":
        A.pack_nodes(*part.local_nodes(rank))              # full-stress form: record-form companion (follows re-assembly)
    rp, ci, shp = lay.local_pattern(fe_data.pattern_B(), lay.inv, lay.b, solver_cols=False)
    B = DeviceCSR.from_pattern(ctx, shp[0], shp[1], rp, ci)
    b0v = DeviceVector(ctx, lay.inv.n_own)
    fe.assemble(L.NPG_MAT_B, B, scale=1.0 / params.alpha, lift=b0v)
    wind = np.zeros(d.nu + d.np)                           # build_b_inversion, src/inversion.jl:226-249 (host, surface only)
    for comp, tau in ((0, forcings.tau_x), (1, forcings.tau_y)):
        if callable(tau) or float(tau) != 0.0:
            fn = tau if callable(tau) else (lambda x, c=float(tau): np.full(x.shape[:-1], c))
            load = fe_data.mesh.surface_load(lambda x: params.alpha * fn(x))
            pos = fe_data.tables.u_pos[:, comp]
            wind[pos[pos >= 0]] += load[pos >= 0]
    if np.any(wind != 0.0):
        b0v.axpby(1.0, DeviceVector.from_host(ctx, wind[lay.inv.owned]), 1.0)
    h_sol_i, h_ext_i = _make_halos(ctx, dist, rank, lay.inv, lay.owner_inv)
    ws = GmresWorkspace(ctx, lay.inv.n_own, memory=memory)
    L.check(L.lib().npg_gmres_set_halo(ws.h, h_sol_i.h))
    x_inv = DeviceVector(ctx, lay.inv.n_loc)
    x_inv.fill(0.0)
    h = fe_data.mesh.median_edge_length()
    kw = dict(atol=atol, rtol=rtol, itmax=itmax, history=True, verbose=0, restart=True, reorth_eta=reorth_eta)
    inv = SimpleNamespace(arch=arch, B=B, b=b0v)
    inv.solver = PartitionedSolverToolkit(A, Diagonal(scalar=1.0 / h ** getattr(fe_data.mesh, "dim", 3), n=lay.inv.n_own), DeviceVector(ctx, lay.inv.n_own),
                                          ws, kw, "Inversion", x_inv, lay.inv, h_sol_i, h_ext_i)
    # ---- evolution (src/evolution.jl:62-126) -------------------------------------------------------------------------
    fe.set_coeff("kappa_h", forcings.kappa_h)
    fe.set_coeff("kappa_v", forcings.kappa_v)
    nbl, nbo = lay.b.n_loc, lay.b.n_own
    pat_b = lay.local_pattern(fe_data.pattern_b(), lay.b, lay.b)
    proto = DeviceCSR.from_pattern(ctx, pat_b[2][0], pat_b[2][1], pat_b[0], pat_b[1])
    ev = SimpleNamespace(arch=arch, fe=fe, fe_data=fe_data, params=params, forcings=forcings)
    ev.rhs_M, ev.rhs_h, ev.rhs_v = (DeviceVector(ctx, nbl) for _ in range(3))       # owned entries meaningful
    for v in (ev.rhs_M, ev.rhs_h, ev.rhs_v):
        v.fill(0.0)
    ev.M = fe.assemble(L.NPG_MAT_M, proto.clone(), lift=ev.rhs_M)
    ev.Kh = fe.assemble(L.NPG_MAT_KH, proto.clone(), lift=ev.rhs_h)
    ev.Kv = fe.assemble(L.NPG_MAT_KV, proto.clone(), lift=ev.rhs_v)
    ev.rhs_diff = fe.rhs_diff(params.N2, DeviceVector(ctx, nbl))
    flux = np.zeros(d.nb)                                   # build_rhs_flux, src/evolution.jl:280-296
    bc = forcings.b_surface_bc
    if isinstance(bc, SurfaceFluxBC):
        fn = bc.flux if callable(bc.flux) else (lambda x, c=float(bc.flux): np.full(x.shape[:-1], c))
        load = fe_data.mesh.surface_load(lambda x: params.alpha * fn(x))[:fe_data.spaces.nb_nodes]
        pos = fe_data.tables.b_pos
        flux[pos[pos >= 0]] = load[pos >= 0]
    ev.rhs_flux = DeviceVector.from_host(ctx, flux[lay.b.globals()])
    ts1 = BDF1(t_start=ts.t_start, t_stop=ts.t_stop, dt=ts.dt) if first_step_lhs == "bdf1" else ts
    A_evo = proto.clone()
    P_evo = Diagonal(DeviceVector(ctx, nbo))
    collect_evolution_LHS_into(A_evo, P_evo, params, ts1, ev.M, ev.Kh, ev.Kv)
    h_sol_b, h_ext_b = _make_halos(ctx, dist, rank, lay.b, lay.owner_b)
    wsb = CgWorkspace(ctx, nbo)
    L.check(L.lib().npg_cg_set_halo(wsb.h, h_sol_b.h))
    b_vec = DeviceVector(ctx, nbl)
    b_vec.fill(0.0)
    y_full = DeviceVector(ctx, nbl)                         # the element kernels write all local rows; the solver reads the owned ones
    kwb = dict(atol=atol, rtol=rtol, itmax=itmax, history=True, verbose=0)
    ev.solver = PartitionedSolverToolkit(A_evo, P_evo, y_full.view(0, nbo), wsb, kwb, "Evolution", b_vec, lay.b, h_sol_b,
                                         h_ext_b)
    ev.solver.y_full = y_full
    model = PartitionedModel(arch, params, forcings, fe_data, inv, ev, ts, lay, dist, fe)
    if b0 is not None:
        model.set_b(b0)
    ctx.sync()                     # (the library's own stream; torch is only the launcher / bootstrap)
    dist.barrier()
    model.comm_layout = dict(n_owned_inv=lay.inv.n_own, n_ghost_inv=len(lay.inv.g_sol), n_ghost_inv_extra=len(lay.inv.g_ext),
                             n_owned_b=lay.b.n_own, n_ghost_b=len(lay.b.g_sol), n_ghost_b_extra=len(lay.b.g_ext),
                             cells=int(len(lay.cells)), cells_global=int(fe_data.mesh.ncell),
                             peers_inv=[int(q) for q in h_sol_i._keep["peers"]],
                             matrix_bytes=int(sum(M.stored_spmv_bytes() for M in (A, B, ev.M, ev.Kh, ev.Kv, A_evo))))
    return model


class PartitionedModel(Model):
    """Model whose mesh, matrices and state are partitioned (see the module docstring); run!, evolve!, invert! of model.py
    drive it unchanged - the differences are the hooks below."""

    def __init__(self, arch, params, forcings, fe_data, inversion, evolution, timestepper, layout, dist, fe):
        self.arch, self.params, self.forcings, self.fe_data = arch, params, forcings, fe_data
        self.inversion, self.evolution, self.timestepper = inversion, evolution, timestepper
        self.layout, self.dist, self.fe = layout, dist, fe
        self.partition = layout.part
        self.b_vec = evolution.solver.x
        self.state = PartitionedState(self)
        self.step_index = 1
        self.extrapolate_guess = False
        self.stats = []
        self._prev = None
        self._u_view = inversion.solver.x.view(0, layout.n_own_u)
        self.comm = _Comm(arch.ctx)

    def set_b(self, b):
        """set_b!(model, b) - src/model.jl:77-88 on the rank's slice (owned + both ghost layers at once)"""
        s, d = self.fe_data.spaces, self.fe_data.dofs
        vals = s.interpolate_b(b) if callable(b) else np.asarray(b, dtype=float)
        dev = np.empty(d.nb)
        dev[d.inv_p_b] = vals                                # native -> device (p_b) order
        self.b_vec.upload(dev[self.layout.b.globals()])
        return self

    def h_cells(self):
        return self.fe.fe_data.mesh.h_cells()

    def verify_transport(self):
        """End-to-end check of the communication layer on THIS hardware (collective; True on every rank or on none): a
        known function of the global DoF id is placed in the owned entries of scratch vectors, both halo plans of both fields
        run, and every ghost must hold its owner's value bit for bit; the small all-reduce must give the closed-form sum."""
        ctx, lay = self.arch.ctx, self.layout
        ok = True
        for f, sol in ((lay.inv, self.inversion.solver), (lay.b, self.evolution.solver)):
            g = f.globals()
            want = np.sin(0.001 * g) + 1e-3 * g
            x = DeviceVector(ctx, f.n_loc)
            x.fill(0.0)
            x.view(0, f.n_own).upload(want[:f.n_own])
            for rep in range(3):                         # both window slots and the acknowledgement path
                sol.halo.exchange(x.view(0, f.n_sol))
                if sol.halo_ext is not None:
                    sol.halo_ext.exchange(x)
            ok = ok and np.array_equal(x.to_host(), want)
        n = ctx.nranks
        s = ctx.allreduce_sum(np.arange(1.0, 6.0) * (ctx.rank + 1))
        ok = ok and np.array_equal(s, np.arange(1.0, 6.0) * n * (n + 1) / 2)
        # the verdict travels over the BOOTSTRAP channel (torch.distributed object collectives), never over the transport under
        # test: a broken all-reduce must not be able to hand different ranks different verdicts
        verdicts = [None] * self.dist.get_world_size()
        self.dist.all_gather_object(verdicts, bool(ok))
        return all(verdicts)

    def reassemble_A(self):
        """the eddy closure's refresh (src/model.jl:160-170): full-stress A on the rank's cells into the rank's rows"""
        prm = self.params
        self.fe.assemble(L.NPG_MAT_A, self.inversion.solver.A, scale=prm.alpha ** 2 * prm.eps ** 2, full_stress=True)


# ---- named workloads, partitioned ------------------------------------------------------------------------------------------
def example_model(arch, mesh_model, dist, dt=1e-3, t_stop=1e9, preconditioner="diagonal", **kw):
    """workloads.example_model (examples/bowl_mixing.jl:171-190) with the mesh partitioned over the ranks of `dist`.
    preconditioner="multigrid": `mesh_model` is the LABEL of a refined bowl mesh; its refinement hierarchy preconditions the
    inversion (finest level row-partitioned, coarser levels replicated)."""
    from . import workloads
    from .timesteppers import BDF2
    prm, frc = workloads.example_parameters()
    ts = BDF2(t_start=0.0, t_stop=t_stop, dt=dt)
    if preconditioner == "multigrid":
        hier = [workloads.example_fe_data(m) for m in workloads.bowl_hierarchy_models(mesh_model)]
        # two partitioned levels where the hierarchy has a third one to keep replicated (NPG_MG_DIST_LEVELS=1: only the finest)
        nlev = int(os.environ.get("NPG_MG_DIST_LEVELS", 2 if len(hier) >= 3 else 1))
        return use_multigrid(partitioned_model(arch, hier[-1], prm, frc, ts, dist, **kw), hier, distributed_levels=nlev)
    fed = workloads.example_fe_data(workloads.bowl_mesh_model(mesh_model) if isinstance(mesh_model, str) else mesh_model)
    return partitioned_model(arch, fed, prm, frc, ts, dist, **kw)


def channel_basin_model(arch, mesh_model, dist, surface="flux", itmax=1000, CFL_factor=0.8, element_precision="fp32",
                        atol=1e-6, rtol=1e-6, fe_data=None, invert_now=True, **kw):
    """workloads.channel_basin_model (scratch/run.jl:146-172: BASELINE configs[4]) with the mesh partitioned over the ranks
    of `dist`: x-periodic mesh, P1 buoyancy, full-stress A, BDF1 with the CFL step, both closures - each re-evaluated and
    re-assembled on the rank's own cells."""
    from . import workloads
    from .model import invert
    fed = fe_data if fe_data is not None else workloads.channel_basin_fe_data(mesh_model, surface)   # (fe_data: the caller's FEData of this mesh)
    prm, frc, _, _, dt, b0 = workloads.channel_basin_parameters(surface)
    ts = BDF1(t_start=0.0, t_stop=prm.mu_rho / prm.eps ** 2, dt=dt, adaptive=True, CFL_factor=CFL_factor)
    model = partitioned_model(arch, fed, prm, frc, ts, dist, atol=atol, rtol=rtol, itmax=itmax,
                              element_precision=element_precision, b0=b0, **kw)
    if invert_now:          # (a caller that swaps the inversion solver first - use_multigrid - inverts afterwards)
        invert(model)
    return model


# ---- multigrid-preconditioned inversion on the partitioned mesh -----------------------------------------------------------
class DistributedMultigridPreconditioner:
    """The geometric multigrid of multigrid.MultigridPreconditioner with its FINEST level distributed like the partitioned
    system and the coarser levels replicated (every rank runs the coarse part of the cycle redundantly on the all-reduced
    restricted residual; levels of <= a few 1e5 unknowns are latency-bound anyway).  Same algorithm, same parameters: the
    Braess-Sarazin step needs the ghosts of three kinds of vectors (whole vectors for A, velocity parts for D, pressure parts
    for G and S) - three halo plans - and ONE operator that is not a row block of something local: S = D Dinv G, whose rows
    reach through ghost velocity nodes.  T = Dinv G is formed on the owned rows, the rows a neighbour needs travel once at
    set-up, and S_own = D_own T follows.  The set-up of the distributed level is host-side scipy on the rank's block; with the
    eddy closure `refresh` repeats it on the re-assembled matrix (same layouts, new values; the coarser levels are re-assembled
    with the child-volume average of the fine viscosity, as on one GPU - `_refresh_coarse_levels_averaged`)."""

    def __init__(self, arch, params, forcings, hierarchy, model, omega=2.5, jacobi_weight=0.7, schur_sweeps=3, nu1=2, nu2=2,
                 coarse_sweeps=20, cycle="V", coarse_dense=None, distributed_levels=1, smoother=None, coarse_nu="average"):
        """distributed_levels: 1 = the finest level row-partitioned, every coarser level replicated; 2 = the level below it
        partitioned as well (a coarse node belongs to the rank that owns the fine node it coincides with; its rows are assembled
        on that rank's cells of the coarse mesh; P / R between the two levels are row blocks with halo plans of their own) -
        hierarchies of >= 3 levels.  `refresh` follows the eddy closure on both."""
        import ctypes as C
        from . import multigrid as mgm
        from .inversion import build_A_inversion
        if len(hierarchy) < 2:
            raise ValueError("DistributedMultigridPreconditioner: needs a refinement hierarchy (>= 2 levels)")
        if distributed_levels not in (1, 2):
            raise ValueError("distributed_levels: 1 or 2")
        if distributed_levels == 2 and len(hierarchy) < 3:
            raise ValueError("two distributed levels need a hierarchy of >= 3 levels (the coarsest stays replicated)")
        self.distributed_levels = distributed_levels
        self.coarse_nu = coarse_nu      # "average" | "inject": how the coarser levels follow the eddy closure (refresh)
        self._avg = None
        # "zline": the velocity blocks of the smoother are the unknowns of the nodes above one another (multigrid.line_blocks) -
        # on a partitioned level the part of each line that this rank owns (a line cut by a rank boundary smooths in pieces)
        self.smoother = smoother or os.environ.get("NPG_MG_SMOOTHER", "node")
        if self.smoother not in ("node", "zline"):
            raise ValueError(f"smoother = {self.smoother!r} (\"node\" or \"zline\")")
        ctx = arch.ctx
        self.ctx, self.arch = ctx, arch
        self.prm, self.frc, self.hierarchy = params, forcings, hierarchy
        h = C.c_void_p()
        L.check(L.lib().npg_precond_create(ctx.h, L.NPG_PC_MG, len(hierarchy), C.byref(h)))
        self.h, self._keep, self.levels = h, [], []
        full = callable(forcings.nu) or forcings.eddy_param.is_on      # (the eddy closure re-assembles A in the full-stress form)
        self._full = full
        # ---- replicated coarse levels: exactly MultigridPreconditioner's set-up --------------------------------------
        prev = None
        self.cA, self.cops = [], []
        for lev, fed in enumerate(hierarchy[:len(hierarchy) - distributed_levels]):
            d = fed.dofs
            A = build_A_inversion(arch, fed, params, forcings.nu, structural=full)
            ops = mgm._LevelOperators(ctx, fed, fed.pattern_A(structural=full), smoother=self.smoother).update(A)
            if not full and A.shape[0] >= 100000:
                A.block_nodes(d.n_full, d.n_surf)
            Pd = Rd = None
            if prev is not None:
                P = mgm.prolongation(prev, fed)
                Pd, Rd = DeviceCSR.from_scipy(ctx, P), DeviceCSR.from_scipy(ctx, sp.csr_matrix(P.T))
            self._keep += [Pd, Rd]
            self.cA.append(A)
            self.cops.append(ops)
            L.check(L.lib().npg_precond_mg_set_level(self.h, lev, A.h, int(d.nu), ops.G.h, ops.D.h, ops.Dinv.h, ops.S.h,
                                                     None if Pd is None else Pd.h, None if Rd is None else Rd.h))
            if os.environ.get("NPG_MG_SCALED_GRADIENT", "1") != "0" and ops.Gh is not None:
                L.check(L.lib().npg_precond_mg_set_scaled_gradient(self.h, lev, ops.Gh.h))
            self.levels.append(d.nu + d.np)
            prev = fed
        # ---- the distributed level(s) ----------------------------------------------------------------------------------
        fed, lay = hierarchy[-1], model.layout
        f = lay.inv
        dist, rank, world = model.dist, model.dist.get_rank(), model.dist.get_world_size()
        top = len(hierarchy) - 1
        lv0 = SimpleNamespace(fed=fed, lay=lay, part=model.partition, fe=model.fe, dist=dist, hx=model.inversion.solver.halo, st={})
        self._lv = [lv0]
        lv1 = None
        if distributed_levels == 2:
            # the level below: ownership inherited through the injection (a coarse node IS a fine node), rows assembled by an
            # engine over this rank's cells of the coarse mesh - what partitioned_model does for the finest level
            fed_c = hierarchy[-2]
            inj = mgm.injection(fed_c.mesh, fed.mesh, False)
            part_c = NodePartition(fed_c, world, node_owner=model.partition.node_owner[inj])
            counts = np.bincount(part_c.inv_owner(), minlength=world)
            if counts.min() == 0:
                raise ValueError(f"two distributed multigrid levels: a rank owns no row of the second level ({counts.tolist()})")
            lay_c = RankLayout(fed_c, part_c, rank)
            fe_c = DeviceFE(ctx, LocalFEData(fed_c, lay_c))
            fe_c.set_precision(model.fe.precision)
            fe_c.set_coeff("nu", forcings.nu)
            fe_c.set_coeff("f", params.f)
            rp, ci, shp = lay_c.local_pattern(fed_c.pattern_A(structural=full), lay_c.inv, lay_c.inv)
            A_c = DeviceCSR.from_pattern(ctx, shp[0], shp[1], rp, ci)
            fe_c.assemble(L.NPG_MAT_A, A_c, scale=params.alpha ** 2 * params.eps ** 2, full_stress=full)
            hx_c, _ = _make_halos(ctx, dist, rank, lay_c.inv, lay_c.owner_inv)
            lv1 = SimpleNamespace(fed=fed_c, lay=lay_c, part=part_c, fe=fe_c, dist=dist, hx=hx_c, st={}, A=A_c)
            self._lv.append(lv1)
            G1, D1, Dinv1, S1 = self._level_operators(lv1, first=True)
            fc = lay_c.inv
            Pg1 = mgm.prolongation(hierarchy[-3], fed_c)
            Pl1 = sp.csr_matrix(Pg1[fc.owned])
            ops1 = [DeviceCSR.from_scipy(ctx, M) for M in (G1, D1, sp.csr_matrix(Dinv1), S1, Pl1, sp.csr_matrix(Pl1.T))]
            lv1.ops = ops1
            L.check(L.lib().npg_precond_mg_set_level_dist(self.h, top - 1, A_c.h, int(lay_c.n_own_u), ops1[0].h, ops1[1].h, ops1[2].h,
                                                          ops1[3].h, ops1[4].h, ops1[5].h, hx_c.h, lv1.st["hu"].h, lv1.st["hp"].h))
            self.levels.append(fed_c.dofs.nu + fed_c.dofs.np)
        Gl, Dh, Dinv, Sl = self._level_operators(lv0, first=True)
        self.hx, self.hu, self.hp = lv0.hx, lv0.st["hu"], lv0.st["hp"]
        self._want, self._gp = lv0.st["want"], lv0.st["gp"]
        A_sol = model.inversion.solver.A
        if lv1 is None:
            Pg = mgm.prolongation(hierarchy[-2], fed)
            Pl = sp.csr_matrix(Pg[f.owned])
            ops = [DeviceCSR.from_scipy(ctx, M) for M in (Gl, Dh, sp.csr_matrix(Dinv), Sl, Pl, sp.csr_matrix(Pl.T))]
            self._fine_ops = ops
            L.check(L.lib().npg_precond_mg_set_level_dist(self.h, top, A_sol.h, int(lay.n_own_u), ops[0].h, ops[1].h,
                                                          ops[2].h, ops[3].h, ops[4].h, ops[5].h, self.hx.h, self.hu.h, self.hp.h))
        else:
            ops = [DeviceCSR.from_scipy(ctx, M) for M in (Gl, Dh, sp.csr_matrix(Dinv), Sl)]
            self._fine_ops = ops
            L.check(L.lib().npg_precond_mg_set_level_dist(self.h, top, A_sol.h, int(lay.n_own_u), ops[0].h, ops[1].h,
                                                          ops[2].h, ops[3].h, None, None, self.hx.h, self.hu.h, self.hp.h))
            # transfers between the two partitioned levels: row blocks with [owned | ghosts] column spaces and plans of their own
            fc, owner_c, owner_f = lv1.lay.inv, lv1.lay.owner_inv, lay.owner_inv
            Pg = sp.csr_matrix(mgm.prolongation(lv1.fed, fed))                   # n_fine x n_coarse, both in their device orders
            Rg = sp.csr_matrix(Pg.T)

            def row_block(M, rows, own_cols, owner_cols):
                """rows `rows` of M with the columns renumbered [own_cols | ghosts sorted by owner]; (block, ghost list)"""
                B = sp.csr_matrix(M[rows])
                used = np.unique(B.indices)
                gh = _by_owner(used[owner_cols[used] != rank], owner_cols) if len(used) else np.zeros(0, np.int64)
                lut = np.full(M.shape[1], -1, dtype=np.int64)
                lut[own_cols] = np.arange(len(own_cols))
                lut[gh] = len(own_cols) + np.arange(len(gh))
                lc = lut[B.indices]
                assert (lc >= 0).all()
                Q = sp.csr_matrix((B.data, lc, B.indptr), shape=(len(rows), len(own_cols) + len(gh)))
                Q.sort_indices()
                return Q, gh
            P_loc, gP = row_block(Pg, f.owned, fc.owned, owner_c)
            R_loc, gR = row_block(Rg, fc.owned, f.owned, owner_f)
            allg = [None] * world
            dist.all_gather_object(allg, (gP, gR))
            hP = Halo(ctx, fc.n_own, len(gP), halo_plan(rank, fc.owned, owner_c, [a[0] for a in allg]))
            hR = Halo(ctx, f.n_own, len(gR), halo_plan(rank, f.owned, owner_f, [a[1] for a in allg]))
            tr = [DeviceCSR.from_scipy(ctx, P_loc), DeviceCSR.from_scipy(ctx, R_loc)]
            self._keep += tr + [hP, hR]
            L.check(L.lib().npg_precond_mg_set_transfer_dist(self.h, top, tr[0].h, tr[1].h, hP.h, hR.h))
            self.layout_mg2 = dict(rows=int(fc.n_own), ghost_x=int(len(fc.g_sol)), ghost_P=int(len(gP)), ghost_R=int(len(gR)))
        self.levels.append(fed.dofs.nu + fed.dofs.np)
        L.check(L.lib().npg_precond_mg_set_params(self.h, float(omega), float(jacobi_weight), int(schur_sweeps), int(nu1),
                                                  int(nu2), int(coarse_sweeps)))
        L.check(L.lib().npg_precond_mg_set_cycle(self.h, {"V": 1, "W": 2}[cycle]))
        if coarse_dense is None:                 # as MultigridPreconditioner: scaled fp16 storage of the coarsest level's inverse
            coarse_dense = "fp16" if self.levels[0] <= 40000 else False
        if coarse_dense and os.environ.get("NPG_MG_COARSE_DENSE"):
            coarse_dense = os.environ["NPG_MG_COARSE_DENSE"]
        self._dense_mode = 0 if not coarse_dense else {"fp64": 1, "fp16": 3}.get(coarse_dense, 2)
        if self._dense_mode:
            L.check(L.lib().npg_precond_mg_set_coarse_dense(self.h, self._dense_mode))
        self.coarse_dense = bool(coarse_dense)
        self.params = dict(omega=omega, jacobi_weight=jacobi_weight, schur_sweeps=schur_sweeps, nu1=nu1, nu2=nu2,
                           coarse_sweeps=coarse_sweeps, cycle=cycle)
        self.layout_mg = dict(ghost_u=int(len(self._want)), ghost_p=int(len(self._gp)), S_nnz=int(Sl.nnz))
        self._inj = None

    def _level_operators(self, lv, first):
        """(G, D, Dinv, S) of a distributed level as host matrices in the level's local layouts, from the rank's rows of the
        level's CURRENT matrix (assembled afresh into a plain-CSR copy with whatever viscosity table the level's engine holds).
        lv: the level's (fed, lay, part, fe, dist, st).  Collective: the rows of T = Dinv G that belong to a neighbour's ghost
        velocity DoFs travel between the ranks.  The first call also fixes the layouts - ghost velocity / pressure lists, halo
        plans (lv.st) - which later calls reuse."""
        from . import multigrid as mgm
        ctx, params = self.ctx, self.prm
        fed, lay, part, dist = lv.fed, lv.lay, lv.part, lv.dist
        rank, world = dist.get_rank(), dist.get_world_size()
        full = self._full
        f = lay.inv
        nu_g = fed.dofs.nu
        nu_o, n_own, n_sol = lay.n_own_u, f.n_own, f.n_sol
        a2e2 = params.alpha ** 2 * params.eps ** 2
        if not first and lv.st.get("dev") is not None:
            return self._device_operators(lv)                                 # same layouts, new values: nothing leaves the device
        rp, ci, shp = lay.local_pattern(fed.pattern_A(structural=full), f, f)
        Ap = DeviceCSR.from_pattern(ctx, shp[0], shp[1], rp, ci)             # a plain-CSR copy of the rank's rows for the host
        lv.fe.assemble(L.NPG_MAT_A, Ap, scale=a2e2, full_stress=full)
        Ah = Ap.to_scipy_csr()
        # (Ap stays: the device plan re-assembles into it)
        g = f.globals()[:n_sol]                                              # global id of every local column
        ghost = np.arange(n_own, n_sol)
        gu_idx, gp_idx = ghost[g[ghost] < nu_g], ghost[g[ghost] >= nu_g]      # (kept in ghost order: sorted by owner, id)
        u_cols = np.concatenate([np.arange(nu_o), gu_idx])
        p_cols_A = np.concatenate([np.arange(nu_o, n_own), gp_idx])
        Atag = sp.csr_matrix((np.arange(1, len(ci) + 1, dtype=np.float64), ci, rp), shape=shp).tocsc()   # value positions + 1
        Ah = Ah.tocsc()
        G0 = sp.csr_matrix(Ah[:nu_o][:, p_cols_A])                            # own_u x [own_p | ghost p of A]
        Dh = sp.csr_matrix(Ah[nu_o:n_own][:, u_cols])                         # own_p x [own_u | ghost u]
        if self.smoother == "zline":
            if "lines" not in lv.st:                                          # this rank's pieces of the level's lines
                line_of = mgm.line_blocks(fed)[2][f.owned[:nu_o]]
                order = np.lexsort((np.arange(nu_o), line_of)).astype(np.int64)
                cut = np.concatenate([[0], np.flatnonzero(np.diff(line_of[order])) + 1, [nu_o]]).astype(np.int64)
                lv.st["lines"] = (cut, order)
            Dinv = mgm.line_block_inverse(sp.csr_matrix(Ah[:nu_o][:, :nu_o]), *lv.st["lines"])
        else:
            nfl, nsl = part.local_nodes(rank)
            Dinv = mgm.node_block_inverse(sp.csr_matrix(Ah[:nu_o][:, :nu_o]), nfl, nsl)
        # T = Dinv G on the owned velocity rows, columns as GLOBAL pressure ids; its ghost rows come from their owners
        T = sp.csr_matrix(Dinv @ G0)
        T = sp.csr_matrix((T.data, g[p_cols_A][T.indices], T.indptr), shape=(nu_o, fed.dofs.nu + fed.dofs.np))
        want = g[gu_idx]
        wants = [None] * world
        dist.all_gather_object(wants, want)
        lut_u = np.full(nu_g, -1, dtype=np.int64)
        lut_u[f.owned[:nu_o]] = np.arange(nu_o)
        replies = {}
        for q in range(world):
            if q == rank:
                continue
            mine = wants[q][lay.owner_inv[wants[q]] == rank]
            if len(mine):
                rows = T[lut_u[mine]]
                replies[q] = (mine, rows.indptr, rows.indices, rows.data)
        allrep = [None] * world
        dist.all_gather_object(allrep, replies)
        pos = {}
        for q in range(world):
            rep = allrep[q].get(rank) if q != rank else None
            if rep is not None:
                ids, rptr, rind, rdat = rep
                for k, gid in enumerate(ids):
                    pos[int(gid)] = (q, k)
        Text_rows = [T]
        if len(want):
            blocks = []
            for gid in want:                                                  # ghost rows in D's column order
                q, k = pos[int(gid)]
                ids, rptr, rind, rdat = allrep[q][rank]
                blocks.append((rind[rptr[k]:rptr[k + 1]], rdat[rptr[k]:rptr[k + 1]]))
            indptr = np.concatenate([[0], np.cumsum([len(b[0]) for b in blocks])])
            Tg = sp.csr_matrix((np.concatenate([b[1] for b in blocks]) if indptr[-1] else np.zeros(0),
                                np.concatenate([b[0] for b in blocks]) if indptr[-1] else np.zeros(0, dtype=np.int64), indptr),
                               shape=(len(want), T.shape[1]))
            Text_rows.append(Tg)
        Text = sp.vstack(Text_rows, format="csr")                             # rows [own_u | ghost u], global columns
        Sg = sp.csr_matrix(Dh @ Text)                                         # own_p x global ids
        own_p = f.owned[nu_o:]
        G0g = sp.csr_matrix((G0.data, g[p_cols_A][G0.indices], G0.indptr), shape=(nu_o, fed.dofs.nu + fed.dofs.np))
        if first:
            # pressure layout [own_p | ghost p]: everything G and S touch
            cols_used = np.union1d(np.unique(Sg.indices), g[p_cols_A])
            gp = cols_used[lay.owner_inv[cols_used] != rank]
            gp = gp[np.lexsort((gp, lay.owner_inv[gp]))]
            lut_p = np.full(fed.dofs.nu + fed.dofs.np, -1, dtype=np.int64)
            lut_p[own_p] = np.arange(len(own_p))
            lut_p[gp] = len(own_p) + np.arange(len(gp))
            lv.st.update(lut_p=lut_p, npl=len(own_p) + len(gp), want=want, gp=gp)
            # halo plans of the velocity-part and pressure-part vectors
            allg = [None] * world
            dist.all_gather_object(allg, (want, gp))
            own_u = f.owned[:nu_o]
            plan_u = halo_plan(rank, own_u, lay.owner_inv, [a[0] for a in allg])
            plan_p = halo_plan(rank, own_p, lay.owner_inv, [a[1] for a in allg])
            lv.st["hu"] = Halo(ctx, nu_o, len(want), plan_u)
            lv.st["hp"] = Halo(ctx, len(own_p), len(gp), plan_p)

        def to_p_layout(M_global_cols, pattern=None):
            M = sp.csr_matrix(M_global_cols)
            lc = lv.st["lut_p"][M.indices]
            if not (lc >= 0).all():
                raise RuntimeError("distributed multigrid: a re-assembled operator reaches a pressure column outside the level's layout")
            Q = sp.csr_matrix((M.data, lc, M.indptr), shape=(M.shape[0], lv.st["npl"]))
            Q.sort_indices()
            return Q
        Gl, Sl = to_p_layout(G0g), to_p_layout(Sg)
        if first and os.environ.get("NPG_MG_DIST_DEVICE", "1") != "0":
            # ---- the device plan of later refreshes (npg_csr_gather_values / _node_block_inverse or _line_block_inverse / _product
            # and a halo plan on the VALUES of T = Dinv G): index work on the patterns, done once ---------------------------------
            from .architectures import DeviceIndex
            one = lambda M: sp.csr_matrix((np.ones(M.nnz, dtype=np.float32), M.indices, M.indptr), shape=M.shape)
            G0t = sp.csr_matrix(Atag[:nu_o][:, p_cols_A])
            Gt = to_p_layout(sp.csr_matrix((G0t.data, g[p_cols_A][G0t.indices], G0t.indptr), shape=G0g.shape))
            Dt = sp.csr_matrix(Atag[nu_o:n_own][:, u_cols])
            assert np.array_equal(Gt.indices, Gl.indices) and np.array_equal(Dt.indices, Dh.indices)
            nfl, nsl = part.local_nodes(rank)
            blocks = None
            if self.smoother == "zline":                                      # the rank's pieces of the level's lines (round 5)
                cut, order = lv.st["lines"]
                piece_of = np.empty(nu_o, dtype=np.int64)
                piece_of[order] = np.repeat(np.arange(len(cut) - 1, dtype=np.int64), np.diff(cut))
                irp, icol = mgm._line_block_pattern(nu_o, cut, order, piece_of)
                blocks = (DeviceIndex(ctx, cut, nu_o + 1), DeviceIndex(ctx, order, max(nu_o, 1)))
            else:
                irp, icol = mgm._node_block_pattern(nu_o, nfl, nsl)
            Ip = sp.csr_matrix((np.ones(len(icol), dtype=np.float32), icol, irp), shape=(nu_o, nu_o))
            Tp = sp.csr_matrix(Ip @ one(Gl))
            Tp.sort_indices()
            p_glob = np.concatenate([own_p, lv.st["gp"]])                     # global id of every column of the pressure layout
            # what the neighbours want of my rows of T, in their order; the columns travel once as global ids
            out = {}
            for q in range(world):
                if q == rank:
                    continue
                mine = wants[q][lay.owner_inv[wants[q]] == rank]
                if len(mine):
                    rows = lut_u[mine]
                    cnt = np.diff(Tp.indptr)[rows]
                    pos = np.repeat(Tp.indptr[rows], cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
                    out[q] = (mine, cnt, p_glob[Tp.indices[pos]], pos)
            allout = [None] * world
            dist.all_gather_object(allout, {q: v[:3] for q, v in out.items()})
            peers = sorted(set(out) | {q for q in range(world) if q != rank and rank in allout[q]})
            send_ptr, send_idx, recv_ptr = [0], [], [0]
            grow = {}                                                         # ghost row gid -> (offset in the received stream, local columns)
            for q in peers:
                send_idx.append(out[q][3] if q in out else np.zeros(0, np.int64))
                send_ptr.append(send_ptr[-1] + len(send_idx[-1]))
                nrecv = 0
                if rank in allout[q]:
                    ids, cnt, cols = allout[q][rank]
                    off = np.concatenate([[0], np.cumsum(cnt)])
                    lc = lv.st["lut_p"][cols]
                    # (lc < 0: a column outside this rank's pressure layout - the row belongs to a ghost velocity unknown that only
                    #  this rank's VELOCITY rows reach, no row of D does: S never reads it, the entry is left out of T_ext below)
                    for k, gid in enumerate(ids):
                        grow[int(gid)] = (recv_ptr[-1] + off[k], lc[off[k]:off[k + 1]])
                    nrecv = int(off[-1])
                recv_ptr.append(recv_ptr[-1] + nrecv)
            nnz_own, nnz_g = int(Tp.nnz), int(recv_ptr[-1])
            assert sorted(grow) == sorted(int(x) for x in want)
            # T_ext = [my rows of T | the ghost rows in D's column order], every row ascending; its values come out of the vector
            # [my values | received values] through mapT
            rptr, cols_e, mapT = [Tp.indptr.astype(np.int64)], [Tp.indices.astype(np.int64)], [np.arange(nnz_own, dtype=np.int64)]
            gptr = [nnz_own]
            for gid in want:
                o, lc = grow[int(gid)]
                srt = np.argsort(lc, kind="stable")
                srt = srt[lc[srt] >= 0]
                cols_e.append(lc[srt])
                mapT.append(nnz_own + o + srt)
                gptr.append(gptr[-1] + len(srt))
            indptr_e = np.concatenate([rptr[0], np.asarray(gptr[1:], dtype=np.int64)])
            cols_e, mapT = np.concatenate(cols_e), np.concatenate(mapT)
            dev = SimpleNamespace(
                Ap=Ap, nfl=nfl, nsl=nsl, blocks=blocks,
                G=DeviceCSR.from_pattern(ctx, Gl.shape[0], Gl.shape[1], Gl.indptr, Gl.indices),
                D=DeviceCSR.from_pattern(ctx, Dh.shape[0], Dh.shape[1], Dh.indptr, Dh.indices),
                Dinv=DeviceCSR.from_pattern(ctx, nu_o, nu_o, irp, icol),
                T=DeviceCSR.from_pattern(ctx, nu_o, Gl.shape[1], Tp.indptr, Tp.indices),
                Text=DeviceCSR.from_pattern(ctx, nu_o + len(want), Gl.shape[1], indptr_e, cols_e.astype(np.int32)),
                S=DeviceCSR.from_pattern(ctx, Sl.shape[0], Sl.shape[1], Sl.indptr, Sl.indices),
                mapG=DeviceIndex(ctx, np.rint(Gt.data).astype(np.int64) - 1, len(ci)),
                mapD=DeviceIndex(ctx, np.rint(Dt.data).astype(np.int64) - 1, len(ci)),
                mapT=DeviceIndex(ctx, mapT, nnz_own + nnz_g),
                tv=DeviceVector(ctx, nnz_own + nnz_g),
                hT=Halo(ctx, nnz_own, nnz_g, dict(peers=np.asarray(peers, np.int32), send_ptr=np.asarray(send_ptr, np.int64),
                                                  send_idx=(np.concatenate(send_idx) if send_idx else np.zeros(0)).astype(np.int32),
                                                  recv_ptr=np.asarray(recv_ptr, np.int64))))
            lv.st["dev"] = dev
            Gd, Dd, Did, Sd = self._device_operators(lv, assemble=False)
            if os.environ.get("NPG_MG_DIST_CHECK") == "1":                    # the device's values against the host's (tests)
                for name, a, b in (("G", Gd, Gl), ("D", Dd, Dh), ("Dinv", Did, sp.csr_matrix(Dinv)), ("S", Sd, Sl)):
                    err = abs(a.to_scipy_csr() - b).max() / max(abs(b).max(), 1e-300)
                    if not err < 1e-10:
                        raise RuntimeError(f"distributed multigrid: device-side {name} differs from the host's by {err:.2e}")
        return Gl, Dh, Dinv, Sl

    def _device_operators(self, lv, assemble=True):
        """refresh (G, D, Dinv, S) of a distributed level on the device from the rank's rows of the level's current matrix: values
        gathered from the re-assembled rows, node-block (or z-line piece) inverse, T = Dinv G by the fixed-pattern product, its ghost
        rows' VALUES through a halo plan, S = D T.  Collective (the halo exchange)."""
        dev, prm = lv.st["dev"], self.prm
        if assemble:
            lv.fe.assemble(L.NPG_MAT_A, dev.Ap, scale=prm.alpha ** 2 * prm.eps ** 2, full_stress=self._full)
        dev.G.gather_values(dev.Ap, dev.mapG)
        dev.D.gather_values(dev.Ap, dev.mapD)
        if dev.blocks is not None:
            L.check(L.lib().npg_csr_line_block_inverse(dev.Dinv.h, dev.Ap.h, dev.blocks[0].h, dev.blocks[1].h))
        else:
            L.check(L.lib().npg_csr_node_block_inverse(dev.Dinv.h, dev.Ap.h, int(dev.nfl), int(dev.nsl)))
        L.check(L.lib().npg_csr_product(dev.T.h, dev.Dinv.h, dev.G.h))
        L.check(L.lib().npg_csr_values_to_vec(dev.T.h, dev.tv.h))
        dev.hT.exchange(dev.tv)
        L.check(L.lib().npg_csr_values_from_vec(dev.Text.h, dev.tv.h, dev.mapT.h))
        L.check(L.lib().npg_csr_product(dev.S.h, dev.D.h, dev.Text.h))
        return dev.G, dev.D, dev.Dinv, dev.S

    def refresh(self, A, model=None):
        """the solver's matrix has been re-assembled on every rank (eddy closure, src/model.jl:160-170): recompute the distributed
        level's smoother from it (same layouts, new values) and re-assemble the replicated coarser levels with the eddy viscosity of
        the buoyancy injected into their meshes - what MultigridPreconditioner.refresh does on one GPU.  Collective."""
        from . import multigrid as mgm
        from .inversion import build_A_inversion, device_fe
        if model is None:
            raise ValueError("DistributedMultigridPreconditioner.refresh needs the model (its engine holds the viscosity table)")
        top = len(self.hierarchy) - 1
        Gl, Dh, Dinv, Sl = self._level_operators(self._lv[0], first=False)
        # (device handles when the level has its device plan - refreshed in place -, host matrices otherwise)
        new = [Gl, Dh, Dinv, Sl] if isinstance(Gl, DeviceCSR) else [DeviceCSR.from_scipy(self.ctx, M) for M in (Gl, Dh, sp.csr_matrix(Dinv), Sl)]
        L.check(L.lib().npg_precond_mg_update_level(self.h, top, A.h, new[0].h, new[1].h, new[2].h, new[3].h))
        self._fine_ops[:4] = new
        ep = self.frc.eddy_param
        if ep.is_on and os.environ.get("NPG_MG_COARSE_NU", self.coarse_nu) == "average":
            self._refresh_coarse_levels_averaged()
        elif ep.is_on:
            fine = self.hierarchy[-1]
            if self._inj is None:
                p1 = fine.spaces.b_order == 1
                self._inj = [mgm.injection(self.hierarchy[k].mesh, self.hierarchy[k + 1].mesh, p1) for k in range(top)]
            s_f = fine.spaces
            b_glob = model.state.b                                            # collective gather of the owned slices, native order
            nodal = np.where(s_f.b_dof >= 0, b_glob[np.maximum(s_f.b_dof, 0)], s_f.b_diri_val)
            lo = top - 1
            if self.distributed_levels == 2:
                # the second partitioned level: the injected buoyancy on this rank's coarse cells -> its engine's viscosity table ->
                # its rows of A and its smoother, as on the finest level
                lv1 = self._lv[1]
                fed_c = lv1.fed
                nodal = nodal[self._inj[top - 1]]
                s = fed_c.spaces
                bl = DeviceVector.from_host(self.ctx, nodal[s.b_dof >= 0], fed_c.dofs.p_b[lv1.lay.b.globals()])
                lv1.fe.update_nu_eddy(ep.N2min, self.prm.alpha, self.prm.N2, bl)
                lv1.fe.assemble(L.NPG_MAT_A, lv1.A, scale=self.prm.alpha ** 2 * self.prm.eps ** 2, full_stress=self._full)
                G1, D1, Dinv1, S1 = self._level_operators(lv1, first=False)
                new1 = ([G1, D1, Dinv1, S1] if isinstance(G1, DeviceCSR) else
                        [DeviceCSR.from_scipy(self.ctx, M) for M in (G1, D1, sp.csr_matrix(Dinv1), S1)])
                L.check(L.lib().npg_precond_mg_update_level(self.h, top - 1, lv1.A.h, new1[0].h, new1[1].h, new1[2].h, new1[3].h))
                lv1.ops[:4] = new1
                lo = top - 2
            for lev in range(lo, -1, -1):
                fed = self.hierarchy[lev]
                nodal = nodal[self._inj[lev]]
                s = fed.spaces
                fe = device_fe(self.arch, fed)
                bl = DeviceVector.from_host(self.ctx, nodal[s.b_dof >= 0], fed.dofs.p_b)
                fe.update_nu_eddy(ep.N2min, self.prm.alpha, self.prm.N2, bl)
                build_A_inversion(self.arch, fed, self.prm, None, A=self.cA[lev])
                ops = self.cops[lev].update(self.cA[lev])
                L.check(L.lib().npg_precond_mg_update_level(self.h, lev, self.cA[lev].h, ops.G.h, ops.D.h, ops.Dinv.h, ops.S.h))
            if self._dense_mode:
                L.check(L.lib().npg_precond_mg_set_coarse_dense(self.h, self._dense_mode))
        return self

    def _refresh_coarse_levels_averaged(self):
        """The coarser levels follow the eddy closure through the FINE viscosity, as MultigridPreconditioner does on one GPU
        (npg_fe_restrict_coeff there): a coarse cell's viscosity = the volume-weighted average of its eight children's cell means.
        The children of a rank's coarse cell live on several ranks, so: every rank takes the cell means of its engine's table
        (npg_fe_coeff_cell_mean), sums vol x mean and vol over the fine cells it OWNS (the lowest rank holding a cell owns it - fixed at
        the first call) per coarse cell, the sparse partial sums travel once (all_gather_object, summed in rank order: identical
        bits everywhere), and every level below is an average of that array on the host.  Collective."""
        from .inversion import build_A_inversion, device_fe
        lv0, top = self._lv[0], len(self.hierarchy) - 1
        dist = lv0.dist
        rank, world = dist.get_rank(), dist.get_world_size()
        fine = self.hierarchy[-1]
        if self._avg is None:
            sets = [None] * world
            dist.all_gather_object(sets, lv0.lay.cells)
            owner = np.full(fine.mesh.ncell, world, dtype=np.int32)
            for q in range(world - 1, -1, -1):
                owner[sets[q]] = q
            mine = owner[lv0.lay.cells] == rank
            cells = lv0.lay.cells[mine]
            idx, inv = np.unique(cells // 8, return_inverse=True)
            self._avg = SimpleNamespace(mine=mine, idx=idx, inv=inv, vol=fine.mesh.detJ[cells], vec=DeviceVector(self.ctx, len(lv0.lay.cells)))
        a = self._avg
        mean = lv0.fe.coeff_cell_mean("nu", a.vec).to_host()[a.mine]
        part = (a.idx, np.bincount(a.inv, weights=a.vol * mean, minlength=len(a.idx)), np.bincount(a.inv, weights=a.vol, minlength=len(a.idx)))
        parts = [None] * world
        dist.all_gather_object(parts, part)
        ncc = self.hierarchy[top - 1].mesh.ncell
        num, den = np.zeros(ncc), np.zeros(ncc)
        for q in range(world):
            num[parts[q][0]] += parts[q][1]
            den[parts[q][0]] += parts[q][2]
        if not (den > 0).all():
            raise RuntimeError("distributed multigrid: a coarse cell has no child on any rank")
        nu = num / den                                                     # the level below the finest, every cell, on every rank
        lo = top - 1
        if self.distributed_levels == 2:
            lv1 = self._lv[1]
            nq = len(lv1.fed.mesh.q_w)
            tab = np.repeat(nu[lv1.lay.cells][:, None], nq, axis=1)
            lv1.fe.set_coeff("nu", lambda xq, t=tab: t)
            lv1.fe.assemble(L.NPG_MAT_A, lv1.A, scale=self.prm.alpha ** 2 * self.prm.eps ** 2, full_stress=self._full)
            G1, D1, Dinv1, S1 = self._level_operators(lv1, first=False)
            new1 = ([G1, D1, Dinv1, S1] if isinstance(G1, DeviceCSR) else
                    [DeviceCSR.from_scipy(self.ctx, M) for M in (G1, D1, sp.csr_matrix(Dinv1), S1)])
            L.check(L.lib().npg_precond_mg_update_level(self.h, top - 1, lv1.A.h, new1[0].h, new1[1].h, new1[2].h, new1[3].h))
            lv1.ops[:4] = new1
            vol = lv1.fed.mesh.detJ
            nu = (nu * vol).reshape(-1, 8).sum(axis=1) / vol.reshape(-1, 8).sum(axis=1)
            lo = top - 2
        for lev in range(lo, -1, -1):
            fed = self.hierarchy[lev]
            fe = device_fe(self.arch, fed)
            tab = np.repeat(nu[:, None], len(fed.mesh.q_w), axis=1)
            fe.set_coeff("nu", lambda xq, t=tab: t)
            build_A_inversion(self.arch, fed, self.prm, None, A=self.cA[lev])
            ops = self.cops[lev].update(self.cA[lev])
            L.check(L.lib().npg_precond_mg_update_level(self.h, lev, self.cA[lev].h, ops.G.h, ops.D.h, ops.Dinv.h, ops.S.h))
            if lev > 0:
                vol = fed.mesh.detJ
                nu = (nu * vol).reshape(-1, 8).sum(axis=1) / vol.reshape(-1, 8).sum(axis=1)
        if self._dense_mode:
            L.check(L.lib().npg_precond_mg_set_coarse_dense(self.h, self._dense_mode))

    def counters(self):
        import ctypes as C
        a, b = C.c_int64(), C.c_int64()
        L.check(L.lib().npg_precond_counters(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def __del__(self):
        try:
            if self.h:
                L.lib().npg_precond_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def __repr__(self):
        return (f"DistributedMultigridPreconditioner({self.levels}: finest level row-partitioned, coarser ones replicated; "
                f"{self.params}, coarsest level: {'dense inverse' if self.coarse_dense else 'smoothing steps'}"
                f"{', z-line smoother' if self.smoother == 'zline' else ''})")


def use_multigrid(model, hierarchy, memory=20, **mg_kw):
    """Replace the partitioned model's inversion solver (GMRES + Diagonal(1/h^3)) by flexible GMRES behind the distributed
    multigrid; the stopping rule keeps the reference's 1/h^dim scaling.  Collective."""
    from .multigrid import FgmresWorkspace
    s = model.inversion.solver
    if hierarchy[-1] is not model.fe_data:
        raise ValueError("use_multigrid: hierarchy[-1] must be the model's own fe_data")
    P = DistributedMultigridPreconditioner(model.arch, model.params, model.forcings, hierarchy, model, **mg_kw)
    ws = FgmresWorkspace(model.arch.ctx, s.lay.n_own, memory=memory)
    L.check(L.lib().npg_fgmres_set_halo(ws.h, s.halo.h))
    kw = dict(s.kwargs, scale=float(s.P.scalar))
    model.inversion.solver = PartitionedSolverToolkit(s.A, P, s.y, ws, kw, s.label, s.x, s.lay, s.halo, s.halo_ext)
    model._u_view = model.inversion.solver.x.view(0, model.layout.n_own_u)
    model.extrapolate_guess = True
    model.dist.barrier()
    return model
