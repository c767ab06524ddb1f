"""A numpy restatement of the interior buoyancy forcing (nupgcm_amd.interior) and the checks shared by
tests/test_interior.py (CPU()) and tests/test_gpu_interior.py (GPU()).

The restatement is written from the definitions with the mesh (cell nodes, vertex coordinates, detJ), the engine's volume rule
(Mesh.q_lam, Mesh.q_w) and fe.p2_tables: the points are sum_k lambda_k(q) X_k, the shape values those of the space at the rule's
barycentric points, rows come from the native table b_pos, Dirichlet values from Spaces.b_diri_val, the functions are evaluated at the
points here, and the time rule is forcing_ref's restated one.  Every entry of the load and of R is kept as the list of its TERMS
w_q detJ piece_q N_k(q) - one per additive piece of the point value ((1 - w) Qa, w Qb, gamma (1 - w) b*a, gamma w b*b and
-gamma N_i(q) bD_i per Dirichlet node i of the cell), point and cell.  Rows of the load are summed with math.fsum; the entries of R (a
hundred thousand of them) in x87 extended precision, whose own error n 2^-64 sum |terms| is 1/4096 of the bound.

The bound of an entry is its own:  (number of non-zero terms in the entry's sum + 8) eps sum |terms|  (Higham eq. 4.4 for the additions
in any order, the 8 for the multiplications that form a term).  Device against host library: the same bound."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

import nupgcm_amd as npg
from nupgcm_amd import _lib as L
from nupgcm_amd import fe as F
from nupgcm_amd.evolution import evolution_parameter, lhs_timestepper, scheme_constant
from nupgcm_amd.inversion import device_fe
from tests import forcing_ref as fr
from tests import helpers
from tests import sampling_ref as sr

EPS = np.finfo(np.float64).eps
assert np.finfo(np.longdouble).eps < 2.0 ** -60, "the reference sums of R need an extended-precision long double"
NEW = {"npg_interior_create", "npg_interior_set_series", "npg_interior_set_gamma", "npg_interior_apply", "npg_interior_matrix",
       "npg_interior_budget", "npg_interior_info", "npg_interior_destroy"}
EDGE_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257)

# smooth, non-polynomial fields
GAMMA = lambda x: 0.5 + np.sin(x[..., 0] + 2.0 * x[..., 1] - x[..., 2]) ** 2
TARGET = lambda x: np.exp(-x[..., 0] ** 2) * np.sin(3.0 * x[..., 1]) + x[..., 2]
TARGET2 = lambda x: np.cos(x[..., 0] * x[..., 1]) - 0.5 + 2.0 * x[..., 2]
Q1 = lambda x: 1e-2 * np.sin(3.0 * x[..., 0]) * np.exp(x[..., 1] + x[..., 2])
Q2 = lambda x: 1e-2 * np.cos(5.0 * x[..., 0] + x[..., 2]) / (1.5 + x[..., 1])
Q3 = lambda x: 1e-2 * np.exp(np.sin(x[..., 0] - x[..., 1] + 4.0 * x[..., 2]))
TIMES, PERIOD = fr.TIMES, fr.PERIOD                         # dyadic: the rule's arithmetic is exact
QSERIES = (TIMES, [Q1, Q2, Q3], PERIOD)
FULL = dict(source=QSERIES, gamma=GAMMA, target=TARGET)


def make(model, spec, cells=None):
    """InteriorForcing(model, ...) of a spec {source, gamma, target}: numbers, functions, tables or (times, fields, period)"""
    kw = {}
    if "source" in spec:
        kw["source"] = fr.as_arg(spec["source"])
    if "gamma" in spec:
        kw["restoring"] = (spec["gamma"], fr.as_arg(spec["target"]))
    return npg.InteriorForcing(model, cells=cells, **kw)


def _fn(v, xq):
    if isinstance(v, np.ndarray) and v.ndim == 2:
        return v
    return fr._fn(v, xq)


def _pieces(v, xq, t):
    if isinstance(v, tuple):
        times, fields, period = v
        k, k1, w = fr.ref_key_weight(list(times), period, t)
        return [_fn(fields[k], xq)] if w == 0.0 else [(1.0 - w) * _fn(fields[k], xq), w * _fn(fields[k1], xq)]
    return [_fn(v, xq)]


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
class Ref:
    """all cells of the mesh, their points, weights, shape values, destination rows and Dirichlet values"""

    def __init__(self, model):
        fed = model.fe_data
        m = self.mesh = fed.mesh
        X = m.geo_coords[m.cell_geo]                                                       # (nc, 4, 3)
        self.xq = np.einsum("qk,cki->cqi", m.q_lam, X)
        self.w = np.asarray(m.q_w, dtype=float)
        self.detJ = np.asarray(m.detJ, dtype=float)
        vol6 = np.abs(np.linalg.det(X[:, 1:] - X[:, :1]))
        assert np.allclose(vol6, self.detJ, rtol=1e-12, atol=0.0)                          # the weights are those of the cells' own vertices
        self.p2 = fed.spaces.b_order == 2
        self.N = F.p2_tables(m.q_lam, F._TET_EDGE_A, F._TET_EDGE_B)[0] if self.p2 else np.asarray(m.q_lam, dtype=float)
        nodes = m.cell_nodes if self.p2 else m.cells
        self.rows = fed.tables.b_pos[nodes]                                                # (nc, NB), -1: Dirichlet
        self.bd = np.where(self.rows < 0, fed.spaces.b_diri_val[nodes], 0.0)              # (nc, NB)
        self.nb = fed.dofs.nb
        self.ncell, self.NB = self.rows.shape

    def point_pieces(self, spec, t, restoring=True, lift=True):
        """the additive pieces (each (nc, nq)) of Q + gamma (b* - b_D) at time t"""
        pieces = []
        v = spec.get("source", 0.0)
        if isinstance(v, (tuple, np.ndarray)) or callable(v) or float(v) != 0.0:
            pieces += _pieces(v, self.xq, t)
        if "gamma" in spec and restoring:
            g = _fn(spec["gamma"], self.xq)
            pieces += [g * p for p in _pieces(spec["target"], self.xq, t)]
            if lift:
                for i in np.nonzero((self.rows < 0).any(axis=0))[0]:
                    pieces.append(-g * self.N[None, :, i] * self.bd[:, i, None])
        return pieces

    def load(self, spec, t, keep=None):
        """int (Q + gamma (b* - b_D)) phi_r over the kept cells: (value, bound, touched) per row, value = fsum of the terms"""
        val, bnd, touched = np.zeros(self.nb), np.zeros(self.nb), np.zeros(self.nb, dtype=bool)
        keep = np.ones(self.ncell, dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
        pieces = self.point_pieces(spec, t)
        sel = keep[:, None] & (self.rows >= 0)
        touched[self.rows[sel]] = True
        if not pieces or not sel.any():
            return val, bnd, touched
        P = np.stack(pieces)                                                               # (np, nc, nq)
        terms = np.einsum("c,q,pcq,qk->ckpq", self.detJ, self.w, P, self.N)               # (nc, NB, np, nq)
        r, tt = self.rows[sel], terms[sel].reshape(int(sel.sum()), -1)
        order = np.argsort(r, kind="stable")
        r, tt = r[order], tt[order]
        start = np.flatnonzero(np.r_[True, r[1:] != r[:-1]])
        for a, b in zip(start, np.r_[start[1:], len(r)]):
            x = tt[a:b].ravel()
            val[r[a]] = math.fsum(x)
            bnd[r[a]] = (np.count_nonzero(x) + 8) * EPS * math.fsum(np.abs(x))
        return val, bnd, touched

    def matrix(self, gamma, keep=None):
        """R = int gamma phi_i phi_j over the kept cells: (rows, cols, values, bounds) of the touched entries, sorted by (row, col)"""
        keep = np.ones(self.ncell, dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
        kc = np.nonzero(keep)[0]
        g = _fn(gamma, self.xq)[kc]
        terms = np.einsum("c,q,cq,qi,qj->cijq", self.detJ[kc], self.w, g, self.N, self.N)                 # (nk, NB, NB, nq)
        rows = self.rows[kc]
        ri, cj = np.broadcast_to(rows[:, :, None], terms.shape[:3]), np.broadcast_to(rows[:, None, :], terms.shape[:3])
        sel = (ri >= 0) & (cj >= 0)
        key, tt = (ri[sel].astype(np.int64) * self.nb + cj[sel]), terms[sel]
        if not len(key):
            z = np.zeros(0)
            return z.astype(np.int64), z.astype(np.int64), z, z
        order = np.argsort(key, kind="stable")
        key, tt = key[order], tt[order]
        start = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
        flat = tt.reshape(-1)
        at = start * tt.shape[1]
        vv = np.add.reduceat(flat.astype(np.longdouble), at).astype(np.float64)
        sabs = np.add.reduceat(np.abs(flat), at)
        cnt = np.add.reduceat((flat != 0.0).astype(np.int64), at)
        return key[start] // self.nb, key[start] % self.nb, vv, (cnt + 8) * EPS * sabs

    def budget(self, spec, t, b_nodal, keep=None):
        """(volume, int Q, int gamma (b* - b)) over the kept cells and their bounds; b_nodal (nc, NB): the state at the cells' nodes"""
        keep = np.ones(self.ncell, dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
        W = (self.detJ[:, None] * self.w[None, :])[keep]                                   # (nk, nq)
        out = []
        g = _fn(spec["gamma"], self.xq) if "gamma" in spec else None
        groups = [[np.ones_like(W)], [p[keep] for p in self.point_pieces(spec, t, restoring=False)],
                  [] if g is None else [p[keep] for p in self.point_pieces(dict(spec, source=0.0), t, lift=False)]
                  + [-(g * self.N[None, :, i] * b_nodal[:, i, None])[keep] for i in range(self.NB)]]
        for pieces in groups:
            x = np.concatenate([(W * p).ravel() for p in pieces]) if pieces else np.zeros(0)
            out.append((math.fsum(x), (np.count_nonzero(x) + 8) * EPS * math.fsum(np.abs(x))))
        return out


_REFS = {}


def ref_of(model):
    """one restatement per model (the mesh tables are built once and left unchanged)"""
    if id(model.fe_data) not in _REFS:
        _REFS[id(model.fe_data)] = (model.fe_data, Ref(model))
    return _REFS[id(model.fe_data)][1]


def report(label, err, bound):
    err, bound = np.asarray(err), np.asarray(bound)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    print(f"interior {label}: max |err| {err.max(initial=0.0):.2e}, worst |err| / bound {ratio.max(initial=0.0):.3f} over {err.size} entries")
    return ratio


# ---- models ---------------------------------------------------------------------------------------------------------------------------
def light_model(arch, mesh, b_order=2, config="bowl_surface_flux", b_diri_vals=None):
    """what InteriorForcing reads of a model, without an inversion toolkit: a real EvolutionToolkit on the mesh"""
    prm, frc, btags, bvals, dt, _ = helpers.product_config(config)
    bvals = bvals if b_diri_vals is None else [b_diri_vals] * len(btags)
    fed = npg.FEData(mesh, npg.Spaces(mesh, b_diri_tags=btags, b_diri_vals=bvals, b_order=b_order))
    ts = npg.BDF2(t_start=0.0, t_stop=dt, dt=dt)
    ev = npg.EvolutionToolkit(arch, fed, prm, frc, ts)
    n = fed.dofs.nu + fed.dofs.np
    inv = SimpleNamespace(b=npg.DeviceVector(arch.ctx, n), b_lift=npg.DeviceVector(arch.ctx, n))
    return SimpleNamespace(arch=arch, params=prm, forcings=frc, fe_data=fed, evolution=ev, inversion=inv, timestepper=ts, step_index=1,
                           tracers=None, surface_forcing=None, interior_forcing=None, b_vec=ev.solver.x)


def bowl_mesh():
    import os
    return npg.Mesh(os.path.join(helpers.GOLDEN, "mesh_bowl3D_h0.1.npz"))


def snapshot(model):
    return model.evolution.rhs_flux.to_host(), model.inversion.b.to_host(), model.evolution.solver.A.to_scipy_csr().data.copy()


same_bits = fr.same_bits


def first_cells(nc, n):
    mk = np.zeros(nc, dtype=bool)
    mk[:n] = True
    return mk


# ---- the checks (arch = npg.CPU() or npg.GPU()) -------------------------------------------------------------------------------------------
def check_exports():
    assert "InteriorForcing" in npg.__all__
    assert NEW <= set(L.declared_symbols()) and L.NPG_ITR_NSERIES == 2 and L.NPG_ITR_NBUDGET == 3
    hdr = open(L.HEADER_PATH).read()
    for path in (L.HOST_LIB_PATH, L.LIB_PATH):
        lib = C.CDLL(path)
        assert not [s for s in NEW if not hasattr(lib, s) or s + "(" not in hdr], path


def check_loads(model, label, cells=None, spec=FULL, t=0.625, matrix=True):
    """checks 2 - 4: the load rows, the untouched rows, R entry by entry and its untouched entries against the restatement"""
    before = snapshot(model)
    ref = ref_of(model)
    f = make(model, spec, cells)
    try:
        n = ref.ncell if cells is None else int(np.sum(cells))
        assert f.info()["nkept"] == n == len(f.cells) and np.array_equal(f.cells, np.nonzero(np.ones(ref.ncell, bool) if cells is None else cells)[0])
        assert np.array_equal(f.points, ref.xq[f.cells]) and np.allclose(f.weights, ref.detJ[f.cells, None] * ref.w, rtol=4 * EPS, atol=0)
        f.apply(model, t)
        got = f.rhs_src.to_host()
        val, bnd, touched = ref.load(spec, t, cells)
        report(f"{label}: load rows", np.abs(got - val)[touched], bnd[touched])
        assert (np.abs(got - val)[touched] <= bnd[touched]).all(), label
        assert (got[~touched] == 0.0).all() and f.info()["load_slots"] == int(((ref.rows >= 0) & (np.ones(ref.ncell, bool) if cells is None else cells)[:, None]).sum())
        f.apply(model, t)                                                                  # the same bits on every call
        assert np.array_equal(got, f.rhs_src.to_host())
        if n:
            assert touched.any() and np.abs(val[touched]).max() > 1e3 * bnd[touched].max()
        if matrix:
            R = f.R.to_scipy_csr()
            rr, cc, vv, bb = ref.matrix(spec["gamma"], cells)
            gotR = np.asarray(R[rr, cc]).ravel() if len(rr) else np.zeros(0)
            report(f"{label}: R entries", np.abs(gotR - vv), bb)
            assert (np.abs(gotR - vv) <= bb).all(), label
            mask = sp.csr_matrix((np.ones(len(rr)), (rr, cc)), shape=R.shape)
            assert (R - R.multiply(mask)).count_nonzero() == 0                             # entries no kept cell touches: 0
            assert f.info()["matrix_entries"] == len(rr)
    finally:
        f.detach()
    assert same_bits(snapshot(model), before) and model.evolution.R is None and model.evolution.rhs_src is None
    return got


def check_single_tet(arch):
    from tests import boundary_ref as br
    mesh = br.single_tet(arch).fe_data.mesh
    for order in (2, 1):
        model = light_model(arch, mesh, b_order=order)
        assert ref_of(model).ncell == 1
        check_loads(model, f"single tetrahedron P{order}")


def check_known_answers(arch, flux_model):
    """check 5: gamma = g gives g M; Q = 1 gives M 1 + the Dirichlet columns' share; b* = b_D's own extension gives no load"""
    ref = ref_of(flux_model)
    g = 0.75
    f = make(flux_model, dict(gamma=g, target=0.0))
    try:
        R, M = f.R.to_scipy_csr(), flux_model.evolution.M.to_scipy_csr()
        rr, cc, _, bb = ref.matrix(g)
        err = np.abs(np.asarray(R[rr, cc]).ravel() - g * np.asarray(M[rr, cc]).ravel())
        report("known answers: R - g M (NPG_MAT_M)", err, bb)
        assert (err <= bb).all() and len(rr) == M.nnz == R.nnz
    finally:
        f.detach()
    # Q = 1 on a model whose Dirichlet values are 1: load = M 1 + rhs_M.  A row's terms: w_q detJ N_i N_j over cells, points and ALL j
    ones = light_model(arch, flux_model.fe_data.mesh, config="bowl_mixing", b_diri_vals=1.0)
    r1 = ref_of(ones)
    assert (r1.rows < 0).any() and (r1.bd[r1.rows < 0] == 1.0).all()
    f = make(ones, dict(source=1.0))
    try:
        f.apply(ones, 0.0)
        got = f.rhs_src.to_host()
        M = ones.evolution.M.to_scipy_csr()
        want = np.array([math.fsum(list(M.data[M.indptr[i]:M.indptr[i + 1]]) + [x]) for i, x in enumerate(ones.evolution.rhs_M.to_host())])
        T = np.abs(np.einsum("c,q,qi,qj->cij", r1.detJ, r1.w, r1.N, r1.N))
        sabs, cnt = np.zeros(r1.nb), np.zeros(r1.nb)
        sel = r1.rows >= 0
        np.add.at(sabs, r1.rows[sel], T.sum(axis=2)[sel])
        np.add.at(cnt, r1.rows[sel], len(r1.w) * r1.NB)
        _, lb, touched = r1.load(dict(source=1.0), 0.0)
        bound = (cnt + 8) * EPS * sabs + lb
        report("known answers: load(Q = 1) - (M 1 + rhs_M with Dirichlet values 1)", np.abs(got - want), bound)
        assert touched.all() and (np.abs(got - want) <= bound).all() and np.abs(ones.evolution.rhs_M.to_host()).max() > 0
    finally:
        f.detach()
    # b* = the extension of the Dirichlet values by the cell's own shape functions, as a table: gamma (b* - b_D) = 0 at every point
    diri = light_model(arch, flux_model.fe_data.mesh, config="bowl_diri")
    rd = ref_of(diri)
    assert np.abs(rd.bd).max() > 0.1
    bstar = np.einsum("qi,ci->cq", rd.N, rd.bd)
    spec = dict(gamma=GAMMA, target=bstar)
    f = make(diri, spec)
    try:
        f.apply(diri, 0.0)
        got = f.rhs_src.to_host()
        _, bnd, touched = rd.load(spec, 0.0)
        # rows all of whose cell neighbours are Dirichlet nodes
        alone = (rd.rows >= 0) & ((rd.rows < 0).sum(axis=1) == rd.NB - 1)[:, None]
        cnt_all, cnt_alone = np.zeros(rd.nb), np.zeros(rd.nb)
        np.add.at(cnt_all, rd.rows[rd.rows >= 0], 1)
        np.add.at(cnt_alone, rd.rows[alone], 1)
        only = (cnt_all > 0) & (cnt_all == cnt_alone)
        report(f"known answers: load(b* = b_D) (rows with Dirichlet neighbours only: {only.sum()})", np.abs(got), bnd)
        assert (np.abs(got) <= bnd).all() and bnd[touched].max() > 0
    finally:
        f.detach()


def check_time_rule(model):
    """check 6: w = 0 returns the keyframe's bits; the periodic wrap and the held ends; tables(t)"""
    ref = ref_of(model)
    fields, tfields = [Q1, Q2, Q3], [TARGET, TARGET2, TARGET]

    def run(spec, t):
        f = make(model, spec)
        try:
            f.apply(model, t)
            return f.rhs_src.to_host()
        finally:
            f.detach()
    one = [run(dict(source=fields[k], gamma=GAMMA, target=tfields[k]), 0.0) for k in range(3)]
    for period, cases in ((None, ((-1.0, 0), (0.0, 0), (0.25, 1), (1.0, 2), (5.0, 2))), (PERIOD, ((0.25, 1), (1.0, 2), (2.0, 0), (-1.75, 1)))):
        spec = dict(source=(TIMES, fields, period), gamma=GAMMA, target=(TIMES, tfields, period))
        for t, k in cases:
            assert np.array_equal(run(spec, t), one[k]), (period, t, k)
    spec = dict(source=(TIMES, fields, PERIOD), gamma=GAMMA, target=(TIMES, tfields, PERIOD))
    f = make(model, spec)
    try:
        for t, (k, k1, w) in ((0.625, (1, 2, 0.5)), (1.5, (2, 0, 0.5)), (0.125, (0, 1, 0.5))):
            assert fr.ref_key_weight(TIMES, PERIOD, t) == (k, k1, w) and f.key_weights(t) == dict(source=(k, w), target=(k, w))
            assert f.key_weights(t)["source"] == npg.series_key_weight(TIMES, PERIOD, t)
            f.apply(model, t)
            val, bnd, touched = ref.load(spec, t)
            got = f.rhs_src.to_host()
            report(f"time rule t={t}: keys {k}, {k1}, w = {w}", np.abs(got - val)[touched], bnd[touched])
            assert (np.abs(got - val)[touched] <= bnd[touched]).all()
            tab = f.tables(t)
            assert np.array_equal(tab["source"], 0.5 * fr._fn(fields[k], ref.xq) + 0.5 * fr._fn(fields[k1], ref.xq))
            assert np.array_equal(tab["target"], 0.5 * fr._fn(tfields[k], ref.xq) + 0.5 * fr._fn(tfields[k1], ref.xq))
        f.apply(model, 1.5)
        wrap = f.rhs_src.to_host()
        assert not np.array_equal(wrap, one[2]) and not np.array_equal(wrap, one[0])
        for n in (1, 1000, -1000):
            f.apply(model, 1.5 + n * PERIOD)
            assert np.array_equal(wrap, f.rhs_src.to_host()), n
        assert np.array_equal(f.tables(0.25)["source"], fr._fn(Q2, ref.xq)) and np.array_equal(f.tables(7.0)["source"], f.tables(1.0)["source"])
    finally:
        f.detach()


def matrices(model):
    ev = model.evolution
    return tuple(M.to_scipy_csr() for M in (ev.M, ev.Kh, ev.Kv))


def check_lhs(model, R, c, theta, label, S=None, dt=0.0):
    """solver.A = M + theta (Kh + Kv) [+ dt S] + c R entry by entry: its terms and the inner sums"""
    M, Kh, Kv = matrices(model)
    A = model.evolution.solver.A.to_scipy_csr()
    parts = [M.data, theta * Kh.data, theta * Kv.data, c * R.data] + ([dt * S.data] if S is not None else [])
    want = sum(parts[1:], parts[0])
    bound = (len(parts) + 1 + 8) * EPS * sum(np.abs(p) for p in parts)
    report(f"{label}: A - (M + theta (Kh + Kv){' + dt S' if S is not None else ''} + c R), c = {c:.6g}", np.abs(A.data - want), bound)
    assert (np.abs(A.data - want) <= bound).all() and np.abs(c * R.data).max() > 1e3 * bound.max()
    return A


def small_channel(arch, scheme):
    from nupgcm_amd import channel_basin as cb
    from nupgcm_amd import workloads
    # (the wind of bowl_wind without its Dirichlet tags: a flow spins up from the first inversion on, so the adaptive step does change)
    prm, frc, _, _, dt, b0 = helpers.product_config("bowl_wind")
    mesh = npg.Mesh(cb.channel_basin_model(0.125, workloads.CB_ALPHA, dz=0.125))           # the small channel basin: seconds per case
    fed = npg.FEData(mesh, npg.Spaces(mesh, u_diri_tags=helpers.U_TAGS, u_diri_vals=helpers.U_VALS, u_diri_masks=helpers.U_MASKS))
    dt = 0.3
    ts = npg.BDF2(t_start=0.0, t_stop=4 * dt, dt=dt) if scheme == "BDF2" else npg.BDF1(t_start=0.0, t_stop=1e9, dt=dt, adaptive=True)
    model = npg.Model(arch, prm, frc, fed, npg.InversionToolkit(arch, fed, prm, frc), npg.EvolutionToolkit(arch, fed, prm, frc, ts), ts)
    npg.set_b(model, b0)
    return model


def check_operator(arch, scheme):
    """check 7: after every step solver.A = M + theta (Kh + Kv) + c R with that step's c and theta (BDF2: c = dt, 2/3 dt, 2/3 dt with the
    default first_step_lhs; adaptive BDF1: c = dt, a dt that changes) and rhs_src is the restatement's load at that step's t_{n+1}"""
    model = small_channel(arch, scheme)
    prm, ts = model.params, model.timestepper
    ref = ref_of(model)
    spec = dict(source=(TIMES, [lambda x, q=q: 1e-2 * q(x) for q in (Q1, Q2, Q3)], PERIOD), gamma=GAMMA, target=lambda x: x[..., 2] / 0.5)
    f = make(model, spec)
    R = f.R.to_scipy_csr()
    dts, cs = [], []
    for step in range(1, 4):
        t_before = ts.t
        npg.run(model, n_steps=1)
        t1 = t_before + ts.dt
        dts.append(ts.dt)
        lts = npg.BDF1(t_start=0.0, t_stop=1.0, dt=ts.dt) if (scheme == "BDF2" and step == 1) else ts
        c = scheme_constant(lts)
        cs.append(c / ts.dt)
        check_lhs(model, R, c, evolution_parameter(prm, lts), f"{scheme} step {step}")
        val, bnd, touched = ref.load(spec, t1)
        got = f.rhs_src.to_host()
        report(f"{scheme} step {step}, t = {t1:.4f}: rhs_src", np.abs(got - val)[touched], bnd[touched])
        assert (np.abs(got - val)[touched] <= bnd[touched]).all()
        # the vector evolve() handed to npg_fe_evolution_rhs: rhs_flux + (c / dt) rhs_src, two products and a sum per row
        flux, mix = model.evolution.rhs_flux.to_host(), model.evolution._rhs_flux_src.to_host()
        assert (np.abs(mix - (flux + (c / ts.dt) * got)) <= 4 * EPS * (np.abs(flux) + np.abs((c / ts.dt) * got))).all()
    if scheme == "BDF2":
        assert np.allclose(cs, [1.0, 2.0 / 3.0, 2.0 / 3.0], rtol=4 * EPS, atol=0.0), cs
    else:
        assert cs == [1.0, 1.0, 1.0] and len(set(dts)) > 1, (cs, dts)                      # the step did adapt
    f.detach()
    return dts


def check_with_surface_forcing(model):
    """check 7, with a SurfaceForcing(restoring=...) attached as well: + dt S appears; detach in both orders, the bits return"""
    before = snapshot(model)
    ev, prm, ts = model.evolution, model.params, model.timestepper
    lts = lhs_timestepper(ev, ts, model.step_index)
    theta, c = evolution_parameter(prm, lts), scheme_constant(lts)
    spec = dict(gamma=GAMMA, target=TARGET)
    for order in ("interior first", "surface first"):
        if order == "interior first":
            f = make(model, spec)
            sf = npg.SurfaceForcing(model, restoring=(fr.GAMMA, fr.TARGET))
        else:
            sf = npg.SurfaceForcing(model, restoring=(fr.GAMMA, fr.TARGET))
            f = make(model, spec)
        both = check_lhs(model, f.R.to_scipy_csr(), c, theta, f"both forcings, {order}", S=sf.S.to_scipy_csr(), dt=lts.dt).data.copy()
        flux = ev.rhs_flux.to_host()
        f.apply(model, 0.3)
        assert np.array_equal(flux, ev.rhs_flux.to_host())                                # never each other's vectors
        src = f.rhs_src.to_host()
        sf.apply(model, 0.3)
        assert np.array_equal(src, f.rhs_src.to_host())
        (f if order == "interior first" else sf).detach()
        one = ev.solver.A.to_scipy_csr().data
        assert not np.array_equal(one, both) and not np.array_equal(one, before[2])
        (sf if order == "interior first" else f).detach()
        assert same_bits(snapshot(model), before), order
    assert model.interior_forcing is None and model.surface_forcing is None and ev.R is None and ev.S is None and ev.rhs_src is None


def stopping_rule(model, A, label):
    return fr.stopping_rule(model, A, label)


def check_one_step_budget(arch, lu):
    """check 8: bowl_surface_flux (no buoyancy Dirichlet tags, N2 = 0) at rest, a sponge and a source, one evolve.  With r = y - A b1 the
    discrete budget is  1'M (b1 - b0) - dt 1'rhs_flux - c (1'load - 1'R b1) + 1'r = -theta 1'(Kh + Kv) b1 = 0  (the columns of the
    stiffness matrices sum to zero; c = dt: the first step's BDF1 left-hand side).  Bound, as forcing_ref.check_one_step_budget: every
    sum here is math.fsum over explicit terms, what is left is the rounding of the device's sums, at most N = (longest row of A) x 11
    terms each: (N + 8) eps T with T the sum of the magnitudes of all terms.  budget() against the 1'-sums of the restatement's terms."""
    model = sr.bowl_model(arch, "bowl_surface_flux")
    assert (model.fe_data.spaces.b_dof >= 0).all() and float(model.params.N2) == 0.0
    ref = ref_of(model)
    spec = dict(source=QSERIES, gamma=GAMMA, target=TARGET)
    f = make(model, spec)
    ts, prm, ev = model.timestepper, model.params, model.evolution
    b0 = model.b_vec.to_host()
    t1 = ts.t + ts.dt
    f.apply(model, t1)
    pv = dict(x_prev=model.inversion.solver.x.copy(), b_prev=model.b_vec.copy())
    npg.evolve(model, pv["x_prev"], pv["b_prev"])
    b1, y, flux, load = model.b_vec.to_host(), ev.solver.y.to_host(), ev.rhs_flux.to_host(), f.rhs_src.to_host()
    R = f.R.to_scipy_csr()
    lts = npg.BDF1(t_start=0.0, t_stop=1.0, dt=ts.dt)
    theta, c = evolution_parameter(prm, lts), scheme_constant(lts)
    assert c == ts.dt
    A = check_lhs(model, R, c, theta, "one step")
    M, Kh, Kv = matrices(model)
    r = y - A @ b1
    terms = np.concatenate([M.data * (b1 - b0)[M.indices], -ts.dt * flux, -c * load, c * R.data * b1[R.indices], r])
    gap = abs(math.fsum(terms))
    N = int(np.diff(A.indptr).max()) * 11
    T = (abs(M) @ (np.abs(b1) + 2 * np.abs(b0))).sum() + ts.dt * 2 * np.abs(flux).sum() + c * (2 * np.abs(load).sum() + (abs(R) @ np.abs(b1)).sum()) \
        + theta * ((abs(Kh) + abs(Kv)) @ np.abs(b1)).sum() + np.abs(r).sum()
    bound = (N + 8) * EPS * T
    print(f"interior one step budget: |1'M (b1 - b0) - dt 1'f - c (1'load - 1'R b1) + 1'r| = {gap:.2e}, bound {bound:.2e}; 1'r = {math.fsum(r):.2e}, "
          f"c 1'R b1 = {c * math.fsum(R.data * b1[R.indices]):.2e}, c 1'load = {c * math.fsum(load):.2e}")
    assert gap <= bound and abs(c * math.fsum(R.data * b1[R.indices])) > 1e3 * bound and abs(c * math.fsum(load)) > 1e3 * bound
    if lu:
        rb = (np.diff(A.indptr) + 8) * EPS * (abs(A) @ np.abs(b1) + np.abs(y))
        assert ev.solver.workspace.stats.get("direct") and np.abs(r).max() <= rb.max()
    else:
        stopping_rule(model, A, "one step")
    # budget(): the device-resident b1 at the cells' nodes (no Dirichlet node here)
    got = f.budget(model, t1)
    want = ref.budget(spec, t1, b1[ref.rows])
    for name, (v, bnd) in zip(("volume", "source", "restoring"), want):
        print(f"interior budget {name}: {got[name]:.6e}, restatement {v:.6e}, |err| / bound {abs(got[name] - v) / bnd:.3f}")
        assert abs(got[name] - v) <= bnd and abs(v) > 1e3 * bnd
    # ... and the matrix identities: int gamma (b* - b1) = 1'load(gamma b*) - 1'R b1, int Q = 1'load(Q)
    lq = ref.load(dict(source=QSERIES), t1)
    lr = ref.load(dict(gamma=GAMMA, target=TARGET), t1)
    rr, cc, vv, bb = ref.matrix(GAMMA)
    assert abs(got["source"] - math.fsum(lq[0])) <= want[1][1] + lq[1].sum()
    assert abs(got["restoring"] - (math.fsum(lr[0]) - math.fsum(vv * b1[cc]))) <= want[2][1] + lr[1].sum() + (bb * np.abs(b1[cc])).sum()
    assert got == f.budget(model, t1)                                                     # one order of every sum
    f.detach()
    return gap, bound


def sponge_spec(model):
    """a sponge over the cells with y > 0.5 (all four vertices), b* linear in z"""
    m = model.fe_data.mesh
    cells = (m.geo_coords[m.cell_geo][:, :, 1] > 0.5).all(axis=1)
    return cells, dict(gamma=2.0, target=lambda x: 1.5 * x[..., 2])


def check_in_the_loop(arch, nsteps=20):
    """check 9: run() for 20 steps on the h = 0.1 bowl with a sponge over y > 0.5: the distance ||b - b*|| over the sponge's nodes
    decreases monotonically"""
    model = sr.bowl_model(arch, "bowl_surface_flux")
    model.timestepper.t_stop = 1e9
    cells, spec = sponge_spec(model)
    assert 256 < cells.sum() < model.fe_data.mesh.ncell // 2
    ref = ref_of(model)
    f = make(model, spec, cells)
    assert np.array_equal(f.cells, np.nonzero(cells)[0])
    rows = np.unique(ref.rows[cells][ref.rows[cells] >= 0])
    # b* at the nodes: interpolate through the model's own set_b path on a scratch vector
    bstar = npg.DeviceVector(arch.ctx, model.fe_data.dofs.nb)
    bstar.upload(model.fe_data.spaces.interpolate_b(spec["target"]), model.fe_data.dofs.p_b)
    bs = bstar.to_host()
    dist = [float(np.linalg.norm((model.b_vec.to_host() - bs)[rows]))]
    for _ in range(nsteps):
        npg.run(model, n_steps=1)
        dist.append(float(np.linalg.norm((model.b_vec.to_host() - bs)[rows])))
    print("interior in the loop: ||b - b*|| over the sponge's nodes:", " ".join(f"{d:.4e}" for d in dist))
    assert all(b < a for a, b in zip(dist, dist[1:])) and dist[-1] < 0.5 * dist[0], dist
    f.detach()
    return dist


def check_parent_bits(arch):
    """check 9, second half: a model that had a forcing attached, applied and detached runs with interior_forcing = None to the bits of a
    model that never had one - the code path of a model without the feature"""
    plain, other = small_channel(arch, "BDF2"), small_channel(arch, "BDF2")
    g = make(other, dict(source=QSERIES, gamma=GAMMA, target=TARGET))
    g.apply(other, 0.1)
    g.detach()
    assert other.interior_forcing is None and plain.interior_forcing is None
    for mdl in (plain, other):
        npg.run(mdl, n_steps=3)
    assert np.array_equal(plain.b_vec.to_host(), other.b_vec.to_host()) and np.abs(plain.b_vec.to_host()).max() > 0
    assert np.array_equal(plain.inversion.solver.x.to_host(), other.inversion.solver.x.to_host())
    assert same_bits(snapshot(plain), snapshot(other)) and not hasattr(plain.evolution, "_rhs_flux_src")


def check_refusals(arch, model):
    """check 10: each refusal leaves rhs_flux, inversion.b and solver.A bit-identical"""
    import pytest
    before = snapshot(model)
    nc = model.fe_data.mesh.ncell
    fake = lambda **kw: SimpleNamespace(**{**model.__dict__, **kw})
    for kw in (dict(layout=SimpleNamespace(cell_owner=np.zeros(1))), dict(comm=object()), dict(partition=object())):
        with pytest.raises(NotImplementedError):
            npg.InteriorForcing(fake(**kw), source=1.0)
    with pytest.raises(NotImplementedError):
        npg.InteriorForcing(SimpleNamespace(fe_data=SimpleNamespace(mesh=SimpleNamespace(dim=2))), source=1.0)
    with pytest.raises(NotImplementedError):
        npg.InteriorForcing(model, restoring=(npg.ForcingSeries([0.0, 1.0], [1.0, 2.0]), 0.0))           # a time-dependent gamma
    bad = [dict(source=lambda x: np.where(x[..., 0] > 0.2, np.nan, 1.0)), dict(source=np.inf), dict(restoring=(lambda x: x[..., 0], 1.0)),
           dict(restoring=(np.nan, 1.0)), dict(restoring=(1.0, lambda x: np.inf * x[..., 0])), dict(source=1.0, cells=np.ones(nc + 1, dtype=bool)),
           dict(source=1.0, cells=np.ones(nc, dtype=np.int64)), dict(source=np.zeros((nc, 10))), dict(restoring=1.0)]
    for kw in bad:
        with pytest.raises(ValueError):
            npg.InteriorForcing(model, **kw)
    assert model.interior_forcing is None and same_bits(snapshot(model), before)
    # restoring and tracers, in either order; a pure source and tracers get along
    model.tracers = npg.PassiveTracers(model, [npg.TracerSpec("dye", initial=lambda x: x[..., 2])])
    try:
        with pytest.raises(NotImplementedError):
            npg.InteriorForcing(model, restoring=(1.0, 0.0))
        npg.InteriorForcing(model, source=1.0).detach()
    finally:
        model.tracers = None
    assert same_bits(snapshot(model), before)
    f = npg.InteriorForcing(model, restoring=(1.0, 0.0))
    try:
        with pytest.raises(NotImplementedError):
            npg.PassiveTracers(model, [npg.TracerSpec("dye")])
        with pytest.raises(ValueError):
            npg.InteriorForcing(model, source=1.0)                                         # one interior forcing per model
    finally:
        f.detach()
    assert same_bits(snapshot(model), before)
    # dropped cells: outside the mask, or gamma and every keyframe of Q zero at all points
    half = lambda x: np.where(x[..., 1] > 0.0, 1.0, 0.0)
    f = npg.InteriorForcing(model, source=npg.ForcingSeries([0.0, 1.0], [0.0, half]), cells=first_cells(nc, 1000))
    xq = model.fe_data.mesh.quad_points()
    assert np.array_equal(f.cells, np.nonzero((xq[:1000, :, 1] > 0.0).any(axis=1))[0]) and f.R is None and 0 < len(f.cells) < 1000
    f.detach()
    # the C ABI's own checks
    f = npg.InteriorForcing(model, source=1.0, restoring=(1.0, 0.0), cells=first_cells(nc, 10))
    f.detach()
    h, lib = f.h, L.lib()
    key, w = (C.c_int32 * 2)(0, 5), (C.c_double * 2)()
    assert lib.npg_interior_apply(h, key, w, f.rhs_src.h) != 0 and b"key" in lib.npg_last_error()
    key[1], w[1] = 0, 1.5
    assert lib.npg_interior_apply(h, key, w, f.rhs_src.h) != 0 and b"weight" in lib.npg_last_error()
    assert lib.npg_interior_budget(h, key, w, model.b_vec.h, f._out.h) != 0 and b"weight" in lib.npg_last_error()
    w[1] = 0.0
    assert lib.npg_interior_apply(h, key, w, None) != 0 and lib.npg_interior_apply(h, key, w, model.inversion.b.h) != 0
    assert lib.npg_interior_budget(h, key, w, model.b_vec.h, None) != 0 and lib.npg_interior_budget(h, key, w, model.inversion.b.h, f._out.h) != 0
    assert lib.npg_interior_set_series(h, 7, 1, None) != 0 and lib.npg_interior_matrix(h, model.inversion.solver.A.h) != 0
    tab = np.full((model.fe_data.mesh.q_w.size, 10), -1.0)
    assert lib.npg_interior_set_gamma(h, L.ptr(tab)) != 0 and b"negative" in lib.npg_last_error()
    tab[3, 4] = np.nan
    assert lib.npg_interior_set_series(h, 0, 1, L.ptr(tab)) != 0 and b"not finite" in lib.npg_last_error()
    out = C.c_void_p()
    for cells in ([3, 3], [5, 2], [0, nc], [-1, 2]):
        ids = L.as_i32(cells)
        assert lib.npg_interior_create(f.fe.h, 2, L.ptr(ids), None, C.byref(out)) != 0
    assert lib.npg_interior_create(f.fe.h, 2, None, None, C.byref(out)) != 0 and lib.npg_interior_create(f.fe.h, -1, None, None, C.byref(out)) != 0
    assert same_bits(snapshot(model), before)


# ---- the host library beside the device library ------------------------------------------------------------------------------------------
def host_library(model, f, t, b):
    """(rhs_src, R values or None, budget) of forcing `f` at time t through libnupgcm_host.so, loaded BESIDE the library the model runs
    on and driven through its C ABI alone, with the kept cells and keyframe tables of `f`"""
    H = C.CDLL(L.HOST_LIB_PATH)
    L._declare(H, partial=True)

    def ok(rc):
        assert rc == 0, H.npg_last_error().decode()
    fed = model.fe_data
    m = fed.mesh
    k = device_fe(model.arch, fed)._keep
    d = L.FeDesc(ncell=m.ncell, nq=len(m.q_w), nloc_b=k["cb"].shape[1], grad_lambda=k["G"].ctypes.data, wdet=k["wdet"].ctypes.data,
                 qw=k["qw"].ctypes.data, N2=k["N2"].ctypes.data, dN2=k["dN2"].ctypes.data, Nb=k["Nb"].ctypes.data, dNb=k["dNb"].ctypes.data,
                 N1=k["N1"].ctypes.data, cell_u=k["cu"].ctypes.data, cell_p=k["cp"].ctypes.data, cell_b=k["cb"].ctypes.data,
                 u_diri=k["ud"].ctypes.data, n_u_diri=k["ud"].size, b_diri=k["bd"].ctypes.data, n_b_diri=k["bd"].size,
                 n_inv=fed.dofs.nu + fed.dofs.np, n_b=fed.dofs.nb)
    ctx, fe, Fh, pat = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(H.npg_ctx_create(0, C.byref(ctx)))
    ok(H.npg_fe_create(ctx, C.byref(d), C.byref(fe)))
    rp, ci, shape = fed.pattern_b()
    rp, ci = L.as_i64(rp), L.as_i32(ci)
    ok(H.npg_csr_create(ctx, shape[0], shape[1], L.ptr(rp), L.ptr(ci), None, C.byref(pat)))
    ok(H.npg_interior_create(fe, len(f.cells), L.ptr(f.cells), pat, C.byref(Fh)))
    key, w = (C.c_int32 * 2)(), (C.c_double * 2)()
    for name, tab in f.key_tables.items():
        i = npg.interior.SERIES.index(name)
        ok(H.npg_interior_set_series(Fh, i, len(tab), L.ptr(L.as_f64(np.transpose(tab, (0, 2, 1))))))
        key[i], w[i] = f.series[name].key_weight(t)
    vecs = []
    for a in (np.zeros(d.n_b), b, np.zeros(3)):
        v = C.c_void_p()
        ok(H.npg_vec_create(ctx, len(a), C.byref(v)))
        ok(H.npg_vec_upload(v, L.ptr(L.as_f64(a))))
        vecs.append(v)
    Rval = None
    if f.restoring:
        ok(H.npg_interior_set_gamma(Fh, L.ptr(L.as_f64(f.gamma_table.T))))
        ok(H.npg_interior_matrix(Fh, pat))
        Rval = np.empty(len(ci))
        ok(H.npg_csr_download(pat, None, None, L.ptr(Rval)))
    ok(H.npg_interior_apply(Fh, key, w, vecs[0]))
    ok(H.npg_interior_budget(Fh, key, w, vecs[1], vecs[2]))
    src, bud = np.empty(d.n_b), np.empty(3)
    ok(H.npg_vec_download(vecs[0], L.ptr(src)))
    ok(H.npg_vec_download(vecs[2], L.ptr(bud)))
    H.npg_interior_destroy(Fh)
    for v in vecs:
        H.npg_vec_destroy(v)
    H.npg_csr_destroy(pat)
    H.npg_fe_destroy(fe)
    H.npg_ctx_destroy(ctx)
    return src, Rval, bud


def check_device_against_host(model, label, cells=None, spec=FULL, t=0.625):
    """the device kernels against the host library on the same tables: the same arithmetic in the same order - within the restatement's
    bound of every row and entry (not a tolerance of its own); prints how many have identical bits.  The budget's three sums are
    folded in a different order by the two libraries (waves and workgroups / chunks of 256 cells): within the restatement's bound."""
    ref = ref_of(model)
    f = make(model, spec, cells)
    try:
        f.apply(model, t)
        b = model.b_vec.to_host()
        got = (f.rhs_src.to_host(), f.R.to_scipy_csr().data, f.budget(model, t))
        host = host_library(model, f, t, b)
    finally:
        f.detach()
    _, lb, touched = ref.load(spec, t, cells)
    rr, cc, _, bb = ref.matrix(spec["gamma"], cells)
    rp, ci, shape = model.fe_data.pattern_b()
    bnd = sp.csr_matrix((bb, (rr, cc)), shape=shape)
    sb = np.asarray(bnd[np.repeat(np.arange(shape[0]), np.diff(rp)), ci]).ravel()
    for name, g, h, bound in (("load rows", got[0], host[0], lb), ("R", got[1], host[1], sb)):
        err = np.abs(g - h)
        print(f"interior device vs host library {label}: {name} worst |err| / bound {np.max(err / np.maximum(bound, 1e-300), initial=0.0):.2e}, "
              f"identical bits {np.mean(g == h) if g.size else 1.0:.4f}")
        assert (err <= bound).all(), (label, name)
    assert np.array_equal(got[0][~touched], host[0][~touched])
    nodal = np.where(ref.rows >= 0, b[np.maximum(ref.rows, 0)], ref.bd)
    want = ref.budget(spec, t, nodal, cells)
    for i, name in enumerate(("volume", "source", "restoring")):
        print(f"interior device vs host library {label}: budget {name} {got[2][name]:.6e} / {host[2][i]:.6e}, |diff| / bound "
              f"{abs(got[2][name] - host[2][i]) / max(want[i][1], 1e-300):.2e}")
        assert abs(got[2][name] - host[2][i]) <= want[i][1] and abs(got[2][name] - want[i][0]) <= want[i][1]
