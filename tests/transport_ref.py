"""A numpy restatement of the tracers' transport operator (nupgcm_amd.transport, csrc/transport_core.h) and the checks
shared by tests/test_transport.py (CPU()) and tests/test_gpu_transport.py (GPU()).

Written from the definition, in the manner of redi_ref and tracers_ref and not from the code under test: geometry from the cells' own
vertex coordinates (redi_ref.geom), nodal values through Spaces' native tables, coefficients from the forcing functions.  With
W = w_q |J| and kappa^ = alpha^2 eps^2 / mu_rho

    u(q)  = scale sum_a N2[q][a] u_a                                                            10 terms per component
    C_ij  = sum_{cells, q} W phi_i ( u_x g_jx + u_y g_jy + u_z g_jz )                            3 nq terms per cell that carries the pair
    g_i   = sum W S phi_i - sum W u_z Gamma phi_i - sum W ( u . grad c_D ) phi_i - sum W lambda c_D phi_i
            - kappa^ sum W ( kappa_h grad_h c_D . grad_h phi_i + kappa_v d_z c_D d_z phi_i ) - kappa^ Gamma sum W kappa_v d_z phi_i + flux_i

Sums are taken in extended precision (np.longdouble / math.fsum).  Bound: a recursive sum of n terms differs from the exact one by at
most (n - 1) eps sum |t| in any order (Higham, eq. 4.4); every bound here is (n + 8) eps sum |t| of the sum in question - the 8 covers
the roundings inside a term - derived, not tuned.  Two evaluations of the same quantity (device and host library) may differ by twice
that.  C and g are restated from the velocity tables the library itself built (they are checked against their own restatement first),
so their bounds are those of their own sums alone."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import nupgcm_amd as npg
from nupgcm_amd import _lib as L
from nupgcm_amd import fe as F
from tests import helpers
from tests import integrals_ref as ir
from tests import redi_ref as rr
from tests import tracers_ref as tr

EPS = np.finfo(np.float64).eps
LD = np.longdouble
NPG_EINVAL = -1
SEED = 20261021
NEW = {"npg_tracers_transport_update", "npg_tracers_transport_matrix", "npg_tracers_transport_load", "npg_tracers_transport_info",
       "npg_tracers_transport_tables"}
DECAY3 = (0.0, 0.37, 2.5)


def report(label, err, bound):
    err, bound = np.asarray(err, dtype=float).ravel(), np.asarray(bound, dtype=float).ravel()
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    print(f"transport {label}: max |err| {err.max(initial=0.0):.3e}, worst |err| / bound {ratio.max(initial=0.0):.3e} over {err.size} entries")
    return float(ratio.max(initial=0.0))


def kappa_hat(model):
    p = model.params
    return p.alpha ** 2 * p.eps ** 2 / p.mu_rho


def check_exports():
    """check 1"""
    assert "TracerTransport" in npg.__all__
    assert NEW <= set(L.declared_symbols())
    hdr = open(L.HEADER_PATH).read()
    for path in (L.HOST_LIB_PATH, L.LIB_PATH):
        lib = C.CDLL(path)
        assert not [s for s in NEW if not hasattr(lib, s) or s + "(" not in hdr], path


# ---- the entry points on a tracer handle, through either library -------------------------------------------------------------------------
class Raw:
    """the five entry points on the handle of a PassiveTracers (the library the model runs on)"""

    def __init__(self, model, specs):
        self.model, self.fed = model, model.fe_data
        self.t = npg.PassiveTracers(model, specs)
        self.lib, self.h, self.ctx = L.lib(), self.t.h, model.arch.ctx
        self.K, self.nb = len(specs), self.fed.dofs.nb
        self.rd = model.evolution.fe.rhs_diff(1.0, npg.DeviceVector(self.ctx, self.nb))
        self.C = model.evolution.fe.new_matrix("b")

    def update(self, x_dev, scale):
        L.check(self.lib.npg_tracers_transport_update(self.h, x_dev.h, float(scale)))
        return self

    def tables(self):
        g = rr.geom(self.fed)
        out = [np.empty((g.nq, g.nc)) for _ in range(3)]
        L.check(self.lib.npg_tracers_transport_tables(self.h, *(L.ptr(a) for a in out)))
        return np.stack([a.T for a in out], axis=-1)                        # (nc, nq, 3)

    def matrix(self):
        L.check(self.lib.npg_tracers_transport_matrix(self.h, self.C.h))
        A = self.C.to_scipy_csr()
        A.sort_indices()
        return A

    def load(self, khat, decay=None):
        out = npg.DeviceVector(self.ctx, self.K * self.nb)
        dec = None if decay is None else L.as_f64(np.asarray(decay, dtype=float))
        L.check(self.lib.npg_tracers_transport_load(self.h, float(khat), None if dec is None else L.ptr(dec), self.rd.h,
                                                    None if self.t.flux is None else self.t.flux.h, out.h))
        return out.to_host()


class HostRaw(rr.HostLibrary):
    """the same through libnupgcm_host.so loaded beside the device library (redi_ref.HostLibrary: the model's own tables)"""

    def handle(self, specs, flux_host):
        H, fed = self.H, self.fed
        T = C.c_void_p()
        self.ok(H.npg_tracers_create(self.fe, len(specs), C.byref(T)))
        dn = tr.diri_nodes(fed)
        for j, s in enumerate(specs):
            cd, _ = tr.spec_arrays(self.model, s)
            dv = np.zeros(self.k["bd"].size)
            dv[:len(dn)] = cd[dn]
            self.ok(H.npg_tracers_set(T, j, L.ptr(L.as_f64(dv)), float(s.get("gamma", 0.0)), float(s.get("source", 0.0))))
        self.T, self.K, self.nb = T, len(specs), fed.dofs.nb
        self.rd = self.vec(np.zeros(self.nb))
        self.ok(H.npg_fe_assemble_rhs_diff(self.fe, 1.0, self.rd))
        self.fl = None if flux_host is None else self.vec(flux_host)
        return self

    def update(self, x, scale):
        self.ok(self.H.npg_tracers_transport_update(self.T, self.vec(x), float(scale)))
        return self

    def tables(self):
        g = rr.geom(self.fed)
        out = [np.empty((g.nq, g.nc)) for _ in range(3)]
        self.ok(self.H.npg_tracers_transport_tables(self.T, *(L.ptr(a) for a in out)))
        return np.stack([a.T for a in out], axis=-1)

    def matrix(self):
        rp, ci, shape = self.fed.pattern_b()
        rp, ci = L.as_i64(rp), L.as_i32(ci)
        K = C.c_void_p()
        self.ok(self.H.npg_csr_create(self.ctx, shape[0], shape[1], L.ptr(rp), L.ptr(ci), None, C.byref(K)))
        self.ok(self.H.npg_tracers_transport_matrix(self.T, K))
        v = np.empty(len(ci))
        rp2, ci2 = np.empty_like(rp), np.empty_like(ci)
        self.ok(self.H.npg_csr_download(K, L.ptr(rp2), L.ptr(ci2), L.ptr(v)))
        A = sp.csr_matrix((v, ci2, rp2), shape=shape)
        A.sort_indices()
        return A

    def load(self, khat, decay=None):
        vy = self.vec(np.zeros(self.K * self.nb))
        dec = None if decay is None else L.as_f64(np.asarray(decay, dtype=float))
        self.ok(self.H.npg_tracers_transport_load(self.T, float(khat), None if dec is None else L.ptr(dec), self.rd, self.fl, vy))
        out = np.empty(self.K * self.nb)
        self.ok(self.H.npg_vec_download(vy, L.ptr(out)))
        return out


def random_flow(model, seed=SEED):
    fed = model.fe_data
    x = np.random.default_rng(seed).standard_normal(fed.dofs.nu + fed.dofs.np)
    return x, npg.DeviceVector.from_host(model.arch.ctx, x)


# ---- check 2: the velocity tables -----------------------------------------------------------------------------------------------------------
def restate_velocity(fed, x, scale):
    """(u (nc, nq, 3), bound) from the nodal velocities: 10 terms per component"""
    m = fed.mesh
    _, _, _, lam, _, ea, eb = ir.geometry(m)
    N, _ = F.p2_tables(lam, ea, eb)
    un = tr.velocity_nodal(fed, x)[m.cell_nodes]                            # (nc, 10, 3)
    u = np.asarray(scale * np.einsum("qi,cia->cqa", N.astype(LD), un.astype(LD)), dtype=float)
    sabs = abs(scale) * np.einsum("qi,cia->cqa", np.abs(N), np.abs(un))
    return u, (10 + 8) * EPS * sabs


def check_tables(model, label, specs=({"name": "a"},), against=None):
    raw = Raw(model, list(specs))
    x, xd = random_flow(model)
    got = raw.update(xd, 0.7).tables()
    want, bound = restate_velocity(model.fe_data, x, 0.7)
    out = dict(tables=report(f"{label}: velocity tables against the restatement", np.abs(got - want), bound))
    assert (np.abs(got - want) <= bound).all() and np.abs(got).max() > 0.1
    st, um = C.c_int(), C.c_double()
    L.check(raw.lib.npg_tracers_transport_info(raw.h, C.byref(st), C.byref(um)))
    assert st.value == L.NPG_TRANSPORT_UPDATED and um.value == np.sqrt((got ** 2).sum(axis=-1)).max()
    if against is not None:
        host = against.handle(list(specs), None).update(x, 0.7).tables()
        print(f"transport {label}: device tables against the host library's: {int(np.count_nonzero(got != host))} entries differ")
        assert np.array_equal(got, host)
    zero = raw.update(xd, 0.0).tables()
    Cz = raw.matrix()
    assert not zero.any() and not Cz.data.any()                              # scale = 0: exact zeros in the tables and in C
    return out


# ---- check 3: the matrix -----------------------------------------------------------------------------------------------------------------
def node_matrix(fed, terms, nterm):
    """a node-level matrix (Dirichlet nodes included) from per-point terms: `terms(q)` yields arrays (nc, nl, nl), nterm of them per
    point -> SimpleNamespace(K, S = sum |term|, bound = (n + 8) eps S) as scipy CSR matrices on one pattern"""
    g = rr.geom(fed)
    val = np.zeros((g.nc, g.nl, g.nl), dtype=LD)
    sab = np.zeros((g.nc, g.nl, g.nl), dtype=LD)
    for q in range(g.nq):
        for t in terms(q):
            val += t
            sab += np.abs(t)
    nn = fed.spaces.nb_nodes
    key = (g.cells_b[:, :, None].astype(np.int64) * nn + g.cells_b[:, None, :]).ravel()
    uk, inv = np.unique(key, return_inverse=True)
    V, S, Nn = np.zeros(len(uk), dtype=LD), np.zeros(len(uk), dtype=LD), np.zeros(len(uk))
    np.add.at(V, inv, val.ravel())
    np.add.at(S, inv, sab.ravel())
    np.add.at(Nn, inv, nterm * g.nq)
    ri, ci = uk // nn, uk % nn
    mk = lambda d: sp.csr_matrix((np.asarray(d, dtype=float), (ri, ci)), shape=(nn, nn))
    return SimpleNamespace(K=mk(V), S=mk(S), bound=mk((Nn + 8) * EPS * np.asarray(S, dtype=float)), n=mk(Nn))


def restate_matrix(fed, u):
    g = rr.geom(fed)
    wphi = g.W[:, :, None] * g.Nb[None, :, :]                                # (nc, nq, nl): W phi_i

    def terms(q):
        for a in range(3):
            yield (wphi[:, q, :, None] * (u[:, q, a, None] * g.gphi[:, q, :, a])[:, None, :]).astype(LD)
    return node_matrix(fed, terms, 3)


def restate_mass(fed):
    g = rr.geom(fed)
    return node_matrix(fed, lambda q: [(g.W[:, q, None, None] * g.Nb[q][None, :, None] * g.Nb[q][None, None, :]).astype(LD)], 1)


def restate_diffusion(model):
    """Kh + Kv (3 terms per point) - for the bounds of the engine's own entries"""
    fed, f = model.fe_data, model.forcings
    g = rr.geom(fed)
    kh, kv = ir.coefficient(fed.mesh, f.kappa_h, g.xq), ir.coefficient(fed.mesh, f.kappa_v, g.xq)

    def terms(q):
        for a, k in ((0, kh), (1, kh), (2, kv)):
            yield ((g.W * k)[:, q, None, None] * g.gphi[:, q, :, None, a] * g.gphi[:, q, None, :, a]).astype(LD)
    return node_matrix(fed, terms, 3)


def check_matrix(model, label, against=None):
    fed = model.fe_data
    raw = Raw(model, [dict(name="a")])
    x, xd = random_flow(model)
    u = raw.update(xd, 0.7).tables()
    A = raw.matrix()
    ref = restate_matrix(fed, u)
    Kff, Kfd = rr.free_block(fed, ref.K)
    Bff, Bfd = rr.free_block(fed, ref.bound)
    got, P = rr.entries(A, Bff)
    want, _ = rr.entries(Kff, Bff)
    out = dict(entries=report(f"{label}: C entry by entry", np.abs(got - want), P.data))
    assert (np.abs(got - want) <= P.data).all() and np.abs(got).max() > 1e3 * P.data.max()
    mask = sp.csr_matrix((np.ones(len(P.data)), (P.row, P.col)), shape=A.shape)
    assert (A - A.multiply(mask)).count_nonzero() == 0                       # nothing outside the restated entries
    absA = abs(A)
    rs = np.asarray(A.sum(axis=1)).ravel() + np.asarray(Kfd.sum(axis=1)).ravel()
    rb = np.asarray(Bff.sum(axis=1)).ravel() + np.asarray(Bfd.sum(axis=1)).ravel() \
        + (np.diff(A.indptr) + Kfd.getnnz(axis=1) + 8) * EPS * (np.asarray(absA.sum(axis=1)).ravel() + np.asarray(abs(Kfd).sum(axis=1)).ravel())
    out["rowsum"] = report(f"{label}: row sums over free and Dirichlet columns (the basis sums to 1)", np.abs(rs), rb)
    assert (np.abs(rs) <= rb).all()
    assert np.array_equal(A.data, raw.matrix().data)                         # the same bits on every call
    if against is not None:
        H = against.handle([dict(name="a")], None).update(x, 0.7).matrix()
        goth, _ = rr.entries(H, Bff)
        out["host"] = report(f"{label}: device vs host library, C ({int(np.count_nonzero(got != goth))} entries differ)", np.abs(got - goth), 2 * P.data)
        assert (np.abs(got - goth) <= 2 * P.data).all()
    return out


# ---- check 4: a known answer that does not go through the restatement ---------------------------------------------------------------------------
def check_linear_tracer(model, label):
    """c = a . x: u . grad c = u . a lies in the P2 space and every integrand has degree 4, which the rule integrates exactly, so
    C c = M (u_j . a) row by row with the engine's own M.  n = the terms of an entry's sum (3 nq per cell of the pair) + the row's
    entries + 8."""
    fed = model.fe_data
    assert fed.spaces.b_order == 2 and not np.any(fed.tables.b_pos < 0)
    raw = Raw(model, [dict(name="a")])
    x, xd = random_flow(model)
    A = raw.update(xd, 1.0).matrix()
    M = model.evolution.M.to_scipy_csr()
    a = np.array([0.7, -1.3, 0.45])
    pos = fed.tables.b_pos
    X = fed.mesh.node_coords[:fed.spaces.nb_nodes]
    un = tr.velocity_nodal(fed, x)[:fed.spaces.nb_nodes]
    c, ua = np.zeros(raw.nb), np.zeros(raw.nb)
    c[pos] = X @ a
    ua[pos] = un @ a
    lhs, rhs = spmv(A, c)[0], spmv(M, ua)[0]
    g = rr.geom(fed)
    cells_per_pair = np.bincount(g.cells_b.ravel()).max()
    n = 3 * g.nq * cells_per_pair + np.diff(A.indptr) + 8
    bound = n * EPS * (abs(A) @ np.abs(c) + abs(M) @ np.abs(ua))
    out = report(f"{label}: C (a . x) = M (u . a)", np.abs(lhs - rhs), bound)
    assert (np.abs(lhs - rhs) <= bound).all() and np.abs(lhs).max() > 1e3 * bound.max()
    return out


def _row_terms(A, x):
    A = A.tocsr()
    prod = (A.data * x[A.indices]).tolist()
    return [prod[a:b] for a, b in zip(A.indptr[:-1], A.indptr[1:])]


def spmv(A, x):
    """(A x in extended precision, (row entries + 8) eps |A| |x|)"""
    y = np.array([math.fsum(r) for r in _row_terms(A, x)])
    return y, (np.diff(A.tocsr().indptr) + 8) * EPS * (abs(A) @ np.abs(x))


# ---- check 6: the load ---------------------------------------------------------------------------------------------------------------------
def restate_load(model, spec, u, khat, lam):
    """one tracer from the velocity tables u (nc, nq, 3) -> SimpleNamespace(total (nb,), bound) over the free rows"""
    fed, f = model.fe_data, model.forcings
    g = rr.geom(fed)
    cd, flux_load = tr.spec_arrays(model, spec)
    gamma, source = float(spec.get("gamma", 0.0)), float(spec.get("source", 0.0))
    rows = fed.tables.b_pos[g.cells_b]
    nb = fed.dofs.nb
    W, phi, gphi = g.W, g.Nb[None, :, :], g.gphi
    tab = lambda v: ir.coefficient(fed.mesh, v, g.xq)
    lines = {}
    if source != 0.0:
        lines["source"] = (source * W)[..., None] * phi
    if gamma != 0.0:
        lines["gamma_adv"] = (-gamma * W * u[..., 2])[..., None] * phi
        lines["gamma_diff"] = -khat * gamma * (W * tab(f.kappa_v))[..., None] * gphi[..., 2]
    if np.any(cd != 0.0):
        cdc = cd[g.cells_b]
        cdq = np.einsum("qi,ci->cq", g.Nb, cdc)
        gd = np.einsum("cqij,ci->cqj", gphi, cdc)
        for a in range(3):
            lines[f"adv_lift{a}"] = (-W * u[..., a] * gd[..., a])[..., None] * phi
        if lam != 0.0:
            lines["decay_lift"] = (-lam * W * cdq)[..., None] * phi
        kh, kv = tab(f.kappa_h), tab(f.kappa_v)
        lines["lift_h0"] = -khat * (W * kh * gd[..., 0])[..., None] * gphi[..., 0]
        lines["lift_h1"] = -khat * (W * kh * gd[..., 1])[..., None] * gphi[..., 1]
        lines["lift_v"] = -khat * (W * kv * gd[..., 2])[..., None] * gphi[..., 2]
    shape = (g.nc, g.nq, g.nl)
    rr_ = np.broadcast_to(rows[:, None, :], shape)
    keep = rr_ >= 0
    rall = [rr_[keep]] * len(lines)
    vall = [np.broadcast_to(v, shape)[keep] for v in lines.values()]
    if flux_load is not None:
        free = np.nonzero(fed.tables.b_pos >= 0)[0]
        rall.append(fed.tables.b_pos[free])
        vall.append(flux_load[free])
    if not vall:
        return SimpleNamespace(total=np.zeros(nb), bound=np.zeros(nb))
    rall, vall = np.concatenate(rall), np.concatenate(vall)
    order = np.argsort(rall, kind="stable")
    rall, vall = rall[order], vall[order]
    cut = np.searchsorted(rall, np.arange(nb + 1))
    vl = vall.tolist()
    total = np.array([math.fsum(vl[a:b]) for a, b in zip(cut[:-1], cut[1:])])
    sabs = np.bincount(rall, weights=np.abs(vall), minlength=nb)
    return SimpleNamespace(total=total, bound=(np.diff(cut) + 8) * EPS * sabs)


def check_load(model, label, specs=tr.SPECS3, decay=DECAY3, against=None):
    raw = Raw(model, specs)
    nb, khat = raw.nb, kappa_hat(model)
    x, xd = random_flow(model)
    u = raw.update(xd, 0.7).tables()
    got = raw.load(khat, decay)
    ref = [restate_load(model, s, u, khat, lam) for s, lam in zip(specs, decay)]
    out = {}
    for k, r in enumerate(ref):
        err = np.abs(got[k * nb:(k + 1) * nb] - r.total)
        out[k] = report(f"{label}: load of tracer {k} ({specs[k]['name']}, lambda = {decay[k]:g})", err, r.bound)
        assert (err <= r.bound).all() and np.abs(r.total).max() > 1e3 * r.bound.max()
    assert np.array_equal(got, raw.load(khat, decay))                        # the same bits on every call
    for k in range(len(specs)):                                              # tracer k of a K = 3 call has the bits of a K = 1 call
        one = Raw(model, [specs[k]])
        assert np.array_equal(one.update(xd, 0.7).load(khat, [decay[k]]), got[k * nb:(k + 1) * nb]), k
    if against is not None:
        host = against.handle(specs, None if raw.t.flux is None else raw.t.flux.to_host()).update(x, 0.7).load(khat, decay)
        b2 = 2 * np.concatenate([r.bound for r in ref])
        out["host"] = report(f"{label}: device vs host library, loads ({int(np.count_nonzero(got != host))} rows differ)", np.abs(got - host), b2)
        assert (np.abs(got - host) <= b2).all()
    return out


# ---- check 5: the explicit twin -----------------------------------------------------------------------------------------------------------------
def check_twin(model, label, specs=tr.SPECS3, dt=0.013):
    """npg_tracers_rhs(BDF1, dt, theta = dt kappa^, c, c, x, x) is the explicit step's right-hand side: the diffusion is on its LEFT
    (A = M + theta (Kh + Kv)), so with T = C + kappa^ (Kh + Kv) as TracerTransport combines it

        y = M c + dt (g - T c) + theta (Kh + Kv) c          (= M c + dt (g - C c)),

    row by row over the free rows.  The bound is the sum of the terms' bounds: the right-hand side's own summation bound
    (tracers_ref.restate_set), dt times the load's, the entries' bounds of M and C times |c|, and the four products'."""
    fed, ev = model.fe_data, model.evolution
    raw = Raw(model, specs)
    nb, khat = raw.nb, kappa_hat(model)
    theta = dt * khat
    x, xd = random_flow(model)
    rng = np.random.default_rng(SEED + 1)
    c = rng.standard_normal(raw.K * nb)
    raw.t.c.upload(c)
    raw.t.c_prev.upload(c)
    y = raw.t.rhs(L.NPG_BDF1, dt, theta, xd, xd).to_host()
    rref = tr.restate_set(model, specs, L.NPG_BDF1, dt, theta, x, x, c, c)
    u = raw.update(xd, 1.0).tables()
    raw.matrix()
    T = ev.fe.new_matrix("b").combine(1.0, raw.C, khat, ev.Kh, ev.Kv).to_scipy_csr()
    M, Kh, Kv = ev.M.to_scipy_csr(), ev.Kh.to_scipy_csr(), ev.Kv.to_scipy_csr()
    g = raw.load(khat, None)
    Bc, _ = rr.free_block(fed, restate_matrix(fed, u).bound)
    Bm, _ = rr.free_block(fed, restate_mass(fed).bound)
    out = {}
    for k, s in enumerate(specs):
        ck = c[k * nb:(k + 1) * nb]
        lref = restate_load(model, s, u, khat, 0.0)
        Mc, bM = spmv(M, ck)
        Tc, bT = spmv(T, ck)
        Hc, bH = spmv(Kh, ck)
        Vc, bV = spmv(Kv, ck)
        want = Mc + dt * (g[k * nb:(k + 1) * nb] - Tc) + theta * (Hc + Vc)
        # (T's entries carry the two roundings of the combination: 2 eps of their terms, inside 4 eps |T| + ... below)
        bound = rref[k].bound + dt * lref.bound + bM + dt * bT + theta * (bH + bV) + Bm @ np.abs(ck) + dt * (Bc @ np.abs(ck)) \
            + 4 * EPS * (dt * (abs(T) @ np.abs(ck)) + theta * ((abs(Kh) + abs(Kv)) @ np.abs(ck))) + 8 * EPS * (np.abs(want) + np.abs(Mc))
        out[k] = report(f"{label}: explicit twin, tracer {k} ({s['name']})", np.abs(y[k * nb:(k + 1) * nb] - want), bound)
        assert (np.abs(y[k * nb:(k + 1) * nb] - want) <= bound).all() and np.abs(want).max() > 1e3 * bound.max()
    return out


# ---- checks 7 and 8 on a model with a flow of its own -------------------------------------------------------------------------------------------
_FLOW = {}


def flow_model(arch, config):
    """helpers.build_model(config) after three steps, built once per architecture"""
    key = (type(arch).__name__, config)
    if key not in _FLOW:
        m = helpers.build_model(config, nsteps=3, arch=arch)
        npg.run(m)
        _FLOW[key] = m
    return _FLOW[key]


def system(tt, k):
    """(T_k, g_k, 1 / diag T_k) on the host"""
    T = tt.operator(k).to_scipy_csr()
    T.sort_indices()
    return T, tt.load(k).to_host(), 1.0 / T.diagonal()


def true_residual(T, g, c, Pd):
    """(||P (g - T c)|| in extended precision, the bound of that sum)"""
    Tc, bT = spmv(T, c)
    r = (g.astype(LD) - Tc.astype(LD)) * Pd.astype(LD)
    nrm = float(np.sqrt((r * r).sum()))
    # |d ||Pr||| <= ||P dr||: dr from the product's bound and one rounding of the difference; the norm's own sum adds (n + 8) eps / 2 of it
    dr = Pd * (bT + EPS * (np.abs(g) + np.abs(Tc)))
    return nrm, float(np.sqrt((dr * dr).sum())) + (len(c) + 8) * EPS * nrm


def check_equilibrium(tt, k, label, rtol=1e-8):
    """the three conditions of check 8 on tracer k after tt.equilibrium(rtol=rtol)"""
    T, g, Pd = system(tt, k)
    c = tt.view(k).to_host()
    st = tt.stats[k]
    rn, r0 = tt.residual[k]
    true, bound = true_residual(T, g, c, Pd)
    true0, bound0 = true_residual(T, g, np.zeros_like(c), Pd)
    print(f"transport {label}: solved {st['solved']} in {st['niter']} iterations, {st['passes']} pass(es); ||P r|| {true:.3e} "
          f"(reported {rn:.3e}, |diff| / bound {abs(true - rn) / bound:.3e}), ||P r0|| {true0:.3e} (reported {r0:.3e}), "
          f"||P r|| / (rtol ||P r0||) {true / (rtol * true0):.3e}")
    assert st["solved"] == 1
    assert true <= rtol * true0 + bound and abs(true - rn) <= 2 * bound and abs(true0 - r0) <= 2 * bound0
    # the cap against stagnation: scipy's restarted GMRES on the same left-preconditioned system, restart and tolerance
    count = [0]
    PT = sp.diags(Pd) @ T
    _, info = spla.gmres(PT, Pd * g, x0=np.zeros_like(g), rtol=rtol, atol=0.0, restart=tt.memory, maxiter=2 * len(g),
                         callback=lambda _r: count.__setitem__(0, count[0] + 1), callback_type="pr_norm")
    print(f"transport {label}: scipy gmres({tt.memory}) info {info}, {count[0]} iterations; cap {2 * count[0] + 20}")
    assert info == 0 and st["niter"] <= 2 * count[0] + 20
    return st["niter"], count[0]


def check_ideal_age(arch):
    """8 (a): bowl_mixing after three steps, S = 1, Dirichlet 0, lambda = 0, scale = 1"""
    m = flow_model(arch, "bowl_mixing")
    tt = npg.TracerTransport(m, [dict(name="age", source=1.0, dirichlet=0.0)])
    tt.equilibrium(rtol=1e-8)
    out = check_equilibrium(tt, 0, "ideal age on bowl_mixing")
    v = tt.values("age")
    print(f"transport ideal age: {v.min():.3f} .. {v.max():.3f}; largest cell Peclet number {tt.peclet().max():.3e}")
    assert v.min() > 0
    return tt, out


def check_decaying(arch):
    """8 (b): bowl_surface_flux (no Dirichlet nodes, kappa^ = 0.025), S = 1, lambda = 1, the flow of 8 (a) - bowl_mixing after three
    steps, the same mesh and velocity space - at scale = 100.  The configuration's OWN flow after three steps is the wrong one for
    this case: at scale 100 a diagonal entry of T is -1.9e-4 even with lambda = 1 (min C_ii = -3.9e-6 at scale 1), which set_flow
    refuses - asserted here, as the refusal on a real flow."""
    m = flow_model(arch, "bowl_surface_flux")
    x = flow_model(arch, "bowl_mixing").inversion.solver.x
    assert not np.any(m.fe_data.tables.b_pos < 0) and x.n == m.inversion.solver.x.n
    with np.testing.assert_raises(ValueError) as e:
        npg.TracerTransport(m, [dict(name="dye", source=1.0)], scale=100.0, decay=[1.0])
    print("transport:", e.exception)
    assert "Peclet" in str(e.exception)
    tt = npg.TracerTransport(m, [dict(name="dye", source=1.0)], flow=x, scale=100.0, decay=[1.0])
    tt.equilibrium(rtol=1e-8)
    return check_equilibrium(tt, 0, "decaying tracer on bowl_surface_flux, scale 100")


def check_constant(arch, mesh):
    """a tracer with Dirichlet value 1 and S = Gamma = lambda = 0 on bowl_diri: c = 1 is the solution, g = T_ff 1 exactly"""
    from tests import interior_ref as itr
    m = itr.light_model(arch, mesh, config="bowl_diri")
    x, xd = random_flow(m)
    tt = npg.TracerTransport(m, [dict(name="one", dirichlet=1.0)], flow=xd, scale=1e-5)
    T, g, Pd = system(tt, 0)
    fed = m.fe_data
    u = np.stack(tt.tables(), axis=-1)
    T1, bT = spmv(T, np.ones(len(g)))
    lref = restate_load(m, dict(name="one", dirichlet=1.0), u, tt.kappa_hat, 0.0)
    Bc, _ = rr.free_block(fed, restate_matrix(fed, u).bound)
    Bk, _ = rr.free_block(fed, restate_diffusion(m).bound)
    # the load's own sum, the product's, the entries' of C and of kappa^ (Kh + Kv), the two roundings of the combination
    bound = lref.bound + bT + np.asarray(Bc.sum(axis=1)).ravel() + tt.kappa_hat * np.asarray(Bk.sum(axis=1)).ravel() \
        + 4 * EPS * np.asarray(abs(T).sum(axis=1)).ravel()
    out = report("bowl_diri: g = T_ff 1 for a tracer that is 1 on the boundary", np.abs(g - T1), bound)
    assert (np.abs(g - T1) <= bound).all() and np.abs(g).max() > 1e3 * bound.max()
    tt.equilibrium(rtol=1e-8)
    true, b = true_residual(T, g, tt.view(0).to_host(), Pd)
    true0, _ = true_residual(T, g, np.zeros_like(g), Pd)
    dev = np.abs(tt.values(0) - 1.0).max()
    print(f"transport constant tracer: ||P r|| / (rtol ||P r0||) {true / (1e-8 * true0):.3e}, max |c - 1| {dev:.3e}, {tt.stats[0]['niter']} iterations")
    assert tt.stats[0]["solved"] == 1 and true <= 1e-8 * true0 + b
    return out


# ---- check 7: the step's algebra ------------------------------------------------------------------------------------------------------------
def check_step_algebra(arch, tt_eq=None):
    m = flow_model(arch, "bowl_mixing")
    specs = [dict(name="age", source=1.0, dirichlet=0.0), dict(name="dye", dirichlet=lambda x: 0.3 + 0.5 * x[..., 0], source=-0.4, gamma=0.6,
                                                              initial=lambda x: np.sin(3.0 * x[..., 0]) * x[..., 2])]
    tt = npg.TracerTransport(m, specs, decay=[0.0, 0.8])
    M = m.evolution.M.to_scipy_csr()
    nb, dt = tt.nb, 0.37
    rng = np.random.default_rng(SEED + 3)
    out = {}
    for scheme in ("BDF1", "BDF2"):
        c, cp = rng.standard_normal(2 * nb), rng.standard_normal(2 * nb)
        tt.c.upload(c)
        tt.c_prev.upload(cp)
        tt.step(dt, scheme, rtol=1e-10)
        assert np.array_equal(tt.c_prev.to_host(), c)                        # the history rotated
        for k in range(2):
            A_dev, _, cdt, c1, c2 = tt.step_system(k, dt, scheme)
            assert tt.step_system(k, dt, scheme)[0] is A_dev                 # cached per (cdt, lambda)
            A, (T, g, _) = A_dev.to_scipy_csr(), system(tt, k)
            A.sort_indices()
            M.sort_indices()
            assert np.array_equal(A.indices, T.indices) and np.array_equal(A.indices, M.indices)
            e = np.abs(A.data - (M.data + cdt * T.data))
            out[(scheme, k, "A")] = report(f"step {scheme} tracer {k}: A = M + cdt T entry by entry", e, 2 * EPS * (np.abs(M.data) + np.abs(cdt * T.data)))
            assert (e <= 2 * EPS * (np.abs(M.data) + np.abs(cdt * T.data))).all()
            ck, cpk = c[k * nb:(k + 1) * nb], cp[k * nb:(k + 1) * nb]
            w = c1 * ck + c2 * cpk
            Mw, bM = spmv(M, w)
            want = Mw + cdt * g
            bound = bM + abs(M) @ (2 * EPS * (np.abs(c1 * ck) + np.abs(c2 * cpk))) + 2 * EPS * (np.abs(Mw) + np.abs(cdt * g))
            y = tt.y.view(k * nb, nb).to_host()
            out[(scheme, k, "y")] = report(f"step {scheme} tracer {k}: right-hand side", np.abs(y - want), bound)
            assert (np.abs(y - want) <= bound).all()
            assert tt.step_stats[k]["solved"] == 1
    # at an equilibrium c* (c = c_prev = c*) the step's initial residual is cdt times the steady one
    te = tt_eq if tt_eq is not None else npg.TracerTransport(m, [dict(name="age", source=1.0, dirichlet=0.0)]).equilibrium()
    cs = te.view(0).to_host()
    T, g, _ = system(te, 0)
    for scheme in ("BDF1", "BDF2"):
        te.c.upload(cs)
        te.c_prev.upload(cs)
        A_dev, _, cdt, c1, c2 = te.step_system(0, dt, scheme)
        A = A_dev.to_scipy_csr()
        te.step(dt, scheme, itmax=1)
        y = te.y.view(0, nb).to_host()
        Ac, bA = spmv(A, cs)
        Tc, bT = spmv(T, cs)
        Mc, bM = spmv(M, cs)
        lhs, rhs = y - Ac, cdt * (g - Tc)
        bound = bA + cdt * bT + 2 * bM + 4 * EPS * (np.abs(y) + np.abs(Ac) + cdt * (np.abs(g) + np.abs(Tc)) + np.abs(Mc)) \
            + 2 * EPS * ((abs(M) + cdt * abs(T)) @ np.abs(cs))
        out[(scheme, "eq")] = report(f"step {scheme} at the equilibrium: y - A c* = cdt (g - T c*)", np.abs(lhs - rhs), bound)
        assert (np.abs(lhs - rhs) <= bound).all()
    return out


# ---- check 9: passive -------------------------------------------------------------------------------------------------------------------
def check_passive(arch):
    """three steps of bowl_mixing with a PassiveTracers attached give the same u, p, b' and tracer bits whether or not a TracerTransport
    was created, solved and stepped in between"""
    runs = []
    for with_transport in (False, True):
        m = helpers.build_model("bowl_mixing", nsteps=3, arch=arch)
        t = m.tracers = npg.PassiveTracers(m, tr.SPECS3)
        npg.run(m, n_steps=2)
        if with_transport:
            tt = npg.TracerTransport(m, [dict(name="age", source=1.0, dirichlet=0.0), dict(name="dye", dirichlet=0.4, gamma=0.3)], decay=[0.0, 1.0])
            tt.equilibrium(rtol=1e-6)
            tt.step(0.5, "BDF2")
            assert tt.stats[0]["solved"] == 1 and np.abs(tt.values("age")).max() > 0
        npg.run(m)
        runs.append([getattr(m.state, n) for n in ("u", "p", "b")] + [t.values(k) for k in range(3)])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    print("transport: u, p, b' and three attached tracers keep their bits with a TracerTransport created, solved and stepped after step 2")


# ---- check 10: refusals -------------------------------------------------------------------------------------------------------------------
def check_refusals(model, flat_model=None):
    """every NPG_EINVAL leaves the tables' state, `out` and C untouched; the Python class raises"""
    lib = L.lib()
    ctx, fed = model.arch.ctx, model.fe_data
    other_ctx = npg.architectures.Context(ctx.device)                        # a second context of the same library
    nb, ninv = fed.dofs.nb, fed.dofs.nu + fed.dofs.np
    raw = Raw(model, [dict(name="a"), dict(name="b", gamma=0.5)])
    err = lambda: lib.npg_last_error().decode()
    V = lambda n: npg.DeviceVector(ctx, n)
    x, xd = random_flow(model)
    out = V(2 * nb)
    out.fill(-7.0)
    Cm = model.evolution.fe.new_matrix("b")
    filler = Raw(model, [dict(name="z")]).update(xd, 1.0)                    # (held: a handle must outlive the call)
    L.check(lib.npg_tracers_transport_matrix(filler.h, Cm.h))
    before = Cm.to_scipy_csr().data.copy()
    khat = kappa_hat(model)
    untouched = lambda: np.array_equal(out.to_host(), np.full(2 * nb, -7.0)) and np.array_equal(Cm.to_scipy_csr().data, before)
    state = lambda: (C.c_int(), C.c_double())

    def info():
        st, um = state()
        L.check(lib.npg_tracers_transport_info(raw.h, C.byref(st), C.byref(um)))
        return st.value
    # before an update: matrix, load and tables are refused
    assert lib.npg_tracers_transport_matrix(raw.h, Cm.h) == NPG_EINVAL and "npg_tracers_transport_update first" in err()
    assert lib.npg_tracers_transport_load(raw.h, khat, None, raw.rd.h, None, out.h) == NPG_EINVAL and "npg_tracers_transport_update first" in err()
    buf = np.zeros(3)
    assert lib.npg_tracers_transport_tables(raw.h, L.ptr(buf), L.ptr(buf), L.ptr(buf)) == NPG_EINVAL
    assert info() == L.NPG_TRANSPORT_OFF and untouched()
    # update
    for s in (np.nan, np.inf, -np.inf):
        assert lib.npg_tracers_transport_update(raw.h, xd.h, s) == NPG_EINVAL and "scale" in err()
    short = V(ninv - 1)
    assert lib.npg_tracers_transport_update(raw.h, short.h, 1.0) == NPG_EINVAL and "flow vector" in err()
    assert info() == L.NPG_TRANSPORT_OFF
    raw.update(xd, 1.0)
    # matrix
    wrong = npg.DeviceCSR.from_pattern(ctx, nb - 1, nb - 1, np.arange(nb), np.arange(nb - 1))
    assert lib.npg_tracers_transport_matrix(raw.h, wrong.h) == NPG_EINVAL and "buoyancy pattern" in err()
    if nb > 1:
        diag = npg.DeviceCSR.from_pattern(ctx, nb, nb, np.arange(nb + 1), np.arange(nb))
        assert lib.npg_tracers_transport_matrix(raw.h, diag.h) == NPG_EINVAL and "buoyancy pattern" in err()
    # load
    for bad in (-1e-3, np.nan, np.inf):
        assert lib.npg_tracers_transport_load(raw.h, bad, None, raw.rd.h, None, out.h) == NPG_EINVAL and "kappa_hat" in err()
        dec = L.as_f64(np.array([0.0, bad]))
        assert lib.npg_tracers_transport_load(raw.h, khat, L.ptr(dec), raw.rd.h, None, out.h) == NPG_EINVAL and "decay" in err()
    one = V(nb)
    assert lib.npg_tracers_transport_load(raw.h, khat, None, raw.rd.h, None, one.h) == NPG_EINVAL and "output vector" in err()
    assert lib.npg_tracers_transport_load(raw.h, khat, None, raw.rd.h, one.h, out.h) == NPG_EINVAL and "flux" in err()
    assert lib.npg_tracers_transport_load(raw.h, khat, None, out.h, None, out.h) == NPG_EINVAL and "rhs_diff1" in err()
    assert lib.npg_tracers_transport_load(raw.h, khat, None, None, None, out.h) == NPG_EINVAL and "background gradient" in err()
    assert untouched()
    # handles of different contexts
    xo, oo = npg.DeviceVector(other_ctx, ninv), npg.DeviceVector(other_ctx, 2 * nb)
    Co = npg.DeviceCSR.from_scipy(other_ctx, model.evolution.M.to_scipy_csr())
    assert lib.npg_tracers_transport_update(raw.h, xo.h, 1.0) == NPG_EINVAL and "different contexts" in err()
    assert lib.npg_tracers_transport_matrix(raw.h, Co.h) == NPG_EINVAL and "different contexts" in err()
    assert lib.npg_tracers_transport_load(raw.h, khat, None, raw.rd.h, None, oo.h) == NPG_EINVAL and "different contexts" in err()
    assert untouched()
    assert lib.npg_tracers_transport_load(raw.h, khat, None, raw.rd.h, None, out.h) == 0, err()
    assert not untouched()
    # the class
    with np.testing.assert_raises(NotImplementedError):
        npg.TracerTransport(model, [dict(name="a")], flow=xd, isoneutral=npg.Isoneutral(1.0, 1.0, 0.1))
    fake = SimpleNamespace(**{k: getattr(model, k) for k in ("arch", "fe_data", "params", "forcings", "evolution", "inversion")}, comm=object())
    with np.testing.assert_raises(NotImplementedError):
        npg.TracerTransport(fake, [dict(name="a")], flow=xd)
    bare = SimpleNamespace(**{k: getattr(model, k) for k in ("arch", "fe_data", "params", "forcings", "inversion")}, evolution=None)
    with np.testing.assert_raises(ValueError):
        npg.TracerTransport(bare, [dict(name="a")], flow=xd)
    with np.testing.assert_raises(ValueError):
        npg.TracerTransport(model, [dict(name="a")], flow=xd, scale=1e-6, decay=[-1.0])
    with np.testing.assert_raises(ValueError):
        npg.TracerTransport(model, [dict(name="a")], flow=xd, scale=1e-6, decay=[0.0, 1.0])
    with np.testing.assert_raises(ValueError) as e:                          # a random O(1) flow is far too strong for kappa^ on this mesh
        npg.TracerTransport(model, [dict(name="a")], flow=xd, scale=1.0)
    assert "Peclet" in str(e.exception) and "non-positive diagonal" in str(e.exception)
    if not np.any(fed.tables.b_pos < 0):                                     # no Dirichlet nodes and no decay: singular
        tt = npg.TracerTransport(model, [dict(name="a", source=1.0)], flow=xd, scale=1e-6)
        with np.testing.assert_raises(ValueError) as e:
            tt.equilibrium()
        assert "singular" in str(e.exception)
        with np.testing.assert_raises(ValueError):
            tt.step(0.1, scheme="BDF3")
    if flat_model is not None:                                               # an embedded 2-D engine
        with np.testing.assert_raises(L.DeviceError) as e:
            npg.TracerTransport(flat_model, [dict(name="a")])
        assert "embedded 2-D" in str(e.exception)
