"""A numpy restatement of the isoneutral mixing of the passive tracers (nupgcm_amd.tracers.Isoneutral, csrc/redi_core.h)
and the checks shared by tests/test_redi.py (CPU()) and tests/test_gpu_redi.py (GPU()).

The restatement is written from the definition, in the manner of tracers_ref.restate and not from the code under test: geometry from
the cells' own vertex coordinates (integrals_ref.geometry), native P2 / P1 tables, nodal buoyancy through Spaces' native tables.  With
B = N2 z + b' at a quadrature point

    Bz+ = max(d_z B, bz_min),  S = -grad_h B / Bz+,  S <- S min(1, slope_max / |S|),  kxz = k S_x,  kyz = k S_y,  kzz = k |S|^2

    K_ij = sum_{cells, q} W [ k g_ix g_jx + k g_iy g_jy + kxz g_ix g_jz + kxz g_iz g_jx + kyz g_iy g_jz + kyz g_iz g_jy + kzz g_iz g_jz ]

with W = w_q |J|: seven terms per (cell, q).  Sums are accumulated in extended precision (numpy.longdouble).

Bounds.  A sum of n terms evaluated in any order differs from the exact sum by at most n eps sum |t| (Higham, eq. 4.4, with the
rounding of the terms themselves: every count below carries + 8).  A matrix entry: n = 7 nq (cells that carry the pair), S_abs = the
sum of the seven terms' magnitudes.  A tensor table entry is a quotient of two such sums; its bound follows by propagating the two
sums' bounds through the quotient and the clip (tensor_bound).  Two evaluations of the same quantity (device and host library) differ
by at most twice the bound.  Nothing here is tuned to what the code gives."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

import nupgcm_amd as npg
from nupgcm_amd import _lib as L
from nupgcm_amd import fe as F
from nupgcm_amd.evolution import evolution_parameter
from nupgcm_amd.inversion import device_fe
from tests import helpers
from tests import integrals_ref as ir
from tests import interior_ref as itr
from tests import tracers_ref as tr

EPS = np.finfo(np.float64).eps
LD = np.longdouble
NPG_EINVAL = -1
SEED = 20261020
NEAR = 1e-9
NEW = {"npg_tracers_set_isoneutral", "npg_tracers_isoneutral_update", "npg_tracers_isoneutral_matrix", "npg_tracers_isoneutral_info",
       "npg_tracers_isoneutral_tables"}

_GEOM = {}


def geom(fed):
    """the restatement's tables of a mesh, built once: cells_b (nc, nl) node numbers, Nb (nq, nl), gphi (nc, nq, nl, 3), W (nc, nq),
    xq (nc, nq, 3)"""
    if id(fed) not in _GEOM:
        m, s = fed.mesh, fed.spaces
        X, G, wdet, lam, w, ea, eb = ir.geometry(m)
        N, dN = F.p2_tables(lam, ea, eb)
        if s.b_order == 2:
            cells_b, Nb, dNb = m.cell_nodes, N, dN
        else:
            cells_b, Nb, dNb = m.cells, lam, np.broadcast_to(np.eye(lam.shape[1]), (len(w),) + (lam.shape[1],) * 2)
        _GEOM[id(fed)] = (fed, SimpleNamespace(cells_b=cells_b, Nb=Nb, gphi=np.einsum("qik,ckj->cqij", dNb, G), W=w[None, :] * wdet[:, None],
                                               xq=np.einsum("qk,cki->cqi", lam, X), nq=len(w), nl=cells_b.shape[1], nc=m.ncell))
    return _GEOM[id(fed)][1]


def report(label, err, bound):
    err, bound = np.asarray(err, dtype=float).ravel(), np.asarray(bound, dtype=float).ravel()
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    print(f"redi {label}: max |err| {err.max(initial=0.0):.3e}, worst |err| / bound {ratio.max(initial=0.0):.3e} over {err.size} entries")
    return float(ratio.max(initial=0.0))


# ---- states ----------------------------------------------------------------------------------------------------------------------------
def smooth_b(model, amp, seed=SEED):
    """a random smooth b' in device order: D(x) + z (s0 + amp p(x)), p a sum of six random Fourier modes of unit amplitude; D = the
    model's own Dirichlet field (bowl_diri: y) and s0 = 2 where N2 = 0, so that d_z B stays near 2 for small amp"""
    rng = np.random.default_rng(seed)
    kk, ph, am = rng.uniform(-4.0, 4.0, (6, 3)), rng.uniform(0, 2 * np.pi, 6), rng.uniform(0.3, 1.0, 6)
    fed = model.fe_data
    dv = fed.spaces.b_diri_val
    has_d = bool(np.any(np.asarray(dv) != 0.0))
    s0 = 2.0 if float(model.params.N2) == 0.0 else 0.0

    def fn(x):
        p = sum(a * np.sin(x @ k + f) for a, k, f in zip(am, kk, ph)) / 6.0
        return (x[..., 1] if has_d else 0.0) + x[..., 2] * (s0 + amp * p)
    return np.ascontiguousarray(fed.spaces.interpolate_b(fn)[fed.dofs.p_b])


def nodal_b(fed, b_dev):
    return tr.nodal(fed, b_dev, fed.spaces.b_diri_val)


# ---- the tensor --------------------------------------------------------------------------------------------------------------------------
def restate_tensor(fed, bn, N2, kiso, slope_max, bz_min):
    """-> SimpleNamespace(kxz, kyz, kzz (nc, nq), floored, clipped, near (bool), bxz, byz, bzz: the bounds)"""
    g = geom(fed)
    bc = bn[g.cells_b]
    gB = np.einsum("cqij,ci->cqj", g.gphi, bc)
    gabs = np.einsum("cqij,ci->cqj", np.abs(g.gphi), np.abs(bc))
    n = 4 * g.nl + 8
    Bz = N2 + gB[..., 2]
    dBz = n * EPS * (abs(N2) + gabs[..., 2])
    floored = Bz < bz_min
    Bzp = np.where(floored, bz_min, Bz)
    dBzp = np.where(floored, 0.0, dBz)
    sx, sy = -gB[..., 0] / Bzp, -gB[..., 1] / Bzp
    dsx = n * EPS * gabs[..., 0] / Bzp + np.abs(sx) * dBzp / Bzp + 4 * EPS * np.abs(sx)
    dsy = n * EPS * gabs[..., 1] / Bzp + np.abs(sy) * dBzp / Bzp + 4 * EPS * np.abs(sy)
    smag = np.hypot(sx, sy)
    clipped = smag > slope_max
    near = (np.abs(Bz - bz_min) <= NEAR * bz_min) | (np.abs(smag - slope_max) <= NEAR * max(slope_max, 1e-300))
    f = np.where(clipped, slope_max / np.where(clipped, smag, 1.0), 1.0)
    cx, cy = sx * f, sy * f
    # unclipped: d(k s) = k ds.  clipped: s slope_max / |s|, |d (s / |s|)| <= 2 |ds| / |s|
    sm = slope_max if np.isfinite(slope_max) else 0.0                       # (nothing is clipped by an infinite slope_max)
    dcx = np.where(clipped, 2 * sm * (dsx + dsy) / np.where(clipped, smag, 1.0), dsx) + 8 * EPS * np.abs(cx)
    dcy = np.where(clipped, 2 * sm * (dsx + dsy) / np.where(clipped, smag, 1.0), dsy) + 8 * EPS * np.abs(cy)
    c2 = cx * cx + cy * cy
    dc2 = 2 * np.abs(cx) * dcx + 2 * np.abs(cy) * dcy + 8 * EPS * c2
    return SimpleNamespace(kxz=kiso * cx, kyz=kiso * cy, kzz=kiso * c2, floored=floored, clipped=clipped, near=near, bxz=kiso * dcx + 2 * EPS * np.abs(kiso * cx),
                           byz=kiso * dcy + 2 * EPS * np.abs(kiso * cy), bzz=kiso * dc2 + 2 * EPS * kiso * c2, Bz=Bz, smag=smag)


def between(values, share):
    """a threshold between two neighbouring values of the sorted sample, about `share` of them below it: no value lies near it"""
    v = np.unique(np.asarray(values).ravel())
    k = int(np.clip(round(share * len(v)), 1, len(v) - 1))
    while k < len(v) - 1 and v[k] - v[k - 1] <= 1e-6 * abs(v[k]):
        k += 1
    return 0.5 * (v[k - 1] + v[k])


def thresholds(model, b_dev, kind):
    """(slope_max, bz_min) for the state: "free" = nothing floored or clipped; "both" = about 30 % floored and, of the resulting
    slopes, about half clipped; "all" = every point floored and every non-zero slope clipped (the single tetrahedron, whose P1
    gradient is one value)"""
    fed, N2 = model.fe_data, float(model.params.N2)
    r = restate_tensor(fed, nodal_b(fed, b_dev), N2, 1.0, np.inf, 1e-300)
    if kind == "free":
        assert r.Bz.min() > 0
        return 4.0 * float(r.smag.max()) + 1.0, 0.25 * float(r.Bz.min())
    if kind == "all":
        bz_min = 2.0 * float(r.Bz.max())
        assert bz_min > 0
        r2 = restate_tensor(fed, nodal_b(fed, b_dev), N2, 1.0, np.inf, bz_min)
        assert r2.smag.min() > 0
        return 0.5 * float(r2.smag.min()), bz_min
    bz_min = between(r.Bz, 0.3)
    assert bz_min > 0
    r2 = restate_tensor(fed, nodal_b(fed, b_dev), N2, 1.0, np.inf, bz_min)
    return between(r2.smag, 0.5), bz_min


def kappa_iso_fn(x):
    return 0.7 + 0.3 * np.cos(2.0 * x[..., 0]) * np.exp(x[..., 2])


def make(model, kappa, slope_max, bz_min, specs=None, b_dev=None, **kw):
    """PassiveTracers with isoneutral mixing on the model; b_dev (device order) is uploaded to the model's b_vec first"""
    if b_dev is not None:
        model.b_vec.upload(b_dev)
    return npg.PassiveTracers(model, specs or [dict(name="dye")], isoneutral=npg.Isoneutral(kappa, slope_max, bz_min), **kw)


def kiso_table(fed, kappa):
    g = geom(fed)
    return np.ascontiguousarray(ir.coefficient(fed.mesh, kappa if callable(kappa) else (lambda x, c=float(kappa): np.full(x.shape[:-1], c)), g.xq))


# ---- check 1: tables and counts -----------------------------------------------------------------------------------------------------------
def check_tables(model, label, kind, amp=0.4, against=None):
    """the three tables and the two counts against the restatement; `against` = a callable (kiso, slope_max, bz_min, b_dev) -> (tables,
    info) of another library on the same input: compared with twice the bound"""
    fed, N2 = model.fe_data, float(model.params.N2)
    b = smooth_b(model, amp)
    slope_max, bz_min = thresholds(model, b, kind)
    t = make(model, kappa_iso_fn, slope_max, bz_min, b_dev=b)
    assert t.isoneutral_info()["state"] == L.NPG_REDI_SET
    t.update_isoneutral()
    info = t.isoneutral_info()
    r = restate_tensor(fed, nodal_b(fed, b), N2, kiso_table(fed, kappa_iso_fn), slope_max, bz_min)
    npts = r.near.size
    print(f"redi {label} [{kind}]: slope_max {slope_max:.6g}, bz_min {bz_min:.6g}; restated floored {r.floored.mean():.3f}, clipped {r.clipped.mean():.3f}, "
          f"near a threshold {int(r.near.sum())} of {npts}; library floored {info['floored']}, clipped {info['clipped']}")
    assert r.near.sum() == 0 and r.near.sum() <= 1e-3 * npts                # the state and the thresholds leave nothing out
    if kind == "free":
        assert not r.floored.any() and not r.clipped.any()
    elif kind == "all":
        assert r.floored.all() and r.clipped.all()
    else:
        assert 0.05 <= r.floored.mean() <= 0.95 and 0.05 <= r.clipped.mean() <= 0.95
    assert info == dict(floored=int(r.floored.sum()), clipped=int(r.clipped.sum()), points=npts, state=L.NPG_REDI_UPDATED)
    assert t.clip_counts == (r.floored.sum() / npts, r.clipped.sum() / npts)
    got = t.isoneutral_tables()
    out = {}
    for name, gv, rv, bv in zip(("kxz", "kyz", "kzz"), got, (r.kxz, r.kyz, r.kzz), (r.bxz, r.byz, r.bzz)):
        out[name] = report(f"{label} [{kind}] table {name}", np.abs(gv - rv), bv)
        assert (np.abs(gv - rv) <= bv).all(), (label, kind, name)
    assert np.abs(r.kxz).max() > 1e6 * r.bxz.max()                         # (the tables are not noise)
    if against is not None:
        other, oinfo = against(kiso_table(fed, kappa_iso_fn), slope_max, bz_min, b)
        assert oinfo == info
        for name, gv, ov, bv in zip(("kxz", "kyz", "kzz"), got, other, (r.bxz, r.byz, r.bzz)):
            out["host " + name] = report(f"{label} [{kind}] device vs host library, table {name} ({int(np.count_nonzero(gv != ov))} entries differ)",
                                         np.abs(gv - ov), 2 * bv)
            assert (np.abs(gv - ov) <= 2 * bv).all()
    return t, r, b, out


# ---- the matrix ---------------------------------------------------------------------------------------------------------------------------
def restate_matrix(fed, kiso, kxz, kyz, kzz):
    """K over ALL buoyancy nodes (Dirichlet ones included) as scipy CSR matrices: val, sabs and n (terms) on one pattern"""
    g = geom(fed)
    gp, W = g.gphi, g.W
    gx, gy, gz = gp[..., 0], gp[..., 1], gp[..., 2]
    val = np.zeros((g.nc, g.nl, g.nl), dtype=LD)
    sab = np.zeros((g.nc, g.nl, g.nl), dtype=LD)
    pairs = [(W * kiso, gx, gx), (W * kiso, gy, gy), (W * kxz, gx, gz), (W * kxz, gz, gx), (W * kyz, gy, gz), (W * kyz, gz, gy), (W * kzz, gz, gz)]
    for q in range(g.nq):                                                   # (q by q: the (nc, nl, nl) blocks stay small)
        for wk, a, b in pairs:
            t = wk[:, q, None, None] * a[:, q, :, None] * b[:, q, None, :]
            val += t
            sab += np.abs(t)
    nn = fed.spaces.nb_nodes
    key = (g.cells_b[:, :, None].astype(np.int64) * nn + g.cells_b[:, None, :]).ravel()
    uk, inv = np.unique(key, return_inverse=True)
    V, S, Nn = np.zeros(len(uk), dtype=LD), np.zeros(len(uk), dtype=LD), np.zeros(len(uk))
    np.add.at(V, inv, val.ravel())
    np.add.at(S, inv, sab.ravel())
    np.add.at(Nn, inv, 7 * g.nq)
    ri, ci = uk // nn, uk % nn
    mk = lambda d: sp.csr_matrix((np.asarray(d, dtype=float), (ri, ci)), shape=(nn, nn))
    return SimpleNamespace(K=mk(V), S=mk(S), bound=mk((Nn + 8) * EPS * np.asarray(S, dtype=float)), n=mk(Nn), ri=ri, ci=ci)


def free_block(fed, M):
    """(block of the free rows and columns in device order, block free rows x Dirichlet nodes) of a node-level matrix"""
    pos = fed.tables.b_pos
    free, diri = np.nonzero(pos >= 0)[0], np.nonzero(pos < 0)[0]
    order = free[np.argsort(pos[free])]
    M = M.tocsr()
    return M[order][:, order].tocsr(), M[order][:, diri].tocsr()


def entries(A, pattern):
    """the values of A at the entries of `pattern` (a CSR matrix with sorted indices), as an array aligned with pattern.data"""
    P = pattern.tocoo()
    return np.asarray(A.tocsr()[P.row, P.col]).ravel(), P


def check_matrix(model, label, t, r, against=None):
    """check 2 on the tracer set `t` whose tables were just updated (restated tensor r)"""
    fed = model.fe_data
    ref = restate_matrix(fed, kiso_table(fed, kappa_iso_fn), r.kxz, r.kyz, r.kzz)
    Kff, Kfd = free_block(fed, ref.K)
    Bff, Bfd = free_block(fed, ref.bound)
    # the tables the library assembled from differ from the restated ones within their own bounds: that share of the entry's bound
    dref = restate_matrix(fed, 0.0 * r.kxz, r.bxz, r.byz, r.bzz)
    Dff, _ = free_block(fed, dref.S)
    A = t.Kiso.to_scipy_csr()
    A.sort_indices()
    Bff = (Bff + Dff).tocsr()
    got, P = entries(A, Bff)
    want, _ = entries(Kff, Bff)
    out = dict(entries=report(f"{label}: K_iso entry by entry", np.abs(got - want), P.data))
    assert (np.abs(got - want) <= P.data).all() and A.nnz >= Bff.nnz
    mask = sp.csr_matrix((np.ones(len(P.data)), (P.row, P.col)), shape=A.shape)
    assert (A - A.multiply(mask)).count_nonzero() == 0                      # nothing outside the restated entries
    gotT, _ = entries(A.T, Bff)
    bT, _ = entries(Bff.T, Bff)
    out["symmetry"] = report(f"{label}: |A_ij - A_ji|", np.abs(got - gotT), P.data + bT)
    assert (np.abs(got - gotT) <= P.data + bT).all()
    rng = np.random.default_rng(SEED + 1)
    absA, worst = abs(A), 0.0
    for _ in range(20):
        x = rng.standard_normal(A.shape[0])
        q = float(x @ (A @ x))
        bound = float(np.abs(x) @ (Bff @ np.abs(x))) + (A.nnz + 8) * EPS * float(np.abs(x) @ (absA @ np.abs(x)))
        worst = min(worst, q / bound)
        assert q >= -bound
    print(f"redi {label}: x' K_iso x >= -bound for 20 random x (smallest x' K x / bound {worst:.3e}; clipped share {r.clipped.mean():.3f})")
    rs = np.asarray(A.sum(axis=1)).ravel() + np.asarray(Kfd.sum(axis=1)).ravel()
    rb = np.asarray(Bff.sum(axis=1)).ravel() + np.asarray(Bfd.sum(axis=1)).ravel() \
        + (np.diff(A.indptr) + 8) * EPS * (np.asarray(absA.sum(axis=1)).ravel() + np.asarray(abs(Kfd).sum(axis=1)).ravel())
    out["rowsum"] = report(f"{label}: row sums over free and Dirichlet columns", np.abs(rs), rb)
    assert (np.abs(rs) <= rb).all()
    v1 = A.data.copy()
    t.update_isoneutral()
    A2 = t.Kiso.to_scipy_csr()
    A2.sort_indices()
    assert np.array_equal(v1, A2.data)                                      # the same bits on every call
    if against is not None:
        H = against()
        goth, _ = entries(H, Bff)
        out["host"] = report(f"{label}: device vs host library, K_iso ({int(np.count_nonzero(got != goth))} entries differ)", np.abs(got - goth), 2 * P.data)
        assert (np.abs(got - goth) <= 2 * P.data).all()
    return ref, out


# ---- check 3: buoyancy is not mixed ---------------------------------------------------------------------------------------------------------
def full_B(model, b_dev):
    fed = model.fe_data
    z = fed.mesh.node_coords[:fed.spaces.nb_nodes, 2]
    return float(model.params.N2) * z + nodal_b(fed, b_dev)


def kb_terms(fed, A, Kfd, Bn):
    """K B over the free rows from the library's free block and the restated Dirichlet columns: (value, sum_j |K_ij B_j|, n_i)"""
    pos = fed.tables.b_pos
    free, diri = np.nonzero(pos >= 0)[0], np.nonzero(pos < 0)[0]
    order = free[np.argsort(pos[free])]
    Bf, Bd = Bn[order], Bn[diri]
    val = A @ Bf + Kfd @ Bd
    sabs = abs(A) @ np.abs(Bf) + abs(Kfd) @ np.abs(Bd)
    return val, sabs


def check_not_mixed(model, label, amp=0.4, against_clip=True):
    """|K_iso B|_i <= n eps sum_j |K_ij B_j| on an unclipped state (n = the row's quadrature terms: 7 nq per pair of the row); with
    clipping active the same quantity exceeds 1e3 times the bound"""
    fed = model.fe_data
    b = smooth_b(model, amp)
    out = {}
    for kind in ("free", "both") if against_clip else ("free",):
        slope_max, bz_min = thresholds(model, b, kind)
        t = make(model, kappa_iso_fn, slope_max, bz_min, b_dev=b)
        t.update_isoneutral()
        r = restate_tensor(fed, nodal_b(fed, b), float(model.params.N2), kiso_table(fed, kappa_iso_fn), slope_max, bz_min)
        ref = restate_matrix(fed, kiso_table(fed, kappa_iso_fn), r.kxz, r.kyz, r.kzz)
        _, Kfd = free_block(fed, ref.K)
        nff, nfd = free_block(fed, ref.n)
        A = t.Kiso.to_scipy_csr()
        val, sabs = kb_terms(fed, A, Kfd, full_B(model, b))
        n = np.asarray(nff.sum(axis=1)).ravel() + np.asarray(nfd.sum(axis=1)).ravel()
        bound = n * EPS * sabs
        ratio = report(f"{label} [{kind}]: |K_iso B| against n eps sum_j |K_ij B_j|", np.abs(val), bound)
        out[kind] = ratio
        if kind == "free":
            assert (np.abs(val) <= bound).all()
        else:
            assert np.abs(val).max() > 1e3 * bound.max()                    # a tensor that is simply zero cannot pass
    return out


def flow_vectors(model, zero=False, seed=SEED + 2):
    """two [u; p] vectors on the model's context (random unless zero)"""
    fed = model.fe_data
    n = fed.dofs.nu + fed.dofs.np
    rng = np.random.default_rng(seed)
    a, b = (np.zeros(n), np.zeros(n)) if zero else (rng.standard_normal(n), rng.standard_normal(n))
    return a, b, npg.DeviceVector.from_host(model.arch.ctx, a), npg.DeviceVector.from_host(model.arch.ctx, b)


def check_not_mixed_rhs(model, label, amp=0.4):
    """bowl_diri through the right-hand side: a tracer with Gamma = N2 whose values, Dirichlet ones included, are b'.  At rest (u = 0,
    BDF1, theta = 1)   y = M c - L,   L = the lift (K_iso + Kv) (c_D + Gamma z),   so
        Q = K_iso,ff c + (M c - y) - rhs_v + Gamma rhs_diff1 = K_iso B over the free rows
    (rhs_v, rhs_diff1: the engine's own kappa_v lift and background term, which the rotated tensor carries beside K_iso)."""
    fed, ev = model.fe_data, model.evolution
    assert (fed.tables.b_pos < 0).any() and np.abs(fed.spaces.b_diri_val).max() > 0.1
    N2 = float(model.params.N2)
    b = smooth_b(model, amp)
    dn = tr.diri_nodes(fed)
    dvals = np.asarray(fed.spaces.b_diri_val)[dn]
    spec = [dict(name="b", initial=None, dirichlet=(lambda x, v=dvals: v), gamma=N2)]
    out = {}
    for kind in ("free", "both"):
        slope_max, bz_min = thresholds(model, b, kind)
        t = make(model, kappa_iso_fn, slope_max, bz_min, specs=spec, b_dev=b)
        t.c.upload(b), t.c_prev.upload(b)
        t.update_isoneutral()
        _, _, x0, x1 = flow_vectors(model, zero=True)
        y = t.rhs(L.NPG_BDF1, 0.1, 1.0, x0, x1).to_host()
        A, M = t.Kiso.to_scipy_csr(), ev.M.to_scipy_csr()
        rd1 = ev.fe.rhs_diff(1.0, npg.DeviceVector(model.arch.ctx, len(b))).to_host()
        rv = ev.rhs_v.to_host()
        Q = A @ b + (M @ b - y) - rv + N2 * rd1
        r = restate_tensor(fed, nodal_b(fed, b), N2, kiso_table(fed, kappa_iso_fn), slope_max, bz_min)
        ref = restate_matrix(fed, kiso_table(fed, kappa_iso_fn), r.kxz, r.kyz, r.kzz)
        _, Kfd = free_block(fed, ref.K)
        nff, nfd = free_block(fed, ref.n)
        _, sabs = kb_terms(fed, A, Kfd, full_B(model, b))
        sabs = sabs + 2 * (abs(M) @ np.abs(b)) + 2 * np.abs(ev.rhs_M.to_host()) + 2 * np.abs(rv) + 2 * abs(N2) * np.abs(rd1)
        n = 2 * (np.asarray(nff.sum(axis=1)).ravel() + np.asarray(nfd.sum(axis=1)).ravel())
        bound = n * EPS * sabs
        out[kind] = report(f"{label} [{kind}]: lift + K_iso c on the free block", np.abs(Q), bound)
        if kind == "free":
            assert (np.abs(Q) <= bound).all()
        else:
            assert np.abs(Q).max() > 1e3 * bound.max()
    return out


# ---- check 4: the level twin -------------------------------------------------------------------------------------------------------------
def check_level_matrix(model, label):
    """slope_max = 0 and kappa_iso = the model's kappa_h: K_iso = the engine's NPG_MAT_KH matrix within the entries' bound"""
    fed, ev = model.fe_data, model.evolution
    b = smooth_b(model, 0.4)
    t = make(model, model.forcings.kappa_h, 0.0, 1e-3, b_dev=b)
    t.update_isoneutral()
    info = t.isoneutral_info()
    kh = kiso_table(fed, model.forcings.kappa_h)
    z = np.zeros_like(kh)
    ref = restate_matrix(fed, kh, z, z, z)
    Bff, _ = free_block(fed, ref.bound)
    A, Kh = t.Kiso.to_scipy_csr(), ev.Kh.to_scipy_csr()
    got, P = entries(A, Bff)
    want, _ = entries(Kh, Bff)
    ratio = report(f"{label}: K_iso(slope_max = 0, kappa_h) against NPG_MAT_KH", np.abs(got - want), 2 * P.data)
    A.sort_indices(), Kh.sort_indices()
    print(f"redi {label}: bit for bit: {np.array_equal(A.data, Kh.data) and np.array_equal(A.indices, Kh.indices)}; clipped {info['clipped']} of {info['points']}")
    assert (np.abs(got - want) <= 2 * P.data).all() and np.abs(want).max() > 0
    return ratio


def pnorm(P, v):
    return float(np.sqrt(np.sum(P * v * v)))


def _resid(stats, A, P, y, x):
    return pnorm(P, y - A @ x) if stats.get("direct") else float(stats["rnorm"])


def check_level_twin(arch, conv=(0.5, 0.1)):
    """three steps of bowl_mixing with the convection closure on: isoneutral tracers with slope_max = 0 and kappa_iso = kappa_h against
    the plain PassiveTracers of a second, identical model.  With d = c_iso - c_plain and A_c the isoneutral matrix,
        A_c d = (y_iso - y_plain) - r_iso + r_plain - (A_c - A) c_plain
    so ||A_c d||_P <= r_iso + r_plain + ||bound on y_iso - y_plain||_P + ||theta (bound on K_iso - Kh) |c_plain| ||_P: the bound of
    tracers_ref.check_twin (the two CG residuals and the right-hand sides' summation bounds, each from its own state) and the level
    matrix's entry bounds."""
    specs = [dict(name="dye", initial=lambda x: np.exp(-6.0 * (x[..., 0] ** 2 + x[..., 1] ** 2)) * (1.0 + x[..., 2]), dirichlet=0.3, gamma=0.8, source=0.2)]
    a, b = tr.conv_model(arch, "bowl_mixing", conv), tr.conv_model(arch, "bowl_mixing", conv)
    ta = a.tracers = npg.PassiveTracers(a, specs)
    tb = b.tracers = npg.PassiveTracers(b, specs, isoneutral=npg.Isoneutral(b.forcings.kappa_h, 0.0, 1e-3))
    fed, prm, ts = b.fe_data, b.params, b.timestepper
    theta = evolution_parameter(prm, ts)
    kh = kiso_table(fed, b.forcings.kappa_h)
    z = np.zeros_like(kh)
    Bff, _ = free_block(fed, restate_matrix(fed, kh, z, z, z).bound)
    out = []
    for step in range(3):
        st = {}
        for m, t in ((a, ta), (b, tb)):
            pv = m._prev
            x0 = m.inversion.solver.x.to_host()
            st[id(m)] = (x0, x0 if pv is None else pv["x_prev"].to_host(), t.c.to_host(), t.c_prev.to_host(), m.b_vec.to_host())
            npg.run(m, n_steps=1)
        assert np.array_equal(a.b_vec.to_host(), b.b_vec.to_host())        # the two models are the same model
        Ac, A = tb.A.to_scipy_csr(), a.evolution.solver.A.to_scipy_csr()
        P = 1.0 / Ac.diagonal()
        ca, cb = ta.c.to_host(), tb.c.to_host()
        ra = _resid(ta.stats[-1][0], A, 1.0 / A.diagonal(), ta.y.to_host(), ca)
        rb = _resid(tb.stats[-1][0], Ac, P, tb.y.to_host(), cb)
        assert not tb.stats[-1][0].get("direct")                           # isoneutral tracers always take Jacobi-CG
        rr = []
        for m in (a, b):
            x0, xp0, c0, cp0, b0 = st[id(m)]
            kv = tr._kv_now(m, m.b_vec.to_host())                           # kappa_v as evolve() left it: from the b' just solved
            rr.append(tr.restate_set(m, specs, L.NPG_BDF2, ts.dt, theta, x0, xp0, c0, cp0, kv=kv)[0])
        ybound = pnorm(P, rr[0].bound + rr[1].bound + np.abs(rr[0].total - rr[1].total))
        mbound = pnorm(P, theta * 2 * (Bff @ np.abs(ca)))
        lhs = pnorm(P, Ac @ (cb - ca))
        print(f"redi level twin step {step + 1}: ||A_c (c_iso - c_plain)||_P = {lhs:.3e}; r_iso {rb:.3e} + r_plain {ra:.3e} + y bound {ybound:.3e} + "
              f"matrix bound {mbound:.3e} = {ra + rb + ybound + mbound:.3e}; max |c_iso - c_plain| {np.abs(cb - ca).max():.3e} of {np.abs(ca).max():.3e}")
        assert lhs <= ra + rb + ybound + mbound
        out.append((lhs, ra + rb + ybound + mbound))
    return out


# ---- check 5: the right-hand side ----------------------------------------------------------------------------------------------------------
SPECS = [dict(name="age", dirichlet=lambda x: 0.3 + 0.5 * x[..., 0], gamma=0.0, source=1.0),
         dict(name="dye", dirichlet=-0.7, gamma=1.7, source=-0.4),
         dict(name="free", gamma=-0.6)]


def flux_lines(model, cd, gam, theta, kiso, kxz, kyz, kzzv):
    """- theta sum W ( K (grad c_D + Gamma z) ) . grad phi_i over the free rows, K = [kiso 0 kxz; 0 kiso kyz; kxz kyz kzzv], in the cells
    where the tracer has a non-zero Dirichlet value or Gamma != 0: seven terms per (cell, q, i) -> (total (longdouble), S_abs, n)"""
    fed = model.fe_data
    g = geom(fed)
    gd = np.einsum("cqij,ci->cqj", g.gphi, cd[g.cells_b])
    active = (np.any(cd[g.cells_b] != 0.0, axis=1) | (gam != 0.0))[:, None]
    gz = gd[..., 2] + gam
    fl = [[kiso * gd[..., 0], kxz * gz], [kiso * gd[..., 1], kyz * gz], [kxz * gd[..., 0], kyz * gd[..., 1], kzzv * gz]]
    rows = fed.tables.b_pos[g.cells_b]
    nb = fed.dofs.nb
    tot, sab, cnt = np.zeros(nb, dtype=LD), np.zeros(nb), np.zeros(nb)
    rr = np.broadcast_to(rows[:, None, :], (g.nc, g.nq, g.nl))
    keep = rr >= 0
    for a in range(3):
        for f in fl[a]:
            t = -theta * np.where(active, g.W * f, 0.0)[..., None] * g.gphi[..., a]           # (nc, nq, nl)
            np.add.at(tot, rr[keep], t[keep].astype(LD))
            sab += np.bincount(rr[keep], weights=np.abs(t[keep]), minlength=nb)
            cnt += np.bincount(rr[keep], minlength=nb)
    return tot, sab, cnt


def restate_rhs(model, sp, scheme, dt, theta, x, xp, c, cp, r, kiso, kv):
    """one tracer's right-hand side with the mode on: the lines of tracers_ref.restate that do not involve the diffusion (kappa = 0),
    plus flux_lines with the rotated tensor and kzz + kappa_v.  The bound carries the share of the tables' own bounds (the library
    evaluates the lines from ITS tables, which differ from the restated ones within r.bxz, r.byz, r.bzz)."""
    fed = model.fe_data
    g = geom(fed)
    un, unp = tr.velocity_nodal(fed, x), tr.velocity_nodal(fed, xp)
    cd, _ = tr.spec_arrays(model, sp)
    gam = float(sp.get("gamma", 0.0))
    z = np.zeros((g.nc, g.nq))
    base = tr.restate(fed, scheme, dt, theta, un, unp, tr.nodal(fed, c, cd), tr.nodal(fed, cp, cd), cd, gam, float(sp.get("source", 0.0)), z, z)
    # (base's gamma_diff and lift_diff lines are exact zeros: kappa = 0; they only add to n)
    tot, sab, cnt = flux_lines(model, cd, gam, theta, kiso, r.kxz, r.kyz, r.kzz + kv)
    _, tsh, _ = flux_lines(model, cd, gam, theta, 0.0 * kiso, r.bxz, r.byz, r.bzz)
    total = np.asarray(base.total.astype(LD) + tot, dtype=float)
    sabs, n = base.sabs + sab, base.n + cnt
    return SimpleNamespace(total=total, sabs=sabs, n=n, bound=(n + 8) * EPS * sabs + tsh, lift=np.asarray(tot, dtype=float))


def check_rhs(model, label, amp=0.4, dt=0.013, theta=0.021, against=None):
    """Dirichlet values and Gamma != 0, both schemes, clipping active, against the restatement"""
    fed, N2 = model.fe_data, float(model.params.N2)
    nb = fed.dofs.nb
    b = smooth_b(model, amp)
    slope_max, bz_min = thresholds(model, b, "both")
    t = make(model, kappa_iso_fn, slope_max, bz_min, specs=SPECS, b_dev=b)
    t.update_isoneutral()
    r = restate_tensor(fed, nodal_b(fed, b), N2, kiso_table(fed, kappa_iso_fn), slope_max, bz_min)
    rng = np.random.default_rng(SEED + 3)
    c, cp = rng.standard_normal(t.c.n), rng.standard_normal(t.c.n)
    t.c.upload(c), t.c_prev.upload(cp)
    x, xp, xd, xpd = flow_vectors(model)
    kiso = kiso_table(fed, kappa_iso_fn)
    kv = kiso_table(fed, model.forcings.kappa_v)
    out = {}
    for scheme in (L.NPG_BDF1, L.NPG_BDF2):
        y = t.rhs(scheme, dt, theta, xd, xpd).to_host()
        assert np.isfinite(y).all() and np.array_equal(y, t.rhs(scheme, dt, theta, xd, xpd).to_host())
        yh = against(t, SPECS, scheme, dt, theta, x, xp, c, cp, kiso, slope_max, bz_min, b) if against is not None else None
        for k, sp_ in enumerate(SPECS):
            ref = restate_rhs(model, sp_, scheme, dt, theta, x, xp, c[k * nb:(k + 1) * nb], cp[k * nb:(k + 1) * nb], r, kiso, kv)
            bound = ref.bound
            err = np.abs(y[k * nb:(k + 1) * nb] - ref.total)
            out[(scheme, k)] = report(f"{label} rhs scheme {scheme} tracer {k} ({sp_['name']})", err, bound)
            assert (err <= bound).all(), (label, scheme, k)
            assert np.count_nonzero(ref.lift) > 0 or (sp_.get("dirichlet") is None and sp_.get("gamma", 0.0) == 0.0)
            if yh is not None:
                eh = np.abs(y[k * nb:(k + 1) * nb] - yh[k * nb:(k + 1) * nb])
                out[("host", scheme, k)] = report(f"{label} rhs device vs host library scheme {scheme} tracer {k} ({int(np.count_nonzero(eh))} rows differ)",
                                                  eh, 2 * bound)
                assert (eh <= 2 * bound).all()
    return out


def check_mode_off_bits(model, label):
    """with the mode off the right-hand side keeps its bits: a plain handle against a handle whose mode was switched on and off again"""
    b = smooth_b(model, 0.4)
    plain = npg.PassiveTracers(model, tr.SPECS3)
    other = npg.PassiveTracers(model, tr.SPECS3)
    kap = L.as_f64(np.ones((geom(model.fe_data).nq, model.fe_data.mesh.ncell)))
    L.check(L.lib().npg_tracers_set_isoneutral(other.h, L.ptr(kap), 1.0, 0.1))
    bv = npg.DeviceVector.from_host(model.arch.ctx, b)
    L.check(L.lib().npg_tracers_isoneutral_update(other.h, float(model.params.N2), bv.h))
    L.check(L.lib().npg_tracers_set_isoneutral(other.h, None, 0.0, 0.0))
    nf, ncl, npt, st = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
    L.check(L.lib().npg_tracers_isoneutral_info(other.h, C.byref(nf), C.byref(ncl), C.byref(npt), C.byref(st)))
    assert (nf.value, ncl.value, npt.value, st.value) == (0, 0, 0, L.NPG_REDI_OFF)
    rng = np.random.default_rng(SEED + 4)
    c, cp = rng.standard_normal(plain.c.n), rng.standard_normal(plain.c.n)
    for t in (plain, other):
        t.c.upload(c), t.c_prev.upload(cp)
    _, _, xd, xpd = flow_vectors(model)
    for scheme in (L.NPG_BDF1, L.NPG_BDF2):
        y1, y2 = plain.rhs(scheme, 0.013, 0.021, xd, xpd).to_host(), other.rhs(scheme, 0.013, 0.021, xd, xpd).to_host()
        assert np.array_equal(y1, y2) and np.abs(y1).max() > 0, (label, scheme)
    print(f"redi {label}: mode off - the two handles' right-hand sides are bit-identical")


# ---- check 6: in the loop -----------------------------------------------------------------------------------------------------------------
def loop_model(arch, scheme, nsteps=3):
    fed, prm, frc, dt, b0 = helpers.build_fe_data("bowl_surface_flux")
    ts = npg.BDF2(t_start=0.0, t_stop=nsteps * dt, dt=dt) if scheme == "BDF2" else npg.BDF1(t_start=0.0, t_stop=1e9, dt=dt, adaptive=True)
    model = npg.Model(arch, prm, frc, fed, npg.InversionToolkit(arch, fed, prm, frc), npg.EvolutionToolkit(arch, fed, prm, frc, ts), ts)
    npg.set_b(model, lambda x: x[..., 2] / 0.5 + 0.3 * np.sin(2.0 * x[..., 0]) * x[..., 2])
    return model


LOOP_SPECS = [dict(name="dye", initial=lambda x: np.exp(-8.0 * (x[..., 0] ** 2 + x[..., 1] ** 2)) * (1.0 + x[..., 2])),
              dict(name="blob", initial=lambda x: np.exp(-4.0 * ((x[..., 0] - 0.3) ** 2 + x[..., 1] ** 2)))]
LOOP_ISO = (0.05, 0.2, 0.5)                                                 # kappa, slope_max, bz_min (d_z B is near 2 there)


def check_loop(arch, scheme):
    """three steps on bowl_surface_flux (no Dirichlet nodes): the integral of a flux-free, source-free tracer is conserved to the bound
    of tracers_ref.check_conservation (row summation bounds, the CG residual through 1', the rounding of the assembled column sums);
    u, p, b' keep the bits of a model without tracers; batched = the per-tracer bits"""
    plain = loop_model(arch, scheme)
    model, twin = loop_model(arch, scheme), loop_model(arch, scheme)
    fed, ev, prm, ts = model.fe_data, model.evolution, model.params, model.timestepper
    assert (fed.tables.b_pos >= 0).all()
    nb = fed.dofs.nb
    iso = npg.Isoneutral(*LOOP_ISO)
    t = model.tracers = npg.PassiveTracers(model, LOOP_SPECS, isoneutral=iso)
    t2 = twin.tracers = npg.PassiveTracers(twin, LOOP_SPECS, isoneutral=iso, batched=True)
    none = np.zeros(fed.spaces.nb_nodes)
    out, dts = [], []
    for step in range(3):
        pv = model._prev
        x0 = model.inversion.solver.x.to_host()
        xp0 = x0 if pv is None else pv["x_prev"].to_host()
        c0, cp0 = t.c.to_host(), t.c_prev.to_host()
        for m in (plain, model, twin):
            npg.run(m, n_steps=1)
        dts.append(ts.dt)
        theta = evolution_parameter(prm, ts)
        sch = L.NPG_BDF1 if scheme == "BDF1" else L.NPG_BDF2
        ref = tr.restate_set(model, LOOP_SPECS, sch, ts.dt, theta, x0, xp0, c0, cp0)
        A = t.A.to_scipy_csr()
        absA = abs(ev.M.to_scipy_csr()) + theta * (abs(t.Kiso.to_scipy_csr()) + abs(ev.Kv.to_scipy_csr()))
        rowmax = int(np.diff(A.indptr).max())
        c1h, y1 = t.c.to_host(), t.y.to_host()
        fl, cl = t.clip_counts
        for k, r in enumerate(ref):
            ck, yk = c1h[k * nb:(k + 1) * nb], y1[k * nb:(k + 1) * nb]
            got, sabs_int = tr.integral(fed, tr.nodal(fed, ck, none))
            predicted = float(np.sum(r.total.astype(LD)))
            res = yk - A @ ck
            bound = float(r.bound.sum()) + np.sqrt(nb) * float(np.linalg.norm(res)) + 64 * rowmax * EPS * float(np.abs(ck) @ (absA @ np.ones(nb))) \
                + fed.mesh.ncell * len(fed.mesh.q_w) * EPS * sabs_int
            print(f"redi loop {scheme} step {step + 1} tracer {LOOP_SPECS[k]['name']}: int c = {got:.12e}, predicted {predicted:.12e}, |defect| "
                  f"{abs(got - predicted):.3e}, bound {bound:.3e}; dt {ts.dt:.4g}; floored {fl:.3f}, clipped {cl:.3f}; CG its {t.stats[-1][k]['niter']}")
            assert abs(got - predicted) <= bound
            assert not t.stats[-1][k].get("direct") and t.stats[-1][k]["solved"]
            out.append((abs(got - predicted), bound))
        assert np.array_equal(c1h, t2.c.to_host())                          # batched = per-tracer, bit for bit
    for name in ("u", "p", "b"):
        assert np.array_equal(getattr(plain.state, name), getattr(model.state, name)), name
    if scheme == "BDF1":
        print(f"redi loop adaptive BDF1: dt per step {dts}")
    assert 0.0 < t.clip_counts[1] < 1.0                                     # the slopes of this state are clipped somewhere, not everywhere
    return out


def check_forced_model_accepted(arch):
    """a model with a sponge and a restoring surface accepts isoneutral tracers; their A_c after a step is the A_c of the same model
    without those forcings, bit for bit (A_c holds neither evolution.S nor evolution.R); without isoneutral= both are still refused"""
    mesh = itr.bowl_mesh()
    mats = []
    for forced in (False, True):
        model = itr.light_model(arch, mesh)
        model.inversion.solver = SimpleNamespace(x=npg.DeviceVector(arch.ctx, model.fe_data.dofs.nu + model.fe_data.dofs.np))
        model.b_vec.upload(smooth_b(model, 0.4))
        if forced:
            sf = npg.SurfaceForcing(model, restoring=(0.5, lambda x: 0.1 * x[..., 0]))
            inf = npg.InteriorForcing(model, restoring=(lambda x: 1.0 + x[..., 2], 0.0))
            model.surface_forcing, model.interior_forcing = sf, inf
            assert getattr(sf, "restoring", False) and getattr(inf, "restoring", False)
            for kw in (dict(surface_forcing=None), dict(interior_forcing=None), {}):
                fake = SimpleNamespace(**dict(vars(model), **kw))
                with np.testing.assert_raises(NotImplementedError):
                    npg.PassiveTracers(fake, [dict(name="a")])
        t = npg.PassiveTracers(model, [dict(name="a", initial=lambda x: x[..., 0])], isoneutral=npg.Isoneutral(*LOOP_ISO))
        t.step(model, model.inversion.solver.x)
        A = t.A.to_scipy_csr()
        A.sort_indices()
        mats.append((A.data.copy(), t.P.diag.to_host()))
    assert np.array_equal(mats[0][0], mats[1][0]) and np.array_equal(mats[0][1], mats[1][1]) and np.abs(mats[0][0]).max() > 0
    print("redi: a model with a sponge and a restoring surface accepts isoneutral tracers; A_c and P_c bit-identical to the unforced model's")


# ---- check 7: refusals ------------------------------------------------------------------------------------------------------------------
def check_refusals(model, flat_model=None):
    """every validation sentence returns NPG_EINVAL with its message before anything is launched; the update-before-rhs rule"""
    lib = L.lib()
    ctx, fed = model.arch.ctx, model.fe_data
    nb = fed.dofs.nb
    g = geom(fed)
    t = npg.PassiveTracers(model, [dict(name="a", gamma=0.5)])
    good = np.ones((g.nq, g.nc))
    err = lambda: lib.npg_last_error().decode()

    def bad(table, sm, bz, word):
        rc = lib.npg_tracers_set_isoneutral(t.h, L.ptr(L.as_f64(table)), sm, bz)
        assert rc == NPG_EINVAL and word in err(), (word, rc, err())
        assert t.isoneutral_info()["state"] == L.NPG_REDI_OFF
    for v in (np.nan, np.inf, -1.0):
        tab = good.copy()
        tab[g.nq // 2, g.nc // 2] = v
        bad(tab, 1.0, 0.1, "kappa_iso")
    for sm in (-1e-3, np.nan, np.inf):
        bad(good, sm, 0.1, "slope_max")
    for bz in (0.0, -1.0, np.nan, np.inf):
        bad(good, 1.0, bz, "bz_min")
    V = lambda n: npg.DeviceVector(ctx, n)
    K = model.evolution.fe.new_matrix("b")
    # off: update and matrix are refused
    vb, vb1 = V(nb), V(nb + 1)                                                         # (held: a handle must outlive the call)
    assert lib.npg_tracers_isoneutral_update(t.h, 1.0, vb.h) == NPG_EINVAL and "off" in err()
    assert lib.npg_tracers_isoneutral_matrix(t.h, K.h) == NPG_EINVAL
    L.check(lib.npg_tracers_set_isoneutral(t.h, L.ptr(L.as_f64(good)), 1.0, 0.1))
    x = V(fed.dofs.nu + fed.dofs.np)
    y = V(nb)
    y.fill(-7.0)
    rhs = lambda: lib.npg_tracers_rhs(t.h, L.NPG_BDF1, 0.01, 0.02, t.c.h, t.c_prev.h, x.h, x.h, None, None, y.h)
    assert rhs() == NPG_EINVAL and "has not been updated" in err()                   # update before rhs
    assert lib.npg_tracers_isoneutral_matrix(t.h, K.h) == NPG_EINVAL and "has not been updated" in err()
    assert np.array_equal(y.to_host(), np.full(nb, -7.0))                             # nothing was launched
    assert lib.npg_tracers_isoneutral_update(t.h, 1.0, vb1.h) == NPG_EINVAL and "buoyancy vector" in err()
    assert lib.npg_tracers_isoneutral_update(t.h, np.nan, vb.h) == NPG_EINVAL and "N2" in err()
    assert t.isoneutral_info()["state"] == L.NPG_REDI_SET
    L.check(lib.npg_tracers_isoneutral_update(t.h, 1.0, vb.h))
    assert rhs() == 0, err()                                                           # (Gamma != 0 and no rhs_diff1: the mode carries it)
    wrong = npg.DeviceCSR.from_pattern(ctx, nb - 1, nb - 1, np.arange(nb), np.arange(nb - 1))
    assert lib.npg_tracers_isoneutral_matrix(t.h, wrong.h) == NPG_EINVAL and "buoyancy pattern" in err()
    diag = npg.DeviceCSR.from_pattern(ctx, nb, nb, np.arange(nb + 1), np.arange(nb))
    assert lib.npg_tracers_isoneutral_matrix(t.h, diag.h) == NPG_EINVAL and "buoyancy pattern" in err()
    L.check(lib.npg_tracers_isoneutral_matrix(t.h, K.h))
    L.check(lib.npg_tracers_set_isoneutral(t.h, L.ptr(L.as_f64(good)), 1.0, 0.1))     # set again: the tensor is stale again
    assert rhs() == NPG_EINVAL and "has not been updated" in err()
    with np.testing.assert_raises(TypeError):
        npg.PassiveTracers(model, [dict(name="a")], isoneutral=(1.0, 1.0, 1.0))
    with np.testing.assert_raises(TypeError):
        npg.Isoneutral(1.0)                                                            # no defaults for the thresholds
    with np.testing.assert_raises(L.DeviceError):
        npg.PassiveTracers(model, [dict(name="a")], isoneutral=npg.Isoneutral(-1.0, 1.0, 0.1))
    if flat_model is not None:                                                         # an embedded 2-D engine
        with np.testing.assert_raises(L.DeviceError) as e:
            npg.PassiveTracers(flat_model, [dict(name="a")], isoneutral=npg.Isoneutral(1.0, 1.0, 0.1))
        assert "embedded 2-D" in str(e.exception)


# ---- the host library beside the device library (GPU tests) -------------------------------------------------------------------------------
class HostLibrary:
    """libnupgcm_host.so loaded BESIDE the library the model runs on and driven through its C ABI alone, on the model's own tables
    (as tracers_ref.host_library_rhs)"""

    def __init__(self, model):
        from nupgcm_amd.assembly import eval_at_quad_points
        H = self.H = C.CDLL(L.HOST_LIB_PATH)
        L._declare(H, partial=True)
        fed, f = model.fe_data, model.forcings
        self.model, self.fed = model, fed
        m = fed.mesh
        k = self.k = device_fe(model.arch, fed)._keep
        d = L.FeDesc(ncell=m.ncell, nq=len(m.q_w), nloc_b=k["cb"].shape[1], grad_lambda=k["G"].ctypes.data, wdet=k["wdet"].ctypes.data,
                     qw=k["qw"].ctypes.data, N2=k["N2"].ctypes.data, dN2=k["dN2"].ctypes.data, Nb=k["Nb"].ctypes.data, dNb=k["dNb"].ctypes.data,
                     N1=k["N1"].ctypes.data, cell_u=k["cu"].ctypes.data, cell_p=k["cp"].ctypes.data, cell_b=k["cb"].ctypes.data,
                     u_diri=k["ud"].ctypes.data, n_u_diri=k["ud"].size, b_diri=k["bd"].ctypes.data, n_b_diri=k["bd"].size,
                     n_inv=fed.dofs.nu + fed.dofs.np, n_b=fed.dofs.nb)
        self.ctx, self.fe = C.c_void_p(), C.c_void_p()
        self.ok(H.npg_ctx_create(0, C.byref(self.ctx)))
        self.ok(H.npg_fe_create(self.ctx, C.byref(d), C.byref(self.fe)))
        for name, v in (("kappa_h", f.kappa_h), ("kappa_v", f.kappa_v)):
            self.ok(H.npg_fe_set_coeff(self.fe, name.encode(), L.ptr(L.as_f64(eval_at_quad_points(m, v)))))

    def ok(self, rc):
        assert rc == 0, self.H.npg_last_error().decode()

    def vec(self, a):
        v = C.c_void_p()
        self.ok(self.H.npg_vec_create(self.ctx, len(a), C.byref(v)))
        self.ok(self.H.npg_vec_upload(v, L.ptr(L.as_f64(a))))
        return v

    def tracers(self, specs, kiso, slope_max, bz_min, b_dev):
        """a host handle with the mode on and the tensor updated from b_dev"""
        H, fed = self.H, self.fed
        T = C.c_void_p()
        self.ok(H.npg_tracers_create(self.fe, len(specs), C.byref(T)))
        dn = tr.diri_nodes(fed)
        for j, sp_ in enumerate(specs):
            cd, _ = tr.spec_arrays(self.model, sp_)
            dv = np.zeros(self.k["bd"].size)
            dv[:len(dn)] = cd[dn]
            self.ok(H.npg_tracers_set(T, j, L.ptr(L.as_f64(dv)), float(sp_.get("gamma", 0.0)), float(sp_.get("source", 0.0))))
        self.ok(H.npg_tracers_set_isoneutral(T, L.ptr(L.as_f64(np.ascontiguousarray(kiso.T))), float(slope_max), float(bz_min)))
        self.ok(H.npg_tracers_isoneutral_update(T, float(self.model.params.N2), self.vec(b_dev)))
        return T

    def tables(self, kiso, slope_max, bz_min, b_dev):
        T = self.T = self.tracers([dict(name="a")], kiso, slope_max, bz_min, b_dev)
        g = geom(self.fed)
        out = [np.empty((g.nq, g.nc)) for _ in range(3)]
        self.ok(self.H.npg_tracers_isoneutral_tables(T, *(L.ptr(a) for a in out)))
        nf, ncl, npt, st = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
        self.ok(self.H.npg_tracers_isoneutral_info(T, C.byref(nf), C.byref(ncl), C.byref(npt), C.byref(st)))
        return tuple(np.ascontiguousarray(a.T) for a in out), dict(floored=nf.value, clipped=ncl.value, points=npt.value, state=st.value)

    def matrix(self):
        """K_iso of the handle self.tables left, as a scipy CSR matrix"""
        rp, ci, shape = self.fed.pattern_b()
        rp, ci = L.as_i64(rp), L.as_i32(ci)
        K = C.c_void_p()
        self.ok(self.H.npg_csr_create(self.ctx, shape[0], shape[1], L.ptr(rp), L.ptr(ci), None, C.byref(K)))
        self.ok(self.H.npg_tracers_isoneutral_matrix(self.T, K))
        v = np.empty(len(ci))
        rp2, ci2 = np.empty_like(rp), np.empty_like(ci)
        self.ok(self.H.npg_csr_download(K, L.ptr(rp2), L.ptr(ci2), L.ptr(v)))
        return sp.csr_matrix((v, ci2, rp2), shape=shape)

    def rhs(self, t, specs, scheme, dt, theta, x, xp, c, cp, kiso, slope_max, bz_min, b_dev):
        T = self.tracers(specs, kiso, slope_max, bz_min, b_dev)
        vy = self.vec(np.zeros(len(c)))
        self.ok(self.H.npg_tracers_rhs(T, scheme, dt, theta, self.vec(c), self.vec(cp), self.vec(x), self.vec(xp), None, None, vy))
        out = np.empty(len(c))
        self.ok(self.H.npg_vec_download(vy, L.ptr(out)))
        return out
