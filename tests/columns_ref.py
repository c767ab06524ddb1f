"""The checks shared by tests/test_columns.py (CPU()) and tests/test_gpu_columns.py (GPU()) for the column integrals (npg_columns_*,
DESIGN.md 32), and a numpy restatement that is independent of the library.

The restatement (`restate`) takes the handle's segments (cell, z_top, z_bot) and evaluates every integrand at the three Gauss points of
each segment on sampling_ref.Brute's geometry (the inverted edge matrices of the cells' own vertices, not the library's grad lambda)
from nodal values read off the device vectors, and sums term by term in np.longdouble.  Next to every term it accumulates the sum of
ABSOLUTE values the term is made of.  A field value f = sum_i N_i(lambda) v_i counts as A = sum_i |N_i| |v_i| + sum_k D_k Lambda_k: the
second part is what the rounding of the barycentrics does - lambda_k = sum_a G_ka d_a is itself a sum, of absolute values Lambda_k =
sum_a |G_ka| |d_a| (1 + their sum for lambda_0; large in a flat or thin cell), and f moves by at most D_k = sum_i |v_i| |dN_i/dl_k| per
unit of lambda_k.  A gradient counts as sum |v_i| |dN_i/dl_k| |G_k| plus, for P2, its own D_k Lambda_k from the second derivatives of the
shape functions; a product of fields as the product of their A; S_abs of a channel and a column is sum_segments sum_g W_g A(z_g) dz.  The
closed forms (`exact_integrals`) are antiderivatives in z of the polynomial state between z_bot and z_top in np.longdouble: they know
neither the segments nor the Gauss rule.

Bounds.  eps = 2^-52.  One field value at a point of a column costs at most 64 operations on terms whose absolute values sum to A (the
barycentrics 3 x 5, the ten P2 shape functions 30, the sum 10 + 9; a gradient costs less: p2_dlambda 36, the product with grad lambda 7,
the barycentrics 15): tests/surfaces_ref.py counts the same.  An integrand is a product of at most three factors (z, u, b'): 64 + 64 + 3
operations; the Gauss rule adds 6 and the fold of a column at most max_per_col: N_OPS = 137 + max_per_col.  The restatement evaluates
the same integrand in fp64 before it sums in longdouble, and its geometry is another rounding of the same cell, so the two differ by
at most twice that:
    |library - restatement| <= 2 N_OPS eps S_abs            (integrals, channels 0 .. 16)
    |library - restatement| <= 2 . 64 eps A                 (end values: one field value or gradient each)
The closed forms are compared with the same bound plus what the rounding of the polynomial's nodal values adds (`nodal_noise`, derived
there).  A slope - n_x / n_z of a face comes from the cross product n = a x b of two edge vectors; a component of n is two products
of differences of coordinates: 8 operations on S_n = (|v1| + |v0|)(|v2| + |v0|) terms; the library's - G_ix / G_iz comes from the
inverse T of the cell's edge matrix E, whose entries are off by at most dG_a = 3 . 8 eps kappa_inf(E) max_k |T_ka| (the normwise bound
of an inverse, Higham, Accuracy and Stability, section 14.1, with n = 3; 4 times that for lambda_0's row, the sum of three), so
    |slope - slope_ref| <= 16 eps (S_nx / |n_z| + |n_x| S_nz / n_z^2) + (dG_ix / |G_iz| + |G_ix| dG_iz / G_iz^2)
where the column leaves its cell through ONE face; where two constraints of the cell vanish within AMBIG at the end (a column through
a vertex or an edge) the brute force cannot say which face the library's tie-break names, and the slope is not judged.  Derived maps
(gamma, grad gamma, JEBAR, the torque, the stress residual) are sums and products of channels: the bound is the same algebra applied to
the channels' bounds (first-order propagation, written out where it is used)."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np

import nupgcm_amd as npg
from nupgcm_amd import _lib as L
from tests import integrals_ref as ir
from tests import particles_ref as pr
from tests import sampling_ref as sr
from tests import surfaces_ref as ur

EPS = np.finfo(np.float64).eps
NPG_EINVAL = -1
AMBIG = 1e-9
NI, NE = 17, 14
NEW = {"npg_columns_create", "npg_columns_destroy", "npg_columns_info", "npg_columns_columns", "npg_columns_segments",
       "npg_columns_compute"}
LD = np.longdouble
GS = np.array([0.5 * (1 - np.sqrt(0.6)), 0.5, 0.5 * (1 + np.sqrt(0.6))])
GW = np.array([5, 8, 5], dtype=LD) / LD(18)


def check_exports():
    assert NEW <= set(L.declared_symbols()) and L.NPG_NCOLI == NI and L.NPG_NCOLE == NE
    for path in (L.HOST_LIB_PATH, L.LIB_PATH):
        lib = C.CDLL(path)
        assert not [s for s in NEW if not hasattr(lib, s)], path
    assert npg.ColumnIntegrals is npg.columns.ColumnIntegrals and npg.ColumnMaps and npg.ColumnRecorder


def n_ops(CI):
    return 137 + CI.info["max_per_column"]


# ---- the state ------------------------------------------------------------------------------------------------------------------------------
class Quad:
    """c[0] + c[1] x + c[2] y + c[3] z + c[4] x^2 + c[5] x y + c[6] x z + c[7] y^2 + c[8] y z + c[9] z^2"""

    def __init__(self, c):
        self.c = np.asarray(c, dtype=np.float64)

    def __call__(self, X):
        x, y, z = X[..., 0], X[..., 1], X[..., 2]
        c = self.c
        return c[0] + c[1] * x + c[2] * y + c[3] * z + c[4] * x * x + c[5] * x * y + c[6] * x * z + c[7] * y * y + c[8] * y * z + c[9] * z * z

    def d(self, a):
        c = self.c
        rows = {0: [c[1], 2 * c[4], c[5], c[6]], 1: [c[2], c[5], 2 * c[7], c[8]], 2: [c[3], c[6], c[8], 2 * c[9]]}
        return Quad(rows[a] + [0.0] * 6)

    def zpoly(self, x, y):
        """the coefficients [c0, c1, c2] of 1, z, z^2 over the columns (x, y), longdouble"""
        c = self.c.astype(LD)
        return [c[0] + c[1] * x + c[2] * y + c[4] * x * x + c[5] * x * y + c[7] * y * y, c[3] + c[6] * x + c[8] * y, c[9] + 0 * x]


def pmul(a, b):
    out = [0 * a[0] for _ in range(len(a) + len(b) - 1)]
    for i, ai in enumerate(a):
        for j, bj in enumerate(b):
            out[i + j] = out[i + j] + ai * bj
    return out


def pint(a, zb, zt):
    return sum(ak * (zt ** (k + 1) - zb ** (k + 1)) / (k + 1) for k, ak in enumerate(a))


U_POLY = [Quad([0.1, 0.3, -1.0, 0.5, 0.7, -0.2, 0.4, 0.3, -0.6, 0.9]), Quad([-0.2, 2.0, -0.7, 0.25, -0.5, 0.8, 0.1, 0.6, 0.2, -1.1]),
          Quad([0.05, -0.4, 1.5, 1.1, 0.2, 0.3, -0.9, -0.4, 0.5, 0.7])]
B_POLY = Quad([1.0, 1.0, -2.0, 0.5, 1.0, -1.0, 0.3, 0.4, 2.0, 1.0])
B_LIN = Quad([1.0, 1.0, -2.0, 0.5] + [0.0] * 6)
B_OF_Z = Quad([0.3, 0, 0, 0.8, 0, 0, 0, 0, 0, 1.7])
P_GRAD = np.array([0.6, -0.9, 0.35])


def pinned_vertex(model):
    t = model.fe_data.tables
    pin = np.nonzero(t.p_pos < 0)[0]
    assert len(pin) == 1
    return model.fe_data.mesh.node_coords[pin[0]]


def set_state(model, u=U_POLY, b=B_POLY, pgrad=P_GRAD):
    """u_a, b': Quad; p = pgrad . (x - x_pinned), zero at the pinned vertex.  No Dirichlet DoFs on the bare models: represented exactly"""
    fed = model.fe_data
    m, t = fed.mesh, fed.tables
    assert (t.u_pos >= 0).all() and (t.b_pos >= 0).all()
    Xn = m.node_coords
    x = np.zeros(fed.dofs.nu + fed.dofs.np)
    x[t.u_pos] = np.stack([q(Xn) for q in u], axis=-1)
    free = t.p_pos >= 0
    x[t.p_pos[free]] = ((Xn[:m.nv] - pinned_vertex(model)) @ np.asarray(pgrad, dtype=float))[free]
    bv = np.zeros(fed.dofs.nb)
    bv[t.b_pos] = b(Xn[:len(t.b_pos)])
    model.inversion.solver.x.upload(x)
    model.b_vec.upload(bv)


def nodal(model):
    """un (nn, 3), bn (nb_nodes,), pn (nv,) from the device vectors"""
    un, bn = ir.nodal_values(model)
    t = model.fe_data.tables
    x = model.inversion.solver.x.to_host()
    return un, bn, np.where(t.p_pos >= 0, x[np.maximum(t.p_pos, 0)], 0.0)


def all_columns(model):
    """the 33 x 33 grid, the vertex columns and the edge-midpoint columns"""
    mesh = model.fe_data.mesh
    return np.vstack([ur.grid_points(), ur.vertex_columns(mesh), ur.edge_midpoint_columns(mesh)])


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def _fields(model, br, nod, cell, pts, unit=()):
    """values and absolute sums at (cell, pts): dicts u (n, 3), b, p, gb (n, 3), gp (n, 3); the fields named in `unit` enter the absolute
    sums with nodal values 1 (what an error of 1 in every nodal value of that field does)"""
    m, s = model.fe_data.mesh, model.fe_data.spaces
    un, bn, pn = nod
    lam = br.lambdas(pts, cell)
    N = br.p2(lam)
    G = np.concatenate([-br.T[cell].sum(1, keepdims=True), br.T[cell]], axis=1)                  # (n, 4, 3)
    uc, pc = un[m.cell_nodes[cell]], pn[m.cells[cell]]
    mag = lambda name, a: np.ones_like(a) if name in unit else np.abs(a)
    # the barycentrics' own absolute sums: lambda_k = sum_a G_ka d_a (k = 1..3), lambda_0 = 1 - sum
    L123 = np.einsum("nij,nj->ni", np.abs(br.T[cell]), np.abs(pts - br.x0[cell]))
    Lam = np.concatenate([1.0 + L123.sum(-1, keepdims=True), L123], axis=1)
    dNa = np.abs(br.dp2(lam))                                                                    # (n, 10, 4)
    v, A = {}, {}
    v["u"] = np.einsum("ni,nia->na", N, uc)
    A["u"] = np.einsum("ni,nia->na", np.abs(N), mag("u", uc)) + np.einsum("nik,nia,nk->na", dNa, mag("u", uc), Lam)
    if s.b_order == 2:
        bc = bn[m.cell_nodes[cell]]
        bm = mag("b", bc)
        v["b"], A["b"] = np.einsum("ni,ni->n", N, bc), np.einsum("ni,ni->n", np.abs(N), bm) + np.einsum("nik,ni,nk->n", dNa, bm, Lam)
        H2 = np.zeros((len(cell), 4, 4))                                                         # sum_i |v_i| |d2 N_i / dl_k dl_j|
        for k in range(4):
            H2[:, k, k] = 4 * bm[:, k]
        for e in range(6):
            H2[:, sr.EA[e], sr.EB[e]] = H2[:, sr.EB[e], sr.EA[e]] = 4 * bm[:, 4 + e]
        v["gb"] = np.einsum("ni,nik,nka->na", bc, br.dp2(lam), G)
        A["gb"] = np.einsum("ni,nik,nka->na", bm, dNa, np.abs(G)) + np.einsum("nkj,nja,nk->na", H2, np.abs(G), Lam)
    else:
        bc = bn[m.cells[cell]]
        bm = mag("b", bc)
        v["b"], A["b"] = np.einsum("ni,ni->n", lam, bc), np.einsum("ni,ni->n", np.abs(lam), bm) + np.einsum("ni,ni->n", bm, Lam)
        v["gb"], A["gb"] = np.einsum("nk,nka->na", bc, G), np.einsum("nk,nka->na", bm, np.abs(G))
    pm = mag("p", pc)
    v["p"], A["p"] = np.einsum("ni,ni->n", lam, pc), np.einsum("ni,ni->n", np.abs(lam), pm) + np.einsum("ni,ni->n", pm, Lam)
    v["gp"], A["gp"] = np.einsum("nk,nka->na", pc, G), np.einsum("nk,nka->na", pm, np.abs(G))
    return v, A


def _integrands(f, z):
    u, b, p, gb, gp = f["u"], f["b"], f["p"], f["gb"], f["gp"]
    return [np.ones_like(z), u[:, 0], u[:, 1], u[:, 2], b, z * b, p, gp[:, 0], gp[:, 1], gb[:, 0], gb[:, 1], z * gb[:, 0], z * gb[:, 1],
            0.5 * (u[:, 0] ** 2 + u[:, 1] ** 2), u[:, 0] * b, u[:, 1] * b, u[:, 2] * b]


def face_slopes(br, cell, pts, bottom):
    """d_x z, d_y z of the face through which the column leaves `cell` at `pts` (downwards: bottom), from the vertex coordinates of that
    face; the rounding bound of the slopes; ambiguous: not exactly one candidate face within AMBIG"""
    X = br.mesh.geo_coords[br.mesh.cell_geo[cell]]                       # (n, 4, 3)
    lam = br.lambdas(pts, cell)
    G = np.concatenate([-br.T[cell].sum(1, keepdims=True), br.T[cell]], axis=1)
    cand = (np.abs(lam) <= AMBIG) & ((G[..., 2] > 0) if bottom else (G[..., 2] < 0))
    amb = cand.sum(1) != 1
    i = cand.argmax(1)
    others = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])[i]
    r = np.arange(len(cell))
    v0, v1, v2 = (X[r, others[:, k]] for k in range(3))
    a, b = v1 - v0, v2 - v0
    n = np.cross(a, b)
    Aa, Ab = np.abs(v1) + np.abs(v0), np.abs(v2) + np.abs(v0)
    Sn = np.stack([Aa[:, 1] * Ab[:, 2] + Aa[:, 2] * Ab[:, 1], Aa[:, 2] * Ab[:, 0] + Aa[:, 0] * Ab[:, 2], Aa[:, 0] * Ab[:, 1] + Aa[:, 1] * Ab[:, 0]], -1)
    # the library's slope is - G_ix / G_iz of an inverted edge matrix E: |dG_ka| <= 24 eps kappa(E) max_k |T_ka| (T = inv E)
    E = np.transpose(X[:, 1:] - X[:, :1], (0, 2, 1))
    Ta = np.abs(br.T[cell])
    kappa = Ta.sum(2).max(1) * np.abs(E).sum(2).max(1)
    M = 4 * kappa[:, None] * Ta.max(1)                                   # (n, 3); 4: lambda_0's row is the sum of three
    Gi = np.abs(G[r, i])
    with np.errstate(divide="ignore", invalid="ignore"):
        sl = -n[:, :2] / n[:, 2:3]
        bound = 16 * EPS * (Sn[:, :2] / np.abs(n[:, 2:3]) + np.abs(n[:, :2]) * Sn[:, 2:3] / n[:, 2:3] ** 2)
        bound = bound + 24 * EPS * (M[:, :2] / Gi[:, 2:3] + Gi[:, :2] * M[:, 2:3] / Gi[:, 2:3] ** 2)
    return sl, bound, amb


def restate(model, CI, unit=()):
    """SimpleNamespace: tot, sabs (31, ncol) longdouble / float (NaN where dry; for the end channels sabs = A), amb_bot, amb_top,
    and the segment terms (17, nseg)"""
    br = sr.Brute(model.fe_data.mesh)
    nod = nodal(model)
    ptr, cell, zt, zb = CI.segments()
    ncol = CI.ncol
    nseg = np.diff(ptr)
    col = np.repeat(np.arange(ncol), nseg)
    wet = nseg > 0
    dz = (zt - zb).astype(LD)
    terms, tabs = np.zeros((NI, len(cell)), dtype=LD), np.zeros((NI, len(cell)), dtype=LD)
    for g in range(3):
        z = zb + GS[g] * (zt - zb)
        f, A = _fields(model, br, nod, cell, np.column_stack([CI.xy[col], z]), unit)
        for ch, (fv, Av) in enumerate(zip(_integrands(f, z), _integrands(A, np.abs(z)))):
            terms[ch] += GW[g] * fv.astype(LD) * dz
            tabs[ch] += GW[g] * Av.astype(LD) * dz
    tot, sabs = np.full((NI + NE, ncol), np.nan, dtype=LD), np.full((NI + NE, ncol), np.nan)
    for ch in range(NI):
        a, s = np.zeros(ncol, dtype=LD), np.zeros(ncol, dtype=LD)
        np.add.at(a, col, terms[ch])
        np.add.at(s, col, tabs[ch])
        tot[ch, wet], sabs[ch, wet] = a[wet], s[wet].astype(np.float64)
    xyw = CI.xy[wet]
    cb, ct = cell[ptr[1:][wet] - 1], cell[ptr[:-1][wet]]
    pb, pt = np.column_stack([xyw, zb[ptr[1:][wet] - 1]]), np.column_stack([xyw, zt[ptr[:-1][wet]]])
    fb, Ab = _fields(model, br, nod, cb, pb, unit)
    ft, At = _fields(model, br, nod, ct, pt, unit)
    sb, sbb, amb_b = face_slopes(br, cb, pb, True)
    st, stb, amb_t = face_slopes(br, ct, pt, False)
    ends = [(fb["p"], Ab["p"]), (fb["b"], Ab["b"]), (fb["gb"][:, 2], Ab["gb"][:, 2]), (fb["gp"][:, 0], Ab["gp"][:, 0]),
            (fb["gp"][:, 1], Ab["gp"][:, 1]), (fb["gp"][:, 2], Ab["gp"][:, 2]), (sb[:, 0], None), (sb[:, 1], None),
            (ft["p"], At["p"]), (ft["b"], At["b"]), (ft["u"][:, 0], At["u"][:, 0]), (ft["u"][:, 1], At["u"][:, 1]), (st[:, 0], None), (st[:, 1], None)]
    for k, (v, A) in enumerate(ends):
        tot[NI + k, wet] = v
        if A is not None:
            sabs[NI + k, wet] = A
    slope_bound = np.full((4, ncol), np.nan)
    slope_bound[0, wet], slope_bound[1, wet], slope_bound[2, wet], slope_bound[3, wet] = sbb[:, 0], sbb[:, 1], stb[:, 0], stb[:, 1]
    ab, at = np.zeros(ncol, dtype=bool), np.zeros(ncol, dtype=bool)
    ab[wet], at[wet] = amb_b, amb_t
    return SimpleNamespace(tot=tot, sabs=sabs, amb_bot=ab, amb_top=at, slope_bound=slope_bound, terms=terms, wet=wet, col=col)


SLOPE_CH = {NI + 6: (0, "amb_bot"), NI + 7: (1, "amb_bot"), NI + 12: (2, "amb_top"), NI + 13: (3, "amb_top")}


def compare(out, R, nops, label, ref=None, channels=range(NI + NE), extra=None):
    """every channel of out (31, ncol) within its bound of the restatement (or of `ref` with the restatement's S_abs); prints first"""
    ref = R.tot if ref is None else ref
    wet = R.wet
    assert np.isnan(out[:, ~wet]).all() and np.isfinite(out[:, wet]).all()
    worst, fails = [], []
    for ch in channels:
        if ch in SLOPE_CH:
            k, amb = SLOPE_CH[ch]
            sel = wet & ~getattr(R, amb)
            bound = R.slope_bound[k]
        else:
            sel = wet
            bound = (2 * nops if ch < NI else 2 * 64) * EPS * R.sabs[ch] + (0.0 if extra is None else extra[ch])
        err = np.abs(out[ch][sel].astype(LD) - ref[ch][sel]).astype(np.float64)
        ratio = np.where(err == 0, 0.0, err / np.maximum(bound[sel], np.finfo(float).tiny))
        worst.append((ch, float(err.max(initial=0.0)), float(ratio.max(initial=0.0)), int(sel.sum())))
        if (err > bound[sel]).any():
            fails.append(ch)
    print(f"columns {label}: {int(wet.sum())} wet columns; per channel max|err| (of its bound): "
          + ", ".join(f"ch{ch} {e:.1e} ({r:.3f})" for ch, e, r, _ in worst))
    assert not fails, (label, fails)
    return worst


# ---- check 2: the tiling ---------------------------------------------------------------------------------------------------------------------
def check_tiling(model):
    xy = all_columns(model)
    CI = npg.ColumnIntegrals(model, points=xy)
    S = npg.BuoyancySurfaces(model, [0.0], points=xy)
    for a, b in zip(CI.segments(), S.segments()):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert np.array_equal(CI.z_top, S.z_top, equal_nan=True) and np.array_equal(CI.z_bot, S.z_bot, equal_nan=True)
    assert np.array_equal(CI.nseg, S.nseg) and CI.info == S.info and CI.info["dry"] > 0 and CI.info["segments"] > 5000
    print(f"tiling: {CI.info} - the segments, z_top and z_bot of npg_surfaces_* bit for bit")


# ---- check 3: closed forms -------------------------------------------------------------------------------------------------------------------
def exact_integrals(xy, zt, zb, u, b, pgrad, xpin):
    """the 17 integrals between zb and zt of the polynomial state, longdouble (ncol,) each"""
    x, y, zt, zb = (a.astype(LD) for a in (xy[:, 0], xy[:, 1], zt, zb))
    one = [1 + 0 * x]
    zp = [0 * x, 1 + 0 * x]
    up = [q.zpoly(x, y) for q in u]
    bp = b.zpoly(x, y)
    g = np.asarray(pgrad, dtype=LD)
    pp = [g[0] * (x - xpin[0]) + g[1] * (y - xpin[1]) - g[2] * LD(xpin[2]), g[2] + 0 * x]
    bx, by = b.d(0).zpoly(x, y), b.d(1).zpoly(x, y)
    half = [LD(0.5) + 0 * x]
    polys = [one, up[0], up[1], up[2], bp, pmul(zp, bp), pp, [g[0] + 0 * x], [g[1] + 0 * x], bx, by, pmul(zp, bx), pmul(zp, by),
             pmul(half, [a + c for a, c in zip(pmul(up[0], up[0]), pmul(up[1], up[1]))]), pmul(up[0], bp), pmul(up[1], bp), pmul(up[2], bp)]
    return np.stack([pint(p, zb, zt) for p in polys])


USES = {"u": [1, 2, 3, 13, 14, 15, 16, NI + 10, NI + 11], "b": [4, 5, 9, 10, 11, 12, 14, 15, 16, NI + 1, NI + 2, NI + 9],
        "p": [6, 7, 8, NI + 0, NI + 3, NI + 4, NI + 5, NI + 8]}


def nodal_noise(model, CI, u, b, pgrad):
    """(31, ncol): what the rounding of the polynomial state's NODAL values adds to the distance from the closed form.  set_state evaluates
    a Quad at a node in fp64 with at most 25 operations on terms whose absolute values sum to P_abs = sum |c_k| |monomial| (p: 8
    operations on sum |g_a| (|x_a| + |x_pin,a|)): every nodal value of field f is off by at most e_f = 25 eps max_nodes P_abs, and a
    channel moves by at most e_f times its S_abs taken with the nodal values of f set to 1 (restate(unit={f}))."""
    Xa = np.abs(model.fe_data.mesh.node_coords)
    e = {"u": 25 * EPS * max(Quad(np.abs(q.c))(Xa).max() for q in u), "b": 25 * EPS * Quad(np.abs(b.c))(Xa).max(),
         "p": 8 * EPS * ((Xa + np.abs(pinned_vertex(model))) @ np.abs(pgrad)).max()}
    extra = np.zeros((NI + NE, CI.ncol))
    for f, chans in USES.items():
        S1 = restate(model, CI, unit={f}).sabs
        for ch in chans:
            extra[ch] += e[f] * np.nan_to_num(S1[ch])
    return extra


def check_closed_form(arch, b_order=2):
    model = ir.bare_model(arch, b_order=b_order)
    b = B_POLY if b_order == 2 else B_LIN
    set_state(model, b=b)
    CI = npg.ColumnIntegrals(model, points=all_columns(model))
    out = CI.compute_raw()
    R = restate(model, CI)
    extra = nodal_noise(model, CI, U_POLY, b, P_GRAD)
    zt, zb = CI.z_top, CI.z_bot
    ref = R.tot.copy()
    ref[:NI, R.wet] = exact_integrals(CI.xy[R.wet], zt[R.wet], zb[R.wet], U_POLY, b, P_GRAD, pinned_vertex(model))
    compare(out, R, n_ops(CI), f"closed form P{b_order}", ref=ref, channels=range(NI), extra=extra)
    # the end values of a polynomial state are the polynomial at the ends
    xw = CI.xy[R.wet]
    Xb, Xt = np.column_stack([xw, zb[R.wet]]), np.column_stack([xw, zt[R.wet]])
    xpin = pinned_vertex(model)
    for k, v in {0: (Xb - xpin) @ P_GRAD, 1: b(Xb), 2: b.d(2)(Xb), 3: P_GRAD[0], 4: P_GRAD[1], 5: P_GRAD[2], 8: (Xt - xpin) @ P_GRAD, 9: b(Xt),
                 10: U_POLY[0](Xt), 11: U_POLY[1](Xt)}.items():
        ref[NI + k, R.wet] = v
    compare(out, R, n_ops(CI), f"closed form P{b_order}, ends", ref=ref, channels=[NI + k for k in (0, 1, 2, 3, 4, 5, 8, 9, 10, 11)], extra=extra)
    return model, CI, R


# ---- check 4: the restatement on a real state ------------------------------------------------------------------------------------------------
def check_real_state(model):
    CI = npg.ColumnIntegrals(model, points=all_columns(model))
    out = CI.compute_raw()
    R = restate(model, CI)
    namb = int((R.amb_bot | R.amb_top)[R.wet].sum())
    print(f"real state: {namb} of {int(R.wet.sum())} wet columns leave a cell through a vertex or an edge (slopes not judged)")
    assert (~R.amb_bot & R.wet).sum() > 500 and (~R.amb_top & R.wet).sum() > 500
    compare(out, R, n_ops(CI), "real state")
    M = CI.compute()
    assert np.array_equal(M.raw.reshape(NI + NE, -1), out, equal_nan=True) and np.array_equal(M.U[..., 1], out[2], equal_nan=True)
    assert np.array_equal(M.N2_bot, model.params.N2 + out[NI + 2], equal_nan=True) and np.array_equal(M.H, CI.z_top - CI.z_bot, equal_nan=True)
    th = np.abs(M.thickness - M.H)[R.wet]
    assert (th <= CI.info["max_per_column"] * EPS * M.H[R.wet]).all()
    g = M.gamma(full=False)
    assert np.array_equal(g, -out[5], equal_nan=True)
    return M


def check_grid_diagnostics(model):
    """reported only: the 256-point trapezoid of GridDiagnostics against the exact integrals over the same columns"""
    x = ur.GRID
    M = npg.ColumnIntegrals(model, x=x, y=x).compute()
    g = npg.GridDiagnostics(model, x=x, y=x, nz=256).compute()
    wet = ~np.isnan(M.H) & (g.H > 0)
    dH, dU, dV = (np.abs(a - b)[wet].max() for a, b in ((g.H, M.H), (g.U, M.U[..., 0]), (g.V, M.U[..., 1])))
    print(f"GridDiagnostics (256-point trapezoid) against the exact column integrals, {int(wet.sum())} columns: max|dH| = {dH:.3e} of "
          f"{np.nanmax(M.H):.3f}, max|dU| = {dU:.3e} of {np.nanmax(np.abs(M.U[..., 0])):.3e}, max|dV| = {dV:.3e} of {np.nanmax(np.abs(M.U[..., 1])):.3e}")
    assert np.isfinite([dH, dU, dV]).all() and wet.sum() > 500
    psi = M.streamfunction()
    U = np.where(np.isnan(M.U[..., 0]), 0.0, M.U[..., 0])
    ref = -np.concatenate([np.zeros((len(x), 1)), np.cumsum(0.5 * (U[:, 1:] + U[:, :-1]) * np.diff(x), axis=1)], axis=1)
    assert np.array_equal(np.isnan(psi), np.isnan(M.H)) and np.array_equal(psi[wet], ref[wet])
    with np.testing.assert_raises(ValueError):
        npg.ColumnIntegrals(model, points=[[0.0, 0.0]]).compute().streamfunction()


# ---- check 5: Leibniz ------------------------------------------------------------------------------------------------------------------------
def check_leibniz(arch):
    model, CI, R = check_closed_form(arch)
    m1 = ur.with_N2(model, 1.0)
    CI.model = m1
    M = CI.compute()
    ok = R.wet & ~R.amb_bot & ~R.amb_top
    assert ok.sum() > 1000
    x, y = CI.xy[ok, 0].astype(LD), CI.xy[ok, 1].astype(LD)
    zt, zb = CI.z_top[ok].astype(LD), CI.z_bot[ok].astype(LD)
    sb, st = R.tot[NI + 6:NI + 8, ok].T, R.tot[NI + 12:NI + 14, ok].T               # the mesh faces' slopes (n, 2)
    H, gH = zt - zb, st - sb
    zp = [0 * x, 1 + 0 * x]
    Bq = Quad(B_POLY.c + np.array([0, 0, 0, 1.0, 0, 0, 0, 0, 0, 0]))                 # B = N2 z + b', N2 = 1
    Bt, Bb = Bq(np.column_stack([x, y, zt])), Bq(np.column_stack([x, y, zb]))
    gg = np.stack([-pint(pmul(zp, Bq.d(a).zpoly(x, y)), zb, zt) - zt * Bt * st[:, a] + zb * Bb * sb[:, a] for a in (0, 1)], -1)
    gamma = -pint(pmul(zp, Bq.zpoly(x, y)), zb, zt)
    # bounds: the channels' bounds through the algebra, first order
    nops = n_ops(CI)
    bI = lambda ch: 2 * nops * EPS * R.sabs[ch][ok]
    bE = lambda k: 2 * 64 * EPS * R.sabs[NI + k][ok]
    bs = R.slope_bound[:, ok]                                                         # d_x z_bot, d_y z_bot, d_x z_top, d_y z_top
    z3 = 8 * EPS * (np.abs(zt) ** 3 + np.abs(zb) ** 3).astype(float) / 3
    e_gamma = np.abs(M.gamma().ravel()[ok] - gamma).astype(float)
    b_gamma = bI(5) + z3
    aBt, aBb = (R.sabs[NI + 9][ok] + np.abs(zt)).astype(float), (R.sabs[NI + 1][ok] + np.abs(zb)).astype(float)
    b_gg = np.stack([bI(11 + a) + np.abs(zt).astype(float) * (bE(9) + 4 * EPS * aBt) * np.abs(st[:, a]).astype(float)
                     + np.abs(zt).astype(float) * aBt * bs[2 + a]
                     + np.abs(zb).astype(float) * (bE(1) + 4 * EPS * aBb) * np.abs(sb[:, a]).astype(float)
                     + np.abs(zb).astype(float) * aBb * bs[a]
                     + 8 * EPS * (R.sabs[11 + a][ok] + np.abs(zt * st[:, a]).astype(float) * aBt + np.abs(zb * sb[:, a]).astype(float) * aBb)
                     for a in (0, 1)], -1)
    got_gg = M.grad_gamma().reshape(-1, 2)[ok]
    e_gg = np.abs(got_gg - gg).astype(float)
    jeb = (gH[:, 0] * gg[:, 1] - gH[:, 1] * gg[:, 0]) / H ** 2
    b_gH = np.stack([bs[2] + bs[0], bs[3] + bs[1]], -1) + 2 * EPS * (np.abs(st) + np.abs(sb)).astype(float)
    aH, agg, H_ = np.abs(gH).astype(float), np.abs(gg).astype(float), H.astype(float)
    b_jeb = (b_gH[:, 0] * agg[:, 1] + aH[:, 0] * b_gg[:, 1] + b_gH[:, 1] * agg[:, 0] + aH[:, 1] * b_gg[:, 0]
             + 8 * EPS * (aH[:, 0] * agg[:, 1] + aH[:, 1] * agg[:, 0])) / H_ ** 2
    e_jeb = np.abs(M.jebar().ravel()[ok] - jeb).astype(float)
    bpt = P_GRAD[0] * gH[:, 1] - P_GRAD[1] * gH[:, 0]
    ap = np.abs(P_GRAD)
    b_bpt = (bE(3) * aH[:, 1] + ap[0] * b_gH[:, 1] + bE(4) * aH[:, 0] + ap[1] * b_gH[:, 0] + 8 * EPS * (ap[0] * aH[:, 1] + ap[1] * aH[:, 0]))
    e_bpt = np.abs(M.bottom_pressure_torque().ravel()[ok] - bpt).astype(float)
    for name, e, b in (("gamma", e_gamma, b_gamma), ("grad gamma", e_gg, b_gg), ("JEBAR", e_jeb, b_jeb), ("bottom pressure torque", e_bpt, b_bpt)):
        print(f"Leibniz, {name}: {int(ok.sum())} columns, max|err| = {e.max():.2e}, max err / bound = {(e / b).max():.4f}")
        assert (e <= b).all(), name
    # b' = b'(z): grad_h b' = 0, and JEBAR is the algebra of its end terms
    set_state(model, b=B_OF_Z)
    M = CI.compute()
    R2 = restate(model, CI)
    zg = M.z_grad_b_int.reshape(-1, 2)[ok]
    bz = np.stack([2 * nops * EPS * R2.sabs[11][ok], 2 * nops * EPS * R2.sabs[12][ok]], -1)
    print(f"b' = b'(z): max|int z grad_h b' dz| = {np.abs(zg).max():.2e}, max of its bound {(np.abs(zg) / bz).max():.4f}")
    assert (np.abs(zg) <= bz).all()
    Bt, Bb = M.b_top + M.z_top, M.b_bot + M.z_bot
    ends = -(M.z_top * Bt)[..., None] * M.grad_z_top + (M.z_bot * Bb)[..., None] * M.grad_z_bot
    je = (M.grad_H[..., 0] * ends[..., 1] - M.grad_H[..., 1] * ends[..., 0]) / M.H ** 2
    bj = (aH[:, 0] * bz[:, 1] + aH[:, 1] * bz[:, 0]) / H_ ** 2 * 1.01 + 8 * EPS * np.abs(je.ravel()[ok])
    assert (np.abs(M.jebar().ravel()[ok] - je.ravel()[ok]) <= bj).all()


# ---- check 6: geostrophy ---------------------------------------------------------------------------------------------------------------------
def check_geostrophic(arch, f0=0.7):
    model = ir.bare_model(arch)
    zero = Quad([0.0] * 10)
    u = [Quad([-P_GRAD[1] / f0] + [0.0] * 9), Quad([P_GRAD[0] / f0] + [0.0] * 9), zero]
    set_state(model, u=u, b=zero)
    CI = npg.ColumnIntegrals(model, points=all_columns(model))
    M = CI.compute()
    R = restate(model, CI)
    res = M.stress_residual(f0)[R.wet]
    nops = n_ops(CI)
    bound = np.stack([2 * nops * EPS * (f0 * R.sabs[2] + R.sabs[7])[R.wet], 2 * nops * EPS * (f0 * R.sabs[1] + R.sabs[8])[R.wet]], -1)
    print(f"geostrophic: max|f z^ x U + int grad p dz| = {np.abs(res).max():.2e} of max|f U| {f0 * np.nanmax(np.abs(M.U)):.2e}; "
          f"max err / bound = {(np.abs(res) / bound).max():.4f}")
    assert (np.abs(res) <= bound).all() and np.isnan(M.stress_residual(f0)[~R.wet]).all()
    assert np.array_equal(M.stress_residual(lambda x, y: f0 + 0 * x), M.stress_residual(f0), equal_nan=True)


# ---- check 7: edge sizes and determinism -----------------------------------------------------------------------------------------------------
def fold(seg, ptr):
    """segments_out folded in the order of columns_core.h: top to bottom from 0.0, NaN where dry"""
    nseg = np.diff(ptr)
    acc = np.zeros((NI, len(nseg)))
    for k in range(int(nseg.max(initial=0))):
        on = nseg > k
        acc[:, on] = acc[:, on] + seg[:, ptr[:-1][on] + k]
    acc[:, nseg == 0] = np.nan
    return acc


def check_edges(model):
    set_state(model)
    rng = np.random.default_rng(sr.SEED)
    xy = rng.uniform(-1.0, 1.0, (1000, 2))                               # the corners of the square lie outside the disc: dry
    xy[17] = [np.nan, 0.1]
    xy[500] = [0.2, np.nan]
    xy[3] = [0.0, 0.0]
    phi = np.linspace(0.0, 2 * np.pi, 40, endpoint=False)
    xy[600:640] = 0.99 * np.column_stack([np.cos(phi), np.sin(phi)])      # at the coast: columns of one or two segments
    r = np.hypot(xy[:, 0], xy[:, 1])
    full = npg.ColumnIntegrals(model, points=xy)
    nseg = full.nseg
    info = full.info
    assert nseg[17] == 0 and nseg[500] == 0 and (nseg[r > 1.0] == 0).all() and (r > 1.0).sum() > 100 and info["dry"] == (nseg == 0).sum()
    assert (nseg == 1).any() and (nseg == info["max_per_column"]).any() and info["max_per_column"] > 8
    out, seg = full.compute_raw(segments=True)
    out2 = full.compute_raw()
    out3, seg3 = full.compute_raw(segments=True)
    assert out.shape == (NI + NE, 1000) and seg.shape == (NI, info["segments"])
    assert np.array_equal(out, out2, equal_nan=True) and np.array_equal(out, out3, equal_nan=True) and np.array_equal(seg, seg3)
    assert np.isnan(out[:, nseg == 0]).all() and np.isfinite(out[:, nseg > 0]).all()
    ptr = full.segments()[0]
    assert np.array_equal(fold(seg, ptr), out[:NI], equal_nan=True)       # the stated order, bit for bit
    for ncol in (1, 63, 64, 65):
        sub = npg.ColumnIntegrals(model, points=xy[:ncol])
        o, s = sub.compute_raw(segments=True)
        assert o.shape == (NI + NE, ncol) and np.array_equal(o, out[:, :ncol], equal_nan=True) and np.array_equal(s, seg[:, :ptr[ncol]])
    one = np.nonzero(nseg == 1)[0][0]
    o = npg.ColumnIntegrals(model, points=xy[one:one + 1]).compute_raw()
    assert np.array_equal(o[:, 0], out[:, one])
    dry = npg.ColumnIntegrals(model, points=[[np.nan, 0.0], [3.0, 3.0]])
    o, s = dry.compute_raw(segments=True)
    assert np.isnan(o).all() and s.shape == (NI, 0) and dry.info["segments"] == 0
    print(f"edges: ncol 1, 63, 64, 65, 1000 agree bit for bit; {info}; segments_out folds to out bit for bit; a one-segment column and the "
          f"column of {info['max_per_column']} segments among them")


# ---- check 8: refusals -----------------------------------------------------------------------------------------------------------------------
def _refused(rc, entry, word):
    msg = L.lib().npg_last_error().decode()
    assert rc == NPG_EINVAL and entry in msg and word in msg, (rc, msg, entry, word)


def check_refusals(model):
    lib = L.lib()
    set_state(model)
    ctx = model.arch.ctx
    xy = ur.grid_points()[::5].copy()
    CI = npg.ColumnIntegrals(model, points=xy)
    x, b = model.inversion.solver.x, model.b_vec
    ncol, nseg = len(xy), CI.info["segments"]
    sentinel = 12345.0
    out = npg.DeviceVector.from_host(ctx, np.full((NI + NE) * ncol, sentinel))
    seg = npg.DeviceVector.from_host(ctx, np.full(NI * nseg, sentinel))
    short = npg.DeviceVector.from_host(ctx, np.full((NI + NE) * ncol - 1, sentinel))
    xs, bs = npg.DeviceVector(ctx, x.n - 1), npg.DeviceVector(ctx, b.n + 1)
    other = C.c_void_p()
    L.check(lib.npg_ctx_create(getattr(ctx, "device", 0) or 0, C.byref(other)))
    foreign = C.c_void_p()
    L.check(lib.npg_vec_create(other, (NI + NE) * ncol, C.byref(foreign)))
    cases = [((None, x.h, b.h, out.h, seg.h), "NULL"), ((CI.h, None, b.h, out.h, seg.h), "NULL"), ((CI.h, x.h, None, out.h, seg.h), "NULL"),
             ((CI.h, x.h, b.h, None, seg.h), "NULL"), ((CI.h, xs.h, b.h, out.h, seg.h), "entries"), ((CI.h, x.h, bs.h, out.h, seg.h), "entries"),
             ((CI.h, x.h, b.h, short.h, seg.h), "entries"), ((CI.h, x.h, b.h, out.h, short.h), "entries"),
             ((CI.h, x.h, b.h, foreign, seg.h), "contexts")]
    for args, word in cases:
        _refused(lib.npg_columns_compute(*args), "npg_columns_compute", word)
    L.check(lib.npg_ctx_sync(ctx.h))
    for v in (out, seg, short):
        assert (v.to_host() == sentinel).all()                           # nothing was written
    lib.npg_vec_destroy(foreign)
    lib.npg_ctx_destroy(other)
    h = C.c_void_p()
    ch = pr.channel_bare(model.arch)
    chC = npg.ColumnIntegrals(ch, points=[[0.0, 0.0]])
    _refused(lib.npg_columns_create(chC.fe.h, CI.loc.h, L.ptr(xy), ncol, C.byref(h)), "npg_columns_create", "another mesh")
    _refused(lib.npg_columns_create(CI.fe.h, None, L.ptr(xy), ncol, C.byref(h)), "npg_columns_create", "NULL")
    _refused(lib.npg_columns_create(None, CI.loc.h, L.ptr(xy), ncol, C.byref(h)), "npg_columns_create", "NULL")
    _refused(lib.npg_columns_create(CI.fe.h, CI.loc.h, None, ncol, C.byref(h)), "npg_columns_create", "NULL")
    _refused(lib.npg_columns_create(CI.fe.h, CI.loc.h, L.ptr(xy), ncol, None), "npg_columns_create", "NULL")
    _refused(lib.npg_columns_create(CI.fe.h, CI.loc.h, L.ptr(xy), 0, C.byref(h)), "npg_columns_create", "columns")
    _refused(lib.npg_columns_create(CI.fe.h, CI.loc.h, L.ptr(xy), -1, C.byref(h)), "npg_columns_create", "columns")
    part = pr._partitioned_locator(model)
    if part is not None:
        _refused(lib.npg_columns_create(CI.fe.h, part, L.ptr(xy), ncol, C.byref(h)), "npg_columns_create", "partitioned")
        lib.npg_locator_destroy(part)
    assert not h.value
    for entry in ("info", "columns", "segments"):
        _refused(getattr(lib, "npg_columns_" + entry)(None, None, None, None), "npg_columns_" + entry, "NULL")
    print(f"refusals: {len(cases)} bad calls of npg_columns_compute refused, the outputs untouched"
          + ("" if part is not None else " (no partitioned locator in this library)"))
    L.check(lib.npg_columns_compute(CI.h, x.h, b.h, out.h, seg.h))         # and the good call runs
    assert not (out.to_host() == sentinel).any() and not (seg.to_host() == sentinel).any()
    L.check(lib.npg_columns_compute(CI.h, x.h, b.h, out.h, None))
    with np.testing.assert_raises(L.DeviceError):
        npg.ColumnIntegrals(model, points=np.empty((0, 2)))
    standin = SimpleNamespace(fe_data=model.fe_data, arch=model.arch, layout=SimpleNamespace(locator_cells=None, cell_owner=None))
    with np.testing.assert_raises(NotImplementedError) as e:
        npg.ColumnIntegrals(standin, points=xy)
    assert "rank" in str(e.exception)


def check_embedded_2d(arch):
    from tests import helpers
    flat = helpers.build_model("bowl_mixing", mesh="mesh_bowl2D_h0.1", arch=arch)
    assert flat.fe_data.mesh.dim == 2
    with np.testing.assert_raises(NotImplementedError) as e:
        npg.ColumnIntegrals(flat, nx=8, ny=8)
    assert "3-D" in str(e.exception)


# ---- check 9: the periodic channel -----------------------------------------------------------------------------------------------------------
def check_periodic(arch):
    model = sr.channel_model(arch)
    lo, hi = npg.PointLocator(model).bounding_box
    y = np.linspace(lo[1], hi[1], 23)
    W = hi[0] - lo[0]
    xs = np.array([lo[0], lo[0] + 1e-9 * W, lo[0] + 0.03 * W, hi[0] - 0.03 * W, hi[0] - 1e-9 * W, hi[0]])     # on and beside the seam
    X, Y = np.meshgrid(xs, y, indexing="ij")
    xy = np.column_stack([X.ravel(), Y.ravel()])
    CI = npg.ColumnIntegrals(model, points=xy)
    M = CI.compute()
    R = restate(model, CI)
    assert R.wet.sum() > 60 and R.wet.reshape(6, -1)[[0, 5]].any(axis=1).all()
    Hd = npg.column_depth(model, xy[:, 0], xy[:, 1])
    assert np.array_equal(M.H[R.wet], Hd[R.wet]) and not Hd[~R.wet].any()
    compare(M.raw.reshape(NI + NE, -1), R, n_ops(CI), "periodic channel, seam")
    # the two sides of the seam are one line of the periodic mesh: the same columns
    a, b = M.raw.reshape(NI + NE, 6, -1)[:NI, 0], M.raw.reshape(NI + NE, 6, -1)[:NI, 5]
    both = ~np.isnan(a[0]) & ~np.isnan(b[0])
    bound = 2 * 2 * n_ops(CI) * EPS * np.maximum(R.sabs[:NI].reshape(NI, 6, -1)[:, 0], R.sabs[:NI].reshape(NI, 6, -1)[:, 5])
    ch = [0, 3, 4, 5, 6, 9, 10, 11, 12, 16]                                  # (u = 0 here; every channel that is continuous in x)
    print(f"periodic channel: {int(R.wet.sum())} wet columns on and beside the seam, H = column_depth bit for bit; x = lo against x = hi: "
          f"max|diff| {np.abs(a - b)[:, both][ch].max():.2e}")
    assert both.sum() > 5 and (np.abs(a - b)[:, both][[0, 4, 5, 6]] <= bound[:, both][[0, 4, 5, 6]]).all()


# ---- check 10: the recorder ------------------------------------------------------------------------------------------------------------------
def check_recorder(arch, tmp_path, nsteps=3):
    a = sr.bowl_model(arch, "bowl_surface_flux")
    a.timestepper.t_stop = nsteps * a.timestepper.dt
    b = sr.bowl_model(arch, "bowl_surface_flux")
    b.timestepper.t_stop = nsteps * b.timestepper.dt
    npg.run(b)
    rec = npg.ColumnRecorder(npg.ColumnIntegrals(a, x=ur.GRID[::2], y=ur.GRID[::2]))
    a.on_plot = rec
    npg.run(a, n_plot=1)
    for f in ("u", "p", "b"):
        assert np.array_equal(getattr(a.state, f), getattr(b.state, f)), f
    t, raw = rec.as_arrays()
    assert t.shape == (nsteps,) and raw.shape == (nsteps, NI + NE, 17, 17) and t[-1] == a.timestepper.t
    last = rec.columns.compute()
    assert np.array_equal(raw[-1], last.raw, equal_nan=True) and not np.array_equal(raw[0], raw[-1], equal_nan=True)
    path = os.path.join(str(tmp_path), "columns.npz")
    rec.save(path)
    t2, maps = npg.ColumnRecorder.load(path)
    assert np.array_equal(t2, t) and len(maps) == nsteps
    for k in range(nsteps):
        assert np.array_equal(maps[k].raw, raw[k], equal_nan=True) and np.array_equal(maps[k].jebar(), rec.maps[k].jebar(), equal_nan=True)
        assert np.array_equal(maps[k].streamfunction(), rec.maps[k].streamfunction(), equal_nan=True)
    assert np.isfinite(maps[-1].jebar()[8, 8]) and np.isfinite(maps[-1].gamma()[8, 8])
    print(f"recorder: {nsteps} calls, saved and loaded; the run's u, p, b' unchanged bit for bit")


# ---- check 11: CPU() against GPU() -----------------------------------------------------------------------------------------------------------
def cross_setup(model):
    return all_columns(model)
