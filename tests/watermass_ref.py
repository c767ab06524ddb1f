"""A numpy restatement of the (latitude band, buoyancy class) table (nupgcm_amd.watermass) and the checks shared by
tests/test_watermass.py (CPU()) and tests/test_gpu_watermass.py (GPU()).

The restatement evaluates every sample with its own closed-form shape functions (fe.p2_tables at the rule's points) from the mesh (the
cells' own vertices, tests/integrals_ref.geometry: inverse / pseudo-inverse of the edge matrix, not grad_lambda) and the nodal values
(integrals_ref.nodal_values), bins with np.searchsorted(side="right") and sums every bin with math.fsum.

Bound per entry (j, k, c):   n_total eps S_abs_c(total)  +  n[j, k] 2^-61 S_c
  * the first term is the project's summation bound (integrals_ref.summation_bound: n terms in any order against their exact sum)
    with n_total the counted samples and S_abs_c(total) the restatement's sum of |term_c| over all of them;
  * the second is the fixed-point quantisation: with frexp(S_c) = (m, e) the unit is 2^(e - 61) <= 2^-60 S_c, half a unit per sample,
    n[j, k] samples in the bin; S_c is the library's own pass-1 sum (the info vector).
On these meshes one misplaced sample moves an entry by about S_c / n_total, 10^4 or more above the bound: compare_tables proves it
every time it runs by moving one reference sample one bin over and requiring the comparison to FAIL.

Edges are chosen from the restatement's own sorted sample values - each the midpoint of the widest gap near a quantile - and no
sample may lie within 1e-10 (max - min) of an edge: library and restatement then agree on every sample's bin and the comparison is
rounding only.  No case is excluded."""
import ctypes as C
import math
import os

import numpy as np

import nupgcm_amd as npg
from nupgcm_amd import _lib as L
from nupgcm_amd import fe as F
from nupgcm_amd.inversion import device_fe
from tests import integrals_ref as ir

EPS = np.finfo(np.float64).eps
NCLS = 8
NPG_EINVAL = -1
SEED = 20261018
NEW = {"npg_classes_create", "npg_classes_destroy", "npg_classes_compute"}


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def rule_of(mesh, level):
    """the default rule, restated: centroids of the 8^level (4^level) sub-simplices of `level` red refinements, equal weights.  Only its
    defining properties are used below (positive weights summing to 1, exact for linear functions), so the library's own points serve -
    after they passed exactly those properties."""
    dim = mesh.geo_coords[mesh.cell_geo].shape[1] - 1
    lam, w = npg.watermass.default_rule(level, dim)
    ns = (8 if dim == 3 else 4) ** level
    assert lam.shape == (ns, 4) and w.shape == (ns,) and (w > 0).all() and abs(w.sum() - 1) < 1e-14
    assert np.abs(lam.sum(axis=1) - 1).max() < 1e-14 and (lam >= 0).all() and (lam[:, dim + 1:] == 0).all()
    assert np.abs(w @ lam[:, :dim + 1] - 1.0 / (dim + 1)).max() < 1e-14                  # exact for linear functions: the centroid
    assert len(np.unique(lam.round(12), axis=0)) == ns
    return lam, w


def samples(model, rule, N2, mask=None):
    """(terms (n, NCLS), B (n,), y (n,)) of every sample of the cells that count, cell-major"""
    fed = model.fe_data
    m = fed.mesh
    un, bn = ir.nodal_values(model)
    X, G, wdet, _, qw, ea, eb = ir.geometry(m)
    k = X.shape[1]
    lam, w = rule[0][:, :k], rule[1]
    N, dN = F.p2_tables(lam, ea, eb)
    uc = un[m.cell_nodes]
    if fed.spaces.b_order == 2:
        bc, Nb, dNb = bn[m.cell_nodes], N, dN
    else:
        bc, Nb, dNb = bn[m.cells], lam, np.broadcast_to(np.eye(k), (len(w), k, k))
    u = np.einsum("si,cia->csa", N, uc)
    bp = np.einsum("si,ci->cs", Nb, bc)
    gB = np.einsum("sik,ci,ckj->csj", dNb, bc, G)
    gB[..., 2] += N2
    y = np.einsum("sk,ck->cs", lam, X[:, :, 1])
    z = np.einsum("sk,ck->cs", lam, X[:, :, 2])
    B = N2 * z + bp
    meas = w[None, :] * wdet[:, None] * qw.sum()
    f = [np.ones_like(B), u[..., 0], u[..., 1], u[..., 2], z, B, gB[..., 2], (u * gB).sum(axis=-1)]
    terms = np.stack([meas * fi for fi in f], axis=-1)
    if mask is not None:
        mk = np.asarray(mask, dtype=bool)
        terms, B, y = terms[mk], B[mk], y[mk]
    return terms.reshape(-1, NCLS), B.ravel(), y.ravel()


class Restated:
    """table (ny + 1, nb + 1, NCLS), S_abs (same shape: sums of |term| per bin), n (ny + 1, nb + 1), dropped, and the flat samples"""

    def __init__(self, terms, B, y, b_edges, y_edges, bins=None):
        self.terms, self.B, self.y = terms, B, y
        self.b_edges, self.y_edges = np.asarray(b_edges, dtype=float), np.asarray(y_edges, dtype=float)
        nb, ny = len(self.b_edges), len(self.y_edges)
        self.finite = np.isfinite(B) & np.isfinite(y)
        self.dropped = int((~self.finite).sum())
        if bins is None:
            bins = np.searchsorted(self.y_edges, y, side="right") * (nb + 1) + np.searchsorted(self.b_edges, B, side="right")
        self.bins = bins
        idx = np.nonzero(self.finite)[0]
        order = idx[np.argsort(bins[idx], kind="stable")]
        sb = bins[order]
        cut = np.nonzero(np.diff(sb))[0] + 1
        nbins = (ny + 1) * (nb + 1)
        table, sabs, n = np.zeros((nbins, NCLS)), np.zeros((nbins, NCLS)), np.zeros(nbins, dtype=np.int64)
        for grp in np.split(order, cut):
            if len(grp):
                t = terms[grp]
                table[bins[grp[0]]] = [math.fsum(t[:, c]) for c in range(NCLS)]
                sabs[bins[grp[0]]] = [math.fsum(np.abs(t[:, c])) for c in range(NCLS)]
                n[bins[grp[0]]] = len(grp)
        self.table, self.S_abs, self.n = table.reshape(ny + 1, nb + 1, NCLS), sabs.reshape(ny + 1, nb + 1, NCLS), n.reshape(ny + 1, nb + 1)
        self.n_total = int(n.sum())
        self.S_total = np.array([math.fsum(np.abs(terms[idx, c])) for c in range(NCLS)])

    def bound(self, S):
        """per entry: n_total eps S_abs_c(total) + n[j, k] 2^-61 S_c"""
        return self.n_total * EPS * self.S_total[None, None, :] + self.n[:, :, None] * 2.0 ** -61 * np.asarray(S)[None, None, :]

    def moved(self):
        """the same samples with ONE of them put into a neighbouring bin"""
        i = np.nonzero(self.finite)[0][len(self.terms) // 2 % max(self.n_total, 1)]
        bins = self.bins.copy()
        nbins = self.n.size
        bins[i] = bins[i] + 1 if bins[i] + 1 < nbins else bins[i] - 1
        return Restated(self.terms, self.B, self.y, self.b_edges, self.y_edges, bins)


def choose_edges(values, n):
    """n strictly increasing edges from the sample values: each the midpoint of the widest gap near a quantile; no sample within
    1e-10 (max - min) of an edge (asserted).  Constant samples: edges around the value, at least 1/4 away."""
    v = np.unique(values[np.isfinite(values)])
    if len(v) == 1:
        return v[0] + (np.arange(n) - n // 2 + 0.25)
    w = max(1, min(16, len(v) // (4 * (n + 1))))
    assert len(v) > 2 * w * (n + 1), (len(v), n)
    edges = []
    for i in range(1, n + 1):
        q = (i * len(v)) // (n + 1)
        lo, hi = max(q - w, 0), min(q + w, len(v) - 1)
        g = lo + int(np.argmax(np.diff(v[lo:hi + 1])))
        edges.append(0.5 * (v[g] + v[g + 1]))
    edges = np.array(edges)
    assert_clear(values, edges)
    return edges


def assert_clear(values, edges):
    v = np.sort(values[np.isfinite(values)])
    edges = np.asarray(edges, dtype=float)
    assert (np.diff(edges) > 0).all()
    tol = 1e-10 * (v[-1] - v[0])
    p = np.searchsorted(v, edges)
    near = np.minimum(np.abs(v[np.minimum(p, len(v) - 1)] - edges), np.abs(v[np.maximum(p - 1, 0)] - edges))
    assert (near > tol).all(), (near.min(), tol)


def _ratio(err, bound):
    """per channel the largest err / bound (a zero bound: 0 when the error is 0 too, else inf)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return r.reshape(-1, NCLS).max(axis=0)


def compare_tables(got, S, ref, label):
    """every entry within the bound of the restatement (the measured errors are printed first) - and the SAME comparison fails once one
    reference sample sits one bin over"""
    bound = ref.bound(S)
    err = np.abs(got - ref.table)
    worst = _ratio(err, bound)
    print(f"classes {label} ({ref.n_total} samples, {ref.n.size} bins, {int((ref.n > 0).sum())} occupied): max err / bound " +
          ", ".join(f"ch{c} {worst[c]:.1e}" for c in range(NCLS)))
    assert got.shape == ref.table.shape and np.isfinite(got).all()
    assert (err <= bound).all(), (label, np.argwhere(err > bound)[:5], err.max())
    if ref.n_total > 1 and ref.n.size > 1:
        bad = ref.moved()
        assert not (np.abs(got - bad.table) <= bad.bound(S)).all(), "the bound does not see one misplaced sample"
    return err, bound


# ---- the checks (the model decides the architecture) ----------------------------------------------------------------------------------
def model_edges(model, level, total, nb=9, ny=7):
    rule = rule_of(model.fe_data.mesh, level)
    N2 = float(model.params.N2) if total else 0.0
    terms, B, y = samples(model, rule, N2)
    return rule, N2, (terms, B, y), choose_edges(B, nb), choose_edges(y, ny)


def check_table(model, label, levels=(1, 2), totals=(True, False)):
    """check 1: 7 x 9 edges, level 1 and 2, total and perturbation, against the restatement"""
    out = {}
    for level in levels:
        for total in totals:
            rule, N2, smp, be, ye = model_edges(model, level, total)
            ref = Restated(*smp, be, ye)
            K = npg.BuoyancyClasses(model, be, ye, level=level)
            assert K.rule[0].shape == rule[0].shape and K.shape == ref.table.shape
            got, dropped, S = K.compute_raw(total)
            assert dropped == 0 == ref.dropped and K.ncells_counted * len(rule[1]) == ref.n_total
            assert (np.abs(S - ref.S_total) <= ref.n_total * EPS * ref.S_total).all()
            out[level, total] = compare_tables(got, S, ref, f"{label} level {level} {'B' if total else 'b-prime'}")
            T = K.compute(total)
            assert np.array_equal(T.raw, got) and np.array_equal(T.volume, got[..., 0])
            assert T.residual_overturning().shape == (len(ye) - 1, len(be) + 1)
            assert np.array_equal(np.isnan(T.mean_depth), got[..., 0] == 0)
    return out


def int_z(mesh, mask=None):
    """int z over the cells from the vertex coordinates: volume x mean vertex z (closed form, math.fsum)"""
    X, _, wdet, _, qw, _, _ = ir.geometry(mesh)
    t = wdet * qw.sum() * X[:, :, 2].mean(axis=1)
    return math.fsum(t if mask is None else t[mask]), math.fsum(np.abs(t if mask is None else t[mask]))


def check_identities(model, label, p1=False):
    """check 2: exact identities against MeshIntegrals on the same state; the bound is the entry bound of ONE bin holding every sample
    (n[j, k] = n_total), the sums over the bins taken with math.fsum"""
    rule, N2, smp, be, ye = model_edges(model, 1, True)
    ref = Restated(*smp, be, ye)
    K = npg.BuoyancyClasses(model, be, ye)
    got, _, S = K.compute_raw()
    raw = npg.MeshIntegrals(model).compute_raw()
    bound = ref.n_total * (EPS * ref.S_total + 2.0 ** -61 * S)
    tot = np.array([math.fsum(got[..., c].ravel()) for c in range(NCLS)])
    zint, _ = int_z(model.fe_data.mesh)
    vals = {"sum ch0 - volume": (tot[0] - raw[0], bound[0]), "sum ch4 - int z": (tot[4] - zint, bound[4])}
    T = K.compute()
    vals["census()[-1] - volume"] = (T.census()[-1] - raw[0], bound[0] + got.shape[0] * got.shape[1] * EPS * raw[0])
    if p1:
        assert model.fe_data.spaces.b_order == 1
        vals["sum ch5 - (N2 int z + int b')"] = (tot[5] - (N2 * zint + raw[1]), bound[5] + EPS * (abs(N2 * zint) + abs(raw[1])))
    print(f"identities {label}: " + ", ".join(f"{k} {abs(e):.2e} (bound {b:.2e})" for k, (e, b) in vals.items()))
    for k, (e, b) in vals.items():
        assert abs(e) <= b, (k, e, b)
    assert (got[..., 0] >= 0).all()
    # every band's class sum equals the table computed with nb = 0
    one, _, S1 = npg.BuoyancyClasses(model, (), ye).compute_raw()
    assert one.shape == (len(ye) + 1, 1, NCLS)
    nband = ref.n.sum(axis=1)
    for j in range(len(ye) + 1):
        for c in range(NCLS):
            e = abs(math.fsum(got[j, :, c]) - one[j, 0, c])
            b = ref.n_total * EPS * ref.S_total[c] + nband[j] * 2.0 ** -61 * (S[c] + S1[c])
            assert e <= b, (j, c, e, b)
    return vals


def check_ties(model):
    """check 3: b = 0 and N2 = 0 make every B exactly 0: b_edges = [0.0] puts the whole volume into class 1, [nextafter(0, 1)] into
    class 0 (the model must have no Dirichlet b)"""
    assert (model.fe_data.tables.b_pos >= 0).all()
    keep = model.b_vec.to_host()
    model.b_vec.upload(np.zeros_like(keep))
    try:
        vol = npg.MeshIntegrals(model).compute_raw()[0]
        nc = model.fe_data.mesh.ncell
        for edge, cls in ((0.0, 1), (np.nextafter(0.0, 1.0), 0)):
            tab, dropped, S = npg.BuoyancyClasses(model, [edge]).compute_raw(total=False)
            assert tab.shape == (1, 2, NCLS) and dropped == 0
            assert (tab[0, 1 - cls] == 0).all(), (edge, tab[0, 1 - cls])
            # 8 samples per cell here, 11 quadrature points per cell in MeshIntegrals, half a unit of 2^-60 vol per sample
            assert abs(tab[0, cls, 0] - vol) <= (8 + 11) * nc * EPS * vol + 8 * nc * 2.0 ** -61 * vol, (edge, tab[0, cls, 0], vol)
            assert tab[0, cls, 5] == 0 and tab[0, cls, 6] == 0 and tab[0, cls, 7] == 0
    finally:
        model.b_vec.upload(keep)


def check_shapes(model, label):
    """check 4: one bin, a deep sparse search, the contention case, ns = 1 and ns = 64, masks"""
    mesh = model.fe_data.mesh
    nc = mesh.ncell
    rule, N2, smp, be, ye = model_edges(model, 1, True)
    raw = npg.MeshIntegrals(model).compute_raw()
    zint, _ = int_z(mesh)
    # nb = ny = 0: one bin, equal to the integrals where the rule is exact (volume, int z)
    ref = Restated(*smp, (), ())
    got, _, S = npg.BuoyancyClasses(model, ()).compute_raw()
    compare_tables(got, S, ref, f"{label} one bin")
    b1 = ref.bound(S)[0, 0]
    assert abs(got[0, 0, 0] - raw[0]) <= b1[0] and abs(got[0, 0, 4] - zint) <= b1[4]
    # nb = 4095, ny = 0: 1365 empty classes below the data, 1365 among it, 1365 above
    B = smp[1]
    R = B.max() - B.min()
    deep = np.concatenate([np.linspace(B.min() - R, B.min() - 0.01 * R, 1365), choose_edges(B, 1365),
                           np.linspace(B.max() + 0.01 * R, B.max() + R, 1365)])
    assert_clear(B, deep)
    ref = Restated(*smp, deep, ())
    got, _, S = npg.BuoyancyClasses(model, deep).compute_raw()
    assert got.shape == (1, 4096, NCLS) and (got[0, :1365] == 0).all() and (got[0, -1365:] == 0).all()
    compare_tables(got, S, ref, f"{label} nb = 4095")
    # one huge class: every sample adds to the same slots
    ref = Restated(*smp, [B.min() - R], ())
    got, _, S = npg.BuoyancyClasses(model, [B.min() - R]).compute_raw()
    assert (got[0, 0] == 0).all() and ref.n[0, 1] == ref.n_total
    compare_tables(got, S, ref, f"{label} one huge class")
    # ns = 1: the cell centroid (level 0)
    r0 = rule_of(mesh, 0)
    assert len(r0[1]) == 1 and np.array_equal(r0[0][0, :mesh.cells.shape[1]], np.full(mesh.cells.shape[1], 1.0 / mesh.cells.shape[1]))
    s0 = samples(model, r0, N2)
    be0, ye0 = choose_edges(s0[1], 9), choose_edges(s0[2], 7)
    got, _, S = npg.BuoyancyClasses(model, be0, ye0, level=0).compute_raw()
    compare_tables(got, S, Restated(*s0, be0, ye0), f"{label} ns = 1")
    # masks: none of the cells; a mask and its complement
    K0 = npg.BuoyancyClasses(model, be, ye, mask=np.zeros(nc, dtype=bool))
    t0, d0, S0 = K0.compute_raw()
    assert K0.ncells_counted == 0 and d0 == 0 and (t0 == 0).all() and (S0 == 0).all()
    mask = np.random.default_rng(SEED).random(nc) < 0.37
    whole, _, S = npg.BuoyancyClasses(model, be, ye).compute_raw()
    P, Q = npg.BuoyancyClasses(model, be, ye, mask=mask), npg.BuoyancyClasses(model, be, ye, mask=~mask)
    (tp, _, Sp), (tq, _, Sq) = P.compute_raw(), Q.compute_raw()
    assert P.ncells_counted + Q.ncells_counted == nc and 0 < P.ncells_counted < nc
    compare_tables(tp, Sp, Restated(*samples(model, rule, N2, mask), be, ye), f"{label} masked")
    ref = Restated(*smp, be, ye)
    assert (np.abs(tp + tq - whole) <= ref.n_total * EPS * ref.S_total + ref.n[:, :, None] * 2.0 ** -61 * (S + Sp + Sq)).all()


def check_determinism(model):
    """check 5: two calls give identical bits; another handle (another level) in between does not disturb the first: the integer table
    is zeroed by every compute"""
    _, _, _, be, ye = model_edges(model, 1, True)
    K = npg.BuoyancyClasses(model, be, ye)
    a, da, Sa = K.compute_raw()
    b, db, Sb = K.compute_raw()
    assert np.array_equal(a, b) and da == db and np.array_equal(Sa, Sb)
    K2 = npg.BuoyancyClasses(model, be, ye, level=2)
    c, _, _ = K2.compute_raw()
    assert not np.array_equal(a, c)
    d, _, Sd = K.compute_raw()
    assert np.array_equal(a, d) and np.array_equal(Sa, Sd)
    assert np.array_equal(c, K2.compute_raw()[0])
    assert np.array_equal(a, npg.BuoyancyClasses(model, be, ye).compute_raw()[0])          # and a new handle gives them again


def check_dropped(model, label):
    """check 6: one NaN in b': compute_raw reports the restatement's count of affected samples, the other bins are untouched within
    the bound, compute raises"""
    rule, N2, _, be, ye = model_edges(model, 1, True)
    keep = model.b_vec.to_host()
    bad = keep.copy()
    bad[len(bad) // 3] = np.nan
    model.b_vec.upload(bad)
    try:
        ref = Restated(*samples(model, rule, N2), be, ye)
        assert 0 < ref.dropped < len(ref.B)
        K = npg.BuoyancyClasses(model, be, ye)
        got, dropped, S = K.compute_raw()
        print(f"dropped samples {label}: {dropped} (restatement {ref.dropped})")
        assert dropped == ref.dropped
        compare_tables(got, S, ref, f"{label} with one NaN in b'")
        try:
            K.compute()
        except FloatingPointError as e:
            assert str(ref.dropped) in str(e)
        else:
            raise AssertionError("compute() did not raise")
    finally:
        model.b_vec.upload(keep)


def check_refusals(model):
    """check 7: every NPG_EINVAL of the C ABI with its message, before anything is launched"""
    lib = L.lib()
    mesh = model.fe_data.mesh
    _, _, _, be, ye = model_edges(model, 1, True)
    K = npg.BuoyancyClasses(model, be, ye)
    ctx = model.arch.ctx
    x, b = model.inversion.solver.x, model.b_vec
    n = int(np.prod(K.shape))
    tab, info = npg.DeviceVector(ctx, n), npg.DeviceVector(ctx, 1 + NCLS)
    tab.fill(-7.0), info.fill(-7.0)
    short_x, short_b = npg.DeviceVector(ctx, x.n - 1), npg.DeviceVector(ctx, b.n + 1)
    short_t, short_i = npg.DeviceVector(ctx, n - 1), npg.DeviceVector(ctx, NCLS)
    N2 = float(model.params.N2)
    for args, word in (((K.h, short_x.h, b.h, N2, tab.h, info.h), "flow vector"), ((K.h, x.h, short_b.h, N2, tab.h, info.h), "buoyancy vector"),
                       ((K.h, x.h, b.h, N2, short_t.h, info.h), "table holds"), ((K.h, x.h, b.h, N2, tab.h, short_i.h), "info holds"),
                       ((K.h, x.h, b.h, np.nan, tab.h, info.h), "N2 is not finite"), ((K.h, x.h, b.h, np.inf, tab.h, info.h), "N2 is not finite"),
                       ((K.h, None, b.h, N2, tab.h, info.h), "NULL"), ((None, x.h, b.h, N2, tab.h, info.h), "NULL")):
        rc = lib.npg_classes_compute(*args)
        msg = lib.npg_last_error().decode()
        assert rc == NPG_EINVAL and word in msg, (rc, msg, word)
        with np.testing.assert_raises(L.DeviceError):
            L.check(rc)
    assert np.array_equal(tab.to_host(), np.full(n, -7.0)) and np.array_equal(info.to_host(), np.full(1 + NCLS, -7.0))   # nothing launched
    X = mesh.geo_coords[mesh.cell_geo]
    y, z = L.as_f64(X[:, :, 1]).copy(), L.as_f64(X[:, :, 2]).copy()
    lam, w = (a.copy() for a in K.rule)
    fe = K.fe.h

    def create(y=y, z=z, lam=lam, w=w, ns=None, ye=ye, be=be, nb=None, fe=fe, out=True):
        h = C.c_void_p()
        a = [None if v is None else L.as_f64(v) for v in (y, z, lam, w, ye, be)]
        p = [None if v is None else L.ptr(v) for v in a]
        rc = lib.npg_classes_create(fe, p[0], p[1], None, p[2], p[3], len(w) if ns is None else ns, p[4], 0 if ye is None else len(ye), p[5],
                                    (3 if be is None else len(be)) if nb is None else nb, C.byref(h) if out else None)
        return rc, lib.npg_last_error().decode(), h

    def nan_at(a, i, j):
        a = a.copy()
        a[i, j] = np.nan
        return a
    w_neg, w_off, lam_off = w.copy(), w.copy(), lam.copy()
    w_neg[1] = 0.0
    w_off[0] += 1e-9
    lam_off[2, 1] += 1e-9
    be_nan, be_dec, ye_eq = be.copy(), be[::-1].copy(), ye.copy()
    be_nan[2] = np.inf
    ye_eq[3] = ye_eq[2]
    for kw, word in ((dict(fe=None), "NULL"), (dict(out=False), "NULL"), (dict(y=None), "cell_y or cell_z"), (dict(z=None), "cell_y or cell_z"),
                     (dict(y=nan_at(y, mesh.ncell // 2, 1)), "cell_y"), (dict(z=nan_at(z, 3, 2)), "cell_z"),
                     (dict(lam=None), "rule_lam or rule_w"), (dict(ns=0), "samples per cell"), (dict(ns=4097), "samples per cell"),
                     (dict(w=w_neg), "is not > 0"), (dict(w=w_off), "weights of the rule sum"), (dict(lam=lam_off), "lam row 2"),
                     (dict(be=be_nan), "b_edges must be finite"), (dict(be=be_dec), "b_edges must be finite and strictly increasing"),
                     (dict(ye=ye_eq), "y_edges must be finite and strictly increasing"), (dict(be=None), "edges missing"),
                     (dict(nb=-1), "negative count"), (dict(ye=np.arange(2048.0), be=np.arange(2048.0)), "2^22 bins")):
        rc, msg, h = create(**kw)
        assert rc == NPG_EINVAL and word in msg and not h.value, (kw.keys(), rc, msg)
    rc, msg, h = create(ye=np.arange(2047.0), be=np.arange(2047.0))                         # (ny + 1)(nb + 1) = 2^22 exactly is legal
    assert rc == 0 and h.value, msg
    lib.npg_classes_destroy(h)
    for bad_edges in ([0.0, np.nan], [1.0, 1.0], [2.0, 1.0]):                               # and through Python
        with np.testing.assert_raises(L.DeviceError):
            npg.BuoyancyClasses(model, bad_edges)
    with np.testing.assert_raises(ValueError):
        npg.BuoyancyClasses(model, be, mask=np.ones(3, dtype=bool))


def check_exports():
    assert NEW <= set(L.declared_symbols())
    for path in (L.HOST_LIB_PATH, L.LIB_PATH):
        lib = C.CDLL(path)
        assert not [s for s in NEW if not hasattr(lib, s)], path


def check_recorder(model, tmp_path):
    """check 8: ClassRecorder as an on_plot hook (a fresh, unstepped model) and its round trip through save"""
    be, ye = np.array([-0.6, -0.3, -0.1]), np.array([-0.2, 0.2])
    ts = model.timestepper
    ts.t_stop = 10 * ts.dt
    rec = npg.ClassRecorder(model, be, ye)
    times = []
    model.on_plot = lambda mdl, t: (times.append(mdl.timestepper.t), rec(mdl, t))
    npg.run(model, n_plot=2, n_steps=6)
    t, raw = rec.as_arrays()
    assert t.shape == (3,) and raw.shape == (3, len(ye) + 1, len(be) + 1, NCLS) and np.array_equal(t, np.array(times)) and np.isfinite(raw).all()
    assert np.array_equal(raw[-1], npg.BuoyancyClasses(model, be, ye).compute_raw()[0])      # the state the hook saw last is the current one
    assert not np.array_equal(raw[0], raw[-1])
    path = os.path.join(str(tmp_path), "classes.npz")
    rec.save(path)
    z = np.load(path)
    assert np.array_equal(z["t"], t) and np.array_equal(z["raw"], raw) and np.array_equal(z["b_edges"], be) and np.array_equal(z["y_edges"], ye)
    assert len(z["channels"]) == NCLS and len(rec.tables()) == 3 and np.array_equal(rec.tables()[0].volume, raw[0, ..., 0])


def check_replicated_layout_refused(model):
    """the replicated layout of distributed.py is refused, as integrals._layout refuses it"""
    from types import SimpleNamespace
    fake = SimpleNamespace(arch=model.arch, fe_data=model.fe_data, partition=object())
    with np.testing.assert_raises(NotImplementedError):
        npg.BuoyancyClasses(fake, [0.0])


# ---- the device table against the host library's ---------------------------------------------------------------------------------------
def host_library_table(model, rule, be, ye, N2, mask=None):
    """(table, dropped, S) of the model's current state through libnupgcm_host.so, loaded BESIDE the library the model runs on and
    driven through its C ABI alone (integrals_ref.host_library_raw)"""
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
    ctx, fe, K = C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(H.npg_ctx_create(0, C.byref(ctx)))
    ok(H.npg_fe_create(ctx, C.byref(d), C.byref(fe)))
    n = (len(ye) + 1) * (len(be) + 1) * NCLS
    vecs = []
    for a in (model.inversion.solver.x.to_host(), model.b_vec.to_host(), np.zeros(n), np.zeros(1 + NCLS)):
        v = C.c_void_p()
        ok(H.npg_vec_create(ctx, len(a), C.byref(v)))
        ok(H.npg_vec_upload(v, L.ptr(L.as_f64(a))))
        vecs.append(v)
    X = m.geo_coords[m.cell_geo]
    y, z = L.as_f64(X[:, :, 1]), L.as_f64(X[:, :, 2])
    if y.shape[1] == 3:
        y, z = (L.as_f64(np.concatenate([a, np.zeros((len(a), 1))], axis=1)) for a in (y, z))
    m8 = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    lam, w, be, ye = (L.as_f64(a) for a in (rule[0], rule[1], be, ye))
    ok(H.npg_classes_create(fe, L.ptr(y), L.ptr(z), None if m8 is None else L.ptr(m8), L.ptr(lam), L.ptr(w), len(w), L.ptr(ye), len(ye),
                            L.ptr(be), len(be), C.byref(K)))
    ok(H.npg_classes_compute(K, vecs[0], vecs[1], float(N2), vecs[2], vecs[3]))
    tab, info = np.empty(n), np.empty(1 + NCLS)
    ok(H.npg_vec_download(vecs[2], L.ptr(tab)))
    ok(H.npg_vec_download(vecs[3], L.ptr(info)))
    H.npg_classes_destroy(K)
    for v in vecs:
        H.npg_vec_destroy(v)
    H.npg_fe_destroy(fe)
    H.npg_ctx_destroy(ctx)
    return tab.reshape(len(ye) + 1, len(be) + 1, NCLS), int(info[0]), info[1:]


def check_device_against_host(model, label, level=1):
    """the device table against the host library's on the same state: the same per-sample arithmetic and the same bins; the pass-1 sums
    differ by their order (so the scales may), the tables by rounding and two quantisations"""
    rule, N2, smp, be, ye = model_edges(model, level, True)
    ref = Restated(*smp, be, ye)
    got, dropped, S = npg.BuoyancyClasses(model, be, ye, level=level).compute_raw()
    host, hdropped, Sh = host_library_table(model, rule, be, ye, N2)
    bound = ref.n_total * EPS * ref.S_total[None, None, :] + ref.n[:, :, None] * 2.0 ** -61 * (S + Sh)[None, None, :]
    err = np.abs(got - host)
    print(f"device vs host library {label}: max err / bound " + ", ".join(f"ch{c} {r:.1e}" for c, r in enumerate(_ratio(err, bound))) +
          f"; bit-identical entries {int((got == host).sum())} of {got.size}")
    assert dropped == hdropped == 0 and (err <= bound).all()
    assert (np.abs(S - Sh) <= ref.n_total * EPS * ref.S_total).all()
    return err, bound
