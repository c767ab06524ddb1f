"""A numpy restatement of the time-dependent surface forcing (nupgcm_amd.forcing) and the checks shared by
tests/test_forcing.py (CPU()) and tests/test_gpu_forcing.py (GPU()).

The restatement is written from the definitions with Mesh.boundary_faces, fe.tri_quadrature_degree4 and fe.p2_tables, as
Mesh.surface_load is: a face finds its cell through a dictionary over the sides of all cells (boundary_ref.locate_faces), its nodes are
its sorted vertices and the edge nodes between them, rows come from the native tables u_pos / b_pos, the functions are evaluated at the
face points here, and the time rule is restated (ref_key_weight).  Every entry of a vector or matrix is kept as the list of its TERMS
alpha area2 w_q piece_q N_k(q) - one per additive piece of the point value ((1 - w) a, w b, gamma (1 - w) a*, gamma w b*), point and
slot - and compared with math.fsum of them.

The bound of an entry is the row's own:  (number of terms in the entry's sum + 8) eps sum |terms|  (Higham eq. 4.4 for the additions
in any order, the 8 for the multiplications that form a term and the scaling by alpha).  Device against host library: the same bound."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

import nupgcm_amd as npg
from nupgcm_amd import _lib as L
from nupgcm_amd import fe as F
from nupgcm_amd.evolution import evolution_parameter
from nupgcm_amd.inversion import device_fe
from tests import boundary_ref as br
from tests import sampling_ref as sr

EPS = np.finfo(np.float64).eps
SEED = 20261020
NEW = {"npg_forcing_create", "npg_forcing_set_series", "npg_forcing_set_gamma", "npg_forcing_apply", "npg_forcing_surface_matrix",
       "npg_forcing_info", "npg_forcing_destroy", "npg_csr_axpy"}
EDGE_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257)

# non-polynomial fields
TAUX = lambda x: np.sin(3.0 * x[..., 0]) * np.exp(x[..., 1])
TAUY = lambda x: np.cos(2.0 * x[..., 0] + x[..., 1]) - 0.3
FLUX = lambda x: 1e-3 * np.tanh(2.0 * x[..., 0]) * np.cos(x[..., 1])
GAMMA = lambda x: 0.5 + np.sin(x[..., 0] + 2.0 * x[..., 1]) ** 2
TARGET = lambda x: np.exp(-x[..., 0] ** 2) * np.sin(3.0 * x[..., 1])
TAUX2 = lambda x: np.cos(5.0 * x[..., 0]) / (1.5 + x[..., 1])
TAUX3 = lambda x: np.exp(np.sin(x[..., 0] - x[..., 1]))
TARGET2 = lambda x: np.cos(x[..., 0] * x[..., 1]) - 0.5
FULL = dict(tau_x=TAUX, tau_y=TAUY, flux=FLUX, gamma=GAMMA, target=TARGET)
# times and a period that are dyadic: the rule's arithmetic is exact, w = 1/2 and the bits of t + n period are reachable
TIMES, PERIOD = [0.0, 0.25, 1.0], 2.0


# ---- the time rule, restated ------------------------------------------------------------------------------------------------------
def ref_key_weight(times, period, t):
    """(key, next key, w) from the definition: hold outside the range, or wrap with s = t0 + (t - t0) mod period"""
    K = len(times)
    if K == 1:
        return 0, 0, 0.0
    if period is None:
        if t <= times[0]:
            return 0, 0, 0.0
        if t >= times[-1]:
            return K - 1, K - 1, 0.0
        s = t
    else:
        s = times[0] + math.fmod(math.fmod(t - times[0], period) + period, period)
    for k in range(K - 1):
        if times[k] <= s < times[k + 1]:
            return k, k + 1, (s - times[k]) / (times[k + 1] - times[k])
    return K - 1, 0, (s - times[-1]) / (times[0] + period - times[-1])


def _fn(v, xq):
    return np.broadcast_to(np.asarray(v(xq), dtype=float), xq.shape[:2]) if callable(v) else np.full(xq.shape[:2], float(v))


def _pieces(v, xq, t):
    """the additive pieces (each (nf, 9)) of the point values of v at time t: v a number, a function, or (times, fields, period)"""
    if isinstance(v, tuple):
        times, fields, period = v
        k, k1, w = ref_key_weight(list(times), period, t)
        return [_fn(fields[k], xq)] if w == 0.0 else [(1.0 - w) * _fn(fields[k], xq), w * _fn(fields[k1], xq)]
    return [_fn(v, xq)]


def as_arg(v):
    return npg.ForcingSeries(*v[:2], period=v[2]) if isinstance(v, tuple) else v


def make(model, spec, mask=None):
    """SurfaceForcing(model, ...) of a spec {tau_x, tau_y, flux, gamma, target}: numbers, functions or (times, fields, period)"""
    kw = {k: as_arg(spec[k]) for k in ("tau_x", "tau_y", "flux") if k in spec}
    if "gamma" in spec:
        kw["restoring"] = (spec["gamma"], as_arg(spec["target"]))
    return npg.SurfaceForcing(model, mask=mask, **kw)


# ---- the restatement --------------------------------------------------------------------------------------------------------------
class Ref:
    """the surface faces sorted by cell, their points, face functions and destination rows"""

    def __init__(self, model):
        fed = model.fe_data
        m = self.mesh = fed.mesh
        faces, fgeo = m.boundary_faces(m.surface_tags, with_geometry=True)
        cell = br.locate_faces(m, faces)[0] if len(faces) else np.zeros(0, dtype=np.int64)
        order = np.argsort(cell, kind="stable")
        self.faces, fgeo = faces[order], fgeo[order]
        X = m.geo_coords[fgeo]
        self.area2 = np.linalg.norm(np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]), axis=1)
        lam, self.w = F.tri_quadrature_degree4()
        self.xq = np.einsum("qk,fki->fqi", lam, X)
        self.N2 = F.p2_tables(lam, F._TRI_EDGE_A, F._TRI_EDGE_B)[0]
        en = np.stack([m.edge_ids(self.faces[:, i], self.faces[:, j]) for (i, j) in ((0, 1), (0, 2), (1, 2))], axis=1)
        nodes2 = np.hstack([self.faces, m.nv + en])
        t = fed.tables
        self.rows_u = [t.u_pos[nodes2, c] for c in (0, 1)]
        self.p2 = fed.spaces.b_order == 2
        self.Nb = self.N2 if self.p2 else lam
        self.rows_b = t.b_pos[nodes2] if self.p2 else t.b_pos[self.faces]
        self.n_inv, self.nb = fed.dofs.nu + fed.dofs.np, fed.dofs.nb
        self.alpha = float(model.params.alpha)

    def load(self, pieces, rows, N, n, mask=None):
        """alpha int (sum of pieces) phi_r over the faces that count: (value, sum |terms|, number of terms) per row, value = fsum"""
        val, sabs, cnt = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int64)
        if not pieces or len(self.faces) == 0:
            return val, sabs, cnt
        P = np.stack(pieces)                                                               # (np, nf, 9)
        terms = self.alpha * np.einsum("f,q,pfq,qk->fkpq", self.area2, self.w, P, N)      # (nf, K, np, 9)
        keep = rows >= 0 if mask is None else (rows >= 0) & np.asarray(mask, dtype=bool)[:, None]
        r, tt = rows[keep], terms[keep].reshape(int(keep.sum()), P.shape[0] * 9)
        order = np.argsort(r, kind="stable")
        r, tt = r[order], tt[order]
        start = np.flatnonzero(np.r_[True, r[1:] != r[:-1]]) if len(r) else np.zeros(0, dtype=np.int64)
        for a, b in zip(start, np.r_[start[1:], len(r)]):
            x = tt[a:b].ravel()
            val[r[a]], sabs[r[a]], cnt[r[a]] = math.fsum(x), math.fsum(np.abs(x)), len(x)
        return val, sabs, cnt

    def vectors(self, spec, t, base, mask=None):
        """(b_inv, bound, touched), (rhs_flux, bound, touched) of the spec at time t; base: the lift (n_inv,)"""
        b, bs, bc = np.zeros(self.n_inv), np.zeros(self.n_inv), np.zeros(self.n_inv, dtype=np.int64)
        for c, name in enumerate(("tau_x", "tau_y")):
            v = spec.get(name, 0.0)
            if isinstance(v, tuple) or callable(v) or float(v) != 0.0:
                x, s, n = self.load(_pieces(v, self.xq, t), self.rows_u[c], self.N2, self.n_inv, mask)
                b, bs, bc = b + x, bs + s, bc + n                                          # (x and y rows are disjoint)
        wind = (np.where(bc > 0, np.array([math.fsum(p) for p in zip(base, b)]), base), (bc + 1 + 8) * EPS * (np.abs(base) + bs), bc > 0)
        pieces = []
        v = spec.get("flux", 0.0)
        if isinstance(v, tuple) or callable(v) or float(v) != 0.0:
            pieces += _pieces(v, self.xq, t)
        if "gamma" in spec:
            g = _fn(spec["gamma"], self.xq)
            pieces += [g * p for p in _pieces(spec["target"], self.xq, t)]
        f, fs, fc = self.load(pieces, self.rows_b, self.Nb, self.nb, mask)
        return wind, (f, (fc + 8) * EPS * fs, fc > 0)

    def matrix(self, gamma, mask=None):
        """S = alpha int gamma phi_i phi_j: (scipy csr of the fsums, csr of the bounds, csr of ones on the touched entries)"""
        g = _fn(gamma, self.xq)
        K = self.Nb.shape[1]
        terms = self.alpha * np.einsum("f,q,fq,qi,qj->fijq", self.area2, self.w, g, self.Nb, self.Nb)       # (nf, K, K, 9)
        ri, cj = np.broadcast_to(self.rows_b[:, :, None], terms.shape[:3]), np.broadcast_to(self.rows_b[:, None, :], terms.shape[:3])
        keep = (ri >= 0) & (cj >= 0)
        if mask is not None:
            keep &= np.asarray(mask, dtype=bool)[:, None, None]
        key, tt = (ri[keep] * self.nb + cj[keep]).astype(np.int64), terms[keep]
        order = np.argsort(key, kind="stable")
        key, tt = key[order], tt[order]
        start = np.flatnonzero(np.r_[True, key[1:] != key[:-1]]) if len(key) else np.zeros(0, dtype=np.int64)
        rr, cc, vv, bb = [], [], [], []
        for a, b in zip(start, np.r_[start[1:], len(key)]):
            x = tt[a:b].ravel()
            rr.append(key[a] // self.nb), cc.append(key[a] % self.nb), vv.append(math.fsum(x))
            bb.append((len(x) + 8) * EPS * math.fsum(np.abs(x)))
        shape = (self.nb, self.nb)
        mk = lambda d: sp.csr_matrix((np.array(d, dtype=float), (np.array(rr, dtype=np.int64), np.array(cc, dtype=np.int64))), shape=shape)
        return mk(vv), mk(bb), mk(np.ones(len(vv))), (np.array(rr, dtype=np.int64), np.array(cc, dtype=np.int64), np.array(vv), np.array(bb))


def report(label, err, bound):
    err, bound = np.asarray(err), np.asarray(bound)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    print(f"forcing {label}: max |err| {err.max(initial=0.0):.2e}, worst |err| / bound {ratio.max(initial=0.0):.3f} over {err.size} entries")
    return ratio


def compare_vectors(model, ref, spec, t, base, label, mask=None):
    """inversion.b and rhs_flux as apply left them against the restatement; rows no forced face touches: the base / 0, exactly"""
    (b, bb, bt), (f, fb, ft) = ref.vectors(spec, t, base, mask)
    got_b, got_f = model.inversion.b.to_host(), model.evolution.rhs_flux.to_host()
    report(f"{label}: wind rows", np.abs(got_b - b)[bt], bb[bt])
    report(f"{label}: flux rows", np.abs(got_f - f)[ft], fb[ft])
    assert (np.abs(got_b - b)[bt] <= bb[bt]).all() and (np.abs(got_f - f)[ft] <= fb[ft]).all(), label
    assert np.array_equal(got_b[~bt], base[~bt]) and (got_f[~ft] == 0.0).all(), label
    return bt, ft


# ---- models -------------------------------------------------------------------------------------------------------------------------
class with_base:
    """a random lift in inversion.b_lift for the duration of a check (the bowl's own is zero), then the model's own again"""

    def __init__(self, model, seed=SEED):
        self.v = model.inversion.b_lift
        self.keep = self.v.to_host()
        self.base = np.random.default_rng(seed).standard_normal(len(self.keep))

    def __enter__(self):
        self.v.upload(self.base)
        return self.base

    def __exit__(self, *a):
        self.v.upload(self.keep)


def light_model(arch, mesh, b_order=2):
    """what SurfaceForcing reads of a model, on a mesh too small for an inversion (the single tetrahedron): a real EvolutionToolkit, and
    vectors in place of the inversion toolkit"""
    from tests import helpers
    prm, frc, _, _, dt, _ = helpers.product_config("bowl_surface_flux")
    fed = npg.FEData(mesh, npg.Spaces(mesh, b_order=b_order))
    ts = npg.BDF2(t_start=0.0, t_stop=dt, dt=dt)
    ev = npg.EvolutionToolkit(arch, fed, prm, frc, ts)
    n = fed.dofs.nu + fed.dofs.np
    inv = SimpleNamespace(b=npg.DeviceVector(arch.ctx, n), b_lift=npg.DeviceVector(arch.ctx, n))
    return SimpleNamespace(arch=arch, params=prm, forcings=frc, fe_data=fed, evolution=ev, inversion=inv, timestepper=ts, step_index=1,
                           tracers=None, surface_forcing=None)


def snapshot(model):
    return model.evolution.rhs_flux.to_host(), model.inversion.b.to_host(), model.evolution.solver.A.to_scipy_csr().data.copy()


def same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- the checks (arch = npg.CPU() or npg.GPU()) ---------------------------------------------------------------------------------------
def check_exports():
    assert {"ForcingSeries", "SurfaceForcing", "series_key_weight"} <= set(npg.__all__)
    assert NEW <= set(L.declared_symbols()) and L.NPG_FRC_NSERIES == 4
    for path in (L.HOST_LIB_PATH, L.LIB_PATH):
        lib = C.CDLL(path)
        assert not [s for s in NEW if not hasattr(lib, s)], path


def check_static(model, label):
    """check 2: SurfaceForcing(model) + apply(any t) = the toolkits' own vectors within the restatement's bound; detach() = their bits"""
    before = snapshot(model)
    f = model.forcings
    spec = dict(tau_x=f.tau_x, tau_y=f.tau_y, flux=f.b_surface_bc.flux if isinstance(f.b_surface_bc, npg.SurfaceFluxBC) else 0.0)
    ref = Ref(model)
    sf = npg.SurfaceForcing(model)
    assert model.surface_forcing is sf and sf.S is None and np.array_equal(sf.faces, ref.faces)
    base = model.inversion.b_lift.to_host()
    for t in (0.37, -1e6):
        sf.apply(model, t)
        (b, bb, bt), (fl, fb, ft) = ref.vectors(spec, t, base)
        got_b, got_f = model.inversion.b.to_host(), model.evolution.rhs_flux.to_host()
        report(f"static {label} t={t}: inversion.b vs the toolkit's", np.abs(got_b - before[1]), bb)
        report(f"static {label} t={t}: rhs_flux vs the toolkit's", np.abs(got_f - before[0]), fb)
        assert (np.abs(got_b - before[1]) <= bb).all() and (np.abs(got_f - before[0]) <= fb).all()
        assert same_bits((model.evolution.solver.A.to_scipy_csr().data,), before[2:])
    sf.detach()
    assert model.surface_forcing is None and same_bits(snapshot(model), before)
    return sf


def check_p1_static(model):
    """check 2, P1: the new path uses the P1 face functions (build_rhs_flux's slice of the P2 load is NOT the P1 load) - against the
    restatement's P1 load"""
    ref = Ref(model)
    assert not ref.p2 and ref.Nb.shape == (9, 3)
    sf = npg.SurfaceForcing(model)
    sf.apply(model, 0.0)
    base = model.inversion.b_lift.to_host()
    compare_vectors(model, ref, dict(flux=model.forcings.b_surface_bc.flux), 0.0, base, "static bowl_surface_flux P1")
    sf.detach()
    return model


def check_loads(model, label, mask=None, spec=FULL, t=0.0):
    """check 3: wind rows, flux rows and the untouched rows against the restatement"""
    before = snapshot(model)
    ref = Ref(model)
    with with_base(model) as base:
        sf = make(model, spec, mask)
        try:
            n = len(ref.faces) if mask is None else int(np.sum(mask))
            assert sf.info()["nface"] == n
            sf.apply(model, t)
            bt, ft = compare_vectors(model, ref, spec, t, base, label, mask)
            first = (model.inversion.b.to_host(), model.evolution.rhs_flux.to_host())
            sf.apply(model, t)                                                             # the same bits on every call
            assert same_bits(first, (model.inversion.b.to_host(), model.evolution.rhs_flux.to_host()))
            if n:
                assert bt.any() and ft.any() and not bt.all() and not ft.all()
        finally:
            sf.detach()
    assert same_bits(snapshot(model), before)
    return bt.sum(), ft.sum()


def masks(nf, seed=SEED):
    rng = np.random.default_rng(seed)
    out = {}
    for n in EDGE_COUNTS:
        mk = np.zeros(nf, dtype=bool)
        mk[rng.permutation(nf)[:n]] = True
        out[n] = mk
    return out


def check_single_tet(arch):
    model = light_model(arch, br.single_tet(arch).fe_data.mesh)
    assert len(Ref(model).faces) == 1
    check_loads(model, "single tetrahedron")
    check_matrix(model, "single tetrahedron")
    check_loads(light_model(arch, model.fe_data.mesh, b_order=1), "single tetrahedron P1")


def check_time_rule_function():
    """the (key, w) rule itself against the restated one, and its edge cases"""
    kw = npg.series_key_weight
    assert kw([3.0], None, -7.0) == (0, 0.0) and kw([3.0], 2.0, 11.0) == (0, 0.0)
    assert kw(TIMES, None, -1.0) == (0, 0.0) and kw(TIMES, None, 0.0) == (0, 0.0) and kw(TIMES, None, 1.0) == (2, 0.0) and kw(TIMES, None, 9.0) == (2, 0.0)
    assert kw(TIMES, None, 0.625) == (1, 0.5) and kw(TIMES, PERIOD, 0.625) == (1, 0.5) and kw(TIMES, PERIOD, 0.25) == (1, 0.0)
    assert kw(TIMES, PERIOD, 1.5) == (2, 0.5) and kw(TIMES, PERIOD, 1.5 + 2000.0) == (2, 0.5) and kw(TIMES, PERIOD, 1.5 - 2000.0) == (2, 0.5)
    assert kw(TIMES, PERIOD, 2.0) == (0, 0.0) and kw(TIMES, PERIOD, -1e-30)[0] in (0, 2)
    rng = np.random.default_rng(SEED)
    for period in (None, PERIOD, 1.0 + 1e-9):
        for t in rng.uniform(-7.0, 9.0, 200):
            k, w = kw(TIMES, period, t)
            rk, _, rw = ref_key_weight(TIMES, period, t)
            assert 0.0 <= w <= 1.0 and k == rk and abs(w - rw) <= 64 * EPS, (period, t, k, w, rk, rw)
    s = npg.ForcingSeries(TIMES, [1.0, 2.0, 3.0], period=PERIOD)
    assert s.key_weight(1.5) == (2, 0.5)


def check_time_rule(model):
    """check 4: a keyframe time has the bits of a one-keyframe forcing; midway = w 1/2; the holds; the wrap; many periods out"""
    ref = Ref(model)
    fields = [TAUX, TAUX2, TAUX3]
    tfields = [TARGET, TARGET2, TARGET]
    with with_base(model) as base:
        def run(spec, t):
            sf = make(model, spec)
            try:
                sf.apply(model, t)
                return model.inversion.b.to_host(), model.evolution.rhs_flux.to_host()
            finally:
                sf.detach()
        ffields = [FLUX, lambda x: 1e-3 * TARGET2(x), lambda x: 1e-3 * TAUX3(x)]
        one = [run(dict(tau_x=fields[k], tau_y=TAUY, flux=ffields[k]), 0.0) for k in range(3)]      # (no restoring here: no factorisation)
        for period, cases in ((None, ((-1.0, 0), (0.0, 0), (0.25, 1), (1.0, 2), (5.0, 2))), (PERIOD, ((0.25, 1), (1.0, 2), (2.0, 0), (-1.75, 1)))):
            spec = dict(tau_x=(TIMES, fields, period), tau_y=TAUY, flux=(TIMES, ffields, period))
            for t, k in cases:
                assert same_bits(run(spec, t), one[k]), (period, t, k)
        spec = dict(tau_x=(TIMES, fields, PERIOD), tau_y=TAUY, flux=FLUX, gamma=GAMMA, target=(TIMES, tfields, PERIOD))
        sf = make(model, spec)
        try:
            for t, (k, k1, w) in ((0.625, (1, 2, 0.5)), (1.5, (2, 0, 0.5)), (0.125, (0, 1, 0.5))):
                assert ref_key_weight(TIMES, PERIOD, t) == (k, k1, w) and sf.series["tau_x"].key_weight(t) == (k, w)
                sf.apply(model, t)
                compare_vectors(model, ref, spec, t, base, f"time rule t={t}: keys {k}, {k1}, w = {w}")
            sf.apply(model, 1.5)
            wrap = (model.inversion.b.to_host(), model.evolution.rhs_flux.to_host())
            assert not np.array_equal(wrap[0], one[2][0]) and not np.array_equal(wrap[0], one[0][0])
            for n in (1, 1000, -1000):
                sf.apply(model, 1.5 + n * PERIOD)
                assert same_bits(wrap, (model.inversion.b.to_host(), model.evolution.rhs_flux.to_host())), n
            tab = sf.tables(1.5)                                                           # the blended tables BoundaryIntegrals would take
            assert np.array_equal(tab["tau_x"], 0.5 * _fn(TAUX3, ref.xq) + 0.5 * _fn(TAUX, ref.xq)) and np.array_equal(tab["flux"], _fn(FLUX, ref.xq))
        finally:
            sf.detach()


def check_matrix(model, label, mask=None, gamma=GAMMA):
    """check 5: S entry by entry, symmetric to the bits, S 1 = the load of gamma (no buoyancy Dirichlet node)"""
    before = snapshot(model)
    ref = Ref(model)
    sf = make(model, dict(gamma=gamma, target=TARGET), mask)
    try:
        S = sf.S.to_scipy_csr()
        val, bnd, touched, (rr, cc, vv, bb) = ref.matrix(gamma, mask)
        got = np.asarray(S[rr, cc]).ravel() if len(rr) else np.zeros(0)
        report(f"{label}: S entries", np.abs(got - vv), bb)
        assert (np.abs(got - vv) <= bb).all()
        assert (S - S.multiply(touched)).count_nonzero() == 0                              # entries no face touches: 0
        assert sf.info()["matrix_entries"] == len(rr)
        D = (S - S.T).tocsr()
        assert D.nnz == 0 or np.abs(D.data).max() == 0.0                                   # symmetric to the bits
        assert (model.fe_data.spaces.b_dof >= 0).all()
        g, gs, gc = ref.load([_fn(gamma, ref.xq)], ref.rows_b, ref.Nb, ref.nb, mask)
        row = np.array([math.fsum(S.data[S.indptr[r]:S.indptr[r + 1]]) for r in range(S.shape[0])])
        rb = np.asarray(bnd.sum(axis=1)).ravel() + (gc + 8) * EPS * gs
        report(f"{label}: S 1 - load(gamma)", np.abs(row - g), rb)
        assert (np.abs(row - g) <= rb).all()
    finally:
        sf.detach()
    assert same_bits(snapshot(model), before)
    return S


def check_axpy(arch, model):
    fed = model.fe_data
    rp, ci, shape = fed.pattern_b()
    rng = np.random.default_rng(SEED)
    x, y = rng.standard_normal(len(ci)), rng.standard_normal(len(ci))
    X = npg.DeviceCSR.from_pattern(arch.ctx, shape[0], shape[1], rp, ci, x)
    Y = npg.DeviceCSR.from_pattern(arch.ctx, shape[0], shape[1], rp, ci, y)
    Y.axpy(0.37, X)
    want = sp.csr_matrix((y, ci, rp), shape=shape) + 0.37 * sp.csr_matrix((x, ci, rp), shape=shape)
    assert np.array_equal(Y.to_scipy_csr().data, y + 0.37 * x) and abs(Y.to_scipy_csr() - want).max() <= 2 * EPS * (np.abs(y) + np.abs(x)).max()
    assert np.array_equal(X.to_scipy_csr().data, x)
    Z = npg.DeviceCSR.from_scipy(arch.ctx, sp.identity(shape[0], format="csr"))
    with np.testing.assert_raises(L.DeviceError):
        Y.axpy(1.0, Z)
    with np.testing.assert_raises(L.DeviceError):
        Y.axpy(1.0, Y)


def matrices(model):
    ev = model.evolution
    return tuple(M.to_scipy_csr() for M in (ev.M, ev.Kh, ev.Kv))


def check_lhs(model, S, dt, theta, label):
    """solver.A = M + theta (Kh + Kv) + dt S entry by entry: 4 terms and the inner sum"""
    M, Kh, Kv = matrices(model)
    A = model.evolution.solver.A.to_scipy_csr()
    want = M.data + theta * Kh.data + theta * Kv.data + dt * S.data
    bound = (5 + 8) * EPS * (np.abs(M.data) + np.abs(theta * Kh.data) + np.abs(theta * Kv.data) + np.abs(dt * S.data))
    report(f"{label}: A - (M + theta (Kh + Kv) + dt S)", np.abs(A.data - want), bound)
    assert (np.abs(A.data - want) <= bound).all() and np.abs(dt * S.data).max() > 1e3 * bound.max()
    return A


def stopping_rule(model, A, label):
    """the evolution solve's own stopping rule sqrt(r' P r) <= atol + rtol rnorm0 (cg.hip, P = 1 / diag A) on the residual recomputed
    from the downloaded A, y and x; a direct solve (CPU()) reports no residual: r is rounding, atol alone.  The recurrence's residual
    and the recomputed one differ by the rounding of forming y - A x, (row length + 8) eps (|A| |x| + |y|), in the same norm."""
    s = model.evolution.solver
    y, x, st = s.y.to_host(), s.x.to_host(), s.workspace.stats
    r = y - A @ x
    P = 1.0 / A.diagonal()
    rn = math.sqrt(float(r @ (P * r)))
    round_ = (np.diff(A.indptr) + 8) * EPS * (abs(A) @ np.abs(x) + np.abs(y))
    slack = math.sqrt(float(round_ @ (P * round_))) * (st["niter"] + 1)
    tol = s.kwargs["atol"] + s.kwargs["rtol"] * st["rnorm0"]
    print(f"forcing {label}: evolution solve ||r||_P {rn:.2e} (reported {st['rnorm']:.2e}) <= {tol:.2e} + {slack:.1e}, {st['niter']} iterations")
    assert st["status"] == 1 and rn <= tol + slack
    return r


def check_one_step_budget(arch, lu):
    """check 6: bowl_surface_flux (no buoyancy Dirichlet tags, N2 = 0) at rest, restoring with constant gamma towards a non-constant b*,
    one evolve.  With r = y - A b1 the discrete budget is  1'M (b1 - b0) - dt (1'rhs_flux - 1'S b1) + 1'r = -theta 1'(Kh + Kv) b1 = 0:
    the columns of the stiffness matrices sum to zero.  (Sign: y - A b1 = r gives M (b1 - b0) + theta K b1 + dt S b1 - dt f = -r, so the
    residual enters with a PLUS for this r - with a converged CG, 1'r = -1e-7 on the GPU, the identity only closes with the plus:
    measured 5e-18.)  y is the element kernels' int b0 phi + dt f, equal to M b0 + dt f up to rounding.
    Bound: every sum is taken with math.fsum over explicit terms, so what is left is the rounding of the DEVICE's sums, each relative
    to the magnitude of its terms: a row of y and an entry of M, Kh, Kv add (cells of the row) x 11 quadrature points products, at
    most N = (longest row of A) x 11 terms; bound = (N + 8) eps T with T = 1'|M| (|b1| + 2 |b0|) + dt (2 1'|f| + 1'|S| |b1|) +
    theta 1'(|Kh| + |Kv|) |b1| + 1'|r|."""
    model = sr.bowl_model(arch, "bowl_surface_flux")
    assert (model.fe_data.spaces.b_dof >= 0).all() and float(model.params.N2) == 0.0
    sf = make(model, dict(gamma=0.8, target=TARGET))
    assert sf.S is not None and model.evolution.S is sf.S
    ts, prm, ev = model.timestepper, model.params, model.evolution
    b0 = model.b_vec.to_host()
    sf.apply(model, ts.t + ts.dt)
    pv = dict(x_prev=model.inversion.solver.x.copy(), b_prev=model.b_vec.copy())
    npg.evolve(model, pv["x_prev"], pv["b_prev"])
    b1, y, f = model.b_vec.to_host(), ev.solver.y.to_host(), ev.rhs_flux.to_host()
    S = sf.S.to_scipy_csr()
    theta = evolution_parameter(prm, npg.BDF1(t_start=0.0, t_stop=1.0, dt=ts.dt))           # the first step's left-hand side
    A = check_lhs(model, S, ts.dt, theta, "one step")
    M, Kh, Kv = matrices(model)
    r = y - A @ b1
    terms = np.concatenate([M.data * (b1 - b0)[M.indices], -ts.dt * f, ts.dt * S.data * b1[S.indices], r])
    gap = abs(math.fsum(terms))
    N = int(np.diff(A.indptr).max()) * 11
    T = (abs(M) @ (np.abs(b1) + 2 * np.abs(b0))).sum() + ts.dt * (2 * np.abs(f).sum() + (abs(S) @ np.abs(b1)).sum()) \
        + theta * ((abs(Kh) + abs(Kv)) @ np.abs(b1)).sum() + np.abs(r).sum()
    bound = (N + 8) * EPS * T
    print(f"forcing one step budget: |1'M (b1 - b0) - dt (1'f - 1'S b1) + 1'r| = {gap:.2e}, bound {bound:.2e}; 1'r = {math.fsum(r):.2e}, "
          f"dt 1'S b1 = {ts.dt * math.fsum(S.data * b1[S.indices]):.2e}, dt 1'f = {ts.dt * math.fsum(f):.2e}")
    assert gap <= bound and abs(ts.dt * math.fsum(S.data * b1[S.indices])) > 1e3 * bound
    if lu:
        rb = (np.diff(A.indptr) + 8) * EPS * (abs(A) @ np.abs(b1) + np.abs(y))
        print(f"forcing one step (LU): max |r| {np.abs(r).max():.2e}, bound {rb.max():.2e}")
        assert ev.solver.workspace.stats.get("direct") and np.abs(r).max() <= rb.max()
    else:
        stopping_rule(model, A, "one step")
    return gap, bound


def loop_spec():
    return dict(tau_x=(TIMES, [TAUX, TAUX2, TAUX3], PERIOD), tau_y=TAUY, flux=FLUX, gamma=GAMMA, target=TARGET)


def check_in_the_loop(arch, scheme):
    """check 7: four steps of run() with a periodic wind series and restoring: after each step the two vectors are the restatement's at
    that step's t_{n+1}, solver.A = M + theta (Kh + Kv) + dt S with that step's dt and theta, and the evolution solve meets its rule"""
    from tests import helpers
    prm, frc, btags, bvals, dt, b0 = helpers.product_config("bowl_surface_flux")
    from nupgcm_amd import channel_basin as cb
    from nupgcm_amd import workloads
    mesh = npg.Mesh(cb.channel_basin_model(0.125, workloads.CB_ALPHA, dz=0.125))           # the small channel basin: seconds per case
    fed = npg.FEData(mesh, npg.Spaces(mesh, u_diri_tags=helpers.U_TAGS, u_diri_vals=helpers.U_VALS, u_diri_masks=helpers.U_MASKS))
    dt = 0.3                                                      # t_{n+1} = 0.3 .. 1.2: every interval of the series, the wrap included
    ts = npg.BDF2(t_start=0.0, t_stop=4 * dt, dt=dt) if scheme == "BDF2" else npg.BDF1(t_start=0.0, t_stop=1e9, dt=dt, adaptive=True)
    model = npg.Model(arch, prm, frc, fed, npg.InversionToolkit(arch, fed, prm, frc), npg.EvolutionToolkit(arch, fed, prm, frc, ts), ts)
    npg.set_b(model, b0)
    spec = loop_spec()
    spec = dict(spec, tau_x=(TIMES, [lambda x, f=f: 1e-2 * f(x) for f in spec["tau_x"][1]], PERIOD), tau_y=lambda x: 1e-2 * TAUY(x))
    ref = Ref(model)
    sf = make(model, spec)
    S = sf.S.to_scipy_csr()
    base = model.inversion.b_lift.to_host()
    dts = []
    for step in range(1, 5):
        t_before = ts.t
        npg.run(model, n_steps=1)
        dts.append(ts.dt)
        t1 = t_before + ts.dt
        assert ts.t == t1
        compare_vectors(model, ref, spec, t1, base, f"{scheme} step {step}, t = {t1:.4f}")
        first = scheme == "BDF2" and step == 1
        theta = evolution_parameter(prm, npg.BDF1(t_start=0.0, t_stop=1.0, dt=ts.dt) if first else ts)
        A = check_lhs(model, S, ts.dt, theta, f"{scheme} step {step}")
        stopping_rule(model, A, f"{scheme} step {step}")
    if scheme != "BDF2":
        assert len(set(dts)) > 1, dts                                                      # the step did adapt
    sf.detach()
    return dts


def check_refusals(arch, model):
    """check 8: each refusal leaves rhs_flux, inversion.b and solver.A bit-identical"""
    import pytest
    before = snapshot(model)
    nf = len(Ref(model).faces)
    fake = lambda **kw: SimpleNamespace(**{**model.__dict__, **kw})
    with pytest.raises(NotImplementedError):
        npg.SurfaceForcing(fake(layout=SimpleNamespace(cell_owner=np.zeros(1))))
    with pytest.raises(NotImplementedError):
        npg.SurfaceForcing(fake(comm=object()))
    with pytest.raises(NotImplementedError):
        npg.SurfaceForcing(fake(partition=object()))
    with pytest.raises(NotImplementedError):
        npg.SurfaceForcing(SimpleNamespace(fe_data=SimpleNamespace(mesh=SimpleNamespace(dim=2))))
    with pytest.raises(ValueError):
        npg.SurfaceForcing(fake(inversion=SimpleNamespace(b=model.inversion.b, solver=model.inversion.solver)))          # no b_lift
    bad = [dict(tau_x=lambda x: np.where(x[..., 0] > 0.2, np.nan, 1.0)), dict(flux=np.inf), dict(restoring=(lambda x: x[..., 0], 1.0)),
           dict(restoring=(np.nan, 1.0)), dict(restoring=(1.0, lambda x: np.inf * x[..., 0])), dict(mask=np.ones(nf + 1, dtype=bool)),
           dict(tau_y=np.zeros((nf, 8))), dict(restoring=1.0)]
    for kw in bad:
        with pytest.raises(ValueError):
            npg.SurfaceForcing(model, **kw)
    for args in (([0.0, 0.0], [1.0, 2.0]), ([1.0, 0.5], [1.0, 2.0]), ([0.0, np.nan], [1.0, 2.0]), ([0.0, 1.0], [1.0])):
        with pytest.raises(ValueError):
            npg.ForcingSeries(*args)
    for period in (1.0, 0.5, -2.0, np.inf):
        with pytest.raises(ValueError):
            npg.ForcingSeries([0.0, 1.0], [1.0, 2.0], period=period)
    # restoring and tracers, in either order
    model.tracers = npg.PassiveTracers(model, [npg.TracerSpec("dye", initial=lambda x: x[..., 2])])
    try:
        with pytest.raises(NotImplementedError):
            npg.SurfaceForcing(model, restoring=(1.0, 0.0))
        sf = npg.SurfaceForcing(model, tau_x=1.0)                                          # without restoring the two get along
        sf.detach()
    finally:
        model.tracers = None
    assert same_bits(snapshot(model), before)
    sf = npg.SurfaceForcing(model, restoring=(1.0, 0.0))
    try:
        with pytest.raises(NotImplementedError):
            npg.PassiveTracers(model, [npg.TracerSpec("dye")])
        with pytest.raises(ValueError):
            npg.SurfaceForcing(model)                                                      # one forcing per model
    finally:
        sf.detach()
    assert same_bits(snapshot(model), before)
    # the C ABI's own checks
    h = sf.h
    key, w = (C.c_int32 * 4)(0, 0, 0, 5), (C.c_double * 4)()
    inv, ev = model.inversion, model.evolution
    lib = L.lib()
    assert lib.npg_forcing_apply(h, key, w, 0.5, inv.b_lift.h, inv.b.h, ev.rhs_flux.h) != 0 and b"key" in lib.npg_last_error()
    key[3], w[3] = 0, 1.5
    assert lib.npg_forcing_apply(h, key, w, 0.5, inv.b_lift.h, inv.b.h, ev.rhs_flux.h) != 0 and b"weight" in lib.npg_last_error()
    w[3] = 0.0
    assert lib.npg_forcing_apply(h, key, w, 0.5, inv.b.h, inv.b.h, ev.rhs_flux.h) != 0
    assert lib.npg_forcing_apply(h, key, w, 0.5, inv.b_lift.h, inv.b.h, inv.b.h) != 0
    assert lib.npg_forcing_apply(h, key, w, 0.5, inv.b_lift.h, inv.b.h, None) != 0
    assert lib.npg_forcing_set_series(h, 7, 1, None) != 0 and lib.npg_forcing_surface_matrix(h, np.nan, sf.S.h) != 0
    tab = np.full((9, sf.info()["nface"]), -1.0)
    assert lib.npg_forcing_set_gamma(h, L.ptr(tab)) != 0 and b"negative" in lib.npg_last_error()
    assert same_bits(snapshot(model), before)


def check_dirichlet_refusal(arch, wind_model):
    """restoring, or a non-zero flux, where a buoyancy Dirichlet node lies on a forced face (bowl_wind pins the surface)"""
    import pytest
    before = snapshot(wind_model)
    for kw in (dict(flux=1.0), dict(restoring=(1.0, 0.0)), dict(flux=npg.ForcingSeries([0.0, 1.0], [0.0, FLUX]))):
        with pytest.raises(ValueError):
            npg.SurfaceForcing(wind_model, **kw)
    assert same_bits(snapshot(wind_model), before)
    sf = npg.SurfaceForcing(wind_model, flux=0.0)                                          # a zero flux is no flux
    assert sf.info()["flux_slots"] == 0
    sf.detach()
    assert same_bits(snapshot(wind_model), before)


# ---- the host library beside the device library ------------------------------------------------------------------------------------------
def host_library(model, sf, t):
    """(inversion.b, rhs_flux, S values or None) of forcing `sf` at time t through libnupgcm_host.so, loaded BESIDE the library the model
    runs on and driven through its C ABI alone, with the face tables and keyframe tables of `sf`"""
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
    q, kidx = sf._keep, sf.kept
    ok(H.npg_forcing_create(fe, len(kidx), L.ptr(q["cell"]), L.ptr(q["local"]), L.ptr(q["area2"]), pat, C.byref(Fh)))
    key, w = (C.c_int32 * 4)(), (C.c_double * 4)()
    for name, tab in sf.key_tables.items():
        i = npg.forcing.SERIES.index(name)
        ok(H.npg_forcing_set_series(Fh, i, len(tab), L.ptr(L.as_f64(np.transpose(tab[:, kidx], (0, 2, 1))))))
        key[i], w[i] = sf.series[name].key_weight(t)
    vecs = []
    for a in (model.inversion.b_lift.to_host(), np.zeros(d.n_inv), np.zeros(d.n_b)):
        v = C.c_void_p()
        ok(H.npg_vec_create(ctx, len(a), C.byref(v)))
        ok(H.npg_vec_upload(v, L.ptr(L.as_f64(a))))
        vecs.append(v)
    Sval = None
    if sf.restoring:
        ok(H.npg_forcing_set_gamma(Fh, L.ptr(L.as_f64(sf.gamma_table[kidx].T))))
        ok(H.npg_forcing_surface_matrix(Fh, sf.alpha, pat))
        Sval = np.empty(len(ci))
        ok(H.npg_csr_download(pat, None, None, L.ptr(Sval)))
    ok(H.npg_forcing_apply(Fh, key, w, sf.alpha, vecs[0], vecs[1], vecs[2]))
    b, f = np.empty(d.n_inv), np.empty(d.n_b)
    ok(H.npg_vec_download(vecs[1], L.ptr(b)))
    ok(H.npg_vec_download(vecs[2], L.ptr(f)))
    H.npg_forcing_destroy(Fh)
    for v in vecs:
        H.npg_vec_destroy(v)
    H.npg_csr_destroy(pat)
    H.npg_fe_destroy(fe)
    H.npg_ctx_destroy(ctx)
    return b, f, Sval


def check_device_against_host(model, label, mask=None, spec=None, t=0.625):
    """the device kernels against the host library on the same tables: the same arithmetic in the same order - within the
    restatement's bound of every row and entry (not a tolerance of its own); prints how many have identical bits"""
    spec = spec or loop_spec()
    ref = Ref(model)
    with with_base(model) as base:
        sf = make(model, spec, mask)
        try:
            sf.apply(model, t)
            got = (model.inversion.b.to_host(), model.evolution.rhs_flux.to_host(), sf.S.to_scipy_csr().data)
            host = host_library(model, sf, t)
        finally:
            sf.detach()
        (_, bb, bt), (_, fb, ft) = ref.vectors(spec, t, base, mask)
    _, bnd, _, _ = ref.matrix(spec["gamma"], mask)
    rp, ci, shape = model.fe_data.pattern_b()
    sb = np.asarray(bnd[np.repeat(np.arange(shape[0]), np.diff(rp)), ci]).ravel()
    for name, g, h, bound in (("wind rows", got[0], host[0], bb), ("flux rows", got[1], host[1], fb), ("S", got[2], host[2], sb)):
        err = np.abs(g - h)
        print(f"device vs host library {label}: {name} worst |err| / bound {np.max(err / np.maximum(bound, 1e-300)):.2e}, identical bits "
              f"{np.mean(g == h):.4f}")
        assert (err <= bound).all(), (label, name)
    assert np.array_equal(got[0][~bt], host[0][~bt]) and np.array_equal(got[1][~ft], host[1][~ft])
