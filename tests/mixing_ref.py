"""A numpy restatement of the diffusivity-weighted (latitude band, buoyancy class) table (BuoyancyClasses.mixing, npg_classes_mixing,
DESIGN.md 20) and the checks shared by tests/test_mixing.py (CPU()) and tests/test_gpu_mixing.py (GPU()).

The restatement is written from the definition: at every sample of the rule (geometry from the cells' own vertices and closed-form
shape functions, as tests/watermass_ref.samples) B = N2 z + b', grad B = grad b' + N2 e_z, kappa_h and kappa_v0 the forcing functions
at the physical sample point, kappa_v = kappa_v0 + kappa_c (1 + np.tanh(-alpha (N2c + d_z b') / N2min)) / 2; the eight terms are
binned with np.searchsorted(side="right") and every bin is summed with math.fsum (watermass_ref.Restated).

Bound per entry (j, k, c):   n_total eps S_abs_c(total)  +  n[j, k] 2^-61 S_c  +  sum_{samples in bin} measure kappa_c dg_s |f_c|
  * the first two terms are DESIGN.md 17's (summation in any order, fixed-point quantisation);
  * the third is the closure's: g = (1 + tanh(-a / N2min)) / 2 has |g'| <= 1 / 2 in its argument, the argument carries the rounding
    of d_z b' = sum_i b_i d_z phi_i (NB products, NB - 1 additions and the lambda-derivative before them: (NB + 2) eps sum |b_i d_z phi_i|)
    amplified by |alpha| / N2min, in the library's evaluation and in this one (2 x 1 / 2), and 8 eps covers the two tanh
    implementations and the arithmetic around them:
        dg_s = (|alpha| / N2min) (NB + 2) eps sum_i |b_i d_z phi_i| + 8 eps
    f_c is the factor that multiplies kappa_v in the channel: (d_z B)^2, d_z B, 1, 1 for channels 2, 3, 4, 7 and 0 for the others;
    the term vanishes when kappa_c = 0.
Edges come from the restatement's own sample values (watermass_ref.choose_edges): no sample within the clearance of an edge, so the
bins agree and the comparison is rounding only.  No case is excluded.  compare_tables' self-check stays: with one reference sample
moved one bin over the same comparison must fail."""
import ctypes as C
import math
import os
from types import SimpleNamespace

import numpy as np

import nupgcm_amd as npg
from nupgcm_amd import _lib as L
from nupgcm_amd import fe as F
from nupgcm_amd.architectures import Context
from nupgcm_amd.inversion import device_fe
from tests import helpers
from tests import integrals_ref as ir
from tests.watermass_ref import EPS, NPG_EINVAL, SEED, Restated, _ratio, assert_clear, choose_edges, compare_tables, rule_of

NMIX = 8
OFF = (0.0, 0.0, 0.0, 0.0)                      # closure = (kappa_c, N2min, alpha, N2c)
NEW = {"npg_classes_set_diffusivity", "npg_classes_mixing"}


# two different, non-constant functions of all three coordinates, both > 0 for z <= 0
def kappa_h_fn(x):
    return 0.5 + 0.3 * np.sin(x[..., 0] + 2.0 * x[..., 1]) + 0.1 * np.cos(3.0 * x[..., 2])


def kappa_v_fn(x):
    return 0.2 + 0.1 * np.cos(2.0 * x[..., 0] - x[..., 1]) * np.exp(2.0 * x[..., 2])


def view(model, kappa_h=kappa_h_fn, kappa_v=kappa_v_fn, conv=None, N2=None):
    """the model's state and mesh under other forcings / another N2, leaving the (shared) model as it is: what BuoyancyClasses reads"""
    f, p = model.forcings, model.params
    frc = npg.Forcings(f.nu, kappa_h, kappa_v, f.tau_x, f.tau_y, f.b_surface_bc,
                       conv_param=conv or npg.ConvectionParameterization(0, 0, False), eddy_param=f.eddy_param)
    prm = p if N2 is None else npg.Parameters(p.eps, p.alpha, p.mu_rho, float(N2), p.f, p.H)
    return SimpleNamespace(arch=model.arch, fe_data=model.fe_data, params=prm, forcings=frc, b_vec=model.b_vec, inversion=model.inversion,
                           step_index=getattr(model, "step_index", 1))


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def _coef(v, xs):
    return np.broadcast_to(np.asarray(v(xs), dtype=float), xs.shape[:2]) if callable(v) else np.full(xs.shape[:2], float(v))


def samples(model, rule, N2, closure=OFF, mask=None):
    """(terms (n, NMIX), B (n,), y (n,), g (n,), cterm (n, NMIX)) of every sample of the cells that count, cell-major: g the closure's
    switch (0 when off), cterm the per-sample closure term of the bound"""
    fed = model.fe_data
    m = fed.mesh
    _, bn = ir.nodal_values(model)
    X, G, wdet, _, qw, ea, eb = ir.geometry(m)
    k = X.shape[1]
    lam, w = rule[0][:, :k], rule[1]
    N, dN = F.p2_tables(lam, ea, eb)
    if fed.spaces.b_order == 2:
        bc, Nb, dNb = bn[m.cell_nodes], N, dN
    else:
        bc, Nb, dNb = bn[m.cells], lam, np.broadcast_to(np.eye(k), (len(w), k, k))
    bp = np.einsum("si,ci->cs", Nb, bc)
    gb = np.einsum("sik,ci,ckj->csj", dNb, bc, G)                       # grad b'
    bz = gb[..., 2]
    gx, gy, gz = gb[..., 0], gb[..., 1], bz + N2
    xs = np.einsum("sk,cki->csi", lam, X)
    y, z = xs[..., 1], xs[..., 2]
    B = N2 * z + bp
    kh, kv0 = _coef(model.forcings.kappa_h, xs), _coef(model.forcings.kappa_v, xs)
    kc, N2min, alpha, N2c = closure
    if kc > 0:
        g = (1.0 + np.tanh(-(alpha * (N2c + bz)) / N2min)) / 2.0
        dzphi = np.einsum("sik,ck->csi", dNb, G[:, :, 2])
        dg = (abs(alpha) / N2min) * (bc.shape[1] + 2) * EPS * np.abs(bc[:, None, :] * dzphi).sum(axis=-1) + 8 * EPS
    else:
        g, dg = np.zeros_like(B), np.zeros_like(B)
    kv = kv0 + kc * g
    meas = w[None, :] * wdet[:, None] * qw.sum()
    gh2 = gx * gx + gy * gy
    one = np.ones_like(B)
    f = [one, kh * gh2, kv * gz * gz, kv * gz, kv, kh, gh2 + gz * gz, kc * g]
    fc = [0 * one, 0 * one, gz * gz, np.abs(gz), one, 0 * one, 0 * one, one]
    terms = np.stack([meas * fi for fi in f], axis=-1)
    cterm = np.stack([meas * kc * dg * fi for fi in fc], axis=-1)
    if mask is not None:
        mk = np.asarray(mask, dtype=bool)
        terms, cterm, B, y, g = terms[mk], cterm[mk], B[mk], y[mk], g[mk]
    return terms.reshape(-1, NMIX), B.ravel(), y.ravel(), g.ravel(), cterm.reshape(-1, NMIX)


class MixRestated(Restated):
    """watermass_ref.Restated with the closure's term of the bound summed per bin"""

    def __init__(self, smp, b_edges, y_edges, bins=None):
        terms, B, y, g, cterm = smp
        super().__init__(terms, B, y, b_edges, y_edges, bins)
        self.smp, self.g = smp, g
        cb = np.zeros((self.n.size, NMIX))
        idx = np.nonzero(self.finite)[0]
        np.add.at(cb, self.bins[idx], cterm[idx])
        self.closure_bound = cb.reshape(self.table.shape) * (1.0 + len(idx) * EPS)          # (the sum of the bound is rounded too)

    def bound(self, S):
        return super().bound(S) + self.closure_bound

    def moved(self):
        return MixRestated(self.smp, self.b_edges, self.y_edges, Restated.moved(self).bins)


def choose_closure(model, rule):
    """(kappa_c, N2min, alpha, N2c) from the restatement's own d_z b': alpha and N2c the model's, N2min the 30 % quantile of |a| over the
    samples, so that |a| / N2min < 1 - g in (0.12, 0.88) - on three tenths of them; kappa_c = 1, several times the background"""
    alpha, N2c = float(model.params.alpha), float(model.params.N2)
    _, bn = ir.nodal_values(model)
    m = model.fe_data.mesh
    X, G, _, _, _, ea, eb = ir.geometry(m)
    k = X.shape[1]
    if model.fe_data.spaces.b_order == 2:
        _, dN = F.p2_tables(rule[0][:, :k], ea, eb)
        bz = np.einsum("sik,ci,ck->cs", dN, bn[m.cell_nodes], G[:, :, 2])
    else:
        bz = np.einsum("ci,ci->c", bn[m.cells], G[:, :, 2])
    a = np.abs(alpha * (N2c + bz)).ravel()
    N2min = float(np.quantile(a[np.isfinite(a)], 0.3))
    assert N2min > 0
    return (1.0, N2min, alpha, N2c)


def model_edges(model, level, total, closure=OFF, nb=9, ny=7):
    rule = rule_of(model.fe_data.mesh, level)
    N2 = float(model.params.N2) if total else 0.0
    smp = samples(model, rule, N2, closure)
    return rule, N2, smp, choose_edges(smp[1], nb), choose_edges(smp[2], ny)


def compare(got, S, ref, label):
    return compare_tables(got, S, ref, "mixing " + label)


# ---- the checks (the model decides the architecture) ----------------------------------------------------------------------------------
def check_table(model, label, levels=(1, 2), totals=(True, False)):
    """check 1: 7 x 9 edges, level 1 and 2, total and perturbation, closure off and on, non-constant kappa, against the restatement"""
    mv = view(model)
    worst = np.zeros(NMIX)
    for level in levels:
        rule = rule_of(mv.fe_data.mesh, level)
        on = choose_closure(mv, rule)
        for total in totals:
            for closure in (OFF, on):
                rule, N2, smp, be, ye = model_edges(mv, level, total, closure)
                assert_clear(smp[1], be), assert_clear(smp[2], ye)
                ref = MixRestated(smp, be, ye)
                if closure is on:
                    spread = np.mean((ref.g > 0.05) & (ref.g < 0.95))
                    assert spread >= 0.1, (label, spread)
                K = npg.BuoyancyClasses(mv, be, ye, level=level)
                assert K.shape == ref.table.shape
                got, dropped, S = K.mixing_raw(total, closure=closure)
                assert dropped == 0 == ref.dropped and K.ncells_counted * len(rule[1]) == ref.n_total
                assert (np.abs(S - ref.S_total) <= ref.n_total * EPS * ref.S_total + ref.closure_bound.sum(axis=(0, 1))).all()
                err, bound = compare(got, S, ref, f"{label} level {level} {'B' if total else 'b-prime'} closure {'on' if closure is on else 'off'}")
                worst = np.maximum(worst, _ratio(err, bound))
                if closure is OFF:
                    assert (got[..., 7] == 0).all()
                else:
                    assert (got[..., 7] > 0).any()
                T = K.mixing(total, closure=closure)
                assert np.array_equal(T.raw, got) and T.diffusive_flux().shape == (len(ye) + 1, len(be) - 1)
                assert T.transformation().shape == (len(ye) + 1, len(be) - 2)
    print(f"mixing {label}: worst err / bound over all cases " + ", ".join(f"ch{c} {worst[c]:.1e}" for c in range(NMIX)))
    return worst


def check_census_tie(model, label):
    """check 2: channel 0 is the census's channel 0, bit for bit, on the same handle, state and `total`"""
    mv = view(model)
    for total in (True, False):
        _, _, _, be, ye = model_edges(mv, 1, total)
        K = npg.BuoyancyClasses(mv, be, ye)
        a, _, Sa = K.compute_raw(total)
        b, _, Sb = K.mixing_raw(total)
        assert np.array_equal(a[..., 0], b[..., 0]) and Sa[0] == Sb[0] and a[..., 0].sum() > 0, (label, total)


def linear_kappa_model(arch):
    """bowl3D h = 0.1, P1 buoyancy, kappa_h and kappa_v LINEAR in x (both > 0 on the bowl), closure off, 3 steps"""
    prm, frc, btags, bvals, dt, b0 = helpers.product_config("bowl_mixing")
    frc.kappa_h = lambda x: 0.5 + 0.2 * x[..., 0] + 0.1 * x[..., 1] + 0.3 * x[..., 2]
    frc.kappa_v = lambda x: 0.3 - 0.1 * x[..., 0] + 0.05 * x[..., 1] + 0.2 * x[..., 2]
    mesh = npg.Mesh(os.path.join(helpers.GOLDEN, "mesh_bowl3D_h0.1.npz"))
    spaces = npg.Spaces(mesh, u_diri_tags=helpers.U_TAGS, u_diri_vals=helpers.U_VALS, u_diri_masks=helpers.U_MASKS, b_diri_tags=btags,
                        b_diri_vals=bvals, b_order=1)
    fed = npg.FEData(mesh, spaces)
    ts = npg.BDF2(t_start=0.0, t_stop=3 * dt, dt=dt)
    model = npg.Model(arch, prm, frc, fed, npg.InversionToolkit(arch, fed, prm, frc), npg.EvolutionToolkit(arch, fed, prm, frc, ts), ts)
    npg.run(model)
    return model


def check_integrals_tie(model, label):
    """check 3: P1 buoyancy and kappa linear in x make the integrands of MeshIntegrals' channels 11 - 13 linear in every cell: the
    sample rule and the engine's quadrature both integrate them exactly, so with total=False the sums over all bins are those channels"""
    assert model.fe_data.spaces.b_order == 1 and not model.forcings.conv_param.is_on
    rule, N2, smp, be, ye = model_edges(model, 1, False)
    ref = MixRestated(smp, be, ye)
    K = npg.BuoyancyClasses(model, be, ye)
    got, dropped, S = K.mixing_raw(total=False)
    assert dropped == 0
    raw = npg.MeshIntegrals(model).compute_raw()
    _, _, sabs = ir.restate_model(model)
    nc = model.fe_data.mesh.ncell
    bound = ref.n_total * (EPS * ref.S_total + 2.0 ** -61 * S)
    tot = np.array([math.fsum(got[..., c].ravel()) for c in range(NMIX)])
    vals = {"ch1 + ch2 - raw[11]": (tot[1] + tot[2] - raw[11], bound[1] + bound[2] + 11 * nc * EPS * sabs[11]),
            "ch3 - raw[12]": (tot[3] - raw[12], bound[3] + 11 * nc * EPS * sabs[12]),
            "ch4 - raw[13]": (tot[4] - raw[13], bound[4] + 11 * nc * EPS * sabs[13])}
    print(f"mixing against MeshIntegrals {label}: " + ", ".join(f"{k} {abs(e):.2e} (bound {b:.2e})" for k, (e, b) in vals.items()))
    for k, (e, b) in vals.items():
        assert abs(e) <= b, (k, e, b)
    assert raw[11] > 0 and raw[13] > 0


def check_closed_forms(model, label):
    """check 4: b' = 0 and B = N2 z (the model must have no Dirichlet b): grad B = N2 e_z exactly, so per bin ch1 = 0, ch2 = N2^2 ch4,
    ch3 = N2 ch4, ch6 = N2^2 ch0 and, with a scalar kappa_v0 = k, ch4 = k ch0; the closure's limits on the same state"""
    assert (model.fe_data.tables.b_pos >= 0).all()
    N2, k0 = 1.75, 0.0625
    mv = view(model, kappa_h=kappa_h_fn, kappa_v=k0, N2=N2)
    keep = model.b_vec.to_host()
    model.b_vec.upload(np.zeros_like(keep))
    try:
        rule, _, smp, be, ye = model_edges(mv, 1, True)
        ref = MixRestated(smp, be, ye)
        K = npg.BuoyancyClasses(mv, be, ye)
        off, dropped, S = K.mixing_raw()
        assert dropped == 0
        bound = ref.bound(S)
        compare(off, S, ref, f"{label} b' = 0")
        assert (off[..., 1] == 0).all() and (off[..., 7] == 0).all()

        def within(c, value, factor, cv):
            """|ch_c - factor ch_cv| within the two entries' bounds (the second scaled by the factor)"""
            e, b = np.abs(off[..., c] - factor * value), bound[..., c] + abs(factor) * bound[..., cv] + EPS * np.abs(off[..., c])
            assert (e <= b).all(), (c, e.max(), b[e > b])
        within(2, off[..., 4], N2 * N2, 4)
        within(3, off[..., 4], N2, 4)
        within(6, off[..., 0], N2 * N2, 0)
        within(4, off[..., 0], k0, 0)
        # N2min = 1e300: tanh(-a / N2min) rounds away, kappa_v = kappa_v0 + kappa_c / 2 exactly: ch7 = (kappa_c / 2) ch0
        kc = 0.5
        big, _, Sb = K.mixing_raw(closure=(kc, 1e300, 0.5, 1.0))
        e = np.abs(big[..., 7] - 0.5 * kc * big[..., 0])
        b = ref.n_total * EPS * Sb[7] + ref.n * 2.0 ** -61 * (Sb[7] + 0.5 * kc * Sb[0]) + EPS * np.abs(big[..., 7])
        assert (e <= b).all() and (big[..., 7] > 0).any(), (e.max(), b.min())
        # N2min = 1e-6 and N2c = 1 (b' = 0: a = alpha): tanh saturates to -1, the closure adds exactly 0
        sat, _, Ss = K.mixing_raw(closure=(kc, 1e-6, 0.5, 1.0))
        assert (sat[..., 7] == 0.0).all() and Ss[7] == 0.0
        assert np.array_equal(sat[..., :7], off[..., :7]) and np.array_equal(Ss[:7], S[:7])
    finally:
        model.b_vec.upload(keep)


def check_scalars_equal_tables(model):
    """check 5: NULL + scalar gives the bits of a constant table; a second set_diffusivity replaces the first; the closure's
    arguments taken from model.forcings give the bits of the same arguments passed explicitly"""
    mv = view(model)
    _, _, _, be, ye = model_edges(mv, 1, True)
    K = npg.BuoyancyClasses(mv, be, ye)
    first, _, S1 = K.mixing_raw()                                        # the forcings' functions, evaluated on first use
    K.set_diffusivity(0.375, 0.0625)
    sc, _, Ssc = K.mixing_raw()
    K.set_diffusivity(lambda x: np.full(x.shape[:-1], 0.375), lambda x: np.full(x.shape[:-1], 0.0625))
    tb, _, Stb = K.mixing_raw()
    assert np.array_equal(sc, tb) and np.array_equal(Ssc, Stb) and not np.array_equal(sc, first)
    K.set_diffusivity(0.375, lambda x: np.full(x.shape[:-1], 0.0625))    # one of each
    assert np.array_equal(K.mixing_raw()[0], sc)
    K.set_diffusivity()                                                  # back to the first values: the first bits
    again, _, S2 = K.mixing_raw()
    assert np.array_equal(again, first) and np.array_equal(S1, S2)
    on = choose_closure(mv, K.rule)
    conv = npg.ConvectionParameterization(on[0], on[1], True)
    a = npg.BuoyancyClasses(view(model, conv=conv), be, ye).mixing_raw()[0]
    assert np.array_equal(a, K.mixing_raw(closure=on)[0]) and not np.array_equal(a, first)


def check_determinism(model):
    """check 6: two calls give the same bits; the census and the mixing table interleaved on ONE handle give each its stand-alone bits
    (both zero the integer table on the stream); a fresh handle gives them again"""
    mv = view(model)
    on = choose_closure(mv, rule_of(mv.fe_data.mesh, 1))
    _, _, _, be, ye = model_edges(mv, 1, True, on)
    Kc, Km = npg.BuoyancyClasses(mv, be, ye), npg.BuoyancyClasses(mv, be, ye)
    c0, _, Sc0 = Kc.compute_raw()
    m0, _, Sm0 = Km.mixing_raw(closure=on)
    m1, _, Sm1 = Km.mixing_raw(closure=on)
    assert np.array_equal(m0, m1) and np.array_equal(Sm0, Sm1)
    K = npg.BuoyancyClasses(mv, be, ye)
    for _ in range(2):
        c, _, Sc = K.compute_raw()
        m, _, Sm = K.mixing_raw(closure=on)
        assert np.array_equal(c, c0) and np.array_equal(Sc, Sc0) and np.array_equal(m, m0) and np.array_equal(Sm, Sm0)
    assert not np.array_equal(c0, m0)
    assert np.array_equal(npg.BuoyancyClasses(mv, be, ye).mixing_raw(closure=on)[0], m0)


def check_dropped(model, label):
    """check 7: one NaN in b': mixing_raw reports the restatement's count of affected samples, the other bins stay within the bound,
    mixing() raises"""
    mv = view(model)
    rule = rule_of(mv.fe_data.mesh, 1)
    on = choose_closure(mv, rule)
    N2 = float(mv.params.N2)
    _, _, _, be, ye = model_edges(mv, 1, True, on)
    keep = model.b_vec.to_host()
    bad = keep.copy()
    bad[len(bad) // 3] = np.nan
    model.b_vec.upload(bad)
    try:
        for closure in (OFF, on):
            ref = MixRestated(samples(mv, rule, N2, closure), be, ye)
            assert 0 < ref.dropped < len(ref.B)
            K = npg.BuoyancyClasses(mv, be, ye)
            got, dropped, S = K.mixing_raw(closure=closure)
            print(f"mixing dropped samples {label}: {dropped} (restatement {ref.dropped})")
            assert dropped == ref.dropped
            compare(got, S, ref, f"{label} with one NaN in b'")
            try:
                K.mixing(closure=closure)
            except FloatingPointError as e:
                assert str(ref.dropped) in str(e)
            else:
                raise AssertionError("mixing() did not raise")
    finally:
        model.b_vec.upload(keep)


def check_shapes(model, label):
    """check 8: nb = 0, ny = 0, ns = 1, an empty mask, a mask and its complement"""
    mv = view(model)
    mesh = mv.fe_data.mesh
    nc = mesh.ncell
    rule, N2, smp, be, ye = model_edges(mv, 1, True)
    on = choose_closure(mv, rule)
    for b_e, y_e, tag in (((), ye, "nb = 0"), (be, (), "ny = 0"), ((), (), "one bin")):
        for closure in (OFF, on):
            ref = MixRestated(samples(mv, rule, N2, closure), b_e, y_e)
            K = npg.BuoyancyClasses(mv, b_e, y_e)
            got, _, S = K.mixing_raw(closure=closure)
            assert got.shape == (len(y_e) + 1, len(b_e) + 1, NMIX)
            compare(got, S, ref, f"{label} {tag}")
            T = K.mixing(closure=closure)
            if len(b_e) == 0:
                assert T.diffusive_flux().shape == (len(y_e) + 1, 0) and T.transformation().shape == (len(y_e) + 1, 0)
    r0 = rule_of(mesh, 0)                                                # ns = 1: the cell centroid
    s0 = samples(mv, r0, N2, on)
    be0, ye0 = choose_edges(s0[1], 9), choose_edges(s0[2], 7)
    got, _, S = npg.BuoyancyClasses(mv, be0, ye0, level=0).mixing_raw(closure=on)
    compare(got, S, MixRestated(s0, be0, ye0), f"{label} ns = 1")
    K0 = npg.BuoyancyClasses(mv, be, ye, mask=np.zeros(nc, dtype=bool))
    t0, d0, S0 = K0.mixing_raw(closure=on)
    assert K0.ncells_counted == 0 and d0 == 0 and (t0 == 0).all() and (S0 == 0).all()
    mask = np.random.default_rng(SEED).random(nc) < 0.37
    whole, _, S = npg.BuoyancyClasses(mv, be, ye).mixing_raw(closure=on)
    P, Q = npg.BuoyancyClasses(mv, be, ye, mask=mask), npg.BuoyancyClasses(mv, be, ye, mask=~mask)
    (tp, _, Sp), (tq, _, Sq) = P.mixing_raw(closure=on), Q.mixing_raw(closure=on)
    assert P.ncells_counted + Q.ncells_counted == nc and 0 < P.ncells_counted < nc
    compare(tp, Sp, MixRestated(samples(mv, rule, N2, on, mask), be, ye), f"{label} masked")
    ref = MixRestated(samples(mv, rule, N2, on), be, ye)
    # the same samples evaluated by the same code in other handles: the terms are the same bits, only the quantisations differ
    assert (np.abs(tp + tq - whole) <= ref.n_total * EPS * ref.S_total + ref.n[:, :, None] * 2.0 ** -61 * (S + Sp + Sq)).all()


def check_refusals(model):
    """check 9: every NPG_EINVAL of the two entry points with its message, before anything is launched"""
    lib = L.lib()
    mv = view(model)
    _, _, _, be, ye = model_edges(mv, 1, True)
    K = npg.BuoyancyClasses(mv, be, ye)
    ctx = model.arch.ctx
    b = model.b_vec
    n = int(np.prod(K.shape))
    tab, info = npg.DeviceVector(ctx, n), npg.DeviceVector(ctx, 1 + NMIX)
    tab.fill(-7.0), info.fill(-7.0)
    N2 = float(model.params.N2)
    good = (1.0, 0.5, 0.5, 1.0)
    rc = lib.npg_classes_mixing(K.h, b.h, N2, *good, tab.h, info.h)                     # before set_diffusivity
    msg = lib.npg_last_error().decode()
    assert rc == NPG_EINVAL and "npg_classes_set_diffusivity first" in msg, (rc, msg)
    nc, ns = model.fe_data.mesh.ncell, len(K.rule[1])
    full = np.full((nc, ns), 0.25)

    def spoiled(v):
        a = full.copy()
        a[nc // 2, ns - 1] = v
        return a
    for args, word in (((None, None, 1.0, None, 1.0), "NULL"), ((K.h, None, np.nan, None, 1.0), "scalar kappa_h"),
                       ((K.h, None, -1.0, None, 1.0), "scalar kappa_h"), ((K.h, None, 1.0, None, np.inf), "scalar kappa_v0"),
                       ((K.h, None, 1.0, None, -1e-300), "scalar kappa_v0"), ((K.h, spoiled(np.nan), 1.0, None, 1.0), f"kappa_h[{nc // 2}][{ns - 1}]"),
                       ((K.h, spoiled(-0.5), 1.0, None, 1.0), f"kappa_h[{nc // 2}][{ns - 1}]"),
                       ((K.h, None, 1.0, spoiled(np.inf), 1.0), f"kappa_v0[{nc // 2}][{ns - 1}]"),
                       ((K.h, full, -1.0, spoiled(-1.0), 1.0), f"kappa_v0[{nc // 2}][{ns - 1}]")):
        a = [None if isinstance(v, type(None)) else (L.ptr(v) if isinstance(v, np.ndarray) else v) for v in args]
        rc = lib.npg_classes_set_diffusivity(*a)
        msg = lib.npg_last_error().decode()
        assert rc == NPG_EINVAL and word in msg, (rc, msg, word)
    rc = lib.npg_classes_mixing(K.h, b.h, N2, *good, tab.h, info.h)                     # a refused set_diffusivity set nothing
    assert rc == NPG_EINVAL and "npg_classes_set_diffusivity first" in lib.npg_last_error().decode()
    assert lib.npg_classes_set_diffusivity(K.h, L.ptr(full), -1.0, None, 0.5) == 0      # (the scalar beside a table is not read)
    short_b, short_t, short_i = npg.DeviceVector(ctx, b.n + 1), npg.DeviceVector(ctx, n - 1), npg.DeviceVector(ctx, NMIX)
    other_ctx = Context(ctx.device)                                                     # a second context of the same library
    other = npg.DeviceVector(other_ctx, b.n)
    cases = [((K.h, short_b.h, N2, *good, tab.h, info.h), "buoyancy vector"), ((K.h, b.h, N2, *good, short_t.h, info.h), "table holds"),
             ((K.h, b.h, N2, *good, tab.h, short_i.h), "info holds"), ((None, b.h, N2, *good, tab.h, info.h), "NULL"),
             ((K.h, None, N2, *good, tab.h, info.h), "NULL"), ((K.h, b.h, N2, *good, None, info.h), "NULL"),
             ((K.h, b.h, N2, *good, tab.h, None), "NULL"),
             ((K.h, b.h, np.nan, *good, tab.h, info.h), "N2 must be finite"), ((K.h, b.h, -1.0, *good, tab.h, info.h), "N2 must be finite"),
             ((K.h, b.h, N2, np.inf, 0.5, 0.5, 1.0, tab.h, info.h), "kappa_c must be finite"),
             ((K.h, b.h, N2, -1.0, 0.5, 0.5, 1.0, tab.h, info.h), "kappa_c must be finite"),
             ((K.h, b.h, N2, 1.0, 0.5, np.nan, 1.0, tab.h, info.h), "alpha must be finite"),
             ((K.h, b.h, N2, 1.0, 0.5, -0.5, 1.0, tab.h, info.h), "alpha must be finite"),
             ((K.h, b.h, N2, 1.0, 0.5, 0.5, np.inf, tab.h, info.h), "N2c must be finite"),
             ((K.h, b.h, N2, 1.0, 0.5, 0.5, -1.0, tab.h, info.h), "N2c must be finite"),
             ((K.h, b.h, N2, 1.0, 0.0, 0.5, 1.0, tab.h, info.h), "needs N2min > 0"),
             ((K.h, b.h, N2, 1.0, -1.0, 0.5, 1.0, tab.h, info.h), "needs N2min > 0"),
             ((K.h, b.h, N2, 1.0, np.nan, 0.5, 1.0, tab.h, info.h), "needs N2min > 0")]
    cases.append(((K.h, other.h, N2, *good, tab.h, info.h), "different contexts"))
    for args, word in cases:
        rc = lib.npg_classes_mixing(*args)
        msg = lib.npg_last_error().decode()
        assert rc == NPG_EINVAL and word in msg, (rc, msg, word)
        with np.testing.assert_raises(L.DeviceError):
            L.check(rc)
    assert np.array_equal(tab.to_host(), np.full(n, -7.0)) and np.array_equal(info.to_host(), np.full(1 + NMIX, -7.0))   # nothing launched
    assert lib.npg_classes_mixing(K.h, b.h, N2, 0.0, np.nan, 0.5, 1.0, tab.h, info.h) == 0                # closure off: N2min is not read
    assert np.isfinite(tab.to_host()).all()
    with np.testing.assert_raises(L.DeviceError):
        K.set_diffusivity(-1.0, 1.0)
    with np.testing.assert_raises(L.DeviceError):
        K.set_diffusivity(1.0, lambda x: -np.ones(x.shape[:-1]))


def check_exports():
    assert NEW <= set(L.declared_symbols()) and L.NPG_NMIX == NMIX == npg.watermass.NMIX == len(npg.watermass.MIXING_CHANNELS)
    for path in (L.HOST_LIB_PATH, L.LIB_PATH):
        lib = C.CDLL(path)
        assert not [s for s in NEW if not hasattr(lib, s)], path


def check_mixing_table_arithmetic():
    """check 10: MixingTable on a hand-made raw table: ny = 0, nb = 3 (classes 0 .. 3, interior 1 and 2), edges 1, 2, 4"""
    be = np.array([1.0, 2.0, 4.0])
    raw = np.zeros((1, 4, NMIX))
    #            ch0  ch1  ch2  ch3  ch4  ch5  ch6  ch7
    raw[0, 0] = [2.0, 1.0, 3.0, 0.5, 4.0, 6.0, 8.0, 1.0]
    raw[0, 1] = [4.0, 2.0, 4.0, 0.5, 2.0, 1.0, 3.0, 0.0]
    raw[0, 2] = [8.0, 5.0, 5.0, 0.5, 4.0, 2.0, 0.0, 3.0]
    raw[0, 3] = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    T = npg.MixingTable(raw, be, np.zeros(0))
    assert np.array_equal(T.volume, [[2.0, 4.0, 8.0, 0.0]]) and np.array_equal(T.dissipation, [[4.0, 6.0, 10.0, 0.0]])
    assert np.array_equal(T.diffusive_flux(), [[6.0 / 1.0, 10.0 / 2.0]])                   # interior classes 1 (width 1) and 2 (width 2)
    assert np.array_equal(T.transformation(), [[(5.0 - 6.0) / 1.5]])                       # at the edge 2 between them
    np.testing.assert_array_equal(T.effective_diffusivity, [[0.5, 2.0, np.nan, np.nan]])
    np.testing.assert_array_equal(T.mean_kappa_v, [[2.0, 0.5, 0.5, np.nan]])
    np.testing.assert_array_equal(T.mean_kappa_h, [[3.0, 0.25, 0.25, np.nan]])
    np.testing.assert_array_equal(T.convective_fraction, [[0.25, 0.0, 0.75, np.nan]])
    for nb in (0, 1):                                                                      # nb < 2: no interior class
        T = npg.MixingTable(raw[:, :nb + 1], be[:nb], np.zeros(0))
        assert T.diffusive_flux().shape == (1, 0) and T.transformation().shape == (1, 0)
    T = npg.MixingTable(raw[:, :3], be[:2], np.zeros(0))                                   # nb = 2: one interior class, no edge between two
    assert np.array_equal(T.diffusive_flux(), [[6.0]]) and T.transformation().shape == (1, 0)
    assert "MixingTable" in repr(T)


def check_recorder(make_model, tmp_path):
    """check 11: ClassRecorder(mixing=True) as on_plot through 2 steps of run(); mixing=False writes today's keys"""
    be, ye = np.array([-0.6, -0.3, -0.1]), np.array([-0.2, 0.2])
    keys = {}
    for mixing in (True, False):
        model = make_model()
        ts = model.timestepper
        ts.t_stop = 10 * ts.dt
        rec = npg.ClassRecorder(model, be, ye, mixing=mixing)
        model.on_plot = rec
        npg.run(model, n_plot=1, n_steps=2)
        t, raw = rec.as_arrays()
        assert t.shape == (2,) and raw.shape == (2, len(ye) + 1, len(be) + 1, NMIX)
        path = os.path.join(str(tmp_path), f"classes_{mixing}.npz")
        rec.save(path)
        z = np.load(path)
        keys[mixing] = set(z.files)
        assert np.array_equal(z["raw"], raw)
        if mixing:
            assert z["mixing_raw"].shape == raw.shape and len(z["mixing_channels"]) == NMIX and np.isfinite(z["mixing_raw"]).all()
            assert np.array_equal(z["mixing_raw"][..., 0], raw[..., 0])                                      # the census again
            assert np.array_equal(z["mixing_raw"][-1], npg.BuoyancyClasses(model, be, ye).mixing_raw()[0])   # the current state
            assert not np.array_equal(z["mixing_raw"][0], z["mixing_raw"][-1])
            assert len(rec.mixing_tables()) == 2 and np.array_equal(rec.mixing_tables()[1].raw, z["mixing_raw"][1])
        else:
            assert rec.mixing_raw == []
    assert keys[False] == {"t", "raw", "b_edges", "y_edges", "channels"} and keys[True] == keys[False] | {"mixing_raw", "mixing_channels"}


# ---- the device table against the host library's ---------------------------------------------------------------------------------------
def host_library_mixing(model, rule, be, ye, N2, closure):
    """(table, dropped, S) of the model's current state through libnupgcm_host.so, loaded BESIDE the library the model runs on and
    driven through its C ABI alone (as watermass_ref.host_library_table)"""
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
    n = (len(ye) + 1) * (len(be) + 1) * NMIX
    vecs = []
    for a in (model.b_vec.to_host(), np.zeros(n), np.zeros(1 + NMIX)):
        v = C.c_void_p()
        ok(H.npg_vec_create(ctx, len(a), C.byref(v)))
        ok(H.npg_vec_upload(v, L.ptr(L.as_f64(a))))
        vecs.append(v)
    X = m.geo_coords[m.cell_geo]
    y, z = L.as_f64(X[:, :, 1]), L.as_f64(X[:, :, 2])
    if y.shape[1] == 3:
        y, z = (L.as_f64(np.concatenate([a, np.zeros((len(a), 1))], axis=1)) for a in (y, z))
    lam, w, be, ye = (L.as_f64(a) for a in (rule[0], rule[1], be, ye))
    ok(H.npg_classes_create(fe, L.ptr(y), L.ptr(z), None, L.ptr(lam), L.ptr(w), len(w), L.ptr(ye), len(ye), L.ptr(be), len(be), C.byref(K)))
    xs = np.einsum("sk,cki->csi", lam[:, :X.shape[1]], X)
    kh, kv0 = L.as_f64(_coef(model.forcings.kappa_h, xs)), L.as_f64(_coef(model.forcings.kappa_v, xs))
    ok(H.npg_classes_set_diffusivity(K, L.ptr(kh), 0.0, L.ptr(kv0), 0.0))
    ok(H.npg_classes_mixing(K, vecs[0], float(N2), *(float(v) for v in closure), vecs[1], vecs[2]))
    tab, info = np.empty(n), np.empty(1 + NMIX)
    ok(H.npg_vec_download(vecs[1], L.ptr(tab)))
    ok(H.npg_vec_download(vecs[2], L.ptr(info)))
    H.npg_classes_destroy(K)
    for v in vecs:
        H.npg_vec_destroy(v)
    H.npg_fe_destroy(fe)
    H.npg_ctx_destroy(ctx)
    return tab.reshape(len(ye) + 1, len(be) + 1, NMIX), int(info[0]), info[1:]


def check_device_against_host(model, label, level=1):
    """check 12: the device table against the host library's on the same state.  Closure off: the same per-sample arithmetic and the
    same bins - rounding of the sums and two quantisations.  Closure on: the closure's term of the bound as well (two tanh)."""
    mv = view(model)
    on = choose_closure(mv, rule_of(mv.fe_data.mesh, level))
    for closure in (OFF, on):
        rule, N2, smp, be, ye = model_edges(mv, level, True, closure)
        ref = MixRestated(smp, be, ye)
        got, dropped, S = npg.BuoyancyClasses(mv, be, ye, level=level).mixing_raw(closure=closure)
        host, hdropped, Sh = host_library_mixing(mv, rule, be, ye, N2, closure)
        bound = ref.n_total * EPS * ref.S_total[None, None, :] + ref.n[:, :, None] * 2.0 ** -61 * (S + Sh)[None, None, :] + ref.closure_bound
        err = np.abs(got - host)
        print(f"mixing device vs host library {label} closure {'on' if closure is on else 'off'}: max err / bound " +
              ", ".join(f"ch{c} {r:.1e}" for c, r in enumerate(_ratio(err, bound))) +
              f"; bit-identical entries {int((got == host).sum())} of {got.size}")
        assert dropped == hdropped == 0 and (err <= bound).all()
        assert (np.abs(S - Sh) <= ref.n_total * EPS * ref.S_total + ref.closure_bound.sum(axis=(0, 1))).all()
