"""A numpy restatement of the tangent of the advection load (npg_fe_tangent_rhs, csrc/tangent_core.h), oracles for the
linearised model (nupgcm_amd.linearized) and the checks shared by tests/test_linearized.py (CPU()) and tests/test_gpu_linearized.py
(GPU()).

The restatement is a per-cell einsum over the engine's OWN tables (DeviceFE._keep: what npg_fe_create was given), term by term as
tangent_core.h orders them, in extended precision.  With W = w_q |J|

    T_i = sum_{cells} [ sum_q W (u_base . grad db) phi_i  +  sum_q W (du . grad b_base + du_z N2) phi_i ]

Bound.  A recursive sum of n terms differs from the exact one by at most (n - 1) eps sum |t| in any order (Higham, eq. 4.4), and the
relative errors of the factors of a product add.  One entry of T is a sum over the row's cells (len_r), over the two terms and the
quadrature points (2 nq), of products (3 roundings) of a three-term dot product with N2 (4) of a velocity (10 terms) and a gradient
(nl terms, then 4): bound_r = (10 + nl + 4 + 4 + 3 + 2 nq + len_r) eps S_abs,r with S_abs the same expression over absolute values -
derived, not tuned.  Either library must stay within twice that of the restatement; the device must give the bits of the host library.

The oracles of the operator use entry points that existed before it: F(b) through npg_fe_evolution_rhs and the model's own inversion
(check 3), scipy's eigsh and eig (checks 5, 6)."""
import copy
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse.linalg as spla

import nupgcm_amd as npg
from nupgcm_amd import _lib as L
from nupgcm_amd.inversion import device_fe
from nupgcm_amd.iterative_solvers import LU, iterative_solve
from tests import helpers
from tests import redi_ref as rr

EPS = np.finfo(np.float64).eps
LD = np.longdouble
SEED = 20261021
NEW = {"npg_fe_tangent_rhs"}
FLAT = "mesh_bowl2D_h0.1"


def report(label, err, bound):
    err, bound = np.asarray(err, dtype=float).ravel(), np.asarray(bound, dtype=float).ravel()
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    print(f"linearized {label}: max |err| {err.max(initial=0.0):.3e}, worst |err| / bound {ratio.max(initial=0.0):.3e} over {err.size} entries")
    return float(ratio.max(initial=0.0))


# ---- check 1 -----------------------------------------------------------------------------------------------------------------------------
def check_exports():
    assert "LinearizedModel" in npg.__all__ and "EigenModes" in npg.__all__
    assert NEW <= set(L.declared_symbols())
    hdr = open(L.HEADER_PATH).read()
    for path in (L.HOST_LIB_PATH, L.LIB_PATH):
        lib = C.CDLL(path)
        assert not [s for s in NEW if not hasattr(lib, s) or s + "(" not in hdr], path


# ---- check 2: the tangent load ---------------------------------------------------------------------------------------------------------------
def engine(model):
    return device_fe(model.arch, model.fe_data)


def random_states(model, seed=SEED):
    """(b_base, x_base, db, dx) in the solvers' order, fixed seed"""
    d = model.fe_data.dofs
    rng = np.random.default_rng(seed)
    return tuple(rng.standard_normal(n) for n in (d.nb, d.nu + d.np, d.nb, d.nu + d.np))


def tangent(model, N2, bb, xb, db, dx):
    """npg_fe_tangent_rhs of the library the model runs on"""
    ctx = model.arch.ctx
    v = [npg.DeviceVector.from_host(ctx, a) for a in (bb, xb, db, dx)]
    return engine(model).tangent_rhs(N2, *v, npg.DeviceVector(ctx, len(bb))).to_host()


def host_tangent(host, N2, bb, xb, db, dx):
    """the same through libnupgcm_host.so loaded beside (redi_ref.HostLibrary, on the model's own tables)"""
    out = host.vec(np.zeros(len(bb)))
    host.ok(host.H.npg_fe_tangent_rhs(host.fe, float(N2), host.vec(bb), host.vec(xb), host.vec(db), host.vec(dx), out))
    got = np.empty(len(bb))
    host.ok(host.H.npg_vec_download(out, L.ptr(got)))
    return got


def _term(k, v, sc, N2, absolute):
    """loc (nc, nl) of one term: sum_q W (v_q . grad sc_q + v_z,q N2) phi_i from nodal v (nc, 10, 3) and sc (nc, nl)"""
    f = np.abs if absolute else (lambda a: a)
    G, wdet, qw = f(k["G"].astype(LD)).reshape(-1, 4, 3), f(k["wdet"].astype(LD)), f(k["qw"].astype(LD))
    nq, nl = len(qw), k["cb"].shape[1]
    Nu, Nb, dNb = f(k["N2"].astype(LD)).reshape(nq, 10), f(k["Nb"].astype(LD)).reshape(nq, nl), f(k["dNb"].astype(LD)).reshape(nq, nl, 4)
    v, sc = f(v.astype(LD)), f(sc.astype(LD))
    uq = np.einsum("qi,cia->cqa", Nu, v)
    g = np.einsum("cqk,cka->cqa", np.einsum("qik,ci->cqk", dNb, sc), G)
    integrand = (uq * g).sum(axis=-1) + uq[..., 2] * f(LD(N2))
    return np.einsum("cq,qi->ci", qw[None, :] * wdet[:, None] * integrand, Nb)


def restate(model, N2, bb, xb, db, dx):
    """(T, bound, S2) per free buoyancy DoF; S2 = the absolute sum of the du term alone (what an error of dx is pushed through)"""
    k = engine(model)._keep
    cu, cb = k["cu"].reshape(-1, 10, 3).astype(np.int64), k["cb"].astype(np.int64)
    nq, nl = len(k["qw"]), cb.shape[1]

    def nodal(x, codes, diri):
        dv = np.zeros(1) if diri is None or not len(diri) else np.asarray(diri)
        return np.where(codes >= 0, x[np.maximum(codes, 0)], 0.0 if diri is None else dv[np.minimum(np.maximum(-1 - codes, 0), len(dv) - 1)])
    ub, dun = nodal(xb, cu, k["ud"]), nodal(dx, cu, None)
    bbn, dbn = nodal(bb, cb, k["bd"]), nodal(db, cb, None)
    loc = _term(k, ub, dbn, 0.0, False) + _term(k, dun, bbn, N2, False)
    a2 = _term(k, dun, bbn, N2, True)
    lab = _term(k, ub, dbn, 0.0, True) + a2
    free = cb >= 0
    nb = len(bb)
    T, S, S2 = np.zeros(nb, dtype=LD), np.zeros(nb, dtype=LD), np.zeros(nb, dtype=LD)
    np.add.at(T, cb[free], loc[free])
    np.add.at(S, cb[free], lab[free])
    np.add.at(S2, cb[free], a2[free])
    len_r = np.bincount(cb[free], minlength=nb)
    bound = (10 + nl + 4 + 4 + 3 + 2 * nq + len_r) * EPS * np.asarray(S, dtype=float)
    return np.asarray(T, dtype=float), bound, np.asarray(S2, dtype=float)


def check_load(model, label, host=False, N2=0.7):
    """check 2 on one engine: the library against the restatement within twice the bound; the device against the host library bit for
    bit (host=True: GPU() runs only); exact homogeneity in the perturbation"""
    st = random_states(model)
    got = tangent(model, N2, *st)
    want, bound, _ = restate(model, N2, *st)
    ratio = report(f"{label}: library against the restatement", np.abs(got - want), bound)
    assert np.abs(want).max() > 1e-3 and (bound > 0).all()
    assert (np.abs(got - want) <= 2 * bound).all()
    if host:
        hl = rr.HostLibrary(model)
        hgot = host_tangent(hl, N2, *st)
        report(f"{label}: host library against the restatement", np.abs(hgot - want), bound)
        print(f"linearized {label}: device against the host library: {int(np.count_nonzero(got != hgot))} of {got.size} entries differ")
        assert (np.abs(hgot - want) <= 2 * bound).all()
        assert np.array_equal(got, hgot)
    bb, xb, db, dx = st
    zero = tangent(model, N2, bb, xb, np.zeros_like(db), np.zeros_like(dx))
    twice = tangent(model, N2, bb, xb, 2.0 * db, 2.0 * dx)
    assert not zero.any()                        # a perturbation carries no Dirichlet values: none of the base's leak into it
    assert np.array_equal(twice, 2.0 * got)      # and T is homogeneous in it, exactly for a power of two
    return ratio


def check_dirichlet(model, model_zero, label):
    """bowl_diri: the base state sees the Dirichlet values (zeroing them changes the result, and by what the restatement says); the
    perturbation does not (check_load: a zero perturbation gives exact zeros, whatever stands in the Dirichlet table)"""
    assert np.any(engine(model)._keep["bd"] != 0.0) and not np.any(engine(model_zero)._keep["bd"] != 0.0)
    assert np.array_equal(engine(model)._keep["cb"], engine(model_zero)._keep["cb"])
    st = random_states(model)
    a, b = tangent(model, 0.0, *st), tangent(model_zero, 0.0, *st)
    wa, ba, _ = restate(model, 0.0, *st)
    wb, bz, _ = restate(model_zero, 0.0, *st)
    print(f"linearized {label}: zeroing b_diri of the base moves the load by up to {np.abs(a - b).max():.3e} (restatement {np.abs(wa - wb).max():.3e})")
    assert np.abs(a - b).max() > 1e-3 * np.abs(a).max()
    assert (np.abs((a - b) - (wa - wb)) <= 2 * (ba + bz)).all()


# ---- the operator and its oracle F (check 3) ----------------------------------------------------------------------------------------------
def forward_error(lin, db):
    """the relative error of dx = L db, estimated by one step of iterative refinement through the same solver: ||A^-1 (B db - A dx)|| /
    ||dx|| in the max norm; not below the solver's rtol when it iterates"""
    s = lin.inv_solver
    dx = lin.invert(db).copy()
    lin.B.mul(db, s.y, alpha=1.0, beta=0.0)
    s.A.mul(dx, s.y, alpha=-1.0, beta=1.0)
    s.x.fill(0.0)
    iterative_solve(s)
    e = s.x.maxabs()[0] / dx.maxabs()[0]
    return e if isinstance(s.P, LU) else max(e, lin.rtol)


def allowance(lin, db, margin=10.0):
    """what |apply(db) - exact| may be, per entry: margin x (the solver's relative error pushed through the du term of T + the
    restatement's rounding bound of T)"""
    dx = lin.invert(db).to_host()
    _, bound, S2 = restate(lin.model, lin.N2, lin.b_base.to_host(), lin.x_base.to_host(), db.to_host(), dx)
    err = forward_error(lin, db)
    return margin * (err * S2 + bound), err, bound


def F_of(model, b_host):
    """F(b) from the entry points that existed before the operator: npg_fe_evolution_rhs(BDF1, dt = 1; b, b, x(b), x(b)) -
    (M + c (Kh + Kv)) b with x(b) from the model's own inversion (CPU(): LU, exact to rounding).  Writes the model's solver vectors:
    use a model of its own."""
    ev, ctx = model.evolution, model.arch.ctx
    b = npg.DeviceVector.from_host(ctx, b_host)
    npg.invert(model, b)
    x = model.inversion.solver.x
    c = npg.evolution_parameter(model.params, npg.BDF1(t_start=0.0, t_stop=1.0, dt=1.0))
    y = npg.DeviceVector(ctx, len(b_host))
    ev.fe.evolution_rhs(L.NPG_BDF1, 1.0, model.params.N2, c, b, b, x, x, ev.rhs_diff, ev.rhs_flux, ev.rhs_M, ev.rhs_h, ev.rhs_v, y)
    ev.M.mul(b, y, alpha=-1.0, beta=1.0)
    ev.Kh.mul(b, y, alpha=-c, beta=1.0)
    ev.Kv.mul(b, y, alpha=-c, beta=1.0)
    return y.to_host()


def derivative_case(arch, config, nsteps, seed=SEED):
    """a base state and a perturbation of the same norm on the golden bowl: (model, b_base, x_base, delta) in the solvers' order"""
    model = helpers.build_model(config, nsteps=max(nsteps, 1), arch=arch)
    if nsteps:
        npg.run(model)
    else:
        npg.invert(model)
    bb, xb = model.b_vec.to_host(), model.inversion.solver.x.to_host()
    delta = np.random.default_rng(seed).standard_normal(len(bb))
    delta *= np.linalg.norm(bb) / np.linalg.norm(delta)
    return model, bb, xb, delta


def check_derivative(arch, config, nsteps, label):
    """check 3 on CPU(): F is quadratic, so [F(b + d) - F(b - d)] / 2 = apply(d) up to rounding for ANY size of d"""
    model, bb, xb, delta = derivative_case(arch, config, nsteps)
    assert np.linalg.norm(bb) > 0 and np.isclose(np.linalg.norm(delta), np.linalg.norm(bb), rtol=1e-12)
    lin = npg.LinearizedModel(model)
    ctx = arch.ctx
    got = lin.apply(npg.DeviceVector.from_host(ctx, delta)).to_host()
    tol, err, bound = allowance(lin, npg.DeviceVector.from_host(ctx, delta))
    Fp, Fm = F_of(model, bb + delta), F_of(model, bb - delta)
    central = 0.5 * (Fp - Fm)
    floor = np.abs(Fp - F_of(model, (bb - delta) + 2.0 * delta)).max()     # the oracle's own rounding: the same b, summed in another order
    worst = np.abs(got - central).max()
    print(f"linearized {label}: |apply - central difference| max {worst:.3e} (|apply| max {np.abs(got).max():.3e}); oracle floor {floor:.3e}, "
          f"restatement bound max {bound.max():.3e}, LU forward error {err:.3e}; worst |err| / allowance "
          f"{(np.abs(got - central) / np.maximum(tol, 10 * floor)).max():.3e}")
    assert np.abs(got).max() > 0
    assert (np.abs(got - central) <= np.maximum(tol, 10.0 * floor)).all()
    return model, lin


def check_derivative_against(model, ref, label):
    """check 3 on GPU(): apply on the CPU() run's base state against the CPU() result; the inversion is iterative here - the allowance is
    rtol ||x|| pushed through T, margin 10"""
    ctx = model.arch.ctx
    base = (npg.DeviceVector.from_host(ctx, ref["bb"]), npg.DeviceVector.from_host(ctx, ref["xb"]))
    lin = npg.LinearizedModel(model, base=base)
    d = npg.DeviceVector.from_host(ctx, ref["delta"])
    got = lin.apply(d).to_host()
    tol, err, _ = allowance(lin, d)
    ratio = report(f"{label}: apply against the CPU() architecture's (solver error {err:.1e})", np.abs(got - ref["apply"]), tol)
    assert np.abs(got).max() > 0 and (np.abs(got - ref["apply"]) <= tol).all()
    return ratio


# ---- check 4: linearity and passivity ---------------------------------------------------------------------------------------------------------
def flat_model(arch, nsteps=5, total=None, **inv_kw):
    m = helpers.build_model("bowl_mixing", mesh=FLAT, nsteps=total or max(nsteps, 1), arch=arch, **inv_kw)
    if nsteps:
        npg.run(m, n_steps=nsteps)
    return m


def check_linearity(model, label):
    """apply(a d1 + d2) = a apply(d1) + apply(d2) and apply(a d1) = a apply(d1) with a = 1e-9: under the model's own atol = 1e-6 the
    inversion of a tiny right-hand side returns dx = 0 and both fail"""
    lin = npg.LinearizedModel(model)
    ctx, nb = model.arch.ctx, lin.nb
    rng = np.random.default_rng(SEED + 4)
    d1, d2, a = rng.standard_normal(nb), rng.standard_normal(nb), 1e-9
    up = lambda v: npg.DeviceVector.from_host(ctx, v)
    J1, J2 = lin.apply(up(d1)).to_host(), lin.apply(up(d2)).to_host()
    Js, Jc = lin.apply(up(a * d1)).to_host(), lin.apply(up(a * d1 + d2)).to_host()
    t1, e1, _ = allowance(lin, up(d1))
    t2, e2, _ = allowance(lin, up(d2))
    r_s = report(f"{label}: apply(a d1) against a apply(d1), a = {a:g}", np.abs(Js - a * J1), 2 * a * t1)
    r_c = report(f"{label}: apply(a d1 + d2) against a apply(d1) + apply(d2)", np.abs(Jc - (a * J1 + J2)), 2 * (t2 + a * t1))
    # the advective part alone must be visible at this size, or the check would pass with dx = 0
    dx = lin.invert(up(a * d1)).to_host()
    assert np.abs(dx).max() > 0
    Tdx = tangent(model, lin.N2, lin.b_base.to_host(), lin.x_base.to_host(), np.zeros(nb), dx)
    print(f"linearized {label}: the du term of apply(a d1) is {np.abs(Tdx).max():.3e} against an allowance of {(2 * a * t1).max():.3e}")
    assert np.abs(Tdx).max() > (2 * a * t1).max()
    assert (np.abs(Js - a * J1) <= 2 * a * t1).all()
    assert (np.abs(Jc - (a * J1 + J2)) <= 2 * (t2 + a * t1)).all()
    return lin, max(r_s, r_c)


def check_atol_pitfall(model, label):
    """why atol = 0: with the model's own kwargs (atol = 1e-6 on the 1/h^d-scaled residual) the iterative inversion of a tiny
    right-hand side stops before its first iteration and returns dx = 0 exactly - the operator would lose its advective part there"""
    lin = npg.LinearizedModel(model)
    assert lin.inv_solver.kwargs["atol"] == 0.0 and lin.inv_solver.kwargs["rtol"] == lin.rtol
    assert model.inversion.solver.kwargs["atol"] > 0.0                     # (the model keeps its own)
    d = npg.DeviceVector.from_host(model.arch.ctx, 1e-9 * np.random.default_rng(SEED + 4).standard_normal(lin.nb))
    good = lin.invert(d).maxabs()[0]
    lin.inv_solver.kwargs.update(atol=model.inversion.solver.kwargs["atol"], rtol=model.inversion.solver.kwargs["rtol"])
    bad = lin.invert(d).maxabs()[0]
    print(f"linearized {label}: max |dx| of a 1e-9 perturbation: {good:.3e} with atol = 0, {bad:.3e} with the model's kwargs")
    assert good > 0.0 and bad == 0.0


def snapshot(model):
    s, e = model.inversion.solver, model.evolution.solver
    out = [model.b_vec.to_host(), s.x.to_host(), s.y.to_host(), e.y.to_host(), e.A.to_scipy_csr().data.copy()]
    if getattr(e.P, "diag", None) is not None:
        out.append(e.P.diag.to_host())
    return out


def check_passive(arch, label, **inv_kw):
    """apply, implicit_step and eigenmodes write nothing the model owns; two more steps give the bits of a twin never linearised"""
    model, twin = flat_model(arch, 3, total=5, **inv_kw), flat_model(arch, 3, total=5, **inv_kw)
    before = snapshot(model)
    assert all(np.array_equal(a, b) for a, b in zip(before, snapshot(twin)))
    lin = npg.LinearizedModel(model)
    d = npg.DeviceVector.from_host(arch.ctx, np.random.default_rng(SEED).standard_normal(lin.nb))
    lin.apply(d)
    lin.implicit_step(d, 50.0)
    em = lin.eigenmodes(2, 300.0)
    assert lin.n_inversions > 0 and len(em) == 2
    assert all(np.array_equal(a, b) for a, b in zip(before, snapshot(model)))
    npg.run(model, n_steps=2)
    npg.run(twin, n_steps=2)
    assert all(np.array_equal(a, b) for a, b in zip(snapshot(model), snapshot(twin)))
    assert np.array_equal(model.state.u, twin.state.u)


# ---- check 5: the eigen-solver on a known answer that does not use the tangent kernel -------------------------------------------------------
def check_diffusion_modes(model, n=4):
    """N2 = 0 (bowl_wind), b_base = 0, x_base = 0: J = -c (Kh + Kv), so sigma = -c x the smallest eigenvalues of (Kh + Kv, M)"""
    ctx, d = model.arch.ctx, model.fe_data.dofs
    assert d.nb == 5864 and float(model.params.N2) == 0.0
    lin = npg.LinearizedModel(model, base=(npg.DeviceVector(ctx, d.nb), npg.DeviceVector(ctx, d.nu + d.np)))
    ev = model.evolution
    K = (ev.Kh.to_scipy_csr() + ev.Kv.to_scipy_csr()).tocsc()
    lam = np.sort(spla.eigsh(K, k=n + 2, M=ev.M.to_scipy_csr().tocsc(), sigma=0, which="LM", return_eigenvectors=False))
    want = -lin.c * lam[:n]
    em = lin.eigenmodes(n, dt=1.0 / abs(want[0]), ncv=40)
    err = np.abs(em.sigma - want)
    print(f"linearized diffusion modes: sigma {em.sigma.real}, oracle {want}, |err| / |sigma| {err / np.abs(want)}, residuals {em.residuals}, "
          f"{em.n_applies} applies, {em.n_inner} inner iterations, {em.n_restarts} restarts")
    assert em.converged.all() and (em.residuals <= 1e-8).all()
    assert (np.abs(em.sigma.imag) <= 1e3 * EPS * np.abs(em.sigma)).all()          # a symmetric pencil: real to rounding
    # a symmetric pencil has condition number 1: |d sigma| <= residual |sigma| (first order), margin 10; eigsh's own accuracy beside it
    assert (err <= (10.0 * em.residuals + 1e-10) * np.abs(want)).all()
    assert np.iscomplexobj(em.vectors) and em.vectors.shape == (n, d.nb) and not em.vectors.imag.any()
    return em


# ---- check 6: eigenmodes against a dense oracle -----------------------------------------------------------------------------------------------
def dense_oracle(lin):
    """J column by column with apply, in native order, and scipy's eig(J, M) with both sets of vectors"""
    d, ctx = lin.model.fe_data.dofs, lin.ctx
    nb = lin.nb
    J = np.zeros((nb, nb))
    e, out = npg.DeviceVector(ctx, nb), npg.DeviceVector(ctx, nb)
    for k in range(nb):
        x = np.zeros(nb)
        x[k] = 1.0
        e.upload(x, d.p_b)
        J[:, k] = lin.apply(e, out).to_host(d.inv_p_b)
    Md = lin.M.to_scipy_csr().toarray()
    Mn = Md[np.ix_(d.inv_p_b, d.inv_p_b)]                # native entry (i, j) = device entry (inv_p_b[i], inv_p_b[j])
    w, vl, vr = sla.eig(J, Mn, left=True, right=True)
    return J, Mn, w, vl, vr


def choose_modes(w, dt):
    """the oracle's eigenvalues by distance from the shift 1 / dt, and n <= 6 at the widest gap among the first eight"""
    order = np.argsort(np.abs(w - 1.0 / dt), kind="stable")
    dist = np.abs(w[order] - 1.0 / dt)
    gaps = dist[1:8] - dist[:7]
    n = int(np.argmax(gaps[:6])) + 1
    return order, n


def normalise(v, Mn):
    v = v / np.sqrt(np.vdot(v, Mn @ v).real)
    big = v[np.argmax(np.abs(v))]
    return v * (np.conj(big) / abs(big))


def oracle_modes(lin, dt):
    """dict(sigma, kappa, gap, vectors (n, nb), n) of the n chosen modes, sorted by descending real part as EigenModes sorts"""
    J, Mn, w, vl, vr = dense_oracle(lin)
    order, n = choose_modes(w, dt)
    pick = order[:n]
    pick = pick[np.argsort(-w[pick].real, kind="stable")]
    kappa = np.array([np.linalg.norm(vl[:, i]) * np.linalg.norm(Mn @ vr[:, i]) / abs(np.vdot(vl[:, i], Mn @ vr[:, i])) for i in pick])
    gap = np.array([np.abs(np.delete(w, i) - w[i]).min() for i in pick])
    vecs = np.array([normalise(vr[:, i], Mn) for i in pick])
    asym = np.abs(J - J.T).max() / np.abs(J).max()
    return dict(sigma=w[pick], kappa=kappa, gap=gap, vectors=vecs, n=n, asym=asym, M=Mn)


def compare_modes(em, ref, label, tol=1e-8):
    """the returned modes hold their own residual bound; sigma and the vectors lie within the first-order perturbation bound of the
    oracle's"""
    n = int(ref["n"])
    assert len(em) == n and em.vectors.shape[0] == n
    print(f"linearized {label}: n = {n}, sigma {em.sigma}, residuals {em.residuals}, kappa {ref['kappa']}, {em.n_applies} applies, "
          f"{em.n_inner} inner iterations, {em.n_restarts} restarts")
    assert em.converged.all() and (em.residuals <= tol).all()
    # pair the modes with the oracle's (a conjugate pair may come in either order)
    used, worst = [], 0.0
    for i in range(n):
        j = min((j for j in range(n) if j not in used), key=lambda j: abs(em.sigma[i] - ref["sigma"][j]))
        used.append(j)
        bound = 10.0 * ref["kappa"][j] * em.residuals[i] * abs(em.sigma[i])
        err = abs(em.sigma[i] - ref["sigma"][j])
        v, vo = em.vectors[i], ref["vectors"][j]
        phase = np.vdot(vo, ref["M"] @ v)
        verr = np.linalg.norm(v * (np.conj(phase) / abs(phase)) - vo) / np.linalg.norm(vo)
        vbound = bound / ref["gap"][j]
        print(f"linearized {label}: mode {i}: |d sigma| {err:.3e} / bound {bound:.3e} = {err / bound:.3e}; vector {verr:.3e} / bound {vbound:.3e} "
              f"= {verr / vbound:.3e}")
        worst = max(worst, err / bound, verr / vbound)
        assert err <= bound and verr <= vbound
    return worst


def eigen_case(arch, nsteps, **inv_kw):
    """the embedded 2-D bowl (173 cells) at rest (N2 = 2: the w-feedback alone makes J non-symmetric) or after 5 steps"""
    model = flat_model(arch, nsteps, **inv_kw)
    assert model.fe_data.mesh.ncell == 173
    return model, npg.LinearizedModel(model)


DT_EIG = 300.0          # 1 / dt = 3.3e-3: between the slowest diffusive rate of the 2-D bowl (9e-4) and the next ones


def check_eigenmodes_against(arch, ref, label, **inv_kw):
    """check 6 on GPU(): the CPU() run's base state behind this architecture's inversion; the modes hold their own residual bound, lie
    within the perturbation bound of the CPU() run's dense oracle and, by the same rule with both residuals, of the CPU() run's modes"""
    model = flat_model(arch, 0, **inv_kw)
    ctx = arch.ctx
    lin = npg.LinearizedModel(model, base=(npg.DeviceVector.from_host(ctx, ref["bb"]), npg.DeviceVector.from_host(ctx, ref["xb"])))
    em = lin.eigenmodes(int(ref["n"]), DT_EIG)
    worst = compare_modes(em, ref, label)
    s, sc = np.sort_complex(em.sigma), np.sort_complex(ref["cpu_sigma"])                  # both in the oracle's order below
    bound = 10.0 * ref["kappa"][np.argsort(ref["sigma"])] * (em.residuals.max() + ref["cpu_residuals"].max()) * np.abs(s)
    print(f"linearized {label}: |sigma - CPU() sigma| / bound {np.abs(s - sc) / bound}")
    assert (np.abs(s - sc) <= bound).all()
    return worst, em


def check_eigenmodes(arch, nsteps, label):
    model, lin = eigen_case(arch, nsteps)
    ref = oracle_modes(lin, DT_EIG)
    print(f"linearized {label}: max |J - J'| / max |J| = {ref['asym']:.3e}")
    # (at rest on the 2-D bowl J is symmetric to rounding although A is not: without y-derivatives the along-slope velocity is
    # eliminated from the inversion symmetrically; the advected state is what makes the pencil non-normal)
    assert nsteps == 0 or ref["asym"] > 1e-6
    em = lin.eigenmodes(ref["n"], DT_EIG)
    return compare_modes(em, ref, label), em, ref


# ---- check 7 ----------------------------------------------------------------------------------------------------------------------------------
def check_step(lin, label, dt=50.0):
    ctx, nb = lin.ctx, lin.nb
    v = npg.DeviceVector.from_host(ctx, np.random.default_rng(SEED + 7).standard_normal(nb))
    out = lin.implicit_step(v, dt)
    rtol = 100.0 * lin.rtol
    res = lin.apply(out)
    lin.M.mul(out, res, alpha=1.0, beta=-dt)
    Mv = lin.M.mul(v)
    res.axpby(-1.0, Mv, 1.0)
    print(f"linearized {label}: implicit step dt = {dt}: {lin.last_step}; recomputed ||(M - dt J) out - M v|| / ||M v|| = {res.norm() / Mv.norm():.3e}")
    assert lin.last_step["niter"] >= 1 and res.norm() <= rtol * Mv.norm()
    rel = []
    for small in (1e-2, 1e-4, 1e-6):
        o = lin.implicit_step(v, small)
        o.axpby(-1.0, v, 1.0)
        rel.append(o.norm() / v.norm())
    print(f"linearized {label}: ||step(v, dt) - v|| / ||v|| at dt = 1e-2, 1e-4, 1e-6: {rel}")
    assert rel[2] < rel[1] < rel[0] and rel[2] < 1e-4


# ---- check 8 ----------------------------------------------------------------------------------------------------------------------------------
def check_refusals(model):
    def variant(**kw):
        m = copy.copy(model)
        for k, v in kw.items():
            setattr(m, k, v)
        return m
    with pytest.raises(NotImplementedError, match="mesh-partitioned"):
        npg.LinearizedModel(variant(comm=object()))
    conv = dataclasses.replace(model.forcings, conv_param=npg.ConvectionParameterization(1.0, 1e-3, True))
    with pytest.raises(NotImplementedError, match="closures"):
        npg.LinearizedModel(variant(forcings=conv))
    eddy = dataclasses.replace(model.forcings, eddy_param=npg.EddyParameterization(1.0, 1e-3, True))
    with pytest.raises(NotImplementedError, match="closures"):
        npg.LinearizedModel(variant(forcings=eddy))
    with pytest.raises(NotImplementedError, match="surface_forcing"):
        npg.LinearizedModel(variant(surface_forcing=object()))
    with pytest.raises(NotImplementedError, match="interior_forcing"):
        npg.LinearizedModel(variant(interior_forcing=object()))
    with pytest.raises(TypeError, match="base must be"):
        npg.LinearizedModel(model, base=3)
    with pytest.raises(ValueError, match="base state must hold"):
        npg.LinearizedModel(model, base=(model.inversion.solver.x, model.b_vec))
    # the entry point's own argument checks (csrc/tangent_core.h: check_tangent), on the host of either library
    ctx, d = model.arch.ctx, model.fe_data.dofs
    fe = engine(model)
    b, x = npg.DeviceVector(ctx, d.nb), npg.DeviceVector(ctx, d.nu + d.np)
    short_b, short_x = npg.DeviceVector(ctx, d.nb - 1), npg.DeviceVector(ctx, d.nu + d.np - 1)
    for args, sentence in (((short_b, x, b, x, b), r"\(base state\): the buoyancy vector has"),
                           ((b, short_x, b, x, b), r"\(base state\): the flow vector has"),
                           ((b, x, short_b, x, b), r"\(perturbation\): the buoyancy vector has"),
                           ((b, x, b, short_x, b), r"\(perturbation\): the flow vector has"),
                           ((b, x, b, x, short_b), "the output vector has")):
        with pytest.raises(L.DeviceError, match=sentence):
            fe.tangent_rhs(0.0, *args)
    with pytest.raises(L.DeviceError, match="N2 must be finite"):
        fe.tangent_rhs(float("nan"), b, x, b, x, b)
    lin = npg.LinearizedModel(model)
    with pytest.raises(ValueError, match="n must lie"):
        lin.eigenmodes(0, 1.0)
    with pytest.raises(ValueError, match="dt must be positive"):
        lin.eigenmodes(2, -1.0)
    with pytest.raises(ValueError, match="dt must be positive"):
        lin.implicit_step(b, 0.0)


def check_modes_io(em, model, tmp_path):
    """save / load round trip; as_b gives what set_b accepts"""
    path = em.save(os.path.join(str(tmp_path), "modes.npz"))
    back = npg.EigenModes.load(path)
    for name in ("sigma", "vectors", "residuals", "converged"):
        assert np.array_equal(getattr(em, name), getattr(back, name))
    assert (back.n_applies, back.n_inversions, back.dt) == (em.n_applies, em.n_inversions, em.dt) and back.n_inversions >= back.n_applies > 0
    keep = model.b_vec.to_host()
    npg.set_b(model, em.as_b(0))
    assert np.array_equal(model.state.b, em.vectors[0].real)
    model.b_vec.upload(keep)
    with pytest.raises(ValueError, match="part must be"):
        em.as_b(0, part="modulus")
