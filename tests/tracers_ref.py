"""A numpy restatement of the passive-tracer right-hand side (nupgcm_amd.tracers) and the checks shared by
tests/test_tracers.py (CPU()) and tests/test_gpu_tracers.py (GPU()).

The restatement is written from the weak form, in the manner of integrals_ref.restate and not from the code under test: geometry from
the cells' own vertex coordinates (integrals_ref.geometry), native P2 / P1 tables (6-node triangles on the embedded 2-D meshes),
nodal values through Spaces' native tables, coefficients evaluated at the quadrature points from the forcing functions.  For row i
of tracer k

    y_i = sum_{cells, q} W ( c1 c + c2 c_prev ) phi_i                                        "mass"
        - cdt sum W ( u~ . grad c~ ) phi_i                                                   "adv"
        - cdt Gamma sum W u~_z phi_i                                                         "gamma_adv"
        + cdt S sum W phi_i                                                                  "source"
        - sum W c_D phi_i                                                                    "lift_mass"
        - theta sum W ( kappa_h grad_h c_D . grad_h phi_i + kappa_v d_z c_D d_z phi_i )      "lift_diff"
        - theta Gamma sum W kappa_v d_z phi_i                                                "gamma_diff"
        + dt flux_i                                                                          "flux" (one term: the surface load)

with W = w_q |J|.  A term is one (cell, q) entry of one line above; only the lines a tracer has count (Gamma = 0: no gamma lines; no
Dirichlet value: no lift lines).  Per row it returns the terms' math.fsum, S_abs = sum |term| and their number n.

Bound.  A recursive sum of n terms differs from the exact sum by at most (n - 1) eps sum |t| (Higham, eq. 4.4), in any order; the
bound used everywhere is  n eps S_abs  of the row (integrals_ref.summation_bound per row) - derived, not tuned.  Two evaluations of
the same row (device and host library, tracer and buoyancy kernels) differ by at most twice that."""
import math
from types import SimpleNamespace

import numpy as np

import nupgcm_amd as npg
from nupgcm_amd import _lib as L
from nupgcm_amd import fe as F
from nupgcm_amd.evolution import evolution_parameter
from nupgcm_amd.inversion import device_fe
from tests import helpers
from tests import integrals_ref as ir
from tests import sampling_ref as sr

EPS = np.finfo(np.float64).eps
NPG_EINVAL = -1
SEED = 20261018


def scheme_constants(scheme, dt):
    """(c1, c2, e1, e2, cdt) of k_advection_local's header comment / src/model.jl:292-300"""
    if scheme == L.NPG_BDF2:
        return 4.0 / 3.0, -1.0 / 3.0, 2.0, -1.0, 2.0 / 3.0 * dt
    return 1.0, 0.0, 1.0, 0.0, dt


def kappa_convection(fed, bn, kv0, kappa_c, N2min, alpha, N2):
    """the convection closure restated (src/inputs.jl:87-91): kappa_v0 + kappa_c (1 + tanh(-alpha (N2 + d_z b) / N2min)) / 2 at the
    quadrature points, from the nodal buoyancy"""
    m = fed.mesh
    X, G, wdet, lam, w, ea, eb = ir.geometry(m)
    N, dN = F.p2_tables(lam, ea, eb)
    if fed.spaces.b_order == 2:
        bc, dNb = bn[m.cell_nodes], dN
    else:
        bc, dNb = bn[m.cells], np.broadcast_to(np.eye(lam.shape[1]), (len(w),) + (lam.shape[1],) * 2)
    bz = np.einsum("qik,ci,ck->cq", dNb, bc, G[:, :, 2])
    return kv0 + kappa_c * (1.0 + np.tanh(-alpha * (N2 + bz) / N2min)) / 2.0


def restate(fed, scheme, dt, theta, un, un_prev, cn, cn_prev, cd, gamma, source, kh, kv, flux_load=None):
    """one tracer.  un, un_prev (nn, 3); cn, cn_prev (nb_nodes,) nodal values, Dirichlet nodes with the tracer's values; cd
    (nb_nodes,) the Dirichlet values at the Dirichlet nodes and 0 elsewhere; kh, kv: forcing functions / numbers or (ncell, nq)
    tables; flux_load (nb_nodes,) = alpha int_Gamma F phi_i or None.
    -> SimpleNamespace(total (nb,), sabs, n, bound = n eps sabs, lift (nb,) = the sum of the lift lines) over the free rows"""
    m, s, t = fed.mesh, fed.spaces, fed.tables
    c1, c2, e1, e2, cdt = scheme_constants(scheme, dt)
    X, G, wdet, lam, w, ea, eb = ir.geometry(m)
    N, dN = F.p2_tables(lam, ea, eb)
    if s.b_order == 2:
        cells_b, Nb, dNb = m.cell_nodes, N, dN
    else:
        cells_b, Nb, dNb = m.cells, lam, np.broadcast_to(np.eye(lam.shape[1]), (len(w),) + (lam.shape[1],) * 2)
    nb = fed.dofs.nb
    rows = t.b_pos[cells_b]                                                # (nc, nl): the row of local function i, -1 = Dirichlet
    W = w[None, :] * wdet[:, None]                                         # (nc, nq)
    u = np.einsum("qi,cia->cqa", N, (e1 * un + e2 * un_prev)[m.cell_nodes])
    gphi = np.einsum("qik,ckj->cqij", dNb, G)                              # grad phi_i at q
    cm = np.einsum("qi,ci->cq", Nb, (c1 * cn + c2 * cn_prev)[cells_b])
    gc = np.einsum("cqij,ci->cqj", gphi, (e1 * cn + e2 * cn_prev)[cells_b])
    xq = np.einsum("qk,cki->cqi", lam, X)
    tab = lambda v: np.asarray(v, dtype=float) if isinstance(v, np.ndarray) else ir.coefficient(m, v, xq)
    phi = Nb[None, :, :]                                                   # (1, nq, nl)
    lines = {"mass": (W * cm)[..., None] * phi, "adv": (-cdt * W * (u * gc).sum(axis=-1))[..., None] * phi}
    if gamma != 0.0:
        lines["gamma_adv"] = (-cdt * gamma * W * u[..., 2])[..., None] * phi
        lines["gamma_diff"] = -theta * gamma * (W * tab(kv))[..., None] * gphi[..., 2]
    if source != 0.0:
        lines["source"] = (cdt * source * W)[..., None] * phi
    if np.any(cd != 0.0):
        cdc = cd[cells_b]
        cdq = np.einsum("qi,ci->cq", Nb, cdc)
        gd = np.einsum("cqij,ci->cqj", gphi, cdc)
        lines["lift_mass"] = -(W * cdq)[..., None] * phi
        lines["lift_diff"] = -theta * W[..., None] * (tab(kh)[..., None] * (gd[..., None, 0] * gphi[..., 0] + gd[..., None, 1] * gphi[..., 1])
                                                      + tab(kv)[..., None] * gd[..., None, 2] * gphi[..., 2])
    rr = np.broadcast_to(rows[:, None, :], lines["mass"].shape)
    keep = rr >= 0
    rall = np.concatenate([rr[keep]] * len(lines))
    vall = np.concatenate([v[keep] for v in lines.values()])
    lall = np.concatenate([np.full(int(keep.sum()), k.startswith("lift")) for k in lines])
    if flux_load is not None:
        free = np.nonzero(t.b_pos >= 0)[0]
        rall = np.concatenate([rall, t.b_pos[free]])
        vall = np.concatenate([vall, dt * flux_load[free]])
        lall = np.concatenate([lall, np.zeros(len(free), dtype=bool)])
    order = np.argsort(rall, kind="stable")
    rall, vall, lall = rall[order], vall[order], lall[order]
    cut = np.searchsorted(rall, np.arange(nb + 1))
    n = np.diff(cut)
    vl, ll = vall.tolist(), np.where(lall, vall, 0.0).tolist()
    total = np.array([math.fsum(vl[a:b]) for a, b in zip(cut[:-1], cut[1:])])
    lift = np.array([math.fsum(ll[a:b]) for a, b in zip(cut[:-1], cut[1:])])
    sabs = np.bincount(rall, weights=np.abs(vall), minlength=nb)
    return SimpleNamespace(total=total, sabs=sabs, n=n, bound=n * EPS * sabs, lift=lift)


# ---- a tracer set on a model and its state ---------------------------------------------------------------------------------------
def diri_nodes(fed):
    return np.nonzero(fed.spaces.b_dof < 0)[0]


def nodal(fed, free, diri_node_values):
    """(nb_nodes,) nodal values: free DoFs from the device vector `free`, Dirichlet nodes from the per-node array"""
    pos = fed.tables.b_pos
    return np.where(pos >= 0, free[np.maximum(pos, 0)], diri_node_values)


def spec_arrays(model, spec):
    """(cd (nb_nodes,), flux_load or None) of a tracer specification, evaluated independently of PassiveTracers"""
    fed = model.fe_data
    m, s = fed.mesh, fed.spaces
    cd = np.zeros(s.nb_nodes)
    dn = diri_nodes(fed)
    d = spec.get("dirichlet")
    if d is not None and len(dn):
        cd[dn] = d(m.node_coords[:s.nb_nodes][dn]) if callable(d) else float(d)
    f = spec.get("flux")
    load = None
    if f is not None:
        fn = f if callable(f) else (lambda x, c=float(f): np.full(x.shape[:-1], c))
        load = m.surface_load(lambda x: model.params.alpha * fn(x))[:s.nb_nodes]
    return cd, load


def velocity_nodal(fed, x):
    t, s = fed.tables, fed.spaces
    return np.where(t.u_pos >= 0, x[np.maximum(t.u_pos, 0)], s.u_diri_val)


def restate_set(model, specs, scheme, dt, theta, x, x_prev, c, c_prev, kh=None, kv=None):
    """the restatement of every tracer of `specs` on the host copies of the state; c, c_prev stacked (K nb)"""
    fed, f = model.fe_data, model.forcings
    nb = fed.dofs.nb
    un, unp = velocity_nodal(fed, x), velocity_nodal(fed, x_prev)
    out = []
    for k, sp in enumerate(specs):
        cd, load = spec_arrays(model, sp)
        cn, cnp = nodal(fed, c[k * nb:(k + 1) * nb], cd), nodal(fed, c_prev[k * nb:(k + 1) * nb], cd)
        out.append(restate(fed, scheme, dt, theta, un, unp, cn, cnp, cd, float(sp.get("gamma", 0.0)), float(sp.get("source", 0.0)),
                           f.kappa_h if kh is None else kh, f.kappa_v if kv is None else kv, load))
    return out


SPECS3 = [dict(name="age", dirichlet=lambda x: 0.3 + 0.5 * x[..., 0], gamma=0.0, source=1.0, flux=None),
          dict(name="dye", dirichlet=-0.7, gamma=1.7, source=-0.4, flux=lambda x: 2e-2 * np.cos(2.0 * x[..., 1])),
          dict(name="salt", dirichlet=lambda x: np.cos(3.0 * x[..., 0]) + x[..., 1] + x[..., 2], gamma=-0.6, source=0.25, flux=0.05)]


def random_tracer_state(model, tr, seed=SEED):
    """random [u; p] (current and previous) and random c, c_prev uploaded; returns the host copies"""
    rng = np.random.default_rng(seed)
    x, _ = ir.random_state(model, seed)
    xp = rng.standard_normal(len(x))
    c, cp = rng.standard_normal(tr.c.n), rng.standard_normal(tr.c.n)
    tr.c.upload(c)
    tr.c_prev.upload(cp)
    return x, xp, c, cp, npg.DeviceVector.from_host(model.arch.ctx, xp)


def report(label, err, bound):
    worst = int(np.argmax(err / np.maximum(bound, 1e-300)))
    print(f"tracers {label}: max |y - restated| {err.max():.3e}; worst row {worst}: err {err[worst]:.3e} / bound {bound[worst]:.3e} "
          f"(ratio {err[worst] / max(bound[worst], 1e-300):.3e})")


# ---- check 1: the right-hand side against the restatement -----------------------------------------------------------------------------
def check_rhs(model, label, specs=SPECS3, need_lift=False, dt=0.013, theta=0.021):
    """both schemes, a random state with a random previous state, tracers with distinct Gamma, S, Dirichlet values and flux"""
    tr = npg.PassiveTracers(model, specs)
    nb = model.fe_data.dofs.nb
    x, xp, c, cp, xp_dev = random_tracer_state(model, tr)
    out = {}
    for scheme in (L.NPG_BDF1, L.NPG_BDF2):
        y = tr.rhs(scheme, dt, theta, model.inversion.solver.x, xp_dev).to_host()
        assert np.isfinite(y).all()
        ref = restate_set(model, specs, scheme, dt, theta, x, xp, c, cp)
        for k, r in enumerate(ref):
            err = np.abs(y[k * nb:(k + 1) * nb] - r.total)
            report(f"{label} scheme {scheme} tracer {k} ({specs[k]['name']})", err, r.bound)
            assert (err <= r.bound).all(), (label, scheme, k, float((err / np.maximum(r.bound, 1e-300)).max()))
            out[(scheme, k)] = (err.max(), r.bound.max())
        if need_lift:                                         # the case cannot pass vacuously: rows next to Dirichlet nodes feel the lift
            nz = [int(np.count_nonzero(r.lift)) for r in ref]
            print(f"tracers {label}: rows with a non-zero restated lift per tracer {nz}")
            assert all(v > 0 for v in nz)
    return out


# ---- check 2: the twin of b' -------------------------------------------------------------------------------------------------------
def conv_model(arch, name, conv, nsteps=3):
    """helpers.build_model with the convection closure switched on (conv = (kappa_c, N2min)) or off (None)"""
    fed, prm, frc, dt, b0 = helpers.build_fe_data(name)
    if conv is not None:
        frc.conv_param = npg.ConvectionParameterization(kappa_c=conv[0], N2min=conv[1], is_on=True)
    ts = npg.BDF2(t_start=0.0, t_stop=nsteps * dt, dt=dt)
    model = npg.Model(arch, prm, frc, fed, npg.InversionToolkit(arch, fed, prm, frc), npg.EvolutionToolkit(arch, fed, prm, frc, ts), ts)
    if b0 is not None:
        npg.set_b(model, b0)
    return model


def twin_spec(model, name):
    prm, frc, btags, bvals, dt, b0 = helpers.product_config(name)
    bc = frc.b_surface_bc
    d = None
    if btags:
        vals = model.fe_data.spaces.b_diri_val
        d = (lambda x, v=vals[diri_nodes(model.fe_data)]: v)
    return dict(name="twin", initial=model.state.b, dirichlet=d, gamma=prm.N2, source=0.0,
                flux=bc.flux if isinstance(bc, npg.SurfaceFluxBC) else None)


def _kv_now(model, b_host):
    """kappa_v as evolve() leaves it for a step that starts from b_host: the forcing, or the restated closure"""
    f, prm, fed = model.forcings, model.params, model.fe_data
    if not f.conv_param.is_on:
        return None
    m = fed.mesh
    X, G, wdet, lam, w, ea, eb = ir.geometry(m)
    kv0 = ir.coefficient(m, f.kappa_v, np.einsum("qk,cki->cqi", lam, X))
    bn = nodal(fed, b_host, fed.spaces.b_diri_val)
    return np.ascontiguousarray(kappa_convection(fed, bn, kv0, f.conv_param.kappa_c, f.conv_param.N2min, prm.alpha, prm.N2))


def check_twin(arch, name, conv=None):
    """a tracer with initial = b', the buoyancy's Dirichlet values, Gamma = N2, S = 0 and the buoyancy's flux:
    (a) npg_tracers_rhs = npg_fe_evolution_rhs on a random state within twice the summation bound, row by row;
    (b) 3 steps of run(): after each, d = c - b' obeys ||A d||_P <= ||r_c||_P + ||r_b||_P + ||bound on y_c - y_b||_P, P = 1 / diag(A),
        the norm of the CG stopping rule (cg.hip: sqrt(r' P r)); the residuals as the two solves' own stats report them - a direct
        solve (CPU(): stats['direct']) reports none, its residual y - A x is then evaluated on the host."""
    model = conv_model(arch, name, conv)
    fed, prm, ev, ts = model.fe_data, model.params, model.evolution, model.timestepper
    nb = fed.dofs.nb
    spec = twin_spec(model, name)
    # (a) static comparison on a random state; the closure's kappa_v is the one of that state
    tr = npg.PassiveTracers(model, [spec])
    b_keep = model.b_vec.to_host()
    x, xp, c, cp, xp_dev = random_tracer_state(model, tr)
    scale = 0.05                                                # a buoyancy perturbation of the size of the state's own
    c, cp = scale * c, scale * cp
    tr.c.upload(c), tr.c_prev.upload(cp)
    model.b_vec.upload(c)
    bp_dev = npg.DeviceVector.from_host(arch.ctx, cp)
    kv = _kv_now(model, c)
    if kv is not None:
        cpar = model.forcings.conv_param
        ev.fe.update_kappa_convection(cpar.kappa_c, cpar.N2min, prm.alpha, prm.N2, model.b_vec)
        ev.fe.assemble(L.NPG_MAT_KV, ev.Kv, lift=ev.rhs_v)
        ev.fe.rhs_diff(prm.N2, ev.rhs_diff)
        if tr.rhs_diff1 is not None:
            ev.fe.rhs_diff(1.0, tr.rhs_diff1)
    theta = evolution_parameter(prm, ts)
    res = {}
    for scheme in (L.NPG_BDF1, L.NPG_BDF2):
        yb = npg.DeviceVector(arch.ctx, nb)
        ev.fe.evolution_rhs(scheme, ts.dt, prm.N2, theta, model.b_vec, bp_dev, model.inversion.solver.x, xp_dev, ev.rhs_diff, ev.rhs_flux,
                            ev.rhs_M, ev.rhs_h, ev.rhs_v, yb)
        yc = tr.rhs(scheme, ts.dt, theta, model.inversion.solver.x, xp_dev).to_host()
        r = restate_set(model, [spec], scheme, ts.dt, theta, x, xp, c, cp, kv=kv)[0]
        err = np.abs(yc - yb.to_host())
        report(f"twin {name} conv={conv} scheme {scheme}: tracer rhs vs npg_fe_evolution_rhs (bound = 2 x summation)", err, 2 * r.bound)
        assert (err <= 2 * r.bound).all()
        res[scheme] = (err.max(), 2 * r.bound.max())
    # (b) three steps of run() from the model's own start
    model.b_vec.upload(b_keep)
    model.inversion.solver.x.fill(0.0)
    del tr
    spec = twin_spec(model, name)
    tr = model.tracers = npg.PassiveTracers(model, [spec])
    for step in range(3):
        pv = model._prev
        b0, x0 = model.b_vec.to_host(), model.inversion.solver.x.to_host()
        bp0, xp0 = (b0, x0) if pv is None else (pv["b_prev"].to_host(), pv["x_prev"].to_host())
        c0, cp0 = tr.c.to_host(), tr.c_prev.to_host()
        npg.run(model, n_steps=1)
        A = ev.solver.A.to_scipy_csr()
        P = 1.0 / A.diagonal()
        pnorm = lambda v: float(np.sqrt(np.sum(P * v * v)))
        yc, yb = tr.y.to_host(), ev.solver.y.to_host()
        cc, bb = tr.c.to_host(), model.b_vec.to_host()

        def resid(stats, yv, xv):
            return pnorm(yv - A @ xv) if stats.get("direct") else float(stats["rnorm"])
        rc, rb = resid(tr.stats[-1][0], yc, cc), resid(model.stats[-1][0], yb, bb)
        scheme = L.NPG_BDF2
        # the two right-hand sides were built from (b, b_prev) and (c, c_prev): bound their difference through both restatements' rows
        kvs = _kv_now(model, b0)
        rB = restate_set(model, [spec], scheme, ts.dt, theta, x0, xp0, b0, bp0, kv=kvs)[0]
        rC = restate_set(model, [spec], scheme, ts.dt, theta, x0, xp0, c0, cp0, kv=kvs)[0]
        ybound = pnorm(rB.bound + rC.bound + np.abs(rB.total - rC.total))
        lhs = pnorm(A @ (cc - bb))
        print(f"twin {name} conv={conv} step {step + 1}: ||A (c - b')||_P = {lhs:.3e}, r_c {rc:.3e} + r_b {rb:.3e} + y bound {ybound:.3e} "
              f"= {rc + rb + ybound:.3e}; max |c - b'| = {np.abs(cc - bb).max():.3e} of {np.abs(bb).max():.3e}")
        assert lhs <= rc + rb + ybound
        res[f"step{step + 1}"] = (lhs, rc + rb + ybound)
    return res


# ---- check 3: independence and fusion ----------------------------------------------------------------------------------------------
def check_independence(model, label, specs=SPECS3):
    """tracer k of a K = 3 call has the bits of a K = 1 call with that tracer alone; two identical calls give identical bits"""
    nb = model.fe_data.dofs.nb
    tr = npg.PassiveTracers(model, specs)
    x, xp, c, cp, xp_dev = random_tracer_state(model, tr)
    for scheme in (L.NPG_BDF1, L.NPG_BDF2):
        y1 = tr.rhs(scheme, 0.013, 0.021, model.inversion.solver.x, xp_dev).to_host()
        y2 = tr.rhs(scheme, 0.013, 0.021, model.inversion.solver.x, xp_dev).to_host()
        assert np.array_equal(y1, y2), label
        for k, sp in enumerate(specs):
            one = npg.PassiveTracers(model, [sp])
            one.c.upload(c[k * nb:(k + 1) * nb])
            one.c_prev.upload(cp[k * nb:(k + 1) * nb])
            yk = one.rhs(scheme, 0.013, 0.021, model.inversion.solver.x, xp_dev).to_host()
            assert np.array_equal(yk, y1[k * nb:(k + 1) * nb]), (label, scheme, k)
    print(f"tracers {label}: K = 3 columns bit-identical to K = 1 calls, repeat calls bit-identical")


# ---- check 4: physics ---------------------------------------------------------------------------------------------------------------
def integral(fed, cn):
    """int c over the mesh from nodal values (math.fsum of the quadrature terms) and S_abs"""
    m = fed.mesh
    X, G, wdet, lam, w, ea, eb = ir.geometry(m)
    N, _ = F.p2_tables(lam, ea, eb)
    cc, Nb = (cn[m.cell_nodes], N) if fed.spaces.b_order == 2 else (cn[m.cells], lam)
    t = (w[None, :] * wdet[:, None]) * np.einsum("qi,ci->cq", Nb, cc)
    return math.fsum(t.ravel()), math.fsum(np.abs(t).ravel())


def check_conservation(arch):
    """bowl_surface_flux (no Dirichlet nodes: the basis is a partition of unity, 1' Kh = 1' Kv = 0), 3 steps of run() with two
    tracers, Gamma = 0 and no flux: a dye (S = 0) and an age (S = 1, starting at 0).  Summing the rows of A c^{n+1} = y - r:

        int c^{n+1} = sum_i y_i - 1' r - theta 1' (Kh + Kv) c^{n+1},      sum_i y_i = c1 int c^n + c2 int c^{n-1} - cdt int u~ . grad c~ + cdt S V

    exactly as the code defines the step (a BDF2 right-hand side from the first step on, whatever left-hand side the first step uses).
    The discrete int u~ . grad c~ is not zero for a Taylor-Hood velocity (div u vanishes against the pressure space only), so it is
    taken from the restatement, as integrals_ref.check_buoyancy_conservation takes ch9: the dye's integral is conserved up to that
    advective term, the age's grows by cdt V on top of it (V = the volume; from the second step on the increments approach dt V).
    Bound = sum of the rows' summation bounds  +  sqrt(n_b) ||r||_2 (the CG residual through 1')  +  the rounding of the assembled
    column sums, 64 rowmax eps |1|' (|M| + theta (|Kh| + |Kv|)) |c| (each entry is assembled from at most 64 quadrature terms)."""
    model = helpers.build_model("bowl_surface_flux", nsteps=3, arch=arch)
    fed, ev, prm, ts = model.fe_data, model.evolution, model.params, model.timestepper
    assert (fed.tables.b_pos >= 0).all()
    nb = fed.dofs.nb
    specs = [dict(name="dye", initial=lambda x: np.exp(-8.0 * (x[..., 0] ** 2 + x[..., 1] ** 2)) * (1.0 + x[..., 2])),
             dict(name="age", source=1.0)]
    tr = model.tracers = npg.PassiveTracers(model, specs)
    theta = evolution_parameter(prm, ts)
    none = np.zeros(fed.spaces.nb_nodes)
    V, _ = integral(fed, np.ones(fed.spaces.nb_nodes))
    out = []
    for step in range(3):
        pv = model._prev
        x0 = model.inversion.solver.x.to_host()
        xp0 = x0 if pv is None else pv["x_prev"].to_host()
        c0, cp0 = tr.c.to_host(), tr.c_prev.to_host()
        npg.run(model, n_steps=1)
        ref = restate_set(model, specs, L.NPG_BDF2, ts.dt, theta, x0, xp0, c0, cp0)
        A = ev.solver.A.to_scipy_csr()
        absA = abs(ev.M.to_scipy_csr()) + theta * (abs(ev.Kh.to_scipy_csr()) + abs(ev.Kv.to_scipy_csr()))
        rowmax = int(np.diff(A.indptr).max())
        c1h, y1 = tr.c.to_host(), tr.y.to_host()
        for k, r in enumerate(ref):
            ck, yk = c1h[k * nb:(k + 1) * nb], y1[k * nb:(k + 1) * nb]
            got, sabs_int = integral(fed, nodal(fed, ck, none))
            predicted = math.fsum(r.total)
            res = yk - A @ ck
            bound = float(r.bound.sum()) + np.sqrt(nb) * float(np.linalg.norm(res)) + 64 * rowmax * EPS * float(np.abs(ck) @ (absA @ np.ones(nb))) \
                + fed.mesh.ncell * len(fed.mesh.q_w) * EPS * sabs_int
            I0, _ = integral(fed, nodal(fed, c0[k * nb:(k + 1) * nb], none))
            print(f"tracer {specs[k]['name']} step {step + 1}: int c {I0:.12e} -> {got:.12e}; predicted {predicted:.12e}; |defect| {abs(got - predicted):.3e}, "
                  f"bound {bound:.3e}; dt V = {ts.dt * V:.6e}")
            assert abs(got - predicted) <= bound
            out.append((abs(got - predicted), bound))
    age = tr.values("age")
    print(f"age after 3 steps: min {age.min():.9e}, max {age.max():.9e} (a uniform source keeps it uniform up to the solves' tolerance)")
    assert age.min() > 0.0
    return out


# ---- check 5: refusals -----------------------------------------------------------------------------------------------------------------
def check_refusals(model):
    """every refusal returns NPG_EINVAL with its message, before anything is launched: y keeps its values"""
    import ctypes as C
    lib = L.lib()
    ctx = model.arch.ctx
    fe = model.evolution.fe
    nb, ninv = model.fe_data.dofs.nb, model.inversion.solver.x.n
    h = C.c_void_p()
    for k in (0, -2):
        rc = lib.npg_tracers_create(fe.h, k, C.byref(h))
        assert rc == NPG_EINVAL and "ntracer" in lib.npg_last_error().decode() and not h.value
    tr = npg.PassiveTracers(model, [dict(name="a"), dict(name="b", gamma=0.5)])
    x = model.inversion.solver.x
    V = lambda n: npg.DeviceVector(ctx, n)
    y = V(2 * nb)
    y.fill(-7.0)
    good = dict(c=tr.c, cp=tr.c_prev, x=x, xp=x, rd=tr.rhs_diff1, fl=None, y=y, scheme=L.NPG_BDF2)

    def call(**kw):
        a = dict(good, **kw)
        hh = lambda v: None if v is None else v.h
        rc = lib.npg_tracers_rhs(tr.h, a["scheme"], 0.01, 0.02, a["c"].h, a["cp"].h, a["x"].h, a["xp"].h, hh(a["rd"]), hh(a["fl"]), a["y"].h)
        return rc, lib.npg_last_error().decode()
    cases = [(dict(c=V(2 * nb - 1)), "tracer vectors"), (dict(cp=V(nb)), "tracer vectors"), (dict(x=V(ninv + 1)), "inversion vectors"),
             (dict(xp=V(ninv - 1)), "inversion vectors"), (dict(rd=V(nb + 1)), "rhs_diff1"), (dict(fl=V(nb)), "flux"),
             (dict(y=V(nb)), "output vector"), (dict(rd=None), "background gradient"), (dict(scheme=0), "scheme"), (dict(scheme=3), "scheme")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == NPG_EINVAL and word in msg, (kw.keys(), rc, msg)
        with np.testing.assert_raises(L.DeviceError):
            L.check(rc)
    assert np.array_equal(y.to_host(), np.full(2 * nb, -7.0))                          # nothing was launched
    rc, msg = call()
    assert rc == 0, msg
    assert lib.npg_tracers_set(tr.h, 2, None, 0.0, 0.0) == NPG_EINVAL and "out of range" in lib.npg_last_error().decode()
    assert lib.npg_tracers_set(tr.h, 0, None, float("nan"), 0.0) == NPG_EINVAL
    # coefficient tables that are not set while a tracer has a non-zero Dirichlet value: an engine of its own, without toolkits
    fed = model.fe_data
    assert len(fed.tables.b_diri) > 0
    bare = npg.assembly.DeviceFE(ctx, fed)
    h = C.c_void_p()
    L.check(lib.npg_tracers_create(bare.h, 1, C.byref(h)))
    one, y1 = V(nb), V(nb)
    y1.fill(-7.0)
    args = (h, L.NPG_BDF1, 0.01, 0.02, one.h, one.h, x.h, x.h, None, None, y1.h)
    assert lib.npg_tracers_rhs(*args) == 0                                             # zero Dirichlet values: no table is read
    y1.fill(-7.0)
    dv = L.as_f64(np.ones(len(fed.tables.b_diri)))
    L.check(lib.npg_tracers_set(h, 0, L.ptr(dv), 0.0, 0.0))
    rc = lib.npg_tracers_rhs(*args)
    assert rc == NPG_EINVAL and "kappa_h / kappa_v" in lib.npg_last_error().decode()
    assert np.array_equal(y1.to_host(), np.full(nb, -7.0))
    lib.npg_tracers_destroy(h)
    # a mesh-partitioned model is refused
    fake = SimpleNamespace(**{k: getattr(model, k) for k in ("arch", "fe_data", "params", "forcings", "evolution", "inversion")}, comm=object())
    with np.testing.assert_raises(NotImplementedError):
        npg.PassiveTracers(fake, [dict(name="a")])
    with np.testing.assert_raises(ValueError):
        npg.PassiveTracers(model, [dict(name="a"), dict(name="a")])


# ---- check 6: the device against the host library -------------------------------------------------------------------------------------
def host_library_rhs(model, tr, specs, scheme, dt, theta, x, xp, c, cp):
    """npg_tracers_rhs of libnupgcm_host.so on the same state, loaded BESIDE the library the model runs on and driven through its C
    ABI alone (integrals_ref.host_library_raw)"""
    import ctypes as C
    from nupgcm_amd.assembly import eval_at_quad_points
    H = C.CDLL(L.HOST_LIB_PATH)
    L._declare(H, partial=True)

    def ok(rc):
        assert rc == 0, H.npg_last_error().decode()
    fed, f = model.fe_data, model.forcings
    m = fed.mesh
    k = device_fe(model.arch, fed)._keep
    d = L.FeDesc(ncell=m.ncell, nq=len(m.q_w), nloc_b=k["cb"].shape[1], grad_lambda=k["G"].ctypes.data, wdet=k["wdet"].ctypes.data,
                 qw=k["qw"].ctypes.data, N2=k["N2"].ctypes.data, dN2=k["dN2"].ctypes.data, Nb=k["Nb"].ctypes.data, dNb=k["dNb"].ctypes.data,
                 N1=k["N1"].ctypes.data, cell_u=k["cu"].ctypes.data, cell_p=k["cp"].ctypes.data, cell_b=k["cb"].ctypes.data,
                 u_diri=k["ud"].ctypes.data, n_u_diri=k["ud"].size, b_diri=k["bd"].ctypes.data, n_b_diri=k["bd"].size,
                 n_inv=fed.dofs.nu + fed.dofs.np, n_b=fed.dofs.nb)
    ctx, fe, T = C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(H.npg_ctx_create(0, C.byref(ctx)))
    ok(H.npg_fe_create(ctx, C.byref(d), C.byref(fe)))
    for name, v in (("kappa_h", f.kappa_h), ("kappa_v", f.kappa_v)):
        ok(H.npg_fe_set_coeff(fe, name.encode(), L.ptr(L.as_f64(eval_at_quad_points(m, v)))))
    K, nb = len(specs), fed.dofs.nb

    def vec(a):
        v = C.c_void_p()
        ok(H.npg_vec_create(ctx, len(a), C.byref(v)))
        ok(H.npg_vec_upload(v, L.ptr(L.as_f64(a))))
        return v
    vx, vxp, vc, vcp, vy, vrd = vec(x), vec(xp), vec(c), vec(cp), vec(np.zeros(K * nb)), vec(np.zeros(nb))
    ok(H.npg_fe_assemble_rhs_diff(fe, 1.0, vrd))
    vfl = vec(tr.flux.to_host()) if tr.flux is not None else None
    ok(H.npg_tracers_create(fe, K, C.byref(T)))
    dn = diri_nodes(fed)
    for j, sp in enumerate(specs):
        cd, _ = spec_arrays(model, sp)
        dv = np.zeros(k["bd"].size)
        dv[:len(dn)] = cd[dn]
        ok(H.npg_tracers_set(T, j, L.ptr(L.as_f64(dv)), float(sp.get("gamma", 0.0)), float(sp.get("source", 0.0))))
    ok(H.npg_tracers_rhs(T, scheme, dt, theta, vc, vcp, vx, vxp, vrd, vfl, vy))
    out = np.empty(K * nb)
    ok(H.npg_vec_download(vy, L.ptr(out)))
    H.npg_tracers_destroy(T)
    for v in (vx, vxp, vc, vcp, vy, vrd) + ((vfl,) if vfl is not None else ()):
        H.npg_vec_destroy(v)
    H.npg_fe_destroy(fe)
    H.npg_ctx_destroy(ctx)
    return out


def check_device_against_host(model, label, specs=SPECS3, dt=0.013, theta=0.021):
    """the device right-hand side against the host library's on the same state: the same per-cell arithmetic, within twice the
    summation bound row by row"""
    tr = npg.PassiveTracers(model, specs)
    nb = model.fe_data.dofs.nb
    x, xp, c, cp, xp_dev = random_tracer_state(model, tr)
    for scheme in (L.NPG_BDF1, L.NPG_BDF2):
        y = tr.rhs(scheme, dt, theta, model.inversion.solver.x, xp_dev).to_host()
        host = host_library_rhs(model, tr, specs, scheme, dt, theta, x, xp, c, cp)
        ref = restate_set(model, specs, scheme, dt, theta, x, xp, c, cp)
        bound = 2 * np.concatenate([r.bound for r in ref])
        err = np.abs(y - host)
        report(f"device vs host library {label} scheme {scheme} (bound = 2 x summation; {int(np.count_nonzero(err))} rows differ)", err, bound)
        assert (err <= bound).all()


# ---- check 7: tracers are passive -----------------------------------------------------------------------------------------------------
def check_passive(arch):
    """3 steps of bowl_mixing with model.tracers unset give the same u, p, b bits as 3 steps with tracers set; and among those tracers
    one that starts at 0 with Gamma = S = 0 and zero Dirichlet values stays exactly 0 (beside three that do not)"""
    a = helpers.build_model("bowl_mixing", nsteps=3, arch=arch)
    npg.run(a)
    b = helpers.build_model("bowl_mixing", nsteps=3, arch=arch)
    assert b.tracers is None
    tr = b.tracers = npg.PassiveTracers(b, SPECS3 + [dict(name="nothing")])
    npg.run(b)
    for name in ("u", "p", "b"):
        assert np.array_equal(getattr(a.state, name), getattr(b.state, name)), name
    assert np.array_equal(tr.values("nothing"), np.zeros(tr.nb))
    assert min(np.abs(tr.values(k)).max() for k in ("age", "dye", "salt")) > 0.0
    assert len(tr.stats) == 3 and len(tr.stats[0]) == 4 and len(a.stats) == len(b.stats) == 3


# ---- fp32 element arithmetic (device only) ---------------------------------------------------------------------------------------------
def check_fp32(model, label, dt=0.013):
    """npg_fe_set_precision(fp32): the terms carry fp32 rounding.  The yardstick is the existing npg_fe_advection_rhs in fp32 mode
    against the SAME restatement on the same state (tracer 0 is its twin: Gamma = N2, S = 0, theta = 0 leaves the advection lines
    alone); the measure is max_i |y_i - restated_i| / S_abs_i.  Every tracer of the fused call is allowed twice the yardstick."""
    fe, prm = model.evolution.fe, model.params
    nb = model.fe_data.dofs.nb
    specs = [dict(name="twin", gamma=prm.N2 if prm.N2 != 0.0 else 0.8)] + SPECS3[1:]
    N2 = specs[0]["gamma"]
    tr = npg.PassiveTracers(model, specs)
    x, xp, c, cp, xp_dev = random_tracer_state(model, tr)
    b, bp = npg.DeviceVector.from_host(model.arch.ctx, c[:nb]), npg.DeviceVector.from_host(model.arch.ctx, cp[:nb])
    out = npg.DeviceVector(model.arch.ctx, nb)
    fe.set_precision("fp32")
    try:
        res = {}
        for scheme in (L.NPG_BDF1, L.NPG_BDF2):
            ya = fe.advection_rhs(scheme, dt, N2, b, bp, model.inversion.solver.x, xp_dev, out).to_host()
            y = tr.rhs(scheme, dt, 0.0, model.inversion.solver.x, xp_dev).to_host()
            ref = restate_set(model, specs, scheme, dt, 0.0, x, xp, c, cp)
            yard = float((np.abs(ya - ref[0].total) / ref[0].sabs).max())
            for k, r in enumerate(ref):
                e = float((np.abs(y[k * nb:(k + 1) * nb] - r.total) / r.sabs).max())
                print(f"tracers fp32 {label} scheme {scheme} tracer {k}: max |err| / S_abs = {e:.3e}; npg_fe_advection_rhs fp32: {yard:.3e} "
                      f"(allowed {2 * yard:.3e})")
                assert e <= 2 * yard
                res[(scheme, k)] = (e, yard)
            print(f"tracers fp32 {label} scheme {scheme}: twin column bit-identical to npg_fe_advection_rhs: {np.array_equal(y[:nb], ya)}")
    finally:
        fe.set_precision("fp64")
    return res
