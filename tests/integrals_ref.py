"""A numpy restatement of the mesh integrals (nupgcm_amd.integrals) and the checks shared by tests/test_integrals.py
(CPU()) and tests/test_gpu_integrals.py (GPU()).

The restatement is written from the weak forms and fe.p2_tables, not from the code under test: geometry from the cells' own vertex
coordinates (Mesh.geo_coords[Mesh.cell_geo]; inverse / pseudo-inverse of the edge matrix, not grad_lambda), native P2 / P1 elements
(6-node triangles on the embedded 2-D meshes, not the padded tetrahedron), nodal values through Spaces' native tables, coefficients
evaluated at the quadrature points from the forcing functions.  Per channel it returns the terms w_q |J| integrand as an array
(ncell, nq), their math.fsum and S_abs = sum |term|.

Bounds.  A recursive sum of n terms t_k differs from the exact sum by at most (n - 1) eps sum |t_k| (Higham, Accuracy and Stability,
eq. 4.4); any other order of the same terms obeys the same bound, so two summations differ by at most twice that.  The bound used
everywhere is  n_cells n_q eps S_abs  with n_cells the cells that count - derived, not tuned."""
import math
import os
from types import SimpleNamespace

import numpy as np

import nupgcm_amd as npg
from nupgcm_amd import _lib as L
from nupgcm_amd import fe as F
from nupgcm_amd.inversion import device_fe
from tests import helpers
from tests import sampling_ref as sr

EPS = np.finfo(np.float64).eps
NINT = 15
NPG_EINVAL = -1
SEED = 20261017


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def nodal_values(model):
    """(un (nn, 3), bn (nb_nodes,)): velocity and b' at the nodes, Dirichlet nodes with their values, from the device vectors"""
    fed = model.fe_data
    t, s = fed.tables, fed.spaces
    x, b = model.inversion.solver.x.to_host(), model.b_vec.to_host()
    un = np.where(t.u_pos >= 0, x[np.maximum(t.u_pos, 0)], s.u_diri_val)
    bn = np.where(t.b_pos >= 0, b[np.maximum(t.b_pos, 0)], s.b_diri_val)
    return un, bn


def geometry(mesh):
    """(X (nc, k, 3), G (nc, k, 3) = grad lambda, wdet (nc,), lam (nq, k), w (nq,), ea, eb) from the cells' own vertices"""
    X = mesh.geo_coords[mesh.cell_geo]
    k = X.shape[1]
    J = np.transpose(X[:, 1:] - X[:, :1], (0, 2, 1))                    # (nc, 3, k - 1): columns = edge vectors
    if k == 4:
        g = np.linalg.inv(J)
        wdet = np.abs(np.linalg.det(J))
        lam, w = F.tet_quadrature_degree4()
        ea, eb = F._TET_EDGE_A, F._TET_EDGE_B
    else:
        JtJ = np.einsum("cik,cil->ckl", J, J)
        g = np.einsum("ckl,cil->cki", np.linalg.inv(JtJ), J)            # tangential gradients
        wdet = np.sqrt(np.linalg.det(JtJ))
        lam, w = F.tri_quadrature_degree4()
        ea, eb = F._TRI_EDGE_A, F._TRI_EDGE_B
    G = np.concatenate([-g.sum(axis=1, keepdims=True), g], axis=1)
    return X, G, wdet, lam, w, ea, eb


def coefficient(mesh, v, xq):
    if v is None:
        return np.zeros(xq.shape[:2])
    return np.broadcast_to(np.asarray(v(xq), dtype=float), xq.shape[:2]) if callable(v) else np.full(xq.shape[:2], float(v))


def restate(fed, un, bn, nu=None, kh=None, kv=None, full_stress=False, mask=None):
    """terms (NINT, ncells, nq) of the cells that count, totals (math.fsum) and S_abs per channel"""
    m = fed.mesh
    X, G, wdet, lam, w, ea, eb = geometry(m)
    N, dN = F.p2_tables(lam, ea, eb)                                     # (nq, nl), (nq, nl, k)
    uc = un[m.cell_nodes]                                                # (nc, nl, 3)
    if fed.spaces.b_order == 2:
        bc, Nb, dNb = bn[m.cell_nodes], N, dN
    else:
        bc, Nb, dNb = bn[m.cells], lam, np.broadcast_to(np.eye(lam.shape[1]), (len(w),) + (lam.shape[1],) * 2)
    u = np.einsum("qi,cia->cqa", N, uc)
    gu = np.einsum("qik,cia,ckj->cqaj", dN, uc, G)                        # d_j u_a
    b = np.einsum("qi,ci->cq", Nb, bc)
    gb = np.einsum("qik,ci,ckj->cqj", dNb, bc, G)
    xq = np.einsum("qk,cki->cqi", lam, X)
    zq = xq[..., 2]
    cnu, ckh, ckv = (coefficient(m, v, xq) for v in (nu, kh, kv))
    sig = 0.5 * (gu + np.swapaxes(gu, -1, -2))
    W = w[None, :] * wdet[:, None]
    div = gu[..., 0, 0] + gu[..., 1, 1] + gu[..., 2, 2]
    f = [np.ones_like(b), b, b * b, 0.5 * (u[..., 0] ** 2 + u[..., 1] ** 2), 0.5 * u[..., 2] ** 2, u[..., 2] * b,
         cnu * (gu * gu).sum(axis=(-1, -2)), 2.0 * cnu * (sig * sig).sum(axis=(-1, -2)) if full_stress else np.zeros_like(b),
         zq * b, (u * gb).sum(axis=-1), u[..., 2], ckh * (gb[..., 0] ** 2 + gb[..., 1] ** 2) + ckv * gb[..., 2] ** 2,
         ckv * gb[..., 2], ckv, div * div]
    terms = np.stack([W * fi for fi in f])
    if mask is not None:
        terms = terms[:, np.asarray(mask, dtype=bool)]
    tot = np.array([math.fsum(t.ravel()) for t in terms])
    sabs = np.array([math.fsum(np.abs(t).ravel()) for t in terms])
    return terms, tot, sabs


def restate_model(model, mask=None):
    f = model.forcings
    assert not f.eddy_param.is_on or model.step_index == 1, "the closures rewrite the device tables: restate before stepping"
    un, bn = nodal_values(model)
    return restate(model.fe_data, un, bn, f.nu, f.kappa_h, f.kappa_v, bool(callable(f.nu) or f.eddy_param.is_on), mask)


def summation_bound(ncells, nq, sabs):
    return ncells * nq * EPS * sabs


def compare(got, tot, sabs, ncells, nq, label):
    """every channel within the summation bound of the restatement; prints the measured errors first"""
    bound = summation_bound(ncells, nq, sabs)
    err = np.abs(got - tot)
    print(f"integrals {label} ({ncells} cells, nq = {nq}): " +
          ", ".join(f"ch{k} {err[k]:.1e}/{bound[k]:.1e}" for k in range(NINT)))
    for k in range(NINT):
        assert err[k] <= bound[k], (label, k, got[k], tot[k], err[k], bound[k])
    return err, bound


# ---- models -----------------------------------------------------------------------------------------------------------------------
def random_state(model, seed=SEED, scale=1.0):
    """random [u; p] and b' uploaded to the model's vectors"""
    rng = np.random.default_rng(seed)
    x = scale * rng.standard_normal(model.inversion.solver.x.n)
    b = scale * rng.standard_normal(model.b_vec.n)
    model.inversion.solver.x.upload(x)
    model.b_vec.upload(b)
    return x, b


def bowl2d_model(arch):
    """bowl_mixing on the embedded 2-D golden mesh, 3 steps"""
    m = helpers.build_model("bowl_mixing", mesh="mesh_bowl2D_h0.1", nsteps=3, arch=arch)
    npg.run(m)
    return m


def bare_model(arch, b_order=2):
    """what MeshIntegrals reads of a model, without toolkits: bowl3D h = 0.1 spaces WITHOUT velocity Dirichlet tags (a globally linear u
    is representable) and without coefficient tables (the nu / kappa channels are 0)"""
    prm, frc, _, _, _, _ = helpers.product_config("bowl_surface_flux")
    mesh = npg.Mesh(os.path.join(helpers.GOLDEN, "mesh_bowl3D_h0.1.npz"))
    fed = npg.FEData(mesh, npg.Spaces(mesh, b_order=b_order))
    ctx = arch.ctx
    x = npg.DeviceVector(ctx, fed.dofs.nu + fed.dofs.np)
    return SimpleNamespace(arch=arch, fe_data=fed, params=prm, forcings=frc, b_vec=npg.DeviceVector(ctx, fed.dofs.nb),
                           inversion=SimpleNamespace(solver=SimpleNamespace(x=x)), step_index=1)


# ---- the checks (arch = npg.CPU() or npg.GPU()) --------------------------------------------------------------------------------------
def check_channels(model, label, mask=None):
    terms, tot, sabs = restate_model(model, mask)
    mi = npg.MeshIntegrals(model, mask)
    assert mi.ncells_counted == terms.shape[1]
    got = mi.compute_raw()
    assert got.shape == (NINT,) and np.isfinite(got).all()
    return compare(got, tot, sabs, terms.shape[1], terms.shape[2], label)


# int over a tetrahedron of lambda_i N_j / volume, N the P2 basis in fe.p2_tables' order: from int lambda^a = 3! a! / (3 + |a|)! V
def _lambda_p2_moments():
    M = np.zeros((4, 10))
    for i in range(4):
        for j in range(4):
            M[i, j] = 0.0 if i == j else -1.0 / 60.0
        for e, (a, b) in enumerate(zip(F._TET_EDGE_A, F._TET_EDGE_B)):
            M[i, 4 + e] = 1.0 / 15.0 if i in (a, b) else 1.0 / 30.0
    return M


def check_polynomial(arch):
    """b' = a + c . x + quadratic, u = A x + u0 with constant divergence d: int b', int z b', int (div u)^2 = d^2 V and int u_z against
    closed forms summed cell by cell from the vertex coordinates (P2 moments of the tetrahedron - no quadrature)"""
    model = bare_model(arch)
    fed = model.fe_data
    m, t = fed.mesh, fed.tables
    q = lambda x: 1 + x[..., 0] - 2 * x[..., 1] + 0.5 * x[..., 2] + x[..., 0] ** 2 - x[..., 0] * x[..., 1] + 2 * x[..., 1] * x[..., 2] + x[..., 2] ** 2
    A = np.array([[0.3, -1.0, 0.5], [2.0, -0.7, 0.25], [-0.4, 1.5, 1.1]])
    u0 = np.array([0.2, -0.1, 0.05])
    d = np.trace(A)
    Xn = m.node_coords
    un = Xn @ A.T + u0
    x = np.zeros(fed.dofs.nu + fed.dofs.np)
    assert (t.u_pos >= 0).all() and (t.b_pos >= 0).all()
    x[t.u_pos] = un
    b = np.zeros(fed.dofs.nb)
    b[t.b_pos] = q(Xn)
    model.inversion.solver.x.upload(x)
    model.b_vec.upload(b)
    got = npg.MeshIntegrals(model).compute_raw()
    X = m.geo_coords[m.cell_geo]
    V = np.abs(np.linalg.det(X[:, 1:] - X[:, :1])) / 6.0
    mid = 0.5 * (X[:, F._TET_EDGE_A] + X[:, F._TET_EDGE_B])
    bq = q(np.concatenate([X, mid], axis=1))                                           # (nc, 10) nodal values of the quadratic
    wP2 = np.array([-1.0 / 20.0] * 4 + [1.0 / 5.0] * 6)
    uz_v = X @ A[2] + u0[2]                                                            # (nc, 4)
    exact = {0: math.fsum(V), 1: math.fsum(V * (bq @ wP2)), 8: math.fsum(V * np.einsum("ci,ij,cj->c", X[:, :, 2], _lambda_p2_moments(), bq)),
             10: math.fsum(V * uz_v.mean(axis=1)), 14: d * d * math.fsum(V)}
    terms, _, sabs = restate(fed, un, q(Xn))
    bound = summation_bound(m.ncell, terms.shape[2], sabs)
    print("polynomial exactness: " + ", ".join(f"ch{k} |err| {abs(got[k] - v):.2e} (bound {bound[k]:.2e})" for k, v in exact.items()))
    for k, v in exact.items():
        assert abs(got[k] - v) <= bound[k], (k, got[k], v, bound[k])
    for k in (6, 7, 11, 12, 13):                                                       # no coefficient tables: these channels are 0
        assert got[k] == 0.0, k


def _quad_form_bound(A, x, y=None):
    """(n + longest row) eps |x|' |A| |y|: the rounding of y = A x row by row and of the dot product"""
    A = A.tocsr()
    y = x if y is None else y
    rowmax = int(np.diff(A.indptr).max())
    return (A.shape[0] + rowmax) * EPS * float(np.abs(x) @ (abs(A) @ np.abs(y)))


def check_matrix_identities(model, label, variance=False):
    """random x and b, no solve: dissipation against x' A x, buoyancy production against x' (B b + lift) and - variance=True, a
    configuration without Dirichlet b - ch2 against b' M b and ch11 against b' (Kh + Kv) b"""
    prm = model.params
    x, b = random_state(model)
    mi = npg.MeshIntegrals(model)
    r = mi.compute()
    A = model.inversion.solver.A.to_scipy_csr()
    a2e2 = prm.alpha ** 2 * prm.eps ** 2
    ch = 7 if mi.full_stress else 6
    lhs, bound = abs(r.dissipation - x @ (A @ x)), _quad_form_bound(A, x)
    print(f"{label}: |alpha^2 eps^2 ch{ch} - x'Ax| = {lhs:.3e}, bound {bound:.3e} (x'Ax = {x @ (A @ x):.6e})")
    assert lhs <= bound
    out = {"dissipation": (lhs, bound)}
    f = model.forcings
    if callable(f.tau_x) or callable(f.tau_y) or f.tau_x != 0.0 or f.tau_y != 0.0:
        return out                      # inversion.b also carries the wind stress: x' (B b + b0) is then not the buoyancy production
    B = model.inversion.B.to_scipy_csr()
    lift = model.inversion.b.to_host()
    rhs = B @ b + lift
    lhs2 = abs(r.buoyancy_production - x @ rhs)
    bound2 = (len(x) + int(np.diff(B.indptr).max())) * EPS * float(np.abs(x) @ (abs(B) @ np.abs(b) + np.abs(lift)))
    print(f"{label}: |ch5 / alpha - x'(Bb + lift)| = {lhs2:.3e}, bound {bound2:.3e} (x'(Bb + lift) = {x @ rhs:.6e})")
    assert lhs2 <= bound2
    out["production"] = (lhs2, bound2)
    if variance:
        assert (model.fe_data.tables.b_pos >= 0).all()
        ev = model.evolution
        M, K = ev.M.to_scipy_csr(), ev.Kh.to_scipy_csr() + ev.Kv.to_scipy_csr()
        for name, k, mat in (("b'Mb", 2, M), ("b'(Kh+Kv)b", 11, K)):
            e, bd = abs(r.raw[k] - b @ (mat @ b)), _quad_form_bound(mat, b)
            print(f"{label}: |ch{k} - {name}| = {e:.3e}, bound {bd:.3e} ({name} = {b @ (mat @ b):.6e})")
            assert e <= bd
            out[name] = (e, bd)
    return out


def check_energy_balance(arch):
    """bowl_mixing 3-D (no wind) after 3 steps: |dissipation - buoyancy production| <= 2 |x' r|, r = rhs - A x through npg_spmv"""
    model = sr.bowl_model(arch, "bowl_mixing", nsteps=3)
    inv = model.inversion
    s = inv.solver
    r = npg.DeviceVector(model.arch.ctx, s.x.n)
    r.copy_from(inv.b)
    inv.B.mul(model.b_vec, r, alpha=1.0, beta=1.0)                                     # rhs = B b + b0
    s.A.mul(s.x, r, alpha=-1.0, beta=1.0)                                              # r = rhs - A x
    xr = s.x.dot(r)
    bud = npg.MeshIntegrals(model).compute()
    lhs = abs(bud.dissipation - bud.buoyancy_production)
    print(f"energy balance: dissipation {bud.dissipation:.9e}, production {bud.buoyancy_production:.9e}, |difference| {lhs:.3e}, "
          f"|x'r| {abs(xr):.3e} (bound 2 |x'r| = {2 * abs(xr):.3e})")
    assert bud.dissipation > 0
    assert lhs <= 2 * abs(xr)
    return lhs, abs(xr)


def check_buoyancy_conservation(arch):
    """One BDF1 step of the flux configuration (no Dirichlet b: the basis is a partition of unity), as model.evolve codes it.  Summing
    the rows of  (M + theta (Kh + Kv)) b^{n+1} = int (b^n - dt (u^n . grad b^n + u^n_z N2)) phi + theta rhs_diff + dt rhs_flux
    over all DoFs (the lifts vanish, 1' Kh = 1' Kv = 0, 1' rhs_diff = 0; dt = the step update_dt chose, whatever theta the left-hand side
    was built with):
        int b^{n+1} - int b^n = -dt (ch9 + N2 ch10)^n + dt 1' rhs_flux - 1' r_cg,   |1' r_cg| <= sqrt(n_b) ||r_cg||_2"""
    model = helpers.build_model("bowl_surface_flux", nsteps=4, scheme="BDF1", arch=arch)
    model.timestepper.t_stop = np.inf                                                  # update_dt takes CFL-sized steps: count steps, not time
    npg.run(model, n_steps=3)
    ev, prm, ts = model.evolution, model.params, model.timestepper
    assert (model.fe_data.tables.b_pos >= 0).all()
    mi = npg.MeshIntegrals(model)
    r0 = mi.compute_raw()
    nb = model.b_vec.n
    ones = npg.DeviceVector.from_host(model.arch.ctx, np.ones(nb))
    tmp = npg.DeviceVector(model.arch.ctx, nb)
    for K in (ev.Kh, ev.Kv):                                                           # the diffusion matrices and rhs_diff annihilate 1
        # row i of K 1: nnz_i entries, each assembled from at most 64 quadrature terms (a few cells x 11 points)
        K.mul(ones, tmp)
        Ks = K.to_scipy_csr()
        assert (np.abs(tmp.to_host()) <= 64 * np.diff(Ks.indptr) * EPS * np.asarray(abs(Ks).sum(axis=1)).ravel()).all()
    assert abs(ev.rhs_diff.to_host().sum()) <= nb * EPS * np.abs(ev.rhs_diff.to_host()).sum()
    flux = math.fsum(ev.rhs_flux.to_host())
    npg.run(model, n_steps=1)
    assert model.step_index == 5
    r1 = mi.compute_raw()
    s = ev.solver
    res = npg.DeviceVector(model.arch.ctx, nb)
    res.copy_from(s.y)
    s.A.mul(s.x, res, alpha=-1.0, beta=1.0)                                            # r_cg = rhs - A b^{n+1}
    bound = np.sqrt(nb) * res.norm()
    lhs = (r1[1] - r0[1]) - (-ts.dt * (r0[9] + prm.N2 * r0[10]) + ts.dt * flux)
    print(f"buoyancy conservation: int b' {r0[1]:.12e} -> {r1[1]:.12e}, dt {ts.dt:.6e}, advective {r0[9] + prm.N2 * r0[10]:.3e}, "
          f"flux {flux:.6e}; |defect| {abs(lhs):.3e}, bound sqrt(n_b) ||r_cg|| = {bound:.3e}")
    assert abs(lhs) <= bound
    return abs(lhs), bound


def check_determinism_and_masking(model, label):
    mi = npg.MeshIntegrals(model)
    a, b = mi.compute_raw(), mi.compute_raw()
    assert np.array_equal(a, b)
    nc = model.fe_data.mesh.ncell
    mask = np.random.default_rng(SEED).random(nc) < 0.37
    p, q = npg.MeshIntegrals(model, mask), npg.MeshIntegrals(model, ~mask)
    gp, gq = p.compute_raw(), q.compute_raw()
    assert p.ncells_counted + q.ncells_counted == nc and 0 < p.ncells_counted < nc
    terms, _, sabs = restate_model(model)
    bound = summation_bound(nc, terms.shape[2], sabs)
    err = np.abs(gp + gq - a)
    print(f"masking {label}: " + ", ".join(f"ch{k} {err[k]:.1e}/{bound[k]:.1e}" for k in range(NINT)))
    assert (err <= bound).all()
    assert abs(gp[0] + gq[0] - a[0]) <= nc * EPS * a[0]
    assert np.array_equal(npg.MeshIntegrals(model, np.zeros(nc, dtype=bool)).compute_raw(), np.zeros(NINT))   # nothing counts: zeros
    return a


def check_recorder(arch, tmp_path):
    model = sr.bowl_model(arch, "bowl_surface_flux")
    ts = model.timestepper
    ts.t_stop = 10 * ts.dt
    rec = npg.BudgetRecorder(model)
    times = []
    model.on_plot = lambda mdl, t: (times.append(mdl.timestepper.t), rec(mdl, t))
    npg.run(model, n_plot=2, n_steps=6)
    t, raw = rec.as_arrays()
    assert t.shape == (3,) and raw.shape == (3, NINT) and np.array_equal(t, np.array(times)) and np.isfinite(raw).all()
    assert np.array_equal(raw[-1], npg.MeshIntegrals(model).compute_raw())              # the state the hook saw last is the current one
    path = os.path.join(str(tmp_path), "budgets.npz")
    rec.save(path)
    z = np.load(path)
    assert np.array_equal(z["t"], t) and np.array_equal(z["raw"], raw) and len(z["channels"]) == NINT
    assert len(rec.budgets()) == 3 and rec.budgets()[0].volume == raw[0, 0]


def check_refusals(model):
    """wrong lengths, a short `out`, NaN in cell_z and full_stress = 2: NPG_EINVAL with a message, nothing launched"""
    import ctypes as C
    lib = L.lib()
    mi = npg.MeshIntegrals(model)
    ctx = model.arch.ctx
    x, b, out = model.inversion.solver.x, model.b_vec, npg.DeviceVector(ctx, NINT)
    out.fill(-7.0)
    short_x, short_b, short_out = npg.DeviceVector(ctx, x.n - 1), npg.DeviceVector(ctx, b.n + 1), npg.DeviceVector(ctx, NINT - 1)
    for args, word in (((mi.h, short_x.h, b.h, 0, out.h), "flow vector"), ((mi.h, x.h, short_b.h, 0, out.h), "buoyancy vector"),
                       ((mi.h, x.h, b.h, 0, short_out.h), "NPG_NINT"), ((mi.h, x.h, b.h, 2, out.h), "full_stress")):
        rc = lib.npg_integrals_compute(*args)
        msg = lib.npg_last_error().decode()
        assert rc == NPG_EINVAL and word in msg, (rc, msg)
        with np.testing.assert_raises(L.DeviceError):
            L.check(rc)
    assert np.array_equal(out.to_host(), np.full(NINT, -7.0))                          # nothing was launched
    m = model.fe_data.mesh
    z = L.as_f64(m.geo_coords[m.cell_geo][:, :, 2]).copy()
    z[m.ncell // 2, 1] = np.nan
    h = C.c_void_p()
    rc = lib.npg_integrals_create(mi.fe.h, L.ptr(z), None, C.byref(h))
    assert rc == NPG_EINVAL and "not finite" in lib.npg_last_error().decode() and not h.value
    rc = lib.npg_integrals_create(mi.fe.h, None, None, C.byref(h))
    assert rc == NPG_EINVAL and "cell_z" in lib.npg_last_error().decode() and not h.value


def host_library_raw(model, mask=None):
    """the channels of the model's current state through libnupgcm_host.so, loaded BESIDE the library the model runs on (one process
    runs on one architecture: the host library is driven here through its C ABI alone)"""
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
    ctx, fe, I = C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(H.npg_ctx_create(0, C.byref(ctx)))
    ok(H.npg_fe_create(ctx, C.byref(d), C.byref(fe)))
    for name, v in (("nu", f.nu), ("kappa_h", f.kappa_h), ("kappa_v", f.kappa_v)):
        tab = L.as_f64(eval_at_quad_points(m, v))
        ok(H.npg_fe_set_coeff(fe, name.encode(), L.ptr(tab)))
    vecs = []
    for a in (model.inversion.solver.x.to_host(), model.b_vec.to_host(), np.zeros(NINT)):
        v = C.c_void_p()
        ok(H.npg_vec_create(ctx, len(a), C.byref(v)))
        ok(H.npg_vec_upload(v, L.ptr(L.as_f64(a))))
        vecs.append(v)
    z = L.as_f64(m.geo_coords[m.cell_geo][:, :, 2])
    if z.shape[1] == 3:
        z = L.as_f64(np.concatenate([z, np.zeros((len(z), 1))], axis=1))
    m8 = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    ok(H.npg_integrals_create(fe, L.ptr(z), None if m8 is None else L.ptr(m8), C.byref(I)))
    ok(H.npg_integrals_compute(I, vecs[0], vecs[1], int(bool(callable(f.nu) or f.eddy_param.is_on)), vecs[2]))
    out = np.empty(NINT)
    ok(H.npg_vec_download(vecs[2], L.ptr(out)))
    H.npg_integrals_destroy(I)
    for v in vecs:
        H.npg_vec_destroy(v)
    H.npg_fe_destroy(fe)
    H.npg_ctx_destroy(ctx)
    return out


def check_device_against_host(model, label, mask=None):
    """the device kernel against the host library on the same state: the same per-cell arithmetic, two summation orders"""
    terms, _, sabs = restate_model(model, mask)
    bound = summation_bound(terms.shape[1], terms.shape[2], sabs)
    got, host = npg.MeshIntegrals(model, mask).compute_raw(), host_library_raw(model, mask)
    err = np.abs(got - host)
    print(f"device vs host library {label} ({terms.shape[1]} cells): " + ", ".join(f"ch{k} {err[k]:.1e}/{bound[k]:.1e}" for k in range(NINT)))
    assert (err <= bound).all()
