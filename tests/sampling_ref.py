"""Brute-force fp64 point evaluator and the checks shared by tests/test_sampling.py (CPU()) and tests/test_gpu_sampling.py (GPU()).

The evaluator is independent of the code under test: for each point the cell maximising min lambda over ALL cells, lambda from the
inverted edge matrices of the cells' own geometry (Mesh.geo_coords[Mesh.cell_geo], not grad_lambda), fields from the nodal values
of io._nodal_fields(model) and the closed-form P2 / P1 shape functions."""
import os

import numpy as np

import nupgcm_amd as npg
from nupgcm_amd import io as pio
from nupgcm_amd.fe import _TET_EDGE_A as EA, _TET_EDGE_B as EB
from tests import helpers

SEED = 20261016
AMBIG = 1e-9          # |min lambda| below this: the brute force cannot say inside / outside (skipped, at most 1 %)


class Brute:
    def __init__(self, mesh):
        X = mesh.geo_coords[mesh.cell_geo]                              # (nc, 4, 3) each cell's own vertices
        E = np.transpose(X[:, 1:] - X[:, :1], (0, 2, 1))                # columns = edge vectors
        self.T = np.linalg.inv(E)                                       # rows = grad lambda_1..3
        self.x0 = X[:, 0]
        self.mesh = mesh

    def lambdas(self, pts, cells=None):
        """(n, nc, 4) barycentric coordinates of every point in every cell, or (n, 4) in the given cell of each point"""
        if cells is None:
            d = pts[:, None, :] - self.x0[None]
            l123 = np.einsum("cij,ncj->nci", self.T, d)
        else:
            l123 = np.einsum("nij,nj->ni", self.T[cells], pts - self.x0[cells])
        return np.concatenate([1.0 - l123.sum(-1, keepdims=True), l123], axis=-1)

    def locate(self, pts, chunk=256):
        """cell (argmax over all cells of min lambda), that min lambda and the lambdas there"""
        pts = np.asarray(pts, dtype=float).reshape(-1, 3)
        cell, mn, lam = np.empty(len(pts), dtype=np.int64), np.empty(len(pts)), np.empty((len(pts), 4))
        for i in range(0, len(pts), chunk):
            L = self.lambdas(pts[i:i + chunk])
            m = L.min(-1)
            c = m.argmax(1)
            r = np.arange(len(c))
            cell[i:i + chunk], mn[i:i + chunk], lam[i:i + chunk] = c, m[r, c], L[r, c]
        return cell, mn, lam

    @staticmethod
    def p2(lam):
        return np.concatenate([lam * (2 * lam - 1), 4 * lam[:, EA] * lam[:, EB]], axis=1)

    @staticmethod
    def dp2(lam):
        dN = np.zeros((len(lam), 10, 4))
        for k in range(4):
            dN[:, k, k] = 4 * lam[:, k] - 1
        for e in range(6):
            dN[:, 4 + e, EA[e]] = 4 * lam[:, EB[e]]
            dN[:, 4 + e, EB[e]] = 4 * lam[:, EA[e]]
        return dN

    def fields(self, model, cell, lam):
        """u (n, 3), p, b (full), grad b (n, 3) at (cell, lam) from the model's nodal fields"""
        m = self.mesh
        un, pn, bn = pio._nodal_fields(model)
        N = self.p2(lam)
        cn = m.cell_nodes[cell]
        u = np.einsum("ni,nia->na", N, un[cn])
        p = np.einsum("ni,ni->n", lam, pn[m.cells[cell]])
        b = np.einsum("ni,ni->n", N, bn[cn])
        G = np.concatenate([-self.T[cell].sum(1, keepdims=True), self.T[cell]], axis=1)      # (n, 4, 3)
        gb = np.einsum("ni,nik,nka->na", bn[cn], self.dp2(lam), G)
        return u, p, b, gb


def bowl_model(arch, name, b_order=2, nsteps=0):
    """helpers.build_model with the buoyancy order as an argument (P1: Spaces(..., b_order=1))"""
    prm, frc, btags, bvals, dt, b0 = helpers.product_config(name)
    mesh = npg.Mesh(os.path.join(helpers.GOLDEN, "mesh_bowl3D_h0.1.npz"))
    spaces = npg.Spaces(mesh, u_diri_tags=helpers.U_TAGS, u_diri_vals=helpers.U_VALS, u_diri_masks=helpers.U_MASKS,
                        b_diri_tags=btags, b_diri_vals=bvals, b_order=b_order)
    fed = npg.FEData(mesh, spaces)
    ts = npg.BDF2(t_start=0.0, t_stop=max(nsteps, 1) * dt, dt=dt)
    model = npg.Model(arch, prm, frc, fed, npg.InversionToolkit(arch, fed, prm, frc), npg.EvolutionToolkit(arch, fed, prm, frc, ts), ts)
    if b0 is not None:
        npg.set_b(model, b0)
    if nsteps:
        npg.run(model)
    return model


def channel_model(arch, b_order=2):
    """a small x-periodic channel-basin model with buoyancy b' = sin(2 pi x / W) z (W = 1), P2 or P1"""
    from nupgcm_amd import channel_basin as cb
    from nupgcm_amd import workloads
    prm, frc, _, _, dt, _ = workloads.channel_basin_parameters("flux")
    mesh = npg.Mesh(cb.channel_basin_model(0.125, workloads.CB_ALPHA, dz=0.125))
    assert mesh.periodic
    spaces = npg.Spaces(mesh, u_diri_tags=helpers.U_TAGS, u_diri_vals=helpers.U_VALS, u_diri_masks=helpers.U_MASKS, b_order=b_order)
    fed = npg.FEData(mesh, spaces)
    ts = npg.BDF1(t_start=0.0, t_stop=dt, dt=dt)
    model = npg.Model(arch, prm, frc, fed, npg.InversionToolkit(arch, fed, prm, frc), npg.EvolutionToolkit(arch, fed, prm, frc, ts), ts)
    npg.set_b(model, lambda x: np.sin(2 * np.pi * x[..., 0]) * x[..., 2])
    return model


def box_points(model, n, seed=SEED):
    lo, hi = npg.PointLocator(model).bounding_box
    return lo + np.random.default_rng(seed).random((n, 3)) * (hi - lo)


def compare_values(model, pts, label=""):
    """check 3 of the sampling tests: u, p, b to 1e-11 max|field| everywhere valid, grad b to 1e-10 max|grad b| at points at least
    1e-6 (in lambda) away from a face; returns the measured relative errors (printed before they are asserted)"""
    br = Brute(model.fe_data.mesh)
    cell, mn, lam = br.locate(pts)
    loc = npg.PointLocator(model).locate(pts)
    ok = (mn > AMBIG) & loc.valid
    assert (np.abs(mn) < AMBIG).mean() <= 0.01
    assert np.array_equal(loc.valid[np.abs(mn) >= AMBIG], (mn > 0)[np.abs(mn) >= AMBIG])
    ref = dict(zip(("u", "p", "b", "grad_b"), br.fields(model, cell, lam)))
    away = ok & (mn >= 1e-6)
    assert (ok & ~away).sum() <= 0.01 * max(1, ok.sum())
    errs = {}
    for f, bound in (("u", 1e-11), ("p", 1e-11), ("b", 1e-11), ("grad_b", 1e-10)):
        got = npg.nan_eval(model, f, pts, loc)
        sel = away if f == "grad_b" else ok
        scale = np.abs(ref[f][ok]).max()
        errs[f] = (np.abs(got[sel] - ref[f][sel]).max() / scale if scale > 0 else np.abs(got[sel]).max(), bound)
    print(f"sampling {label}: " + ", ".join(f"{f} {e:.2e} (bound {b:.0e})" for f, (e, b) in errs.items()))
    for f, (e, b) in errs.items():
        assert e <= b, (f, e, b)
    return errs


# ---- the checks themselves (arch = npg.CPU() or npg.GPU()) ------------------------------------------------------------------------
def check_location(model, n=3000):
    pts = box_points(model, n)
    br = Brute(model.fe_data.mesh)
    cell, mn, _ = br.locate(pts)
    loc = npg.PointLocator(model).locate(pts)
    found, valid = loc.cells, loc.valid
    amb = np.abs(mn) < AMBIG
    print(f"location: {n} points, {(mn > 0).mean():.3f} inside, {amb.sum()} ambiguous")
    assert amb.mean() <= 0.01
    assert np.array_equal(valid[~amb], (mn > 0)[~amb]) and np.array_equal(valid, found >= 0)
    v = valid & ~amb
    assert br.lambdas(pts[v], found[v]).min(-1).min() >= -AMBIG          # the found cell contains the point
    assert 0.3 < valid.mean() < 0.5


def check_boundary_slice(model, n=64):
    lo, hi = npg.PointLocator(model).bounding_box
    s = npg.sample_slice(model, y=0.0, bbox=(lo[0], lo[2], hi[0], hi[2]), n=n)
    valid = s["cache"].valid.reshape(n, n)
    _, mn, _ = Brute(model.fe_data.mesh).locate(s["points"])
    mn = mn.reshape(n, n)
    assert s["axes"][1][-1] == hi[2] and valid[:, -1].all()              # the row z = 0: all n points are found
    assert (np.abs(mn[:, -1]) < AMBIG).all()
    assert np.array_equal(valid, mn >= -1e-10)
    assert np.isnan(s["b"][~valid]).all() and np.isfinite(s["u"][valid]).all() and 0.6 < valid.mean() < 0.7


def check_polynomial(arch, b_order):
    model = bowl_model(arch, "bowl_surface_flux", b_order=b_order)
    if b_order == 2:
        q = lambda x: 1 + x[..., 0] - 2 * x[..., 1] + 0.5 * x[..., 2] + x[..., 0] ** 2 - x[..., 0] * x[..., 1] + 2 * x[..., 1] * x[..., 2] + x[..., 2] ** 2
        g = lambda x: np.stack([1 + 2 * x[..., 0] - x[..., 1], -2 - x[..., 0] + 2 * x[..., 2], 0.5 + 2 * x[..., 1] + 2 * x[..., 2]], -1)
    else:
        q = lambda x: 1 + x[..., 0] - 2 * x[..., 1] + 0.5 * x[..., 2]
        g = lambda x: np.broadcast_to([1.0, -2.0, 0.5], x.shape)
    npg.set_b(model, q)
    m = model.fe_data.mesh
    faces = m.coords[m.cells[::7][:, :3]].mean(1)                        # centroids of cell faces: on a face, shared or boundary
    pts = np.vstack([box_points(model, 4000), m.node_coords[::5], faces])
    loc = npg.PointLocator(model).locate(pts)
    ok = loc.valid
    assert ok[4000:].mean() > 0.99 and ok[:4000].sum() > 1000            # nodes and face points are found
    b = npg.nan_eval(model, "b", pts, loc, perturbation=True)
    gb = npg.nan_eval(model, "grad_b", pts, loc, perturbation=True)
    eb = np.abs(b[ok] - q(pts[ok])).max() / np.abs(q(pts[ok])).max()
    eg = np.abs(gb[ok] - g(pts[ok])).max() / np.abs(g(pts[ok])).max()
    print(f"polynomial exactness P{b_order}: b {eb:.2e} (bound 1e-12), grad b {eg:.2e} (bound 1e-11)")
    assert eb <= 1e-12 and eg <= 1e-11
    assert np.isnan(b[~ok]).all() and np.isnan(gb[~ok]).all()


def check_nan_and_determinism(model):
    pts = box_points(model, 3000, seed=7)
    m = model.fe_data.mesh
    pts = np.vstack([pts, m.coords[m.cells[::11][:, :3]].mean(1), m.node_coords[::9], [[5.0, 0, 0], [0, 0, 0.1], [np.nan, 0, -0.1]]])
    locator = npg.PointLocator(model)
    loc = locator.locate(pts)
    cells, lam = loc.cells, loc.lambdas
    out = cells < 0
    assert out[-3:].all() and np.isnan(lam[out]).all() and np.isfinite(lam[~out]).all() and lam[~out].min() >= -1e-10
    for f in ("u", "p", "b", "grad_b"):
        v = npg.nan_eval(model, f, pts, loc)
        assert np.isnan(v[out]).all() and np.isfinite(v[~out]).all(), f
        assert np.array_equal(npg.nan_eval(model, f, pts, loc), v, equal_nan=True)           # through the cache: bit for bit
        assert np.array_equal(npg.nan_eval(model, f, pts), v, equal_nan=True)
    perm = np.random.default_rng(1).permutation(len(pts))
    assert np.array_equal(locator.locate(pts[perm]).cells, cells[perm])                       # the tie-break does not see the order
    # cells handed in by the caller are bounds-checked: an id outside the mesh evaluates to NaN
    bad = npg.Located.from_host(model.arch.ctx, [m.ncell, -7, 0], np.full((3, 4), 0.25))
    v = npg.nan_eval(model, "u", pts[:3], bad)
    assert np.isnan(v[:2]).all() and np.isfinite(v[2]).all()


def check_periodic(arch):
    for order in (2, 1):
        model = channel_model(arch, order)
        m = model.fe_data.mesh
        lo, hi = npg.PointLocator(model).bounding_box
        W = hi[0] - lo[0]
        assert abs(W - 1.0) < 1e-12
        rng = np.random.default_rng(SEED)
        n = 1200
        side = np.where(rng.random(n) < 0.5, lo[0] + 0.125 * rng.random(n), hi[0] - 0.125 * rng.random(n))   # within one cell of the seam
        pts = np.column_stack([side, -1.0 + 0.5 * rng.random(n), -0.1 * rng.random(n)])                     # in the re-entrant channel
        loc = npg.PointLocator(model).locate(pts)
        _, mn, _ = Brute(m).locate(pts)
        assert np.array_equal(loc.valid, mn >= -1e-10) and loc.valid.mean() > 0.5
        assert loc.valid[pts[:, 0] < lo[0] + 0.125].any() and loc.valid[pts[:, 0] > hi[0] - 0.125].any()
        compare_values(model, pts, label=f"channel basin P{order}")
        b = npg.nan_eval(model, "b", pts, loc)
        exact = np.sin(2 * np.pi * pts[:, 0]) * pts[:, 2]
        # (the closed form differs from the interpolant by the interpolation error of this coarse mesh: reported, not asserted - the
        # check of the values is the one against the brute-force evaluator above)
        print(f"channel basin P{order}: |b - sin(2 pi x) z| max {np.abs(b - exact)[loc.valid].max():.2e} of {np.abs(exact).max():.2e}")


def check_diagnostics(model_rest):
    """model_rest: a model whose velocity is zero"""
    g = npg.sample_to_grid(model_rest, 24, 24, 24, chunk=5000)          # several chunks
    br = Brute(model_rest.fe_data.mesh)
    X, Y, Z = np.meshgrid(g.x, g.y, g.z, indexing="ij")
    _, mn, _ = br.locate(np.column_stack([X.ravel(), Y.ravel(), Z.ravel()]))
    mask = (mn >= -1e-10).reshape(24, 24, 24)
    assert np.array_equal(g.valid, mask)
    trap = getattr(np, "trapezoid", None) or np.trapz
    H = npg.depth(g)
    assert np.array_equal(H, trap(mask.astype(float), x=g.z, axis=2)) and H.max() > 0.4
    assert np.isnan(g["b"][~mask]).all() and np.isfinite(g["u"][mask]).all()
    Psi, U = npg.barotropic_streamfunction(g)
    assert np.array_equal(Psi[H > 0], np.zeros((H > 0).sum())) and np.isnan(Psi[H == 0]).all() and (H == 0).any()
    zlo = g.z[0]
    for (x, y) in ((0.3, 0.2), (-0.55, 0.4)):
        prof = npg.sample_profiles(model_rest, x, y, n=32)
        # bisection on the brute-force validity, from the same bracket
        zs = np.linspace(zlo, 0.0, 256)
        ok = br.locate(np.column_stack([np.full(256, x), np.full(256, y), zs]))[1] >= -1e-10
        k = int(np.argmax(ok))
        z_in, z_out = zs[k], zs[k - 1]
        while abs(z_in - z_out) > 1e-8:
            zm = 0.5 * (z_in + z_out)
            if br.locate([[x, y, zm]])[1][0] >= -1e-10:
                z_in = zm
            else:
                z_out = zm
        print(f"profile at ({x}, {y}): H = {prof['H']:.9f}, brute force {-z_in:.9f}, analytic (smooth bottom) {helpers.H(np.array([x, y, 0.0]), 0.5):.6f}")
        assert abs(prof["H"] + z_in) <= 2e-8
        assert prof["cache"].valid.all() and prof["z"][0] == -prof["H"] and np.isfinite(prof["b"]).all()


def check_run_hook(arch):
    calls = []
    a = bowl_model(arch, "bowl_surface_flux")
    a.timestepper.t_stop = 5 * a.timestepper.dt
    a.on_plot = lambda model, t: calls.append((model.step_index, t, float(np.nanmax(np.abs(npg.nan_eval(model, "b", [[0.0, 0.0, -0.1]]))))))
    npg.run(a, n_plot=2)
    b = bowl_model(arch, "bowl_surface_flux")
    b.timestepper.t_stop = 5 * b.timestepper.dt
    npg.run(b, n_plot=2)                                                 # no hook: n_plot changes nothing
    assert [c[0] for c in calls] == [2, 4]                               # mod(i, n_plot) == 0
    assert np.allclose([c[1] for c in calls], [2 * a.timestepper.dt, 4 * a.timestepper.dt], rtol=1e-12)
    for f in ("u", "p", "b"):
        assert np.array_equal(getattr(a.state, f), getattr(b.state, f))
    c = bowl_model(arch, "bowl_surface_flux")
    c.timestepper.t_stop = 5 * c.timestepper.dt
    c.on_plot = lambda model, t: calls.append("never")
    npg.run(c)                                                           # n_plot = inf: the hook never fires
    assert "never" not in calls and np.array_equal(c.state.b, b.state.b)
