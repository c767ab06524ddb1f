"""The checks of the grid diagnostics (GridDiagnostics / npg_fe_grid_integrals and the host functions on a GridSamples), shared by
tests/test_diagnostics.py (CPU()) and tests/test_gpu_diagnostics.py (GPU()).

The reference values come from the brute-force evaluator of tests/sampling_ref.py (independent of the library: every cell is tried
for every point) reduced with scipy's trapezoid / cumulative_trapezoid written out as postprocess/utils.py:81-94,
streamfunctions.py:14-80 and stratification.py:45-62 write them.

Bounds.  Per sample the library holds 1e-11 max|f| against Brute for u and b and 1e-10 max|grad b| for the gradient
(sampling_ref.compare_values); a trapezoid is a convex combination of samples times the axis extent, and reordering <= 256 terms adds
< 256 eps ~ 3e-14: every integral channel is compared at 1e-10 max|f| extent.  Against the library's own samples (same cells, same
lambda from the same code; what differs is the summation order and instruction selection) the bound is 1e-12 max|f| extent.

Two rules of exclusion, both narrower than a blanket |min lambda| test, because the top row z = 0 of every grid lies ON the mesh's
boundary (min lambda = 0 up to rounding) in every wet column - a blanket rule would exclude all of them:
  * counts: a column / zonal line may differ from the brute-force count only if it holds a point with |min lambda| < 1e-9, and at
    most 1 % of them may (none on the 24^3 grid, where sampling_ref.check_diagnostics already asserts equal masks);
  * d_z b: two cells' gradients legitimately differ at a point within 1e-6 (in lambda) of a face SHARED by two cells, i.e. where
    the second-best cell also holds the point to 1e-6; lines with such a point (at most 1 %) are left out of that channel.  A point
    on a boundary face has one cell and is compared."""
import numpy as np
from scipy.integrate import cumulative_trapezoid, trapezoid

import nupgcm_amd as npg
from nupgcm_amd import _lib as L
from tests import sampling_ref as sr

COL = ("count", "H", "int ux dz", "int uy dz")
ZON = ("count", "width", "int uy dx", "int uz dx", "int b dx", "int max(dz b, 0) dx")
YMIN, YMAX = -0.5, 1.0


def locate2(br, pts, chunk=256):
    """Brute.locate plus the second-largest min lambda over the cells"""
    cell, mn, lam, second = np.empty(len(pts), dtype=np.int64), np.empty(len(pts)), np.empty((len(pts), 4)), np.empty(len(pts))
    for i in range(0, len(pts), chunk):
        Lm = br.lambdas(pts[i:i + chunk])
        m = Lm.min(-1)
        c = m.argmax(1)
        r = np.arange(len(c))
        cell[i:i + chunk], mn[i:i + chunk], lam[i:i + chunk] = c, m[r, c], Lm[r, c]
        m[r, c] = -np.inf
        second[i:i + chunk] = m.max(1)
    return cell, mn, lam, second


def reference_reductions(x, y, z, mask, u, b, bz, alpha):
    """the reference's functions on samples that are zero outside the mesh (mask: 0 / 1 floats)"""
    out = {}
    # utils.depth, calculate_barotropic_streamfunction
    out["H"] = trapezoid(mask, x=z, axis=2)
    U = trapezoid(u[..., 0], x=z, axis=2)
    out["V"] = trapezoid(u[..., 1], x=z, axis=2)
    Psi = trapezoid(U, y, axis=1)[:, None] - cumulative_trapezoid(U, y, axis=1, initial=0)
    nan_mask = np.where(out["H"] == 0)
    out["U_raw"] = U.copy()
    U[nan_mask] = np.nan
    Psi[nan_mask] = np.nan
    out["U"], out["Psi"] = U, Psi
    # utils.zonal_width, zonal_mean, calculate_overturning_streamfunction
    width = trapezoid(mask, x=x, axis=0)
    v_int = trapezoid(u[..., 1], x=x, axis=0)
    out["w_int"] = trapezoid(u[..., 2], x=x, axis=0)
    b_int = trapezoid(b, x=x, axis=0)
    out["b_int"] = b_int
    out["b_bar"] = np.divide(b_int, width, where=width != 0, out=np.full_like(b_int, np.nan))
    psi_bar = -1 / (-z.min()) * cumulative_trapezoid(v_int, z, axis=1, initial=0)
    out["v_raw"] = v_int.copy()
    nan_mask = np.where(width == 0)
    v_int[nan_mask] = np.nan
    psi_bar[nan_mask] = np.nan
    out["width"], out["v_int"], out["psi_bar"] = width, v_int, psi_bar
    # average_stratification
    N2 = alpha * bz
    N2[np.where(N2 < 0)] = 0
    N2[np.where(mask == 0)] = 0
    out["bz_int"] = trapezoid(N2, x=x, axis=0) / alpha
    iymin, iymax = np.searchsorted(y, YMIN), np.searchsorted(y, YMAX)
    area = trapezoid(trapezoid(mask[:, iymin:iymax + 1], x=x, axis=0), x=y[iymin:iymax + 1], axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        out["N2_bar"] = trapezoid(trapezoid(N2[:, iymin:iymax + 1], x=x, axis=0), x=y[iymin:iymax + 1], axis=0) / area
    return out


def _compare(label, names, got, ref, scales, keep, bound):
    """print, then assert, max|got - ref| over the kept entries against bound * scale per channel"""
    worst = []
    for n, g, r, s, k in zip(names, got, ref, scales, keep):
        err = np.abs(g - r)[k].max() if k.any() else 0.0
        worst.append((n, err, bound * s))
    print(f"{label}: " + ", ".join(f"{n} {e:.2e} (bound {t:.2e})" for n, e, t in worst))
    for n, e, t in worst:
        assert e <= t, (label, n, e, t)


def _compare_derived(label, pairs, bound):
    """(name, got, ref[, scale]): NaN in the same places, |got - ref| <= bound * scale elsewhere; scale defaults to max|ref|"""
    for name, got, ref, *scale in pairs:
        assert np.array_equal(np.isnan(got), np.isnan(ref)), (label, name, "NaN masks differ")
        ok = ~np.isnan(ref)
        scale = scale[0] if scale else np.abs(ref[ok]).max()
        err = np.abs(got[ok] - ref[ok]).max()
        print(f"{label}: {name} {err:.2e} of max {scale:.2e} (bound {bound:.0e} relative)")
        assert err <= bound * scale, (label, name, err, scale)


# ---- check 1 -------------------------------------------------------------------------------------------------------------------------
def check_against_brute(model, shape, exact_counts, label=""):
    nx, ny, nz = shape
    gd = npg.GridDiagnostics(model, nx, ny, nz)
    r = gd.compute()
    lo, hi = npg.PointLocator(model).bounding_box
    for a, ax in enumerate((r.x, r.y, r.z)):
        assert np.array_equal(ax, np.linspace(lo[a], hi[a], shape[a]))
    X, Y, Z = np.meshgrid(r.x, r.y, r.z, indexing="ij")
    pts = np.column_stack([X.ravel(), Y.ravel(), Z.ravel()])
    br = sr.Brute(model.fe_data.mesh)
    cell, mn, lam, second = locate2(br, pts)
    valid = (mn >= -1e-10).reshape(shape)
    amb = (np.abs(mn) < sr.AMBIG).reshape(shape)
    shared = (valid.ravel() & (second > -1e-6)).reshape(shape)
    u, _, b, gb = br.fields(model, cell, lam)
    m3 = valid.astype(float)
    u = np.where(valid[..., None], u.reshape(shape + (3,)), 0.0)
    b = np.where(valid, b.reshape(shape), 0.0)
    bz = np.where(valid, gb[:, 2].reshape(shape), 0.0)
    ref = reference_reductions(r.x, r.y, r.z, m3, u, b, bz, model.params.alpha)
    # counts
    bad_c, bad_l = r.count_z != valid.sum(2), r.count_x != valid.sum(0)
    print(f"diagnostics vs brute force {label}{shape}: {valid.sum()} valid points, {amb.sum()} with |min lambda| < 1e-9, {shared.sum()} on a "
          f"shared face; columns / lines whose count differs: {bad_c.sum()} / {bad_l.sum()}; lines left out of dz b: {shared.any(0).sum()}")
    if exact_counts:
        assert not bad_c.any() and not bad_l.any()
    else:
        assert not (bad_c & ~amb.any(2)).any() and not (bad_l & ~amb.any(0)).any()
        assert bad_c.mean() <= 0.01 and bad_l.mean() <= 0.01
    assert shared.any(0).mean() <= 0.01
    Lx, Lz = r.x[-1] - r.x[0], r.z[-1] - r.z[0]
    mu = [np.abs(u[..., a]).max() for a in range(3)]
    okc, okl = ~bad_c, ~bad_l
    _compare(f"columns {label}", COL[1:], r.col[1:], (ref["H"], ref["U_raw"], ref["V"]), (Lz, mu[0] * Lz, mu[1] * Lz), (okc,) * 3, 1e-10)
    _compare(f"zonal lines {label}", ZON[1:], r.zon[1:], (ref["width"], ref["v_raw"], ref["w_int"], ref["b_int"], ref["bz_int"]),
             (Lx, mu[1] * Lx, mu[2] * Lx, np.abs(b).max() * Lx, np.abs(np.maximum(bz, 0)).max() * Lx),
             (okl,) * 4 + (okl & ~shared.any(0),), 1e-10)
    assert mu[0] > 0 and mu[1] > 0 and mu[2] > 0                         # a non-zero flow
    _compare_derived(f"derived {label}", (("H", r.H, ref["H"]), ("U", r.U, ref["U"]), ("Psi", r.Psi, ref["Psi"]), ("width", r.width, ref["width"]),
                                           ("v_int", r.v_int, ref["v_int"]), ("psi_bar", r.psi_bar, ref["psi_bar"]),
                                           ("b_bar", r.b_bar, ref["b_bar"]), ("N2_bar", r.N2_bar(YMIN, YMAX), ref["N2_bar"])), 1e-10)
    return r


# ---- check 2 -------------------------------------------------------------------------------------------------------------------------
def integrals_of_samples(g):
    """col (4, nx, ny) and zon (6, ny, nz) from a GridSamples holding u, b, grad_b"""
    m = g.valid.astype(float)
    z0 = lambda a: np.where(g.valid, np.nan_to_num(a, nan=0.0), 0.0)
    u = [z0(g["u"][..., a]) for a in range(3)]
    col = np.stack([m.sum(2), trapezoid(m, x=g.z, axis=2), trapezoid(u[0], x=g.z, axis=2), trapezoid(u[1], x=g.z, axis=2)])
    zon = np.stack([m.sum(0), trapezoid(m, x=g.x, axis=0), trapezoid(u[1], x=g.x, axis=0), trapezoid(u[2], x=g.x, axis=0),
                    trapezoid(z0(g["b"]), x=g.x, axis=0), trapezoid(np.maximum(z0(g["grad_b"][..., 2]), 0.0), x=g.x, axis=0)])
    scales_c = (1.0, np.abs(u[0]).max(), np.abs(u[1]).max())
    scales_z = (1.0, np.abs(u[1]).max(), np.abs(u[2]).max(), np.abs(z0(g["b"])).max(), np.abs(z0(g["grad_b"][..., 2])).max())
    return col, zon, scales_c, scales_z


def compare_with_samples(r, g, label, bound=1e-12):
    col, zon, sc, sz = integrals_of_samples(g)
    assert np.array_equal(r.count_z, g.valid.sum(2)) and np.array_equal(r.count_x, g.valid.sum(0))
    Lx, Lz = g.x[-1] - g.x[0], g.z[-1] - g.z[0]
    allc, alll = np.ones(col.shape[1:], bool), np.ones(zon.shape[1:], bool)
    _compare(f"columns vs samples {label}", COL[1:], r.col[1:], col[1:], [s * Lz for s in sc], (allc,) * 3, bound)
    _compare(f"zonal lines vs samples {label}", ZON[1:], r.zon[1:], zon[1:], [s * Lx for s in sz], (alll,) * 5, bound)


def check_against_sample_to_grid(model, shape=(24, 24, 24), label=""):
    """the path that exists (sample_to_grid + the host functions) against the fused pass, on the same architecture"""
    nx, ny, nz = shape
    g = npg.sample_to_grid(model, nx, ny, nz, fields=("u", "b", "grad_b"), chunk=5000)
    r = npg.GridDiagnostics(model, nx, ny, nz).compute()
    for a, ax in enumerate((g.x, g.y, g.z)):
        assert np.array_equal((r.x, r.y, r.z)[a], ax)
    compare_with_samples(r, g, label)
    Psi, U = npg.barotropic_streamfunction(g)
    psi_bar, v_int, b_bar = npg.overturning_streamfunction(g)
    width = npg.zonal_width(g)
    N2_bar = npg.average_stratification(g, YMIN, YMAX, alpha=model.params.alpha)
    assert np.array_equal(npg.zonal_mean(g["b"], g), b_bar, equal_nan=True)
    # the derived fields inherit the integrals' bound: 1e-12 x (max|f| x the extents integrated over / the smallest divisor), not
    # 1e-12 of their own maxima - a zonal mean or a streamfunction may be small by cancellation
    _, _, sc, sz = integrals_of_samples(g)
    Lx, Ly, Lz = g.x[-1] - g.x[0], g.y[-1] - g.y[0], g.z[-1] - g.z[0]
    sl = slice(int(np.searchsorted(g.y, YMIN)), int(np.searchsorted(g.y, YMAX)) + 1)
    area = trapezoid(width[sl], x=g.y[sl], axis=0)
    pairs = [("H", r.H, npg.depth(g), Lz), ("width", r.width, width, Lx), ("b_bar", r.b_bar, b_bar, sz[3] * Lx / width[width > 0].min()),
             ("N2_bar", r.N2_bar(YMIN, YMAX), N2_bar, model.params.alpha * sz[4] * Lx * (g.y[sl][-1] - g.y[sl][0]) / area[area > 0].min()),
             ("U", r.U, U, sc[1] * Lz), ("Psi", r.Psi, Psi, sc[1] * Lz * Ly), ("v_int", r.v_int, v_int, sz[1] * Lx),
             ("psi_bar", r.psi_bar, psi_bar, sz[1] * Lx * Lz / -g.z.min())]
    _compare_derived(f"derived vs samples {label}", pairs, 1e-12)
    return r, g


# ---- check 3 -------------------------------------------------------------------------------------------------------------------------
def check_at_rest(model_rest):
    r = npg.GridDiagnostics(model_rest, 24, 24, 24).compute()
    dry, closed = r.H == 0, r.width == 0
    assert dry.any() and (~dry).any() and closed.any() and (~closed).any()
    assert np.array_equal(dry, r.count_z == 0) and np.array_equal(closed, r.count_x == 0)
    for a in (r.U, r.V, r.Psi):
        assert np.isnan(a[dry]).all() and np.array_equal(a[~dry], np.zeros((~dry).sum()))
    for a in (r.v_int, r.w_int, r.psi_bar):
        assert np.isnan(a[closed]).all() and np.array_equal(a[~closed], np.zeros((~closed).sum()))
    assert np.isnan(r.b_bar[closed]).all() and np.isfinite(r.b_bar[~closed]).all()


def check_polynomial(arch, b_order):
    model = sr.bowl_model(arch, "bowl_surface_flux", b_order=b_order)
    if b_order == 2:
        q = lambda x: 1 + x[..., 0] - 2 * x[..., 1] + 0.5 * x[..., 2] + x[..., 0] ** 2 - x[..., 0] * x[..., 1] + 2 * x[..., 1] * x[..., 2] + x[..., 2] ** 2
    else:
        q = lambda x: 1 + x[..., 0] - 2 * x[..., 1] + 0.5 * x[..., 2]
    npg.set_b(model, q)
    N2 = model.params.N2
    r = npg.GridDiagnostics(model, 24, 24, 24).compute()
    X, Y, Z = np.meshgrid(r.x, r.y, r.z, indexing="ij")
    P = np.stack([X, Y, Z], axis=-1)
    _, mn, _ = sr.Brute(model.fe_data.mesh).locate(P.reshape(-1, 3))
    mask = (mn >= -1e-10).reshape(X.shape).astype(float)
    Lx = r.x[-1] - r.x[0]
    qv = q(P)
    ref = trapezoid(mask * (N2 * Z + qv), x=r.x, axis=0)
    eb, tb = np.abs(r.zon[4] - ref).max(), 1e-12 * np.abs(qv[mask > 0]).max() * Lx
    print(f"closed form P{b_order}: int b dx {eb:.2e} (bound {tb:.2e})")
    assert np.array_equal(r.count_x, mask.sum(0)) and eb <= tb
    if b_order == 1:
        eg, tg = np.abs(r.zon[5] - (N2 + 0.5) * r.width).max(), 1e-11 * (N2 + 0.5) * Lx
        print(f"closed form P1: int max(dz b, 0) dx - (N2 + 0.5) width {eg:.2e} (bound {tg:.2e})")
        assert eg <= tg and r.width.max() > 0


# ---- check 4 -------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return np.array_equal(a.col, b.col) and np.array_equal(a.zon, b.zon)


def check_determinism_and_reuse(arch):
    a = sr.bowl_model(arch, "bowl_surface_flux", nsteps=1)
    gd = npg.GridDiagnostics(a, 24, 24, 24)
    r0 = gd.compute()
    assert _same(r0, gd.compute())                                       # the same call twice: the same bits
    for name in ("Psi", "psi_bar", "b_bar"):
        assert np.array_equal(getattr(r0, name), getattr(gd.compute(), name), equal_nan=True)
    a.timestepper.t_stop = 3 * a.timestepper.dt
    npg.run(a)
    r1 = gd.compute()
    assert not _same(r0, r1)                                             # the state moved on
    assert _same(r1, npg.GridDiagnostics(a, 24, 24, 24).compute())       # the kept object = a freshly built one
    # an on_plot hook that computes the diagnostics leaves the run untouched
    seen = []
    h = sr.bowl_model(arch, "bowl_surface_flux")
    h.timestepper.t_stop = 5 * h.timestepper.dt
    hd = npg.GridDiagnostics(h, 24, 24, 24)
    h.on_plot = lambda model, t: seen.append((model.step_index, float(np.nanmax(np.abs(hd.compute().Psi)))))
    npg.run(h, n_plot=2)
    p = sr.bowl_model(arch, "bowl_surface_flux")
    p.timestepper.t_stop = 5 * p.timestepper.dt
    npg.run(p, n_plot=2)
    assert [s[0] for s in seen] == [2, 4] and all(s[1] > 0 for s in seen)
    for f in ("u", "p", "b"):
        assert np.array_equal(getattr(h.state, f), getattr(p.state, f))


# ---- check 5 -------------------------------------------------------------------------------------------------------------------------
def check_periodic(arch):
    model = sr.channel_model(arch, 2)
    r, g = check_against_sample_to_grid(model, (24, 24, 24), label="channel basin P2 ")
    assert r.count_z[0].sum() > 0 and r.count_z[-1].sum() > 0            # the seam columns x = lo and x = hi are both valid
    assert np.array_equal(r.count_z[0], r.count_z[-1])


# ---- check 6 -------------------------------------------------------------------------------------------------------------------------
def check_arguments(model):
    import ctypes as C

    import pytest
    from nupgcm_amd.architectures import Context, DeviceVector
    from nupgcm_amd.assembly import DeviceFE
    with pytest.raises(L.DeviceError, match="strictly increasing"):
        npg.GridDiagnostics(model, 8, 8, 8, y=[-1.0, 0.0, 0.0, 1.0]).compute()
    with pytest.raises(L.DeviceError, match="strictly increasing"):
        npg.GridDiagnostics(model, 8, 8, 8, z=[-0.1, -0.3, 0.0]).compute()
    with pytest.raises(L.DeviceError, match="at least 2 points"):
        npg.GridDiagnostics(model, 1, 8, 8).compute()
    with pytest.raises(L.DeviceError, match="at least 2 points"):
        npg.GridDiagnostics(model, 8, 8, 8, z=[0.0]).compute()
    gd = npg.GridDiagnostics(model, 8, 8, 8)
    ctx = model.arch.ctx
    args = lambda **kw: [kw.get("fe", gd.fe.h), kw.get("loc", gd.loc.h), model.inversion.solver.x.h, kw.get("b", model.b_vec.h),
                         float(model.params.N2), gd._axes.h, 8, 8, 8, kw.get("col", gd._col.h), gd._zon.h]
    short = DeviceVector(ctx, len(model.b_vec) - 1)
    with pytest.raises(L.DeviceError, match="buoyancy vector has"):
        L.check(L.lib().npg_fe_grid_integrals(*args(b=short.h)))
    with pytest.raises(L.DeviceError, match="col must hold"):
        L.check(L.lib().npg_fe_grid_integrals(*args(col=short.h)))
    other = Context(ctx.device)                                          # a second context on the same device
    fe2 = DeviceFE(other, model.fe_data)
    m = model.fe_data.mesh
    loc2 = C.c_void_p()
    L.check(L.lib().npg_locator_create(fe2.h, L.ptr(L.as_f64(m.geo_coords[m.cell_geo[:, 0]])), 0, C.byref(loc2)))
    try:
        with pytest.raises(L.DeviceError, match="different contexts"):
            L.check(L.lib().npg_fe_grid_integrals(*args(loc=loc2)))
    finally:
        L.lib().npg_locator_destroy(loc2)
    gd.compute()                                                         # the object is still usable
    model.partition = object()
    try:
        with pytest.raises(NotImplementedError, match="partitioned"):
            npg.GridDiagnostics(model, 8, 8, 8)
    finally:
        del model.partition
