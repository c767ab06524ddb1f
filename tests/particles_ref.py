"""The checks shared by tests/test_particles.py (CPU()) and tests/test_gpu_particles.py (GPU()) for the particle tracker
(nupgcm_amd.particles), as tests/sampling_ref.py holds those of the sampling.

Every reference is independent of the code under test: closed forms of RK4 on affine flows (the map x -> P4(hA) x + h Q(hA) u0 with
P4, Q the Taylor polynomials of exp and (exp - 1)/z - whatever cells the stage points fall in), a numpy RK4 of the scalar ODE
zeta' = i omega(t) zeta, sampling_ref.Brute for leaving the mesh, and npg.nan_eval / PointLocator (tested by the sampling suites) for
the real state.

Bounds.  An affine field is reproduced by P2 evaluation up to rounding: 10 products and sums per component, |N_i| <= 1.  An RK4 step
adds four evaluations and some ten more operations per component, each relative to max|x| <= 1 with |hA| < 1, and the errors of n
steps add (rotations have norm 1): n . 64 . eps . max|x|.  A uniform flow: k steps of x + (h/6)(6 u0), k . 8 . eps."""
import ctypes as C
import functools
import os
from types import SimpleNamespace

import numpy as np

import nupgcm_amd as npg
from nupgcm_amd import _lib as L
from tests import helpers
from tests import sampling_ref as sr

EPS = np.finfo(np.float64).eps
SEED = 20261018
NPG_EINVAL = -1
SYMBOLS = {"npg_particles_create", "npg_particles_destroy", "npg_particles_set", "npg_particles_set_period", "npg_particles_advance",
           "npg_particles_download", "npg_particles_positions"}
JZ = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
A_GENERAL = np.array([[0.3, -1.0, 0.5], [2.0, -0.7, 0.25], [-0.4, 1.5, 1.1]])         # those of integrals_ref.check_polynomial
U0_GENERAL = np.array([0.2, -0.1, 0.05])


# ---- seeds, flows, closed forms -----------------------------------------------------------------------------------------------------
def safe_seeds(n=2000, rmax=0.6, zmin=-0.25, zmax=-0.02, seed=SEED):
    """n random points of the bowl with r <= rmax and zmin <= z <= zmax.  The bowl's depth is (1 - r^2)/2: on the golden mesh the deepest
    node in 0.6 <= r < 0.7 is at z = -0.320, so a horizontal circle through a point with r <= 0.6, z >= -0.25 stays inside the mesh."""
    rng = np.random.default_rng(seed)
    r, phi = rmax * np.sqrt(rng.random(n)), 2 * np.pi * rng.random(n)
    return np.column_stack([r * np.cos(phi), r * np.sin(phi), zmin + (zmax - zmin) * rng.random(n)])


def affine_vector(model, A, u0):
    """[u; p] with u = A x + u0 at the velocity nodes (no velocity Dirichlet DoFs: represented exactly), p = 0"""
    fed = model.fe_data
    t = fed.tables
    assert (t.u_pos >= 0).all()
    x = np.zeros(fed.dofs.nu + fed.dofs.np)
    x[t.u_pos] = fed.mesh.node_coords @ np.asarray(A, dtype=float).T + np.asarray(u0, dtype=float)
    return x


def set_affine(model, A, u0=(0.0, 0.0, 0.0)):
    model.inversion.solver.x.upload(affine_vector(model, A, u0))


def rk4_affine_maps(A, h):
    """(P, q): one RK4 step of x' = A x + u0 is x -> P x + q u0, P = P4(hA), q = h (I + hA/2 + (hA)^2/6 + (hA)^3/24)"""
    Z = h * np.asarray(A, dtype=float)
    I = np.eye(3)
    return I + Z + Z @ Z / 2 + Z @ Z @ Z / 6 + Z @ Z @ Z @ Z / 24, h * (I + Z / 2 + Z @ Z / 6 + Z @ Z @ Z / 24)


def channel_bare(arch):
    """sampling_ref.channel_model's mesh with tag-free Spaces and no toolkits (integrals_ref.bare_model for the channel basin)"""
    from nupgcm_amd import channel_basin as cb
    from nupgcm_amd import workloads
    prm, frc, _, _, _, _ = workloads.channel_basin_parameters("flux")
    mesh = npg.Mesh(cb.channel_basin_model(0.125, workloads.CB_ALPHA, dz=0.125))
    assert mesh.periodic
    fed = npg.FEData(mesh, npg.Spaces(mesh))
    ctx = arch.ctx
    x = npg.DeviceVector(ctx, fed.dofs.nu + fed.dofs.np)
    return SimpleNamespace(arch=arch, fe_data=fed, params=prm, forcings=frc, b_vec=npg.DeviceVector(ctx, fed.dofs.nb),
                           inversion=SimpleNamespace(solver=SimpleNamespace(x=x)), step_index=1)


def snapshot(tr):
    return dict(x=tr.positions, cells=tr.cells, status=tr.status, wind=tr.wind, t_lost=tr.t_lost)


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=(k == "t_lost")) for k in a)


# ---- 1. affine flow, closed form across cells ---------------------------------------------------------------------------------------
def check_rotation(model, omega=1.0, h=0.05, calls=7, nsub=18):
    """(a) solid-body rotation about z, about one turn in calls x nsub = 126 steps, against P4(hA)^126 x0"""
    x0 = safe_seeds()
    set_affine(model, omega * JZ)
    tr = npg.ParticleTracker(model, x0, t0=0.0, nsub=nsub)
    seen = [tr.cells]
    for _ in range(calls):
        tr.advance(h * nsub)
        seen.append(tr.cells)
    n = calls * nsub
    P, _ = rk4_affine_maps(omega * JZ, h)
    ref = x0.copy()
    for _ in range(n):
        ref = ref @ P.T
    got = tr.positions
    err, tol = np.abs(got - ref).max(), n * 64 * EPS * np.abs(ref).max()
    r0, r1 = np.hypot(x0[:, 0], x0[:, 1]), np.hypot(got[:, 0], got[:, 1])
    shrink = (1 - (omega * h) ** 6 / 144) ** n
    moved = np.mean([len(set(c)) >= 4 for c in np.array(seen).T])        # (after a whole turn a particle is back where it started)
    print(f"rotation: {n} steps of h = {h}, max|x - P4^n x0| = {err:.3e} (bound {tol:.3e}); radius ratio {np.median(r1 / r0):.15f} "
          f"(RK4: {shrink:.15f}); lost {int(tr.status.sum())}; {moved:.2f} of the particles seen in >= 4 cells at the 8 call boundaries; t = {tr.t}")
    assert not tr.status.any() and np.isnan(tr.t_lost).all()
    assert moved > 0.5                                                   # particles cross many cells
    assert err <= tol
    assert abs(tr.t - n * h) <= n * EPS * n * h
    return err, tol


def check_general_affine(model, h=0.02, nsteps=2):
    """(b) a general A and u0, 2 steps; seeds r <= 0.4, z <= -0.12: the displacement is < 0.1, inside the margin"""
    x0 = safe_seeds(rmax=0.4, zmax=-0.12)
    set_affine(model, A_GENERAL, U0_GENERAL)
    tr = npg.ParticleTracker(model, x0, t0=0.0, nsub=1)
    for _ in range(nsteps):
        tr.advance(h)
    P, q = rk4_affine_maps(A_GENERAL, h)
    ref = x0.copy()
    for _ in range(nsteps):
        ref = ref @ P.T + q @ U0_GENERAL
    got = tr.positions
    err, tol = np.abs(got - ref).max(), nsteps * 64 * EPS * np.abs(ref).max()
    print(f"general affine: {nsteps} steps of h = {h}, max|x - closed form| = {err:.3e} (bound {tol:.3e}), "
          f"largest displacement {np.abs(got - x0).max():.3f}, lost {int(tr.status.sum())}")
    assert not tr.status.any() and np.abs(got - x0).max() < 0.1
    assert err <= tol
    return err, tol


# ---- 2. leaving the mesh ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _leaving_reference(h, nsteps):
    """Brute-force prediction for u = (0.5, 0, 0) from the safe seeds: the points of the closed-form path are q_j = x0 + j (h/2) u0;
    step k needs its stage points q_2k, q_2k+1 (twice), q_2k+2 and its end point q_2k+2 located, min lambda >= -1e-10.  Returns the
    step at which each particle is lost (nsteps = never) and whether a min lambda on its path up to there lies within 1e-8 of -1e-10.
    sampling_ref.Brute's lambdas, maximised over every cell that can hold a point of the path: y and z do not change along it, so these
    are the cells whose own (y, z) bounding box, padded by 1e-6, holds the particle's (y, z) - in any other cell min lambda < -1e-6 all
    along.  (All 4259 cells for each of the 130 000 path points take minutes.)  A particle is followed until the prediction has lost it;
    the restriction is cross-checked against Brute.locate itself, over all cells, on the decisive points of 128 particles."""
    mesh = npg.Mesh(os.path.join(helpers.GOLDEN, "mesh_bowl3D_h0.1.npz"))
    br = sr.Brute(mesh)
    x0 = safe_seeds()
    u0 = np.array([0.5, 0.0, 0.0])
    n = len(x0)
    X = mesh.geo_coords[mesh.cell_geo]
    clo, chi = X.min(axis=1) - 1e-6, X.max(axis=1) + 1e-6
    near = np.ones((n, len(X)), dtype=bool)
    for a in (1, 2):
        near &= (x0[:, None, a] >= clo[None, :, a]) & (x0[:, None, a] <= chi[None, :, a])
    pi, pc = np.nonzero(near)                                            # pairs (particle, candidate cell), sorted by particle
    assert len(np.unique(pi)) == n
    lost = np.full(n, nsteps, dtype=np.int64)
    amb = np.zeros(n, dtype=bool)
    alive = np.ones(n, dtype=bool)
    first_out = np.zeros(n, dtype=np.int64)
    for j in range(2 * nsteps + 1):
        if not alive.any():
            break
        sel = alive[pi]
        spi, spc = pi[sel], pc[sel]
        live = np.nonzero(alive)[0]
        mins = br.lambdas(x0[spi] + j * (0.5 * h) * u0, spc).min(-1)
        mn = np.maximum.reduceat(mins, np.searchsorted(spi, live))
        amb[live] |= np.abs(mn + 1e-10) < 1e-8
        out = live[mn < -1e-10]
        lost[out] = max(j - 1, 0) // 2                                   # q_j belongs to step (j - 1) // 2 (q_0: step 0)
        first_out[out] = j
        alive[out] = False
    some = np.nonzero(~alive)[0][:128]
    for dj, inside in ((0, False), (-1, True)):
        jj = first_out[some] + dj
        _, mn, _ = br.locate(x0[some] + (jj * (0.5 * h))[:, None] * u0)
        assert np.array_equal(mn >= -1e-10, np.full(len(some), inside) | (jj < 0))
    return lost, amb


def check_leaving(model, h=0.05, nsteps=60, until=68):
    """u = (0.5, 0, 0) from the safe seeds, 60 steps of h = 0.05 - and 8 more: a seed with x0 = -0.6 is at x = 0.9 after 60 steps,
    inside the bowl near the surface (8 particles of the 2000 are still alive then); after 68 every x >= 1.1, so every particle must
    have been lost.  Every check runs over all 68 steps."""
    u0 = np.array([0.5, 0.0, 0.0])
    x0 = safe_seeds()
    set_affine(model, np.zeros((3, 3)), u0)
    tr = npg.ParticleTracker(model, x0, t0=0.0, nsub=1)
    assert not tr.status.any()
    assert (x0[:, 0] + until * h * u0[0]).min() > 1.0
    lost_at = np.full(len(x0), until, dtype=np.int64)
    t, times, worst, alive60 = 0.0, [], 0.0, None
    for k in range(until):
        times.append(t)
        tr.advance(h)
        t = t + h
        st = tr.status
        lost_at[(st == 1) & (lost_at == until)] = k
        alive = st == 0
        if k == nsteps - 1:
            alive60 = int(alive.sum())
        if alive.any():
            e = np.abs(tr.positions[alive] - (x0[alive] + (k + 1) * h * u0)).max()
            worst = max(worst, e / ((k + 1) * 8 * EPS))
            assert e <= (k + 1) * 8 * EPS, (k, e)
    times = np.array(times + [t])
    ref, amb = _leaving_reference(h, until)
    print(f"leaving: {alive60} alive after {nsteps} steps, all {len(x0)} lost by step {lost_at.max()} (first {lost_at.min()}); while alive "
          f"|x - (x0 + k h u0)| at most {worst:.2f} of k 8 eps; {int(amb.sum())} particles excluded as ambiguous (a brute-force min "
          f"lambda within 1e-8 of -1e-10)")
    assert tr.status.all() and (lost_at < until).all()                   # x has reached r > 1
    assert amb.mean() <= 0.01
    ok = ~amb
    assert np.array_equal(lost_at[ok], ref[ok]), np.nonzero(lost_at[ok] != ref[ok])[0][:10]
    frozen, tl = tr.positions, tr.t_lost
    e = np.abs(frozen - (x0 + lost_at[:, None] * h * u0)) - lost_at[:, None] * 8 * EPS
    print(f"leaving: frozen position against x0 + k h u0: excess over k 8 eps {e.max():.3e} (<= 0); t_lost against the clock: "
          f"{np.abs(tl - times[lost_at]).max():.3e}")
    assert (e <= 0).all()
    assert np.array_equal(tl, times[lost_at])                            # the time at the start of the step, as the clock counted it
    tr.advance(h)
    tr.advance(-3 * h)
    assert np.array_equal(tr.positions, frozen) and np.array_equal(tr.t_lost, tl) and tr.status.all()    # nothing moves the lost


# ---- 3. time blend ------------------------------------------------------------------------------------------------------------------
def check_blend(model, wa=0.5, wb=1.5, dt=0.4, nsub=8):
    x0 = safe_seeds()
    ctx = model.arch.ctx
    xa = npg.DeviceVector.from_host(ctx, affine_vector(model, wa * JZ, np.zeros(3)))
    set_affine(model, wb * JZ)
    tr = npg.ParticleTracker(model, x0, t0=0.0, nsub=nsub)
    tr.advance(dt, x_prev=xa)
    h = dt / nsub
    w = lambda t: wa + (wb - wa) * (t / dt)
    f = lambda t, z: 1j * w(t) * z
    z = x0[:, 0] + 1j * x0[:, 1]
    for j in range(nsub):
        t = j * h
        k1 = f(t, z)
        k2 = f(t + h / 2, z + h / 2 * k1)
        k3 = f(t + h / 2, z + h / 2 * k2)
        k4 = f(t + h, z + h * k3)
        z = z + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    ref = np.column_stack([z.real, z.imag, x0[:, 2]])
    got = tr.positions
    err, tol = np.abs(got - ref).max(), nsub * 64 * EPS * np.abs(ref).max()
    angle = np.median(np.angle((got[:, 0] + 1j * got[:, 1]) / (x0[:, 0] + 1j * x0[:, 1])))
    print(f"time blend: omega {wa} -> {wb} over dt = {dt}, {nsub} steps: max|x - numpy RK4| = {err:.3e} (bound {tol:.3e}); "
          f"turned by {angle:.6f} (mean omega dt = {0.5 * (wa + wb) * dt:.6f}); lost {int(tr.status.sum())}")
    assert not tr.status.any()
    assert abs(angle - 0.5 * (wa + wb) * dt) < 1e-6 and abs(angle - wb * dt) > 0.1       # it is the blend, not either end
    assert np.array_equal(got[:, 2], x0[:, 2])
    assert err <= tol
    # the same vector twice - by handle, or a second handle on the same memory - is the frozen instance, bit for bit
    x = model.inversion.solver.x
    frozen = npg.ParticleTracker(model, x0, t0=0.0, nsub=nsub).advance(dt)
    for same in (x, x.view(0, x.n)):
        twice = npg.ParticleTracker(model, x0, t0=0.0, nsub=nsub).advance(dt, x_prev=same)
        assert same_bits(snapshot(frozen), snapshot(twice))
    assert not np.array_equal(frozen.positions, got)
    return err, tol


# ---- 4. the real state, against nan_eval ----------------------------------------------------------------------------------------------
def half_cell_step(model, cell=0.1):
    """h with h max|u| = half a cell of the golden mesh (h = 0.1)"""
    return 0.5 * cell / float(np.abs(model.state.u).max())


def numpy_step(model, x, h):
    """one RK4 step restated with npg.nan_eval as the velocity: (x+, lost) - lost where a stage velocity is NaN or x+ is outside"""
    u = lambda p: npg.nan_eval(model, "u", p)
    k1 = u(x)
    k2 = u(x + (0.5 * h) * k1)
    k3 = u(x + (0.5 * h) * k2)
    k4 = u(x + h * k3)
    xp = x + (h / 6.0) * (((k1 + 2.0 * k2) + 2.0 * k3) + k4)
    lost = np.isnan(k1).any(1) | np.isnan(k2).any(1) | np.isnan(k3).any(1) | np.isnan(k4).any(1)
    lost[~lost] = ~npg.PointLocator(model).locate(xp[~lost]).valid
    return np.where(lost[:, None], x, xp), lost


def check_real_state(model, label, n=3000, more=20):
    x0 = sr.box_points(model, n)
    h = half_cell_step(model)
    tr = npg.ParticleTracker(model, x0, nsub=1)
    inside = npg.PointLocator(model).locate(x0).valid
    assert np.array_equal(tr.status == 0, inside) and 0.3 < inside.mean() < 0.5          # seeds outside the mesh are lost at t0
    assert np.array_equal(tr.t_lost[~inside], np.full((~inside).sum(), tr.t))
    tr.advance(h)
    ref, lost = numpy_step(model, x0, h)
    lost |= ~inside
    got, st = tr.positions, tr.status
    scale = np.abs(x0).max()
    err = np.abs(got - ref).max()
    print(f"real state {label}: h = {h:.4e} (h max|u| = 0.05), {int(inside.sum())} of {n} seeds inside, {int(lost.sum() - (~inside).sum())} "
          f"lost in the step; max|x - numpy step through nan_eval| = {err:.3e} (bound {1e-12 * scale:.1e})")
    assert np.array_equal(st == 1, lost)
    assert err <= 1e-12 * scale
    assert np.array_equal(got[lost], x0[lost])
    assert np.array_equal(tr.cells, npg.PointLocator(model).locate(got).cells)           # the remembered cell IS the elected cell
    for _ in range(more):
        tr.advance(h)
    got = tr.positions
    moved = np.abs(got - x0).max(axis=1)[tr.status == 0]
    print(f"real state {label}: after {more} more steps {int((tr.status == 0).sum())} alive, median displacement {np.median(moved):.3f}")
    assert np.array_equal(tr.cells, npg.PointLocator(model).locate(got).cells)
    v = tr.sample("u")
    assert np.array_equal(v, npg.nan_eval(model, "u", got), equal_nan=True)
    return err


# ---- 5. determinism -----------------------------------------------------------------------------------------------------------------
def check_determinism(model, dt=0.25, nsub=8):
    """rotation plus a drift, seeds inside and outside: some particles leave on the way.  dt / nsub = 2^-5: the clocks of one call and
    of eight agree to the bit"""
    x0 = np.vstack([safe_seeds(1500), sr.box_points(model, 500)])
    set_affine(model, JZ, (0.3, 0.0, 0.0))
    one = npg.ParticleTracker(model, x0, t0=0.0, nsub=nsub)
    eight = npg.ParticleTracker(model, x0, t0=0.0, nsub=1)
    for _ in range(6):
        one.advance(dt)
        for _ in range(nsub):
            eight.advance(dt / nsub)
    a = snapshot(one)
    on_the_way = (a["status"] == 1) & (a["t_lost"] > 0)
    print(f"determinism: {len(x0)} particles, {int((a['status'] == 0).sum())} alive after {6 * nsub} steps, {int(on_the_way.sum())} lost on the way")
    assert on_the_way.sum() > 10 and (a["status"] == 0).sum() > 10
    assert same_bits(a, snapshot(eight)) and one.t == eight.t
    perm = np.random.default_rng(3).permutation(len(x0))
    p = npg.ParticleTracker(model, x0[perm], t0=0.0, nsub=nsub)
    twin = npg.ParticleTracker(model, x0, t0=0.0, nsub=nsub)
    for _ in range(6):
        p.advance(dt)
        twin.advance(dt)
    assert same_bits({k: v[perm] for k, v in a.items()}, snapshot(p))
    assert same_bits(a, snapshot(twin))


# ---- 6. periodic seam ---------------------------------------------------------------------------------------------------------------
def check_periodic(arch, h=0.07, nsteps=40):
    model = channel_bare(arch)
    set_affine(model, np.zeros((3, 3)), (1.0, 0.0, 0.0))
    lo, hi = npg.PointLocator(model).bounding_box
    W = hi[0] - lo[0]
    assert abs(W - 1.0) < 1e-12
    # drawn as sampling_ref.check_periodic draws them; kept where the channel has its full depth alpha W = 0.125 for every x
    # (channel_basin.depth: y <= -1 + 5/16, on this mesh the rows y <= -0.75), so that a line of constant (y, z) stays in the mesh
    rng = np.random.default_rng(sr.SEED)
    n = 1200
    side = np.where(rng.random(n) < 0.5, lo[0] + 0.125 * rng.random(n), hi[0] - 0.125 * rng.random(n))
    pts = np.column_stack([side, -1.0 + 0.5 * rng.random(n), -0.1 * rng.random(n)])
    x0 = pts[pts[:, 1] <= -0.75]
    assert len(x0) > 400
    tr = npg.ParticleTracker(model, x0, t0=0.0, nsub=1)
    assert np.array_equal(tr.period, [W, 0.0, 0.0])                      # from the mesh's periodic pairing
    for _ in range(nsteps):
        tr.advance(h)
    k = nsteps
    wind = np.floor((x0[:, 0] + k * h - lo[0]) / W).astype(np.int64)
    ref = x0.copy()
    ref[:, 0] = x0[:, 0] + k * h - wind * W
    got, unw = tr.positions, tr.unwrapped
    e1, e2, tol = np.abs(got - ref).max(), np.abs(unw[:, 0] - (x0[:, 0] + k * h)).max(), k * 8 * EPS * W
    print(f"periodic seam: {len(x0)} particles, {k} steps of h = {h} ({k * h / W:.1f} periods), wind {wind.min()} .. {wind.max()}; "
          f"|x - wrapped closed form| = {e1:.3e}, |unwrapped - (x0 + k h)| = {e2:.3e} (bound {tol:.3e}); lost {int(tr.status.sum())}")
    assert not tr.status.any()
    assert np.array_equal(tr.wind[:, 0], wind) and not tr.wind[:, 1:].any() and wind.min() >= 2
    assert e1 <= tol and e2 <= tol + EPS * np.abs(unw).max()           # the sum x + wind W rounds once more
    assert (got[:, 0] >= lo[0]).all() and (got[:, 0] < lo[0] + W).all()
    # without the period the same particles are lost at the seam: the last position is within one step of x = hi
    tr0 = npg.ParticleTracker(model, x0, t0=0.0, nsub=1, periodic=(0, 0, 0))
    for _ in range(nsteps):
        tr0.advance(h)
    xs = tr0.positions[:, 0]
    print(f"periodic seam, period forced to 0: lost {int(tr0.status.sum())} of {len(x0)}, stopped at x in [{xs.min():.4f}, {xs.max():.4f}]")
    assert tr0.status.all() and not tr0.wind.any()
    assert (xs <= hi[0]).all() and (xs + h > hi[0] - 1e-9).all()


# ---- 7. the hook --------------------------------------------------------------------------------------------------------------------
def check_hook(arch, tmp_path, nsteps=4):
    def fresh():
        m = sr.bowl_model(arch, "bowl_surface_flux")
        m.timestepper.t_stop = nsteps * m.timestepper.dt
        return m
    plain = fresh()
    npg.run(plain, n_plot=2)
    x0 = safe_seeds(500)
    for n_plot in (1, 2):
        m = fresh()
        tr = npg.ParticleTracker(m, x0)
        assert tr.t == m.timestepper.t == 0.0
        m.on_plot = tr
        npg.run(m, n_plot=n_plot)
        for f in ("u", "p", "b"):
            assert np.array_equal(getattr(m.state, f), getattr(plain.state, f)), (n_plot, f)     # the run does not see the tracker
        calls = nsteps // n_plot
        t, x, status = tr.as_arrays()
        print(f"hook n_plot = {n_plot}: {calls} calls, tracker.t = {tr.t!r}, model t = {m.timestepper.t!r}, "
              f"largest displacement {np.abs(x[-1] - x0).max():.3e}, lost {int(status[-1].sum())}")
        assert len(tr.history) == calls and t.shape == (calls,) and x.shape == (calls, len(x0), 3) and status.shape == (calls, len(x0))
        assert tr.t == m.timestepper.t == t[-1]
        assert np.allclose(t, n_plot * m.timestepper.dt * np.arange(1, calls + 1), rtol=1e-12)
        assert np.array_equal(x[-1], tr.unwrapped) and np.abs(x[-1] - x0).max() > 0
        path = os.path.join(str(tmp_path), f"particles_{n_plot}.npz")
        tr.save(path)
        z = np.load(path)
        assert np.array_equal(z["t"], t) and np.array_equal(z["x"], x) and np.array_equal(z["status"], status)
        assert np.array_equal(z["t_lost"], tr.t_lost, equal_nan=True) and np.array_equal(z["period"], np.zeros(3))


# ---- 8. errors and ABI --------------------------------------------------------------------------------------------------------------
def check_exports():
    assert SYMBOLS <= set(L.declared_symbols())
    for path in (L.HOST_LIB_PATH, L.LIB_PATH):
        lib = C.CDLL(path)
        assert not [s for s in SYMBOLS if not hasattr(lib, s)], path


def _partitioned_locator(model):
    """a partitioned locator handle over ALL the cells of the mesh (one rank that owns everything), or None where the library has no
    npg_locator_create_cells (the host library: partitioned models are device work)"""
    lib = L.lib()
    if not hasattr(lib, "npg_locator_create_cells"):
        return None
    m = model.fe_data.mesh
    anchor = L.as_f64(m.geo_coords[m.cell_geo[:, 0]])
    G = L.as_f64(m.grad_lambda).reshape(m.ncell, 12)
    geo12 = L.as_f64(np.concatenate([anchor, G[:, 3:]], axis=1))
    box = np.zeros(6)
    L.check(lib.npg_locator_box(L.ptr(G), L.ptr(anchor), int(m.ncell), L.ptr(box)))
    eng, gid, own = L.as_i32(np.arange(m.ncell)), L.as_i64(np.arange(m.ncell)), np.ones(m.ncell, dtype=np.uint8)
    h = C.c_void_p()
    L.check(lib.npg_locator_create_cells(model.arch.ctx.h, L.ptr(geo12), L.ptr(eng), L.ptr(gid), L.ptr(own), int(m.ncell), L.ptr(box),
                                         0, C.byref(h)))
    return h


def check_refusals(model):
    lib = L.lib()
    set_affine(model, JZ)
    x0 = safe_seeds(300)
    tr = npg.ParticleTracker(model, x0, t0=0.0)
    ctx, x = model.arch.ctx, model.inversion.solver.x
    short = npg.DeviceVector(ctx, x.n - 1)
    cases = [((tr.h, tr.fe.h, tr.loc.h, x.h, x.h, 0.0, 1.0, 0.1, 0), "nsub"),
             ((tr.h, tr.fe.h, tr.loc.h, x.h, x.h, 0.0, 1.0, float("nan"), 4), "dt"),
             ((tr.h, tr.fe.h, tr.loc.h, x.h, x.h, 0.0, 1.0, float("inf"), 4), "dt"),
             ((tr.h, tr.fe.h, tr.loc.h, x.h, x.h, float("nan"), 1.0, 0.1, 4), "s0"),
             ((tr.h, tr.fe.h, tr.loc.h, short.h, x.h, 0.0, 1.0, 0.1, 4), "entries"),
             ((tr.h, tr.fe.h, tr.loc.h, x.h, short.h, 0.0, 1.0, 0.1, 4), "entries"),
             ((tr.h, tr.fe.h, None, x.h, x.h, 0.0, 1.0, 0.1, 4), "NULL")]
    part = _partitioned_locator(model)
    if part is not None:
        cases.append(((tr.h, tr.fe.h, part, x.h, x.h, 0.0, 1.0, 0.1, 4), "partitioned"))
    for args, word in cases:
        rc = lib.npg_particles_advance(*args)
        msg = lib.npg_last_error().decode()
        assert rc == NPG_EINVAL and "npg_particles_advance" in msg and word in msg, (rc, msg, word)
        with np.testing.assert_raises(L.DeviceError):
            L.check(rc)
    if part is not None:
        lib.npg_locator_destroy(part)
    bad = np.array([1.0, -1.0, 0.0])
    rc = lib.npg_particles_set_period(tr.h, L.ptr(bad))
    assert rc == NPG_EINVAL and "npg_particles_set_period" in lib.npg_last_error().decode()
    assert np.array_equal(tr.positions, x0) and tr.t == 0.0 and not tr.status.any()       # nothing was launched
    print(f"refusals: {len(cases)} bad calls of npg_particles_advance refused" + ("" if part is not None else " (no partitioned locator in this library)"))
    # n = 0 is legal and does nothing
    none = npg.ParticleTracker(model, np.empty((0, 3)), t0=0.0)
    none.advance(0.1)
    assert none.positions.shape == (0, 3) and none.status.shape == (0,) and none.sample("u").shape == (0, 3) and none.t == 0.1
    # a NaN seed and a seed outside the mesh are lost at t0, the one between them lives
    few = npg.ParticleTracker(model, [[np.nan, 0.0, -0.1], [0.1, 0.0, -0.1], [5.0, 0.0, 0.0]], t0=2.5)
    assert np.array_equal(few.status, [1, 0, 1]) and np.array_equal(few.t_lost, [2.5, np.nan, 2.5], equal_nan=True)
    few.advance(0.1)
    p = few.positions
    assert np.isnan(p[0, 0]) and p[2, 0] == 5.0 and p[1, 0] != 0.1 and np.array_equal(few.cells[[0, 2]], [-1, -1])
    # a mesh-partitioned model: refused, and the message says why
    standin = SimpleNamespace(fe_data=model.fe_data, arch=model.arch, layout=SimpleNamespace(locator_cells=None, cell_owner=None))
    with np.testing.assert_raises(NotImplementedError) as e:
        npg.ParticleTracker(standin, x0)
    assert "rank" in str(e.exception)
