"""The checks shared by tests/test_particles_walk.py (CPU()) and tests/test_gpu_particles_walk.py (GPU()) for diffusing particles and
reflecting walls (npg_particles_walk), as tests/particles_ref.py holds those of the advective tracker.

Every reference is independent of the code under test: a numpy Philox4x32-10 (uint64 arithmetic, checked against the published known
answers), closed recurrences for free diffusion, a linear kappa_v and a flat reflecting surface, and a numpy restatement of the walk
(`Walk.move`: all particles at once, one face event per pass) on sampling_ref.Brute's geometry - the inverted edge matrices of the
cells' own vertices, not the library's grad lambda - with the P2 velocity from io._nodal_fields.

Bounds.  A free random-walk step adds s R to x: one rounding of the product and one of the sum, plus at most two roundings of |x| per
crossed face (q = x + t d, then q + (1 - t) d); k steps: k . 8 . eps . max|x| (particles_ref's bound for a uniform flow).  A step on
the real state: 1e-12 . max|x|, the bound of particles_ref.check_real_state.  Statistics: 5 standard errors; the variance of a sum of
k uniform increments has standard error var . sqrt((2 - 1.2 / k) / n) (excess kurtosis -1.2 / k)."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np

import nupgcm_amd as npg
from nupgcm_amd import _lib as L
from nupgcm_amd import io as pio
from nupgcm_amd.particles import cell_neighbours
from tests import helpers
from tests import particles_ref as pr
from tests import sampling_ref as sr

EPS = np.finfo(np.float64).eps
NPG_EINVAL = -1
AMBIG = 1e-9
SYMBOLS = {"npg_particles_set_walls", "npg_particles_set_diffusion", "npg_particles_walk", "npg_particles_download_walk",
           "npg_particles_uniforms"}
KAPPA = helpers.kappa_bottom(0.5)                                        # 1e-2 + exp(-(z + H) / 0.05), H = (1 - r^2) / 2
CENTRE = np.array([0.0, 0.0, -0.25])


# ---- the generator --------------------------------------------------------------------------------------------------------------------
def philox4x32_10(ctr, key):
    """ctr (..., 4), key (..., 2) uint32 words -> (..., 4) uint32"""
    c = [np.asarray(ctr[..., i], dtype=np.uint64) for i in range(4)]
    k = [np.asarray(key[..., i], dtype=np.uint64) for i in range(2)]
    M0, M1, W0, W1, lo = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85), np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & lo, (p0 >> s32) ^ c[3] ^ k[1], p0 & lo]
        k = [(k[0] + W0) & lo, (k[1] + W1) & lo]
    return np.stack(c, axis=-1).astype(np.uint32)


def words(seed, index, step):
    index = np.asarray(index, dtype=np.uint64)
    lo, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    step = np.broadcast_to(np.uint64(step), index.shape)
    ctr = np.stack([index & lo, index >> s32, step & lo, step >> s32], axis=-1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64), index.shape + (2,))
    return philox4x32_10(ctr, key)


def uniforms(seed, index, step):
    """R (n, 3) of the particles `index` at one step number"""
    return (2.0 * words(seed, index, step)[..., :3].astype(np.float64) + 1.0) * 2.0 ** -32 - 1.0


KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


def lib_uniforms(arch, seed, first, n, step):
    out = npg.DeviceVector(arch.ctx, 3 * n)
    L.check(L.lib().npg_particles_uniforms(arch.ctx.h, seed, first, n, step, out.h))
    return out.to_host().reshape(n, 3)


def check_generator(arch):
    for ctr, key, out in KNOWN:
        got = philox4x32_10(np.array(ctr, dtype=np.uint64), np.array(key, dtype=np.uint64))
        assert " ".join(f"{w:08x}" for w in got) == out, (ctr, got)
        # the same known answer through the library: counter = (index, step), key = seed
        seed, index, step = key[0] | key[1] << 32, ctr[0] | ctr[1] << 32, ctr[2] | ctr[3] << 32
        R = lib_uniforms(arch, seed, index, 1, step)[0]
        w = np.array([int(v, 16) for v in out.split()[:3]], dtype=np.float64)
        assert np.array_equal(R, (2.0 * w + 1.0) * 2.0 ** -32 - 1.0)
    seed = 0x9E3779B97F4A7C15
    n = 1000
    for first, step in ((0, 0), (2 ** 32 - 500, 7), (2 ** 40 + 3, 2 ** 32 + 11)):    # indices across and beyond 2^32, a step beyond 2^32
        R = lib_uniforms(arch, seed, first, n, step)
        w = ((R + 1.0) * 2.0 ** 32 - 1.0) / 2.0                          # exact: R is (2 w + 1) 2^-32 - 1
        assert np.array_equal(w, np.floor(w)) and (np.abs(R) < 1.0).all()
        ref = words(seed, np.uint64(first) + np.arange(n, dtype=np.uint64), step)[:, :3]
        assert np.array_equal(w.astype(np.uint64), ref.astype(np.uint64)), (first, step)
    assert lib_uniforms(arch, seed, 5, 0, 1).shape == (0, 3)
    print("generator: 3 known answers and 3 x 1000 x 3 words equal, integer for integer")


# ---- the neighbour table --------------------------------------------------------------------------------------------------------------
def bowl_mesh():
    return npg.Mesh(os.path.join(helpers.GOLDEN, "mesh_bowl3D_h0.1.npz"))


def check_symmetric(nbr, shift):
    c, i = np.nonzero(nbr >= 0)
    back = (nbr[nbr[c, i]] == c[:, None]) & (shift[nbr[c, i]] == -shift[c, i][:, None, :]).all(axis=2)
    assert back.any(axis=1).all()


def check_neighbours():
    mesh = bowl_mesh()
    nbr, shift = cell_neighbours(mesh)
    assert nbr.shape == (mesh.ncell, 4) and nbr.dtype == np.int32 and shift.shape == (mesh.ncell, 4, 3) and shift.dtype == np.int8
    check_symmetric(nbr, shift)
    nfacets = len(np.asarray(mesh.model.facets).reshape(-1, 3))
    print(f"neighbours, bowl: {int((nbr < 0).sum())} boundary faces, the fixture lists {nfacets} facets")
    assert (nbr < 0).sum() == nfacets == 1732 and not shift.any()
    from nupgcm_amd import channel_basin as cb
    from nupgcm_amd import workloads
    ch = npg.Mesh(cb.channel_basin_model(0.125, workloads.CB_ALPHA, dz=0.125))
    nbr, shift = cell_neighbours(ch)
    check_symmetric(nbr, shift)
    # the seam faces: all three vertices are a periodic node or the master of one
    per = np.asarray(ch.model.periodic, dtype=np.int64)
    on_seam = np.zeros(len(per), dtype=bool)
    on_seam[per != np.arange(len(per))] = True
    on_seam[per[per != np.arange(len(per))]] = True
    opp = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])
    seam = on_seam[ch.cell_geo[:, opp]].all(axis=2)
    x = ch.geo_coords[ch.cell_geo[:, opp]][..., 0]
    seam &= (x.max(axis=2) - x.min(axis=2)) < 1e-12                      # the face lies in the plane of the seam
    print(f"neighbours, channel basin: {int(seam.sum())} seam faces, shifts on x {sorted(set(shift[seam][:, 0].tolist()))}")
    assert seam.sum() > 0 and (nbr[seam] >= 0).all() and (np.abs(shift[seam][:, 0]) == 1).all()
    assert not shift[~seam].any() and not shift[..., 1:].any()
    walled, s0 = cell_neighbours(ch, ch.cell_geo, np.zeros(3))           # matched by the cells' own nodes: the seam is a wall
    assert (walled[seam] < 0).all() and not s0.any()


# ---- the numpy restatement of the walk --------------------------------------------------------------------------------------------------
class Walk:
    """move() and step() of the issue, restated for all particles at once"""

    def __init__(self, mesh, period=(0.0, 0.0, 0.0)):
        self.mesh, self.br = mesh, sr.Brute(mesh)
        self.period = np.asarray(period, dtype=float)
        self.nbr, self.shift = cell_neighbours(mesh, mesh.cells if self.period.any() else mesh.cell_geo, self.period)
        T = self.br.T
        self.G = np.concatenate([-T.sum(axis=1, keepdims=True), T], axis=1)      # (nc, 4, 3) grad lambda_0..3

    def move(self, c, x, d):
        """-> dict(c, x, lam, wind, nrefl, stuck, amb): the end of the move of each particle; amb = the restatement's own decision
        margin was small (some |lambda_i(x + d)| < 1e-9, or two candidate t closer than 1e-9)"""
        n = len(c)
        c, x, r = c.astype(np.int64).copy(), x.copy(), d.copy()
        lam = self.br.lambdas(x, c)
        wind, nrefl = np.zeros((n, 3), dtype=np.int64), np.zeros(n, dtype=np.int64)
        stuck, amb, live = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool), np.ones(n, dtype=bool)
        for ev in range(65):
            idx = np.nonzero(live)[0]
            if not len(idx):
                break
            dl = np.einsum("nia,na->ni", self.G[c[idx]], r[idx])
            e = lam[idx] + dl
            amb[idx] |= (np.abs(e) < AMBIG).any(axis=1)
            bad = ~np.isfinite(e).all(axis=1)
            out = (e < 0).any(axis=1) | bad
            fin = idx[~out]
            x[fin], lam[fin], live[fin] = x[fin] + r[fin], e[~out], False
            if ev == 64 or bad.any():
                stuck[idx[out if ev == 64 else bad]] = True
                live[idx[out if ev == 64 else bad]] = False
                out &= ~bad
            idx, e, dl = idx[out], e[out], dl[out]
            if ev == 64 or not len(idx):
                continue
            l = lam[idx]
            with np.errstate(divide="ignore", invalid="ignore"):
                t = np.where(e < 0, np.clip(l / (l - e), 0.0, 1.0), np.inf)
            f = t.argmin(axis=1)                                         # the first minimum: ties to the lowest i
            ts = np.sort(t, axis=1)
            with np.errstate(invalid="ignore"):
                amb[idx] |= (ts[:, 1] - ts[:, 0]) < AMBIG
            tb = t[np.arange(len(idx)), f]
            q = x[idx] + tb[:, None] * r[idx]
            rem = (1.0 - tb)[:, None] * r[idx]
            nb = self.nbr[c[idx], f]
            wall = nb < 0
            # a boundary face: the remainder reflected, lambda along the segment, 0 on the face
            g = self.G[c[idx], f]
            refl = rem - 2.0 * ((rem * g).sum(axis=1) / (g * g).sum(axis=1))[:, None] * g
            lq = l + tb[:, None] * dl
            lq[np.arange(len(idx)), f] = 0.0
            # a neighbour: the point translated, lambda in the neighbour, 0 on the face that leads back
            s = self.shift[c[idx], f].astype(np.int64)
            qn = q + s * self.period
            cn = np.where(wall, c[idx], nb)
            ln = self.br.lambdas(qn, cn)
            back = (self.nbr[cn] == c[idx][:, None]) & (self.shift[cn] == -s[:, None, :]).all(axis=2)
            assert back[~wall].any(axis=1).all()
            ln[np.arange(len(idx)), back.argmax(axis=1)] = 0.0
            x[idx] = np.where(wall[:, None], q, qn)
            r[idx] = np.where(wall[:, None], refl, rem)
            lam[idx] = np.where(wall[:, None], lq, ln)
            c[idx] = cn
            wind[idx] -= np.where(wall[:, None], 0, s)
            nrefl[idx] += wall
        return dict(c=c, x=x, lam=lam, wind=wind, nrefl=nrefl, stuck=stuck, amb=amb)

    def velocity(self, un, c, lam):
        return np.einsum("ni,nia->na", self.br.p2(lam), un[self.mesh.cell_nodes[c]])

    def displacement(self, kh, kv, cd, h, c, lam, R):
        gh, gv = np.einsum("ni,nia->na", kh[c], self.G[c]), np.einsum("ni,nia->na", kv[c], self.G[c])
        delta = cd * h * np.column_stack([gh[:, 0], gh[:, 1], gv[:, 2]])
        sh = np.maximum((lam * kh[c]).sum(axis=1) + 0.5 * (delta * gh).sum(axis=1), 0.0)
        sv = np.maximum((lam * kv[c]).sum(axis=1) + 0.5 * (delta * gv).sum(axis=1), 0.0)
        return delta + R * np.sqrt(6.0 * cd * h * np.column_stack([sh, sh, sv]))

    def step(self, un, c, x, h, diffusion=None, R=None):
        """one step from the state (c, x) through the frozen nodal velocity un (nn, 3): RK4 with every point walked, then the random
        displacement; diffusion = (kappa_h (nc, 4), kappa_v (nc, 4), c_d).  -> the dict of move() for the whole step"""
        lam0 = self.br.lambdas(x, c)
        amb, stuck = np.zeros(len(c), dtype=bool), np.zeros(len(c), dtype=bool)

        def walked(d):
            nonlocal amb, stuck
            m = self.move(c, x, d)
            amb, stuck = amb | m["amb"], stuck | m["stuck"]
            return m
        k1 = self.velocity(un, c, lam0)
        m = walked((0.5 * h) * k1)
        k2 = self.velocity(un, m["c"], m["lam"])
        m = walked((0.5 * h) * k2)
        k3 = self.velocity(un, m["c"], m["lam"])
        m = walked(h * k3)
        k4 = self.velocity(un, m["c"], m["lam"])
        end = walked((h / 6.0) * (((k1 + 2.0 * k2) + 2.0 * k3) + k4))
        if diffusion is not None:
            kh, kv, cd = diffusion
            m = self.move(end["c"], end["x"], self.displacement(kh, kv, cd, h, end["c"], end["lam"], R))
            amb, stuck = amb | m["amb"], stuck | m["stuck"]
            m["wind"] += end["wind"]
            m["nrefl"] += end["nrefl"]
            end = m
        end["amb"], end["stuck"] = amb, stuck
        return end


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------
def still(model):
    pr.set_affine(model, np.zeros((3, 3)))


def volume_seeds(model, n, seed=pr.SEED):
    """n points uniform in the mesh volume: box points that the locator finds"""
    p = sr.box_points(model, 4 * n, seed)
    p = p[npg.PointLocator(model).locate(p).valid]
    assert len(p) >= n
    return p[:n]


def vertex_table(mesh, fn):
    return np.ascontiguousarray(fn(mesh.geo_coords[mesh.cell_geo]), dtype=np.float64)


def snapshot(tr):
    return dict(pr.snapshot(tr), reflections=tr.reflections)


# ---- free diffusion and a linear kappa_v, exact per particle ---------------------------------------------------------------------------
CD, H_FREE, K_FREE, N_FREE = 0.01, 0.04, 30, 2000


def check_free_diffusion(model, kh=1e-2, kv=4e-3, seed=12345):
    still(model)
    assert K_FREE * np.sqrt(6 * CD * max(kh, kv) * H_FREE) < 0.15        # no walk can reach a wall from the centre
    x0 = np.tile(CENTRE, (N_FREE, 1))
    tr = npg.ParticleTracker(model, x0, t0=0.0, nsub=1, diffusion=(kh, kv, CD), seed=seed)
    assert tr.walls and tr.step == 0
    s = np.sqrt(6.0 * CD * H_FREE * np.array([kh, kh, kv]))
    ref, worst = x0.copy(), 0.0
    for k in range(K_FREE):
        tr.advance(H_FREE)
        ref = ref + uniforms(seed, np.arange(N_FREE), k) * s
        err, tol = np.abs(tr.positions - ref).max(), (k + 1) * 8 * EPS * np.abs(ref).max()
        worst = max(worst, err / tol)
        assert err <= tol, (k, err, tol)
    assert tr.step == K_FREE and not tr.status.any() and not tr.reflections.any()
    assert np.array_equal(tr.cells, npg.PointLocator(model).locate(tr.positions).cells)
    d = tr.positions - x0
    var = 2.0 * CD * np.array([kh, kh, kv]) * K_FREE * H_FREE
    se_mean, se_var = np.sqrt(var / N_FREE), var * np.sqrt((2.0 - 1.2 / K_FREE) / N_FREE)
    zm, zv = d.mean(axis=0) / se_mean, (d.var(axis=0) - var) / se_var
    print(f"free diffusion: {K_FREE} steps, {N_FREE} particles: |x - (x0 + sum R s)| at most {worst:.3f} of k 8 eps max|x|; mean "
          f"{zm.round(2)} and variance {zv.round(2)} standard errors off; {len(set(tr.cells.tolist()))} cells reached")
    assert (np.abs(zm) <= 5).all() and (np.abs(zv) <= 5).all()
    assert len(set(tr.cells.tolist())) > 3                               # the walks do cross faces
    return worst


def check_linear_kappa(model, a=0.012, b=0.02, kh=1e-2, seed=777):
    still(model)
    mesh = model.fe_data.mesh
    assert (a + b * mesh.geo_coords[:, 2]).min() > 0
    x0 = np.tile(CENTRE, (N_FREE, 1))
    tr = npg.ParticleTracker(model, x0, t0=0.0, nsub=1, diffusion=(kh, lambda x: a + b * x[..., 2], CD), seed=seed)
    ref, worst = x0.copy(), 0.0
    sh = np.sqrt(6.0 * CD * kh * H_FREE)
    for k in range(K_FREE):
        tr.advance(H_FREE)
        R = uniforms(seed, np.arange(N_FREE), k)
        dz = CD * H_FREE * b
        ks = np.maximum((a + b * ref[:, 2]) + 0.5 * dz * b, 0.0)
        ref = ref + np.column_stack([R[:, 0] * sh, R[:, 1] * sh, dz + R[:, 2] * np.sqrt(6.0 * CD * ks * H_FREE)])
        # kappa_v (z) is interpolated from the vertices: its value carries some ten roundings of kappa, far inside the bound
        err, tol = np.abs(tr.positions - ref).max(), (k + 1) * 8 * EPS * np.abs(ref).max()
        worst = max(worst, err / tol)
        assert err <= tol, (k, err, tol)
    assert not tr.status.any() and not tr.reflections.any()
    dz_mean = (tr.positions[:, 2] - x0[:, 2]).mean()
    drift = CD * b * K_FREE * H_FREE
    se = np.sqrt(2.0 * CD * (a + b * CENTRE[2]) * K_FREE * H_FREE / N_FREE)
    print(f"linear kappa_v = {a} + {b} z: |x - recurrence| at most {worst:.3f} of k 8 eps max|x|; mean dz = {dz_mean:.3e} against "
          f"c_d b k h = {drift:.3e}: {(dz_mean - drift) / se:.2f} standard errors")
    assert abs(dz_mean - drift) <= 5 * se
    return worst


# ---- the flat surface -------------------------------------------------------------------------------------------------------------------
def check_flat_surface(model, w0=1.0, h=0.03, k=30):
    rng = np.random.default_rng(pr.SEED)
    n = 1000
    r, phi = 0.5 * np.sqrt(rng.random(n)), 2 * np.pi * rng.random(n)
    x0 = np.column_stack([r * np.cos(phi), r * np.sin(phi), -0.1 + 0.09 * rng.random(n)])
    pr.set_affine(model, np.zeros((3, 3)), (0.0, 0.0, w0))
    tr = npg.ParticleTracker(model, x0, t0=0.0, nsub=1, walls=True)
    z, flips, worst = x0[:, 2].copy(), np.zeros(n, dtype=np.int64), 0.0
    for j in range(k):
        tr.advance(h)
        up = z + h * w0
        flips += up > 0
        z = -np.abs(up)
        got = tr.positions
        err = max(np.abs(got[:, 2] - z).max(), np.abs(got[:, :2] - x0[:, :2]).max())
        worst = max(worst, err / ((j + 1) * 8 * EPS))
        assert err <= (j + 1) * 8 * EPS, (j, err)
    print(f"flat surface, w0 = {w0}: {k} steps, |z - recurrence| and |xy - xy0| at most {worst:.3f} of k 8 eps; reflections "
          f"{int(flips.min())} .. {int(flips.max())} per particle")
    assert np.array_equal(tr.reflections, flips) and flips.min() >= 5
    assert not tr.status.any() and np.isnan(tr.t_lost).all() and (tr.positions[:, 2] <= 0).all()
    # with diffusion, no flow, from just under the centre of the surface
    still(model)
    n, kap, seed = 1000, 1e-2, 99
    x0 = np.tile([0.0, 0.0, -0.01], (n, 1))
    td = npg.ParticleTracker(model, x0, t0=0.0, nsub=1, diffusion=(kap, kap, CD), seed=seed)
    s = np.sqrt(6.0 * CD * kap * H_FREE)
    ref, hits, worst = x0.copy(), np.zeros(n, dtype=np.int64), 0.0
    for j in range(K_FREE):
        td.advance(H_FREE)
        ref = ref + uniforms(seed, np.arange(n), j) * s
        hits += ref[:, 2] > 0
        ref[:, 2] = -np.abs(ref[:, 2])
        err, tol = np.abs(td.positions - ref).max(), (j + 1) * 8 * EPS * np.abs(ref).max()
        worst = max(worst, err / tol)
        assert err <= tol, (j, err, tol)
    print(f"flat surface, diffusion: |x - recurrence| at most {worst:.3f} of k 8 eps max|x|; {int(hits.sum())} reflections")
    assert (td.positions[:, 2] <= 0).all() and np.array_equal(td.reflections, hits) and hits.sum() > n and not td.status.any()


# ---- one step against the restatement, on the real state --------------------------------------------------------------------------------
def one_step_setup(model, n=2000):
    """(seeds, h, c_d, kappa table): h max|u| = half a cell, c_d h = 1e-4 as in the census"""
    h = pr.half_cell_step(model)
    return volume_seeds(model, n), h, 1e-4 / h, vertex_table(model.fe_data.mesh, KAPPA)


def check_one_step(model, nsteps=20, seed=4242):
    mesh = model.fe_data.mesh
    x0, h, cd, kap = one_step_setup(model)
    n = len(x0)
    tr = npg.ParticleTracker(model, x0, nsub=1, diffusion=(kap, kap, cd), seed=seed)
    assert not tr.status.any()
    wk = Walk(mesh)
    un = pio._nodal_fields(model)[0]
    scale = np.abs(x0).max()
    amb_all, worst, nref = np.zeros(n, dtype=bool), 0.0, 0
    for k in range(nsteps):
        before = snapshot(tr)
        tr.advance(h)
        after = snapshot(tr)
        ref = wk.step(un, before["cells"], before["x"], h, (kap, kap, cd), uniforms(seed, np.arange(n), k))
        live = before["status"] == 0
        ok = live & ~ref["amb"]
        amb_all |= live & ref["amb"]
        assert np.array_equal(after["status"][ok], np.where(ref["stuck"][ok], 2, 0))
        ok &= ~ref["stuck"]
        err = np.abs(after["x"][ok] - ref["x"][ok]).max()
        worst = max(worst, err)
        assert err <= 1e-12 * scale, (k, err)
        assert np.array_equal(after["cells"][ok], ref["c"][ok])
        assert np.array_equal(after["wind"][ok], before["wind"][ok] + ref["wind"][ok])
        assert np.array_equal(after["reflections"][ok], before["reflections"][ok] + ref["nrefl"][ok])
        assert np.array_equal(after["cells"], npg.PointLocator(model).locate(after["x"]).cells)
        nref += int(ref["nrefl"][ok].sum())
    print(f"one step on the real state, {nsteps} times: h = {h:.4e}, c_d = {cd:.3e}; max|x - restatement| = {worst:.3e} (bound "
          f"{1e-12 * scale:.1e}); {int(amb_all.sum())} of {n} particles set aside as ambiguous at some step; {nref} reflections; "
          f"{int((tr.status != 0).sum())} lost or stuck")
    assert amb_all.mean() <= 0.01 and nref > 100
    return worst


# ---- the well-mixed census ------------------------------------------------------------------------------------------------------------
def census(x):
    H = helpers.H(x, 0.5)
    sigma = np.clip(-x[:, 2] / H, 0.0, 1.0)
    return np.bincount(np.minimum((5 * sigma).astype(int), 4), minlength=5)


def check_census(model, n=3000, h=0.01, nsteps=120, seed=2026):
    still(model)
    x0 = volume_seeds(model, n)
    kap = vertex_table(model.fe_data.mesh, KAPPA)
    tr = npg.ParticleTracker(model, x0, t0=0.0, nsub=nsteps // 4, diffusion=(kap, kap, 0.01), seed=seed)
    for _ in range(4):
        tr.advance(h * (nsteps // 4))
    before, after = census(x0), census(tr.positions)
    print(f"census of sigma = -z / H in 5 classes: before {before.tolist()}, after {nsteps} steps {after.tolist()}; "
          f"{int(tr.reflections.sum())} reflections, {int((tr.status != 0).sum())} lost or stuck")
    assert tr.step == nsteps and not tr.status.any()
    assert (np.abs(after - before) <= 4 * np.sqrt(before + after)).all()
    assert np.array_equal(tr.cells, npg.PointLocator(model).locate(tr.positions).cells)
    return before, after


# ---- the periodic seam ------------------------------------------------------------------------------------------------------------------
def check_periodic(arch, h=0.07, nsteps=40):
    """particles_ref.check_periodic through npg_particles_walk: the same seeds, the same closed forms"""
    model = pr.channel_bare(arch)
    pr.set_affine(model, np.zeros((3, 3)), (1.0, 0.0, 0.0))
    lo, hi = npg.PointLocator(model).bounding_box
    W = hi[0] - lo[0]
    rng = np.random.default_rng(sr.SEED)
    n = 1200
    side = np.where(rng.random(n) < 0.5, lo[0] + 0.125 * rng.random(n), hi[0] - 0.125 * rng.random(n))
    pts = np.column_stack([side, -1.0 + 0.5 * rng.random(n), -0.1 * rng.random(n)])
    x0 = pts[pts[:, 1] <= -0.75]
    assert len(x0) > 400
    tr = npg.ParticleTracker(model, x0, t0=0.0, nsub=1, walls=True)
    assert np.array_equal(tr.period, [W, 0.0, 0.0]) and tr.shift[..., 0].any()
    for _ in range(nsteps):
        tr.advance(h)
    k = nsteps
    wind = np.floor((x0[:, 0] + k * h - lo[0]) / W).astype(np.int64)
    ref = x0.copy()
    ref[:, 0] = x0[:, 0] + k * h - wind * W
    got, unw = tr.positions, tr.unwrapped
    e1, e2, tol = np.abs(got - ref).max(), np.abs(unw[:, 0] - (x0[:, 0] + k * h)).max(), k * 8 * EPS * W
    print(f"periodic seam, walked: {len(x0)} particles, {k} steps of h = {h}, wind {wind.min()} .. {wind.max()}; |x - wrapped closed form| "
          f"= {e1:.3e}, |unwrapped - (x0 + k h)| = {e2:.3e} (bound {tol:.3e}); lost or stuck {int((tr.status != 0).sum())}")
    assert not tr.status.any() and not tr.reflections.any()
    assert np.array_equal(tr.wind[:, 0], wind) and not tr.wind[:, 1:].any() and wind.min() >= 2
    assert e1 <= tol and e2 <= tol + EPS * np.abs(unw).max()
    assert (got[:, 0] >= lo[0]).all() and (got[:, 0] <= lo[0] + W).all()
    # the table's seam shifts zeroed: a walked point would cross the seam without its translation - refused
    lib = L.lib()
    zero = np.zeros_like(tr.shift)
    L.check(lib.npg_particles_set_walls(tr.h, L.ptr(tr.nbr), L.ptr(zero), len(tr.nbr)))
    x = model.inversion.solver.x
    rc = lib.npg_particles_walk(tr.h, tr.fe.h, tr.loc.h, x.h, x.h, 0.0, 1.0, h, 1)
    msg = lib.npg_last_error().decode()
    assert rc == NPG_EINVAL and "npg_particles_walk" in msg and "seam" in msg, (rc, msg)
    assert np.array_equal(tr.positions, got)
    # the period forced to 0: the seam is a wall, the particles bounce between its two sides and none is lost
    t0 = npg.ParticleTracker(model, x0, t0=0.0, nsub=1, walls=True, periodic=(0, 0, 0))
    for _ in range(nsteps):
        t0.advance(h)
    xs = t0.positions[:, 0]
    assert not t0.status.any() and not t0.wind.any() and t0.reflections.min() >= 2 and (xs >= lo[0]).all() and (xs <= hi[0]).all()


# ---- stuck ------------------------------------------------------------------------------------------------------------------------------
def check_stuck(model, h=0.01, nsteps=40):
    """a neighbour table whose interior faces lead to far-away cells that do not lead back: the first step in which a move leaves the
    particle's cell cannot be finished.  u = (0.5, 0, 0): the furthest point of a step is x + h u0 (stages 4 and the end), and a cell is
    convex, so the step is stuck iff lambda_min of x + h u0 in the particle's cell is negative (sampling_ref.Brute); until then the
    particle moves inside its cell.  Stuck: status 2, the state and the time of the start of that step, nothing moves it later."""
    lib = L.lib()
    mesh = model.fe_data.mesh
    nc = int(mesh.ncell)
    u0 = np.array([0.5, 0.0, 0.0])
    x0 = pr.safe_seeds(500)
    pr.set_affine(model, np.zeros((3, 3)), u0)
    tr = npg.ParticleTracker(model, x0, t0=0.0, nsub=1, walls=True)
    cells = np.arange(nc)[:, None]
    far = next(f for f in ((cells + k) % nc for k in range(nc // 2, nc)) if (tr.nbr[f] != cells[:, :, None]).all())   # none leads back
    bad = L.as_i32(np.where(tr.nbr >= 0, far, -1))
    L.check(lib.npg_particles_set_walls(tr.h, L.ptr(bad), L.ptr(tr.shift), nc))
    br = sr.Brute(mesh)
    c, x, alive, amb = tr.cells.astype(np.int64), x0.copy(), np.ones(len(x0), dtype=bool), np.zeros(len(x0), dtype=bool)
    t, t_stuck = 0.0, np.full(len(x0), np.nan)
    for k in range(nsteps):
        tr.advance(h)
        mn = br.lambdas(x + h * u0, c).min(axis=1)
        amb |= alive & (np.abs(mn) < AMBIG)
        now = alive & (mn < 0)
        t_stuck[now] = t
        alive &= ~now
        x[alive] = x[alive] + h * u0
        t = t + h
        ok = ~amb
        assert np.array_equal(tr.status[ok], np.where(alive[ok], 0, 2)), k
        assert np.abs(tr.positions[ok] - x[ok]).max() <= (k + 1) * 8 * EPS
    print(f"stuck: {int((~alive).sum())} of {len(x0)} particles stuck within {nsteps} steps, {int(amb.sum())} ambiguous")
    assert amb.mean() <= 0.01 and (~alive).mean() > 0.9
    ok = ~amb
    assert np.array_equal(tr.t_lost[ok], t_stuck[ok], equal_nan=True) and np.array_equal(tr.cells[ok], c[ok])
    assert not tr.reflections.any() and not tr.wind.any()
    frozen = tr.positions
    tr.advance(h)
    assert np.array_equal(tr.positions[~alive], frozen[~alive])


# ---- determinism ------------------------------------------------------------------------------------------------------------------------
def check_determinism(model, dt=0.25, nsub=8, seed=31):
    """rotation plus a drift that carries particles into the wall, with diffusion.  dt / nsub = 2^-5: the clocks of one call and of eight
    agree to the bit.  The generator is counted by the particle's index: with diffusion a particle's path depends on its own index and
    on nothing else - checked by leaving out the other particles; permuted seeds must give permuted bits where no random number is
    drawn (walls only)."""
    x0 = pr.safe_seeds(1500)
    pr.set_affine(model, pr.JZ, (0.3, 0.0, 0.0))
    dif = (2e-2, 1e-2, CD)
    make = lambda x, nsub=nsub, s=seed, d=dif: npg.ParticleTracker(model, x, t0=0.0, nsub=nsub, diffusion=d, seed=s, walls=True)
    one, eight, twin, other, part = make(x0), make(x0, 1), make(x0), make(x0, s=seed + 1), make(x0[:700])
    for _ in range(6):
        for t in (one, twin, other, part):
            t.advance(dt)
        for _ in range(nsub):
            eight.advance(dt / nsub)
    a = snapshot(one)
    print(f"determinism: {len(x0)} particles, {6 * nsub} steps, {int(a['reflections'].sum())} reflections, {int((a['status'] != 0).sum())} lost or stuck")
    assert a["reflections"].sum() > 100 and (a["status"] == 0).all()
    assert pr.same_bits(a, snapshot(eight)) and one.t == eight.t and one.step == eight.step == 6 * nsub
    assert pr.same_bits(a, snapshot(twin))
    assert pr.same_bits({k: v[:700] for k, v in a.items()}, snapshot(part))
    assert (np.abs(other.positions - a["x"]).max(axis=1) > 0).all()      # another seed: other positions
    perm = np.random.default_rng(3).permutation(len(x0))
    w, wp = make(x0, d=None), make(x0[perm], d=None)
    for _ in range(6):
        w.advance(dt)
        wp.advance(dt)
    b = snapshot(w)
    assert b["reflections"].sum() > 100 and pr.same_bits({k: v[perm] for k, v in b.items()}, snapshot(wp))


# ---- refusals, the opt-in, the hook -----------------------------------------------------------------------------------------------------
def check_exports():
    assert SYMBOLS <= set(L.declared_symbols())
    for path in (L.HOST_LIB_PATH, L.LIB_PATH):
        lib = C.CDLL(path)
        assert not [s for s in SYMBOLS if not hasattr(lib, s)], path


def _refused(rc, entry, word):
    msg = L.lib().npg_last_error().decode()
    assert rc == NPG_EINVAL and entry in msg and word in msg, (rc, msg, entry, word)


def check_refusals(model):
    lib = L.lib()
    pr.set_affine(model, pr.JZ)
    mesh = model.fe_data.mesh
    nc = int(mesh.ncell)
    x0 = pr.safe_seeds(300)
    tr = npg.ParticleTracker(model, x0, t0=0.0)                          # no walls
    x = model.inversion.solver.x
    walk = lambda *a: lib.npg_particles_walk(*a)
    good = (tr.h, tr.fe.h, tr.loc.h, x.h, x.h, 0.0, 1.0, 0.1, 4)
    _refused(walk(*good), "npg_particles_walk", "walls")
    nbr, shift = cell_neighbours(mesh)
    kap = np.full((nc, 4), 1e-2)
    # npg_particles_set_walls
    sw = lambda n_, s_, k_: lib.npg_particles_set_walls(tr.h, None if n_ is None else L.ptr(n_), None if s_ is None else L.ptr(s_), k_)
    _refused(sw(None, shift, nc), "npg_particles_set_walls", "NULL")
    _refused(sw(nbr, None, nc), "npg_particles_set_walls", "NULL")
    _refused(lib.npg_particles_set_walls(None, L.ptr(nbr), L.ptr(shift), nc), "npg_particles_set_walls", "NULL")
    for v in (-2, nc):
        bad = nbr.copy()
        bad[7, 2] = v
        _refused(sw(bad, shift, nc), "npg_particles_set_walls", "nbr")
    for v in (2, -2):
        bad = shift.copy()
        bad[5, 1, 0] = v
        _refused(sw(nbr, bad, nc), "npg_particles_set_walls", "shift")
    bad = shift.copy()
    bad[np.nonzero(nbr >= 0)[0][0], np.nonzero(nbr >= 0)[1][0], 0] = 1  # a translation on an axis whose period is 0
    _refused(sw(nbr, bad, nc), "npg_particles_set_walls", "period")
    # tables of another mesh: refused by the walk, which knows the locator
    L.check(sw(np.ascontiguousarray(np.minimum(nbr[:-1], nc - 2)), np.ascontiguousarray(shift[:-1]), nc - 1))
    _refused(walk(*good), "npg_particles_walk", "ncell")
    L.check(sw(nbr, shift, nc))
    # npg_particles_set_diffusion
    sd = lambda h_, v_, k_, cd: lib.npg_particles_set_diffusion(tr.h, None if h_ is None else L.ptr(h_), None if v_ is None else L.ptr(v_), k_, cd, 1)
    _refused(sd(kap, None, nc, 0.01), "npg_particles_set_diffusion", "NULL")
    _refused(sd(None, kap, nc, 0.01), "npg_particles_set_diffusion", "NULL")
    _refused(lib.npg_particles_set_diffusion(None, L.ptr(kap), L.ptr(kap), nc, 0.01, 1), "npg_particles_set_diffusion", "NULL")
    _refused(sd(kap[:-1].copy(), kap[:-1].copy(), nc - 1, 0.01), "npg_particles_set_diffusion", "ncell")
    for v in (-1e-3, np.nan, np.inf):
        bad = kap.copy()
        bad[11, 3] = v
        _refused(sd(bad, kap, nc, 0.01), "npg_particles_set_diffusion", "kappa")
        _refused(sd(kap, bad, nc, 0.01), "npg_particles_set_diffusion", "kappa")
    for v in (-0.01, np.nan, np.inf):
        _refused(sd(kap, kap, nc, v), "npg_particles_set_diffusion", "c_d")
    L.check(sd(kap, kap, nc, 0.01))
    L.check(sd(None, None, 0, 0.0))                                      # off again
    L.check(sd(kap, kap, nc, 0.01))
    # npg_particles_walk: the refusals of npg_particles_advance
    short = npg.DeviceVector(model.arch.ctx, x.n - 1)
    cases = [((tr.h, tr.fe.h, tr.loc.h, x.h, x.h, 0.0, 1.0, 0.1, 0), "nsub"),
             ((tr.h, tr.fe.h, tr.loc.h, x.h, x.h, 0.0, 1.0, float("nan"), 4), "dt"),
             ((tr.h, tr.fe.h, tr.loc.h, x.h, x.h, 0.0, 1.0, float("inf"), 4), "dt"),
             ((tr.h, tr.fe.h, tr.loc.h, x.h, x.h, float("nan"), 1.0, 0.1, 4), "s0"),
             ((tr.h, tr.fe.h, tr.loc.h, short.h, x.h, 0.0, 1.0, 0.1, 4), "entries"),
             ((tr.h, tr.fe.h, tr.loc.h, x.h, short.h, 0.0, 1.0, 0.1, 4), "entries"),
             ((tr.h, tr.fe.h, None, x.h, x.h, 0.0, 1.0, 0.1, 4), "NULL"),
             ((tr.h, None, tr.loc.h, x.h, x.h, 0.0, 1.0, 0.1, 4), "NULL"),
             ((None, tr.fe.h, tr.loc.h, x.h, x.h, 0.0, 1.0, 0.1, 4), "NULL")]
    part = pr._partitioned_locator(model)
    if part is not None:
        cases.append(((tr.h, tr.fe.h, part, x.h, x.h, 0.0, 1.0, 0.1, 4), "partitioned"))
    for args, word in cases:
        _refused(walk(*args), "npg_particles_walk", word)
    if part is not None:
        lib.npg_locator_destroy(part)
    _refused(lib.npg_particles_download_walk(None, None, None), "npg_particles_download_walk", "NULL")
    _refused(lib.npg_particles_uniforms(model.arch.ctx.h, 1, 0, 4, 0, short.h), "npg_particles_uniforms", "3 n")
    _refused(lib.npg_particles_uniforms(model.arch.ctx.h, 1, 0, 4, 0, None), "npg_particles_uniforms", "NULL")
    assert np.array_equal(tr.positions, x0) and tr.t == 0.0 and not tr.status.any() and tr.step == 0      # nothing was launched
    print(f"refusals: {len(cases)} bad calls of npg_particles_walk refused" + ("" if part is not None else " (no partitioned locator in this library)"))
    L.check(walk(*good))                                                 # and the good call runs
    assert tr.step == 4 and not np.array_equal(tr.positions, x0)
    # n = 0 is legal
    none = npg.ParticleTracker(model, np.empty((0, 3)), t0=0.0, diffusion=(1e-2, 1e-2, CD))
    none.advance(0.1)
    assert none.positions.shape == (0, 3) and none.reflections.shape == (0,) and none.t == 0.1 and none.step == none.nsub
    # a NaN seed and a seed outside the mesh are lost at t0 (status 1), the one between them lives
    few = npg.ParticleTracker(model, [[np.nan, 0.0, -0.1], [0.1, 0.0, -0.1], [5.0, 0.0, 0.0]], t0=2.5, walls=True)
    assert np.array_equal(few.status, [1, 0, 1]) and np.array_equal(few.t_lost, [2.5, np.nan, 2.5], equal_nan=True)
    few.advance(0.1)
    assert np.array_equal(few.status, [1, 0, 1]) and few.positions[1, 0] != 0.1
    # Python: a random walk without walls, a partitioned model
    with np.testing.assert_raises(ValueError):
        npg.ParticleTracker(model, x0, t0=0.0).set_diffusion((1e-2, 1e-2, CD))
    standin = SimpleNamespace(fe_data=model.fe_data, arch=model.arch, layout=SimpleNamespace(locator_cells=None, cell_owner=None))
    with np.testing.assert_raises(NotImplementedError):
        npg.ParticleTracker(standin, x0, diffusion=True)


def check_opt_in(model, dt=0.25, nsub=8):
    """ParticleTracker without the new keywords is the path of the parent commit: the bits of a second handle driven through
    npg_particles_advance directly; and it never walks"""
    lib = L.lib()
    x0 = np.vstack([pr.safe_seeds(1500), sr.box_points(model, 500)])
    pr.set_affine(model, pr.JZ, (0.3, 0.0, 0.0))
    tr = npg.ParticleTracker(model, x0, t0=0.0, nsub=nsub)
    assert not tr.walls
    h = C.c_void_p()
    L.check(lib.npg_particles_create(model.arch.ctx.h, len(x0), C.byref(h)))
    L.check(lib.npg_particles_set(h, L.ptr(L.as_f64(x0)), 0.0))
    x = model.inversion.solver.x
    L.check(lib.npg_particles_advance(h, tr.fe.h, tr.loc.h, x.h, x.h, 0.0, 1.0, 0.0, 1))
    for _ in range(6):
        tr.advance(dt)
        L.check(lib.npg_particles_advance(h, tr.fe.h, tr.loc.h, x.h, x.h, 0.0, 1.0, dt, nsub))
    n = len(x0)
    raw = dict(x=np.empty((n, 3)), cells=np.empty(n, dtype=np.int32), status=np.empty(n, dtype=np.int32),
               wind=np.empty((n, 3), dtype=np.int32), t_lost=np.empty(n))
    L.check(lib.npg_particles_download(h, *(L.ptr(raw[k]) for k in ("x", "cells", "status", "wind", "t_lost"))))
    refl = np.ones(n, dtype=np.int32)
    L.check(lib.npg_particles_download_walk(h, L.ptr(refl), None))
    lib.npg_particles_destroy(h)
    a = pr.snapshot(tr)
    assert pr.same_bits(a, raw) and (a["status"] == 1).sum() > 10 and not (a["status"] == 2).any()
    assert tr.step == 0 and not tr.reflections.any() and not refl.any()


def check_hook(arch, tmp_path, nsteps=4):
    m = sr.bowl_model(arch, "bowl_surface_flux")
    m.timestepper.t_stop = nsteps * m.timestepper.dt
    x0 = pr.safe_seeds(500)
    tr = npg.ParticleTracker(m, x0, diffusion=True, seed=5)
    prm = m.params
    assert tr.walls and tr.c_d == prm.alpha ** 2 * prm.eps ** 2 / prm.mu_rho
    m.on_plot = tr
    npg.run(m, n_plot=1)
    t, x, status = tr.as_arrays()
    moved = np.abs(x[-1] - x0).max(axis=1)
    # kappa = 1e-2, c_d = 0.025, t = 0.4: the random walk's standard deviation is sqrt(2 c_d kappa t) = 0.014 per axis
    print(f"hook with diffusion=True: {len(tr.history)} calls, t = {tr.t!r}, step {tr.step}, median displacement {np.median(moved):.4f}, "
          f"{int(tr.reflections.sum())} reflections, lost or stuck {int((status[-1] != 0).sum())}")
    assert len(tr.history) == nsteps and x.shape == (nsteps, len(x0), 3) and tr.t == m.timestepper.t == t[-1]
    assert tr.step == nsteps * tr.nsub and not status.any()
    assert 0.005 < np.median(moved) < 0.05
    path = os.path.join(str(tmp_path), "walk.npz")
    tr.save(path)
    z = np.load(path)
    assert np.array_equal(z["x"], x) and np.array_equal(z["status"], status)
    tr.set_diffusion(None)                                               # reflecting advection from here on
    before = tr.positions
    tr.advance(m.timestepper.dt)
    assert np.abs(tr.positions - before).max() < 1e-3 and tr.step == (nsteps + 1) * tr.nsub
