"""Lagrangian particles advected through the device-resident flow (npg_particles_advance): where a water parcel goes -
residence times in the bowl, parcels circling the re-entrant channel, the pathways of the overturning.  The reference has no
counterpart; offline it would need the velocity saved every timestep.

One fused kernel carries every particle through `nsub` classical RK4 steps per call: locate -> evaluate u -> next stage, with the
cell of the last location remembered, so that a particle which stays in its cell never looks at the locator's bins.  Between two
calls the velocity is blended linearly in model time between two vectors [u; p]; model time is the particles' clock (the
nondimensional buoyancy equation carries the same factor in front of d_t b and u . grad b).  A particle that would leave the mesh is
LOST: it keeps the position it had at the start of that step, `status` = 1, `t_lost` = the time at the start of that step, and no
later call moves it - there is no reflection and no projection onto the wall.  On periodic axes positions are kept in
[lo, lo + L) and `wind` counts the crossings: `unwrapped` = positions + wind L.

Opt-in (npg_particles_walk): `walls=True` walks every move of a particle from cell to cell through a neighbour table
(`cell_neighbours`) and reflects it at boundary faces; `diffusion=` adds Visser's random-walk displacement with the buoyancy's
diffusivities after each RK4 step, so that a particle is a water parcel of dC/dt + u . grad C = c_d div(K grad C)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .architectures import DeviceVector
from .sampling import _FIELDS, Located, _engine, _evaluate, _partitioned, locator


def mesh_period(mesh):
    """The period vector (3,) of a mesh from its periodic pairing (gmsh's setPeriodic: paired nodes a translation apart), 0 on the
    axes that are not periodic; zeros for a mesh without pairing.  One axis-aligned translation is what is understood."""
    per = getattr(getattr(mesh, "model", None), "periodic", None)
    if per is None or not getattr(mesh, "periodic", False):
        return np.zeros(3)
    per = np.asarray(per, dtype=np.int64)
    img = np.nonzero(per != np.arange(len(per)))[0]
    if not len(img):
        return np.zeros(3)
    d = mesh.geo_coords[img] - mesh.geo_coords[per[img]]
    t = d[0]
    scale = np.abs(mesh.geo_coords).max()
    if np.abs(d - t).max() > 1e-9 * scale or np.count_nonzero(np.abs(t) > 1e-9 * scale) != 1:
        raise ValueError("ParticleTracker: the mesh's periodic pairing is not one axis-aligned translation - pass periodic=(Lx, Ly, Lz)")
    return np.where(np.abs(t) > 1e-9 * scale, np.abs(t), 0.0)


def cell_neighbours(mesh, cells=None, period=None):
    """(nbr (ncell, 4) int32, shift (ncell, 4, 3) int8) of a tetrahedral mesh, in the locator's local vertex order: nbr[c, i] = the cell
    across the face opposite local vertex i, -1 = a boundary face; shift[c, i] = the translation in periods that a point takes when it
    crosses that face, nonzero only across a periodic seam.  `cells` (ncell, 4): the vertex ids the faces are matched by - default
    mesh.cells, the canonical ids (periodic images mapped to their masters), so that the two sides of a seam are one face;
    mesh.cell_geo makes the seam a wall.  The translation is the difference of the two face centroids, each in its own cell's
    geometry, in units of `period` (default mesh_period(mesh))."""
    cells = np.asarray(mesh.cells if cells is None else cells, dtype=np.int64)
    nc = len(cells)
    period = np.asarray(mesh_period(mesh) if period is None else period, dtype=np.float64).reshape(3)
    opp = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])
    key = np.sort(cells[:, opp], axis=2).reshape(-1, 3)                  # row 4 c + i: the face opposite vertex i of cell c
    cen = mesh.geo_coords[np.asarray(mesh.cell_geo)[:, opp]].mean(axis=2).reshape(-1, 3)
    order = np.lexsort((key[:, 2], key[:, 1], key[:, 0]))
    ks = key[order]
    same = (ks[1:] == ks[:-1]).all(axis=1)
    if (same[1:] & same[:-1]).any():
        raise ValueError("cell_neighbours: a face belongs to more than two cells")
    a, b = order[:-1][same], order[1:][same]
    nbr = np.full(4 * nc, -1, dtype=np.int32)
    nbr[a], nbr[b] = b // 4, a // 4
    shift = np.zeros((4 * nc, 3), dtype=np.int8)
    d = cen[b] - cen[a]                                                  # what a point takes going from a's side to b's
    k = np.zeros_like(d)
    on = period > 0.0
    k[:, on] = np.rint(d[:, on] / period[on])
    if np.abs(d - k * period).max(initial=0.0) > 1e-9 * max(np.abs(mesh.geo_coords).max(), 1.0) or np.abs(k).max(initial=0.0) > 1:
        raise ValueError("cell_neighbours: two sides of a face are not a whole period apart - pass the mesh's period")
    shift[a], shift[b] = k, -k
    return nbr.reshape(nc, 4), shift.reshape(nc, 4, 3)


class ParticleTracker:
    """ParticleTracker(model, seeds, t0=None, nsub=4, periodic=None, walls=False, diffusion=None, seed=0): n particles seeded at `seeds` (n, 3) at time t0 (default: the
    model's current time) on the model's architecture.

      .advance(dt, x_prev=None)   nsub RK4 steps of dt / nsub through the model's CURRENT velocity (frozen over the call), or - x_prev a
                                  DeviceVector [u; p] - through the velocity blended linearly from x_prev at the start of the call to
                                  the current one at its end
      tracker(model, t)           the `on_plot` hook (model.run calls it every n_plot steps): advances from its own time to t, blending
                                  between the copy of [u; p] it kept at its last call (at construction, before the first) and the
                                  current one - correct for any n_plot, second order in time for n_plot = 1; it appends
                                  (t, unwrapped positions, status) to `.history` and reads nothing of the run's own bookkeeping
      .positions (n, 3), .unwrapped (n, 3), .wind (n, 3), .status (n,) 0 alive / 1 lost / 2 stuck, .cells (n,), .t_lost (n,) NaN while
                                  alive, .t, .reflections (n,) the hits of boundary faces (0 without walls)
      .sample(field)              nan_eval(model, field, .) at the current positions, located on the device ("u", "p", "b", "grad_b")
      .as_arrays() -> (t (k,), x (k, n, 3) unwrapped, status (k, n)); .save(path): np.savez with keys t, x, status, t_lost, period

    periodic: the period vector (Lx, Ly, Lz), 0 = not periodic; None takes it from the mesh's periodic pairing (`mesh_period`).  A seed
    that is NaN or outside the mesh is lost at t0.  The wrap applies to every particle, also where only a part of the domain is
    re-entrant (the channel of the channel basin: a basin particle does not reach its walls, u . n = 0 there).
    walls=True: every move (the RK4 stage points, the RK4 end point, the random displacement) is walked through `cell_neighbours` -
    into the neighbour across an interior face, with the seam's translation across a periodic one, reflected at a boundary face; no
    particle is lost at a wall.  A particle whose move needs more than 64 face events, or ends where the locator refuses it, is STUCK:
    `status` = 2, otherwise the rule of a lost one.  .advance, the hook, .history and .save are unchanged; they go through
    npg_particles_walk.  diffusion (implies walls): True = the model's kappa_h / kappa_v forcings at the mesh vertices and c_d =
    alpha^2 eps^2 / mu_rho of its parameters (the BACKGROUND diffusivities: the convection closure's part is not followed); or
    (kappa_h, kappa_v[, c_d]) - each a function of the coordinates (..., 3) -> (...), a nodal array (nv,) over the canonical vertices or
    (ncell, 4) over each cell's own, or a number.  After each RK4 step of length h a particle is displaced by delta + R sqrt(6 c_d
    kappa* h), delta = c_d h (d_x kappa_h, d_y kappa_h, d_z kappa_v), R uniform in (-1, 1) from Philox4x32-10 keyed by `seed` and counted
    by (particle index, step number): a path does not depend on the other particles.  .set_diffusion(diffusion, seed=None) replaces
    the tables between calls (None: off).
    Mesh-partitioned models are refused: a particle that leaves a rank's cells would have to be handed to the rank that owns its next
    cell, and that migration is not implemented."""

    def __init__(self, model, seeds, t0=None, nsub=4, periodic=None, walls=False, diffusion=None, seed=0):
        if _partitioned(model):
            raise NotImplementedError("ParticleTracker on a mesh-partitioned model is not implemented: a rank's locator and engine hold "
                                      "its own cells only, so a particle that crosses into another rank's cells would have to migrate "
                                      "between ranks - track particles on a single-device model")
        if int(nsub) < 1:
            raise ValueError(f"ParticleTracker: nsub must be >= 1, got {nsub}")
        self.model, self.nsub = model, int(nsub)
        self.ctx = model.arch.ctx
        self.fe, self.loc = _engine(model), locator(model)     # kept alive for as long as the particles are
        x0 = L.as_f64(seeds).reshape(-1, 3)
        self.n = len(x0)
        ts = getattr(model, "timestepper", None)
        self.t = float(t0 if t0 is not None else (ts.t if ts is not None else 0.0))
        self.period = L.as_f64(mesh_period(model.fe_data.mesh) if periodic is None else periodic).reshape(3).copy()
        h = C.c_void_p()
        L.check(L.lib().npg_particles_create(self.ctx.h, self.n, C.byref(h)))
        self.h = h
        L.check(L.lib().npg_particles_set_period(self.h, L.ptr(self.period)))
        L.check(L.lib().npg_particles_set(self.h, L.ptr(x0), self.t))
        self.walls, self.seed, self.c_d = bool(walls) or diffusion is not None, int(seed), None
        if self.walls:
            mesh = model.fe_data.mesh
            # without a period the seam is a wall: the faces are matched by the cells' own nodes
            self.nbr, self.shift = cell_neighbours(mesh, mesh.cells if self.period.any() else mesh.cell_geo, self.period)
            self.nbr, self.shift = L.as_i32(self.nbr), np.ascontiguousarray(self.shift, dtype=np.int8)
            L.check(L.lib().npg_particles_set_walls(self.h, L.ptr(self.nbr), L.ptr(self.shift), len(self.nbr)))
        if diffusion is not None:
            self.set_diffusion(diffusion)
        self._kept = model.inversion.solver.x.copy()           # the hook's own copy of [u; p], copied on the device
        self.history = []
        x = model.inversion.solver.x                           # settles the seeds: located, or lost at t0 (no step is counted)
        L.check(L.lib().npg_particles_advance(self.h, self.fe.h, self.loc.h, x.h, x.h, 0.0, 1.0, 0.0, 1))

    def __del__(self):
        try:
            if self.h:
                L.lib().npg_particles_destroy(self.h)          # the particles go before the locator and the engine they were advanced with
                self.h = None
            self.loc = self.fe = None
        except Exception:
            pass

    def __len__(self):
        return self.n

    def _advance(self, dt, x_prev, nsub):
        x = self.model.inversion.solver.x
        xa = x if x_prev is None else x_prev
        step = L.lib().npg_particles_walk if self.walls else L.lib().npg_particles_advance
        L.check(step(self.h, self.fe.h, self.loc.h, xa.h, x.h, 0.0, 1.0, float(dt), int(nsub)))
        self.t = self.t + float(dt)                            # the library's clock does the same addition

    def _kappa_table(self, v):
        mesh = self.model.fe_data.mesh
        if callable(v):
            v = v(mesh.geo_coords[mesh.cell_geo])
        v = np.asarray(v, dtype=np.float64)
        if v.shape == (mesh.nv,):
            v = v[mesh.cells]
        return L.as_f64(np.broadcast_to(v, (mesh.ncell, 4)) if v.ndim == 0 or v.shape == (mesh.ncell, 4) else v)

    def set_diffusion(self, diffusion=True, seed=None):
        """replace the diffusivities (and, seed given, the generator's key): True, (kappa_h, kappa_v[, c_d]) as at construction, or
        None = diffusion off (reflecting advection).  The step count goes on, so the random numbers do not repeat."""
        if not self.walls:
            raise ValueError("ParticleTracker.set_diffusion: a random walk needs walls - construct the tracker with walls=True or diffusion=")
        self.seed = self.seed if seed is None else int(seed)
        if diffusion is None or diffusion is False:
            L.check(L.lib().npg_particles_set_diffusion(self.h, None, None, 0, 0.0, 0))
            self.c_d = None
            return self
        prm = self.model.params
        if diffusion is True:
            diffusion = (self.model.forcings.kappa_h, self.model.forcings.kappa_v)
        kh, kv = self._kappa_table(diffusion[0]), self._kappa_table(diffusion[1])
        self.c_d = float(diffusion[2]) if len(diffusion) > 2 else float(prm.alpha ** 2 * prm.eps ** 2 / prm.mu_rho)
        ncell = int(self.model.fe_data.mesh.ncell)
        if kh.shape != (ncell, 4) or kv.shape != (ncell, 4):
            raise ValueError(f"ParticleTracker: a diffusivity must be a function, a number, (nv,) or (ncell, 4); got {kh.shape}, {kv.shape}")
        L.check(L.lib().npg_particles_set_diffusion(self.h, L.ptr(kh), L.ptr(kv), ncell, self.c_d, self.seed))
        return self

    def advance(self, dt, x_prev: DeviceVector = None):
        self._advance(dt, x_prev, self.nsub)
        return self

    def __call__(self, model, t):
        self.advance(float(t) - self.t, self._kept)
        self.t = float(t)                                      # (t - self.t) + self.t can be an ulp off t
        self._kept.copy_from(model.inversion.solver.x)
        self.history.append((self.t, self.unwrapped, self.status))

    def _download(self, what):
        shapes = dict(xyz=((self.n, 3), np.float64), cell=((self.n,), np.int32), status=((self.n,), np.int32),
                      wind=((self.n, 3), np.int32), t_lost=((self.n,), np.float64))
        out = {k: np.empty(*shapes[k]) for k in what}
        args = [L.ptr(out[k]) if k in out else None for k in ("xyz", "cell", "status", "wind", "t_lost")]
        L.check(L.lib().npg_particles_download(self.h, *args))
        return out

    @property
    def positions(self):
        return self._download(("xyz",))["xyz"]

    @property
    def wind(self):
        return self._download(("wind",))["wind"]

    @property
    def unwrapped(self):
        d = self._download(("xyz", "wind"))
        return d["xyz"] + d["wind"] * self.period

    @property
    def status(self):
        return self._download(("status",))["status"]

    @property
    def cells(self):
        """the cell each particle was last located in, -1 for a seed that never was"""
        return self._download(("cell",))["cell"]

    @property
    def reflections(self):
        """how often each particle was reflected at a boundary face (the moves that moved it: stage points do not count)"""
        out = np.zeros(self.n, dtype=np.int32)
        L.check(L.lib().npg_particles_download_walk(self.h, L.ptr(out), None))
        return out

    @property
    def step(self):
        """the generator's step number: the steps walked since the seeds were set"""
        k = C.c_uint64(0)
        L.check(L.lib().npg_particles_download_walk(self.h, None, C.byref(k)))
        return int(k.value)

    @property
    def t_lost(self):
        return self._download(("t_lost",))["t_lost"]

    def sample(self, field):
        """the field at the current positions: the positions are copied on the device (npg_particles_positions), located and evaluated
        as nan_eval does - "b" and "grad_b" are the full buoyancy.  A lost particle is sampled where it stopped."""
        if field not in _FIELDS:
            raise ValueError(f"ParticleTracker.sample: field must be one of {sorted(_FIELDS)}, got {field!r}")
        nc = _FIELDS[field][1]
        if self.n == 0:
            return np.empty((0, nc) if nc > 1 else (0,))
        pv = DeviceVector(self.ctx, 3 * self.n)
        L.check(L.lib().npg_particles_positions(self.h, pv.h))
        found = Located(self.ctx, self.n)
        L.check(L.lib().npg_locator_find(self.loc.h, pv.h, self.n, found.h))
        v = _evaluate(self.model, field, found)
        N2 = self.model.params.N2
        if N2 != 0.0 and field == "b":
            v = v + N2 * pv.to_host().reshape(-1, 3)[:, 2]
        elif N2 != 0.0 and field == "grad_b":
            v[:, 2] += N2
        return v

    def as_arrays(self):
        k = len(self.history)
        return (np.array([h[0] for h in self.history], dtype=np.float64),
                np.array([h[1] for h in self.history], dtype=np.float64).reshape(k, self.n, 3),
                np.array([h[2] for h in self.history], dtype=np.int32).reshape(k, self.n))

    def save(self, path):
        t, x, status = self.as_arrays()
        np.savez(path, t=t, x=x, status=status, t_lost=self.t_lost, period=self.period)
