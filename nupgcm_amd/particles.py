"""Lagrangian particles advected through the device-resident flow (npg_particles_advance): where a water parcel goes -
residence times in the bowl, parcels circling the re-entrant channel, the pathways of the overturning.  The reference has no
counterpart; offline it would need the velocity saved every timestep.

One fused kernel carries every particle through `nsub` classical RK4 steps per call: locate -> evaluate u -> next stage, with the
cell of the last location remembered, so that a particle which stays in its cell never looks at the locator's bins.  Between two
calls the velocity is blended linearly in model time between two vectors [u; p]; model time is the particles' clock (the
nondimensional buoyancy equation carries the same factor in front of d_t b and u . grad b).  A particle that would leave the mesh is
LOST: it keeps the position it had at the start of that step, `status` = 1, `t_lost` = the time at the start of that step, and no
later call moves it - there is no reflection and no projection onto the wall.  On periodic axes positions are kept in
[lo, lo + L) and `wind` counts the crossings: `unwrapped` = positions + wind L."""
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


class ParticleTracker:
    """ParticleTracker(model, seeds, t0=None, nsub=4, periodic=None): n particles seeded at `seeds` (n, 3) at time t0 (default: the
    model's current time) on the model's architecture.

      .advance(dt, x_prev=None)   nsub RK4 steps of dt / nsub through the model's CURRENT velocity (frozen over the call), or - x_prev a
                                  DeviceVector [u; p] - through the velocity blended linearly from x_prev at the start of the call to
                                  the current one at its end
      tracker(model, t)           the `on_plot` hook (model.run calls it every n_plot steps): advances from its own time to t, blending
                                  between the copy of [u; p] it kept at its last call (at construction, before the first) and the
                                  current one - correct for any n_plot, second order in time for n_plot = 1; it appends
                                  (t, unwrapped positions, status) to `.history` and reads nothing of the run's own bookkeeping
      .positions (n, 3), .unwrapped (n, 3), .wind (n, 3), .status (n,) 0 alive / 1 lost, .cells (n,), .t_lost (n,) NaN while alive, .t
      .sample(field)              nan_eval(model, field, .) at the current positions, located on the device ("u", "p", "b", "grad_b")
      .as_arrays() -> (t (k,), x (k, n, 3) unwrapped, status (k, n)); .save(path): np.savez with keys t, x, status, t_lost, period

    periodic: the period vector (Lx, Ly, Lz), 0 = not periodic; None takes it from the mesh's periodic pairing (`mesh_period`).  A seed
    that is NaN or outside the mesh is lost at t0.  The wrap applies to every particle, also where only a part of the domain is
    re-entrant (the channel of the channel basin: a basin particle does not reach its walls, u . n = 0 there).
    Mesh-partitioned models are refused: a particle that leaves a rank's cells would have to be handed to the rank that owns its next
    cell, and that migration is not implemented."""

    def __init__(self, model, seeds, t0=None, nsub=4, periodic=None):
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
        self._kept = model.inversion.solver.x.copy()           # the hook's own copy of [u; p], copied on the device
        self.history = []
        self._advance(0.0, None, 1)                            # settles the seeds: located, or lost at t0

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
        L.check(L.lib().npg_particles_advance(self.h, self.fe.h, self.loc.h, xa.h, x.h, 0.0, 1.0, float(dt), int(nsub)))
        self.t = self.t + float(dt)                            # the library's clock does the same addition

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
