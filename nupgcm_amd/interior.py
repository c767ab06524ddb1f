"""Interior buoyancy forcing: volume sources and sponge layers (npg_interior_*).  The reference - and forcing.SurfaceForcing -
force the buoyancy at the boundary only; nothing acts in the interior.

InteriorForcing(model, ...) adds  Q(x, t) + gamma(x) (b*(x, t) - b')  to the tendency of b': a volume source and a relaxation towards a
prescribed profile at the rate gamma, as the sponge that closes a channel model.  With c the scheme constant of the step (dt for BDF1,
2/3 dt for BDF2 - the factor npg_tracers_rhs puts on a tracer's source) the step solves

    (M + theta (Kh + Kv) [+ dt S] + c R) b1 = ... + c load,     R_ij = int gamma phi_i phi_j,   load_i = int (Q + gamma (b* - b_D)) phi_i

with b_D the finite-element function of the Dirichlet nodal values (the Dirichlet columns of R, lifted into the load; Dirichlet rows get
nothing).  c is that of the left-hand side the solver holds (evolution.lhs_timestepper) on both sides, so b = b* stays a fixed point of
the restoring term on the BDF1 first step of a BDF2 run too.  R is formed once, the load for every time level, both on the device from
keyframe tables at the points of the engine's own volume rule - the rule NPG_MAT_M is assembled with, so a constant gamma gives gamma M
up to rounding.  run() calls apply(model, t_{n+1}) before evolve().  Opt-in like model.tracers and model.surface_forcing: a model
without one computes what it always did; the two forcings never write each other's vectors and attach / detach in any order.

Caveat: the engine's 11-point rule has one negative weight.  For a gamma that varies strongly inside a cell the cell's contribution to R
need not be positive semi-definite; A stays SPD as long as c gamma (its variation over a cell) is small against M.  Choose gamma smooth
on the scale of the cells."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .architectures import DeviceVector
from .evolution import collect_evolution_LHS, lhs_timestepper
from .forcing import ForcingSeries, _as_series, _table

SERIES = ("source", "target")


class InteriorForcing:
    """InteriorForcing(model, source=None, restoring=None, cells=None), set as `model.interior_forcing`.

    source: Q, the tendency added to d_t b' - a number, a function of x, a table (ncell, nq) at the cells' quadrature points
    (Mesh.quad_points()) or a ForcingSeries of those.  restoring = (gamma, target): gamma static, >= 0 at every point (a number, a
    function of x or a table), target = b* in the units of the model's b' (a number, a function of x, a table or a ForcingSeries).
    cells (ncell,) bool restricts the forcing to some cells.  Cells the mask leaves out, and cells where gamma and every keyframe of Q
    vanish at all points, are dropped on the host: the handle holds the kept cells only - `.cells` (ascending), `.points`
    (nkept, nq, 3), `.weights` (nkept, nq).
    `.apply(model, t)` overwrites `.rhs_src` (evolution.rhs_src) with the load of the time level t: two launches, no host arithmetic
    beyond the (key, w) pairs, no download.  `.R`: the sponge's matrix (DeviceCSR, pattern "b") or None.  `.detach()` clears both
    slots of the toolkit and recombines the left-hand side: the model has the bits it had before.  `.tables(t)`: the blended Q and b*
    at the points; `.key_weights(t)`; `.info()`; `.budget(model, t)`: dict(volume, source, restoring) = int dV, int Q dV,
    int gamma (b* - b) dV over the kept cells for the device-resident b (one deterministic device pass, three doubles downloaded).
    Refused: mesh-partitioned and replicated-distributed models, embedded 2-D meshes, a time-dependent gamma, restoring together with
    model.tracers (NotImplementedError; a pure source and tracers get along, and so do isoneutral tracers: their matrix is their own); non-finite values, negative gamma, a second
    InteriorForcing on the model, a mask of the wrong shape or dtype (ValueError).  A failed constructor leaves the model as it was.
    The 11-point rule has a negative weight: keep gamma smooth on the scale of a cell (see the module's caveat)."""

    def __init__(self, model, source=None, restoring=None, cells=None):
        _refuse_model(model)
        if model.evolution is None:
            raise ValueError("InteriorForcing: the model has no EvolutionToolkit")
        if getattr(model, "interior_forcing", None) is not None:
            raise ValueError("InteriorForcing: the model already has an interior forcing - detach() it first")
        if restoring is not None and getattr(model, "tracers", None) is not None and getattr(model.tracers, "isoneutral", None) is None:
            raise NotImplementedError("InteriorForcing(restoring=...) on a model with passive tracers is out of scope: the tracers share "
                                      "the evolution's matrix and would be restored towards 0")   # (isoneutral tracers have their own)
        self.model = model
        fed = model.fe_data
        m = fed.mesh
        self.ctx = model.arch.ctx
        pts = m.quad_points()                                                  # (ncell, nq, 3): the points NPG_MAT_M is assembled at
        nc, nq = pts.shape[:2]
        keep = np.ones(nc, dtype=bool) if cells is None else np.asarray(cells)
        if keep.shape != (nc,) or keep.dtype != bool:
            raise ValueError(f"InteriorForcing: cells must be a bool array of shape ({nc},), got {keep.dtype} {keep.shape}")
        self.mask = keep.copy()
        self.restoring = restoring is not None
        given = dict(source=0.0 if source is None else source)
        gamma_table = np.zeros((nc, nq))
        if self.restoring:
            try:
                gamma, target = restoring
            except (TypeError, ValueError):
                raise ValueError("InteriorForcing: restoring must be (gamma, target)") from None
            if isinstance(gamma, ForcingSeries):
                raise NotImplementedError("InteriorForcing: a time-dependent gamma is out of scope (R would change with time)")
            given["target"] = target
            g = _table(gamma, pts, "InteriorForcing: gamma")
            if not np.isfinite(g).all():
                raise ValueError("InteriorForcing: gamma is not finite at some point")
            if (g[keep] < 0.0).any():
                raise ValueError("InteriorForcing: gamma must be >= 0 at every point")
            gamma_table = np.where(keep[:, None], g, 0.0)
        series, key_tables = {}, {}
        for name, v in given.items():
            s = _as_series(v)
            tab = s.evaluate(pts)                                              # (K, ncell, nq), every keyframe evaluated once
            if not np.isfinite(tab[:, keep]).all():
                raise ValueError(f"InteriorForcing: {name} is not finite at some point")
            series[name], key_tables[name] = s, np.where(keep[None, :, None], tab, 0.0)
        # the kept cells: inside the mask, and gamma or some keyframe of Q non-zero somewhere in the cell
        active = keep & ((gamma_table != 0.0).any(axis=1) | (key_tables["source"] != 0.0).any(axis=(0, 2)))
        kidx = np.nonzero(active)[0]
        self.cells = L.as_i32(kidx)
        self.points = pts[kidx]
        self.weights = m.q_w[None, :] * np.asarray(m.detJ)[kidx, None]
        self.gamma_table = gamma_table[kidx] if self.restoring else None
        if not np.any(key_tables["source"][:, kidx] != 0.0):
            del series["source"], key_tables["source"]
        self.series = series
        self.key_tables = {name: np.ascontiguousarray(tab[:, kidx]) for name, tab in key_tables.items()}      # (K, nkept, nq)
        # the handle, on the kept cells
        ev = model.evolution
        self.fe = ev.fe
        self._pattern = self.fe.new_matrix("b") if self.restoring else None
        self.h = None
        h = C.c_void_p()
        L.check(L.lib().npg_interior_create(self.fe.h, len(kidx), L.ptr(self.cells), None if self._pattern is None else self._pattern.h,
                                            C.byref(h)))
        self.h = h
        for name, tab in self.key_tables.items():
            dev = L.as_f64(np.transpose(tab, (0, 2, 1)))                       # [K][nq][nkept]
            L.check(L.lib().npg_interior_set_series(self.h, SERIES.index(name), len(tab), L.ptr(dev)))
        self.R = None
        if self.restoring:
            gt = L.as_f64(self.gamma_table.T)                                   # [nq][nkept]
            L.check(L.lib().npg_interior_set_gamma(self.h, L.ptr(gt)))
            L.check(L.lib().npg_interior_matrix(self.h, self._pattern.h))
            self.R = self._pattern
        self.rhs_src = DeviceVector(self.ctx, fed.dofs.nb)
        self._key = (C.c_int32 * L.NPG_ITR_NSERIES)()
        self._w = (C.c_double * L.NPG_ITR_NSERIES)()
        self._out = DeviceVector(self.ctx, L.NPG_ITR_NBUDGET)
        ts = getattr(model, "timestepper", None)
        if ts is not None:
            self._load(ts.t + ts.dt)                                           # the next level's load, for a caller that drives evolve() itself
        # from here on the model changes
        model.interior_forcing = self
        ev.rhs_src = self.rhs_src
        if self.R is not None:
            ev.R = self.R
            collect_evolution_LHS(ev, model.params, model.forcings, lhs_timestepper(ev, model.timestepper, model.step_index))

    def __del__(self):
        try:
            if self.h:
                L.lib().npg_interior_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def key_weights(self, t):
        """{series name: (key, w)} at time t"""
        return {name: s.key_weight(t) for name, s in self.series.items()}

    def _set_keys(self, t):
        for name, s in self.series.items():
            i = SERIES.index(name)
            self._key[i], self._w[i] = s.key_weight(t)

    def _load(self, t):
        self._set_keys(t)
        L.check(L.lib().npg_interior_apply(self.h, self._key, self._w, self.rhs_src.h))

    def apply(self, model, t):
        """the volume load of the time level t: `.rhs_src`, overwritten on the device (evolve() scales it by the step's constant c)"""
        self._load(t)
        return self

    def tables(self, t):
        """the blended point tables at time t in the order of `.cells`: {"source": (nkept, nq)} (zeros without a source) and, with
        restoring, {"target": (nkept, nq)}"""
        out = {"source": np.zeros(self.points.shape[:2])}
        for name, tab in self.key_tables.items():
            k, w = self.series[name].key_weight(t)
            out[name] = tab[k].copy() if w == 0.0 else (1.0 - w) * tab[k] + w * tab[(k + 1) % len(tab)]
        return out

    def info(self):
        """dict(nkept, load_slots, matrix_entries, matrix_slots) of the handle's plan"""
        v = [C.c_int64() for _ in range(4)]
        L.check(L.lib().npg_interior_info(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("nkept", "load_slots", "matrix_entries", "matrix_slots"), (x.value for x in v)))

    def budget(self, model, t):
        """dict(volume, source, restoring): int dV, int Q(t) dV and int gamma (b*(t) - b) dV over the kept cells for model.b_vec"""
        self._set_keys(t)
        L.check(L.lib().npg_interior_budget(self.h, self._key, self._w, model.b_vec.h, self._out.h))
        return dict(zip(("volume", "source", "restoring"), (float(x) for x in self._out.to_host())))

    def detach(self):
        """clear the toolkit's two slots and recombine the left-hand side without R: the model has the bits it had before"""
        model = self.model
        if getattr(model, "interior_forcing", None) is not self:
            return self
        ev = model.evolution
        model.interior_forcing = None
        ev.rhs_src = None
        if self.R is not None:
            ev.R = None
            collect_evolution_LHS(ev, model.params, model.forcings, lhs_timestepper(ev, model.timestepper, model.step_index))
        return self


def _refuse_model(model):
    if getattr(model.fe_data.mesh, "dim", 3) != 3:
        raise NotImplementedError("InteriorForcing is implemented for tetrahedral (3-D) meshes")
    if getattr(model, "layout", None) is not None and (hasattr(model.layout, "cell_owner") or hasattr(model.layout, "locator_cells")):
        raise NotImplementedError("InteriorForcing on a mesh-partitioned model is not implemented (every rank would hold the cells it "
                                  "owns and the interface rows would be exchanged): force a single-device model")
    if getattr(model, "partition", None) is not None or getattr(model, "comm", None) is not None \
            or getattr(model.arch.ctx, "nranks", 1) > 1:
        raise NotImplementedError("InteriorForcing of the replicated distributed layout is not implemented: use a single-device model")
