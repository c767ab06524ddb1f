"""Time-dependent surface forcing and a restoring buoyancy condition (npg_forcing_*).  The reference's forcings are
set-up constants: tau_x, tau_y and the flux of a SurfaceFluxBC are integrated once over the surface, on the host.

SurfaceForcing(model, ...) replaces the two constant surface vectors - the wind part of inversion.b and evolution.rhs_flux - by vectors
recomputed on the device for the time level being solved, from keyframe tables at the face points, and optionally adds the restoring
term flux = gamma (b* - b): its load alpha int gamma b* phi_i goes into rhs_flux, its matrix S = alpha int gamma phi_i phi_j into the
evolution's left-hand side, A = M + theta (Kh + Kv) + dt S (dt: the factor of rhs_flux in npg_fe_evolution_rhs, in both schemes - so
b = b* stays a fixed point of the restoring term).  run() calls apply(model, t_{n+1}) before evolve(): both solves of a step produce
level n + 1.  Opt-in like model.tracers: a model without one computes what it always did.

The time rule is one function, series_key_weight: between keyframes (1 - w) a + w b with w formed on the host in fp64; outside the
range the first / last value is held, or, with a period, the last keyframe blends into the first over [times[-1], times[0] + period).

BoundaryIntegrals reads its tau_x / tau_y / flux tables at construction and does NOT follow an attached forcing by itself: keep it
current with  bi.set_coeff(L.NPG_BND_TAUX, forcing.tables(t)["tau_x"], on_surface)  (tables(t) is in the order of forcing.faces)."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib as L
from .boundary import _at_points, face_cells
from .evolution import collect_evolution_LHS, lhs_timestepper
from .fe import tri_quadrature_degree4
from .inputs import SurfaceFluxBC

SERIES = ("tau_x", "tau_y", "flux", "target")


def series_key_weight(times, period, t):
    """The time rule: (key, w) such that the value at time t is (1 - w) field[key] + w field[key + 1] - behind the last keyframe
    field[0], the periodic wrap.  times: strictly increasing keyframe times; period: None, or > times[-1] - times[0].
    Without a period the first value is held before times[0] and the last after times[-1] (w = 0).  With one,
    s = times[0] + (t - times[0]) mod period and the last keyframe blends into the first over [times[-1], times[0] + period).
    One keyframe: (0, 0.0) whatever t is.  w is fp64, in [0, 1]; w = 0 returns the keyframe's own bits."""
    times = np.asarray(times, dtype=np.float64)
    K, t = len(times), float(t)
    if not math.isfinite(t):
        raise ValueError(f"series_key_weight: t must be finite, got {t}")
    if K == 1:
        return 0, 0.0
    t0, t1 = float(times[0]), float(times[-1])
    if period is None:
        if t <= t0:
            return 0, 0.0
        if t >= t1:
            return K - 1, 0.0
        s = t
    else:
        period = float(period)
        r = (t - t0) % period                    # in [0, period]; == period only through rounding (a tiny negative t - t0)
        s = t0 + (r if r < period else 0.0)
    k = min(int(np.searchsorted(times, s, side="right")) - 1, K - 1)
    k = max(k, 0)
    if k < K - 1:
        w = (s - float(times[k])) / (float(times[k + 1]) - float(times[k]))
    else:
        w = (s - t1) / (t0 + period - t1)
    return k, min(max(w, 0.0), 1.0)


class ForcingSeries:
    """ForcingSeries(times, fields, period=None): K >= 1 keyframes at strictly increasing times; each field a number, a function of x
    or a table (nface, 9) at the face points (the order of SurfaceForcing.faces and its .points).  `.key_weight(t)` is
    series_key_weight with this series' times and period."""

    def __init__(self, times, fields, period=None):
        self.times = np.atleast_1d(np.asarray(times, dtype=np.float64))
        self.fields = list(fields)
        if self.times.ndim != 1 or len(self.times) < 1 or len(self.fields) != len(self.times):
            raise ValueError(f"ForcingSeries: one field per keyframe time, got {len(self.fields)} fields for times of shape {self.times.shape}")
        if not np.isfinite(self.times).all() or (np.diff(self.times) <= 0.0).any():
            raise ValueError("ForcingSeries: times must be finite and strictly increasing")
        self.period = None if period is None else float(period)
        if self.period is not None and not (math.isfinite(self.period) and self.period > self.times[-1] - self.times[0]):
            raise ValueError(f"ForcingSeries: the period must exceed times[-1] - times[0] = {self.times[-1] - self.times[0]}, got {period}")

    def key_weight(self, t):
        return series_key_weight(self.times, self.period, t)

    def evaluate(self, points):
        """the keyframes at the face points (nface, 9, 3) -> (K, nface, 9)"""
        out = np.empty((len(self.fields),) + points.shape[:2])
        for k, v in enumerate(self.fields):
            out[k] = _table(v, points, f"ForcingSeries: keyframe {k}")
        return out


def _table(v, points, who):
    if isinstance(v, np.ndarray) and v.ndim > 0:
        if v.shape != points.shape[:2]:
            raise ValueError(f"{who}: a table must have shape {points.shape[:2]}, got {v.shape}")
        return np.asarray(v, dtype=np.float64)
    return _at_points(v, points)


def _as_series(v):
    return v if isinstance(v, ForcingSeries) else ForcingSeries([0.0], [v])


class SurfaceForcing:
    """SurfaceForcing(model, tau_x=None, tau_y=None, flux=None, restoring=None, mask=None), set as `model.surface_forcing`.

    tau_x, tau_y, flux: a number, a function of x or a ForcingSeries; None = the model's own static value (forcings.tau_x, .tau_y, the
    flux of a SurfaceFluxBC, else 0).  restoring = (gamma, target): gamma static (a number or a function of x, >= 0 at every face
    point), target a number, a function of x or a ForcingSeries.  mask (nsurface_faces,) bool restricts the forcing to some of the
    faces carrying the mesh's surface_tags - `.faces` (sorted topological vertex triples, sorted by cell), with `.face_cell`,
    `.face_local`, `.points` (nface, 9, 3).
    `.apply(model, t)` overwrites model.evolution.rhs_flux with alpha [load(F(t) + gamma b*(t))] and model.inversion.b with
    b_lift + alpha load(tau(t)) on the u_x / u_y rows: two launches, no host arithmetic beyond the (key, w) pairs, no download.
    `.detach()` restores the static vectors and the left-hand side without S.  `.tables(t)`: the blended point tables of tau_x, tau_y,
    flux (nface, 9) - what BoundaryIntegrals.set_coeff takes.  `.S`: the surface matrix (DeviceCSR, pattern "b") or None.
    Refused: mesh-partitioned and replicated-distributed models, embedded 2-D meshes (NotImplementedError); restoring together with
    model.tracers (the tracers share solver.A and would be restored towards 0: out of scope - isoneutral tracers have a matrix of their own and are accepted); restoring or a non-zero flux where a
    buoyancy Dirichlet node lies on a forced face, non-finite values, negative gamma, a toolkit without b_lift (ValueError).  A failed
    constructor leaves the model as it was."""

    def __init__(self, model, tau_x=None, tau_y=None, flux=None, restoring=None, mask=None):
        _refuse_model(model)
        if model.evolution is None:
            raise ValueError("SurfaceForcing: the model has no EvolutionToolkit")
        if getattr(model.inversion, "b_lift", None) is None:
            raise ValueError("SurfaceForcing: the InversionToolkit has no b_lift (it was built from ready-made A, P, B, b): the Dirichlet "
                             "lift without the wind is not known")
        if getattr(model, "surface_forcing", None) is not None:
            raise ValueError("SurfaceForcing: the model already has a surface forcing - detach() it first")
        if restoring is not None and getattr(model, "tracers", None) is not None and getattr(model.tracers, "isoneutral", None) is None:
            raise NotImplementedError("SurfaceForcing(restoring=...) on a model with passive tracers is out of scope: the tracers share "
                                      "the evolution's matrix and would be restored towards 0")   # (isoneutral tracers have their own)
        self.model = model
        fed, frc = model.fe_data, model.forcings
        m = fed.mesh
        self.ctx = model.arch.ctx
        self.alpha = float(model.params.alpha)
        # the surface faces, sorted by cell
        faces, fgeo = m.boundary_faces(m.surface_tags, with_geometry=True)
        cell, local = face_cells(m, faces)
        order = np.argsort(cell, kind="stable")
        self.faces, self.face_cell, self.face_local, fgeo = faces[order], cell[order], local[order], fgeo[order]
        nf = len(self.faces)
        keep = np.ones(nf, dtype=bool) if mask is None else np.asarray(mask)
        if keep.shape != (nf,) or keep.dtype != bool:
            raise ValueError(f"SurfaceForcing: mask must be a bool array of shape ({nf},), got {keep.dtype} {keep.shape}")
        self.mask = keep.copy()
        X = m.geo_coords[fgeo]
        self.area2 = np.linalg.norm(np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]), axis=1)
        lam, _ = tri_quadrature_degree4()
        self.points = np.einsum("qk,fki->fqi", lam, X)                         # (nf, 9, 3): the points of Mesh.surface_load
        # the series; None = the model's own static value
        static_flux = frc.b_surface_bc.flux if isinstance(frc.b_surface_bc, SurfaceFluxBC) else 0.0
        given = dict(tau_x=frc.tau_x if tau_x is None else tau_x, tau_y=frc.tau_y if tau_y is None else tau_y,
                     flux=static_flux if flux is None else flux)
        self.restoring = restoring is not None
        self.gamma_table = None
        if self.restoring:
            try:
                gamma, target = restoring
            except (TypeError, ValueError):
                raise ValueError("SurfaceForcing: restoring must be (gamma, target)") from None
            if isinstance(gamma, ForcingSeries):
                raise NotImplementedError("SurfaceForcing: a time-dependent gamma is out of scope (S would change with time)")
            given["target"] = target
            g = _table(gamma, self.points, "SurfaceForcing: gamma")
            if not np.isfinite(g).all():
                raise ValueError("SurfaceForcing: gamma is not finite at some face point")
            if (g[keep] < 0.0).any():
                raise ValueError("SurfaceForcing: gamma must be >= 0 at every face point")
            self.gamma_table = np.where(keep[:, None], g, 0.0)
        self.series, self.key_tables = {}, {}
        for name, v in given.items():
            s = _as_series(v)
            tab = s.evaluate(self.points)                                      # (K, nf, 9), every keyframe evaluated once
            if not np.isfinite(tab[:, keep]).all():
                raise ValueError(f"SurfaceForcing: {name} is not finite at some face point")
            tab = np.where(keep[None, :, None], tab, 0.0)
            if name == "target" or np.any(tab != 0.0):
                self.series[name], self.key_tables[name] = s, tab
        # a prescribed or restoring flux needs free buoyancy nodes under it
        kidx = np.nonzero(keep)[0]
        fnodes = np.sort(self.faces[kidx], axis=1)
        if fed.spaces.b_order == 2:
            en = np.stack([m.edge_ids(fnodes[:, i], fnodes[:, j]) for (i, j) in ((0, 1), (0, 2), (1, 2))], axis=1)
            fnodes = np.hstack([fnodes, m.nv + en])
        if (self.restoring or "flux" in self.series) and (fed.spaces.b_dof[fnodes] < 0).any():
            raise ValueError("SurfaceForcing: a buoyancy Dirichlet node lies on a forced face - its value is pinned, a prescribed or "
                             "restoring flux cannot act there (mask those faces out, or drop the Dirichlet tag)")
        # the handle, on the faces that count
        ev, inv = model.evolution, model.inversion
        self.fe = ev.fe
        self._pattern = self.fe.new_matrix("b") if self.restoring else None
        k = self._keep = dict(cell=L.as_i32(self.face_cell[kidx]), local=np.ascontiguousarray(self.face_local[kidx], dtype=np.uint8),
                              area2=L.as_f64(self.area2[kidx]))
        self.kept = kidx
        self.h = None
        h = C.c_void_p()
        L.check(L.lib().npg_forcing_create(self.fe.h, len(kidx), L.ptr(k["cell"]), L.ptr(k["local"]), L.ptr(k["area2"]),
                                           None if self._pattern is None else self._pattern.h, C.byref(h)))
        self.h = h
        for name, tab in self.key_tables.items():
            dev = L.as_f64(np.transpose(tab[:, kidx], (0, 2, 1)))              # [K][9][nface]
            L.check(L.lib().npg_forcing_set_series(self.h, SERIES.index(name), len(tab), L.ptr(dev)))
        self.S = None
        if self.restoring:
            gt = L.as_f64(self.gamma_table[kidx].T)                             # [9][nface]
            L.check(L.lib().npg_forcing_set_gamma(self.h, L.ptr(gt)))
            L.check(L.lib().npg_forcing_surface_matrix(self.h, self.alpha, self._pattern.h))
            self.S = self._pattern
        # from here on the model changes
        self._static = (inv.b.copy(), ev.rhs_flux.copy())
        self._key = (C.c_int32 * L.NPG_FRC_NSERIES)()
        self._w = (C.c_double * L.NPG_FRC_NSERIES)()
        model.surface_forcing = self
        if self.S is not None:
            ev.S = self.S
            collect_evolution_LHS(ev, model.params, frc, lhs_timestepper(ev, model.timestepper, model.step_index))

    def __del__(self):
        try:
            if self.h:
                L.lib().npg_forcing_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def key_weights(self, t):
        """{series name: (key, w)} at time t"""
        return {name: s.key_weight(t) for name, s in self.series.items()}

    def apply(self, model, t):
        """the surface vectors of the time level t: model.inversion.b and model.evolution.rhs_flux, overwritten on the device"""
        for name, s in self.series.items():
            i = SERIES.index(name)
            self._key[i], self._w[i] = s.key_weight(t)
        L.check(L.lib().npg_forcing_apply(self.h, self._key, self._w, self.alpha, model.inversion.b_lift.h, model.inversion.b.h,
                                          model.evolution.rhs_flux.h))
        return self

    def tables(self, t):
        """the blended point tables of tau_x, tau_y and the prescribed flux at time t: {name: (nface, 9)} in the order of `.faces`
        (zeros on faces the mask leaves out) - what BoundaryIntegrals.set_coeff takes"""
        out = {}
        for name in ("tau_x", "tau_y", "flux"):
            if name not in self.series:
                out[name] = np.zeros(self.points.shape[:2])
                continue
            tab = self.key_tables[name]
            k, w = self.series[name].key_weight(t)
            out[name] = tab[k].copy() if w == 0.0 else (1.0 - w) * tab[k] + w * tab[(k + 1) % len(tab)]
        return out

    def info(self):
        """dict(nface, wind_slots, flux_slots, matrix_entries, matrix_slots) of the handle's plan"""
        v = [C.c_int64() for _ in range(5)]
        L.check(L.lib().npg_forcing_info(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("nface", "wind_slots", "flux_slots", "matrix_entries", "matrix_slots"), (x.value for x in v)))

    def detach(self):
        """give the model its static surface vectors and the left-hand side without S back"""
        model = self.model
        if getattr(model, "surface_forcing", None) is not self:
            return self
        ev, inv = model.evolution, model.inversion
        inv.b.copy_from(self._static[0])
        ev.rhs_flux.copy_from(self._static[1])
        model.surface_forcing = None
        if self.S is not None:
            ev.S = None
            collect_evolution_LHS(ev, model.params, model.forcings, lhs_timestepper(ev, model.timestepper, model.step_index))
        return self


def _refuse_model(model):
    if getattr(model.fe_data.mesh, "dim", 3) != 3:
        raise NotImplementedError("SurfaceForcing is implemented for tetrahedral (3-D) meshes: the surface of an embedded 2-D mesh is made "
                                  "of segments, not of faces")
    if getattr(model, "layout", None) is not None and (hasattr(model.layout, "cell_owner") or hasattr(model.layout, "locator_cells")):
        raise NotImplementedError("SurfaceForcing on a mesh-partitioned model is not implemented (every rank would hold the faces of the "
                                  "cells it owns and the interface rows would be exchanged): force a single-device model")
    if getattr(model, "partition", None) is not None or getattr(model, "comm", None) is not None \
            or getattr(model.arch.ctx, "nranks", 1) > 1:
        raise NotImplementedError("SurfaceForcing of the replicated distributed layout is not implemented: use a single-device model")
