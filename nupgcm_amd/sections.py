"""Transports through sections: exact quadrature of the device-resident state on the polygons that planes cut out of the mesh's cells
(npg_sections_compute) - how much goes through a meridional section of the channel, across a latitude by depth, across
a depth level, through a line between two points.  The reference stops at sampled slices and streamfunctions of a .vtu file.

A plane cuts a tetrahedron in a triangle or a quadrilateral; the fields are piecewise polynomials of degree <= 2, so u . n, b' u . n and
the rest integrate exactly with a degree-4 rule on the cut polygons.  Bins in the two in-plane coordinates are geometric: the polygons
are clipped at the bin edges, every term's destination is static, and every sum has one order - two calls return the same bits.
NPG_NSEC = 14 raw channels per bin (csrc/sections_core.h lists them, and states the cut rule: a vertex ON the plane counts as above,
so a mesh face lying in the plane is counted by exactly one of its two cells)."""
from __future__ import annotations

import ctypes as C
import time

import numpy as np

from . import _lib as L
from .architectures import DeviceVector
from .inversion import device_fe

NSEC = L.NPG_NSEC
CHANNELS = ("one", "u_n", "b", "b_u_n", "z_u_n", "p", "u_x", "u_y", "u_z", "grad_b_n", "kappa_grad_b_n", "kv_n_z", "z", "dz_b")
# the symmetric degree-4 rule of csrc/sections_core.h: barycentrics with respect to a piece's corners
_A1, _A2, _B1, _B2 = 0.108103018168070, 0.445948490915965, 0.816847572980459, 0.091576213509771
RULE_MU = np.array([[_A1, _A2, _A2], [_A2, _A1, _A2], [_A2, _A2, _A1], [_B1, _B2, _B2], [_B2, _B1, _B2], [_B2, _B2, _B1]])
RULE_W = np.array([0.223381589678011] * 3 + [0.109951743655322] * 3)


def _refuse(model):
    if getattr(model.fe_data.mesh, "dim", 3) != 3:
        raise NotImplementedError("SectionTransports is implemented for tetrahedral (3-D) meshes: a plane cuts the cells of an embedded "
                                  "2-D mesh in segments, not in polygons")
    if getattr(model, "layout", None) is not None and (hasattr(model.layout, "cell_owner") or hasattr(model.layout, "locator_cells")):
        raise NotImplementedError("SectionTransports on a mesh-partitioned model is not implemented: every rank would integrate the pieces "
                                  "of the cells it owns (the cell_mask argument of npg_sections_create) and the bin sums would be added "
                                  "over the ranks - integrate the sections of a single-device model")
    if getattr(model, "partition", None) is not None or getattr(model, "comm", None) is not None \
            or getattr(model.arch.ctx, "nranks", 1) > 1:
        raise NotImplementedError("SectionTransports of the replicated distributed layout is not implemented: use a single-device model")


def _edges(e):
    return np.array([-np.inf, np.inf]) if e is None else np.asarray(e, dtype=np.float64).reshape(-1)


class Section:
    """Section(name, origin, normal, e1, e2, edges1=None, edges2=None): a plane through `origin` with unit `normal` - transports are
    positive along it - and in-plane unit axes e1, e2 (mutually orthogonal to 1e-12, any handedness).  edges1 / edges2: strictly
    increasing bin edges of (x - origin) . e1 and (x - origin) . e2, half-open bins [edge_i, edge_i+1); the first / last may be -inf /
    +inf; None: one unbounded bin.  Nothing outside the edges counts."""

    def __init__(self, name, origin, normal, e1, e2, edges1=None, edges2=None):
        self.name = str(name)
        self.origin, self.normal, self.e1, self.e2 = (np.asarray(v, dtype=np.float64).reshape(3) for v in (origin, normal, e1, e2))
        self.edges1, self.edges2 = _edges(edges1), _edges(edges2)
        if len(self.edges1) < 2 or len(self.edges2) < 2:
            raise ValueError(f"Section {self.name}: an edge array needs at least two entries")

    @property
    def shape(self):
        return len(self.edges1) - 1, len(self.edges2) - 1

    @property
    def frame(self):
        return np.concatenate([self.origin, self.normal, self.e1, self.e2])

    @classmethod
    def latitude(cls, y0, x_edges=None, z_edges=None, name=None):
        """the plane y = y0: n = +y, e1 = x, e2 = z (northward transport, binned in x and z)"""
        return cls(name or f"y={y0:g}", [0.0, y0, 0.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0], x_edges, z_edges)

    @classmethod
    def longitude(cls, x0, y_edges=None, z_edges=None, name=None):
        """the plane x = x0: n = +x, e1 = y, e2 = z (eastward transport, binned in y and z)"""
        return cls(name or f"x={x0:g}", [x0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], y_edges, z_edges)

    @classmethod
    def level(cls, z0, x_edges=None, y_edges=None, name=None):
        """the plane z = z0: n = +z, e1 = x, e2 = y (upwelling, binned in x and y)"""
        return cls(name or f"z={z0:g}", [0.0, 0.0, z0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], x_edges, y_edges)

    @classmethod
    def line(cls, p0, p1, s_edges=None, z_edges=None, name=None):
        """the vertical strip from p0 to p1 (their x and y): origin (p0, z = 0), e1 along it, e2 = z, n = z x e1 - to the left of the
        direction of travel.  s_edges (distance from p0) defaults to [0, |p1 - p0|]"""
        p0, p1 = np.asarray(p0, dtype=np.float64).reshape(-1)[:2], np.asarray(p1, dtype=np.float64).reshape(-1)[:2]
        length = float(np.hypot(*(p1 - p0)))
        if not length > 0.0:
            raise ValueError("Section.line: p0 and p1 coincide")
        t = (p1 - p0) / length
        e1 = np.array([t[0], t[1], 0.0])
        n = np.array([-t[1], t[0], 0.0])                                               # z x e1
        return cls(name or "line", [p0[0], p0[1], 0.0], n, e1, [0.0, 0.0, 1.0], [0.0, length] if s_edges is None else s_edges, z_edges)


class SectionFluxes:
    """What SectionTransports.compute() returns.  `names`: the sections; `raw[name]` (n1, n2, NPG_NSEC): the channels of every bin; and,
    with the model's parameters applied, dicts over the sections of (n1, n2) arrays:
      area                ch0                     volume_transport    ch1
      buoyancy_transport  ch3 + N2 ch4            diffusive_flux      -(ch10 + N2 ch11)   (down the gradient, along n)
      mean_b, mean_p, mean_u (n1, n2, 3), mean_dz_b, mean_z   ch2, ch5, ch6..8, ch13, ch12 over ch0 (NaN for a bin without area)
    `.total(quantity)` adds a quantity over a section's bins; `.streamfunction(name)` accumulates the volume transport along one axis.
    `maps` (compute(pieces=True)): SectionMaps."""

    def __init__(self, sections, raw, params, maps=None):
        self.sections = tuple(sections)
        self.names = tuple(s.name for s in self.sections)
        self.maps = maps
        N2 = float(params.N2)
        self.raw, k = {}, 0
        raw = np.asarray(raw, dtype=np.float64).reshape(-1, NSEC)
        for s in self.sections:
            n1, n2 = s.shape
            self.raw[s.name] = raw[k:k + n1 * n2].reshape(n1, n2, NSEC)
            k += n1 * n2
        per = lambda fn: {nm: fn(r) for nm, r in self.raw.items()}

        def mean(ch):
            with np.errstate(invalid="ignore", divide="ignore"):
                v = per(lambda r: np.where(r[..., 0:1] > 0.0, r[..., ch] / r[..., 0:1], np.nan))
            return v if len(ch) > 1 else {nm: a[..., 0] for nm, a in v.items()}
        self.area = per(lambda r: r[..., 0].copy())
        self.volume_transport = per(lambda r: r[..., 1].copy())
        self.buoyancy_transport = per(lambda r: r[..., 3] + N2 * r[..., 4])
        self.diffusive_flux = per(lambda r: -(r[..., 10] + N2 * r[..., 11]))
        self.mean_b, self.mean_p, self.mean_u = mean([2]), mean([5]), mean([6, 7, 8])
        self.mean_dz_b, self.mean_z = mean([13]), mean([12])

    def total(self, quantity):
        """{section: the sum over its bins} of a per-bin quantity (not meaningful for the means)"""
        if quantity.startswith("mean_"):
            raise ValueError(f"SectionFluxes.total: {quantity} is an area mean - add the raw channels and divide by the total area")
        return {nm: float(v.sum()) for nm, v in getattr(self, quantity).items()}

    def streamfunction(self, name, axis=1, from_end=False):
        """the cumulative volume transport of section `name` over the bins of `axis` (0: e1, 1: e2) at the bin EDGES, with a leading zero:
        shape (n1 + 1, n2) or (n1, n2 + 1); from_end: accumulated from the last edge backwards (zero at the end)"""
        v = self.volume_transport[name]
        if axis not in (0, 1):
            raise ValueError(f"SectionFluxes.streamfunction: axis must be 0 or 1, got {axis}")
        if from_end:
            c = np.flip(np.cumsum(np.flip(v, axis), axis=axis), axis)
            return np.concatenate([c, np.zeros_like(np.take(v, [0], axis=axis))], axis=axis)
        return np.concatenate([np.zeros_like(np.take(v, [0], axis=axis)), np.cumsum(v, axis=axis)], axis=axis)

    def __repr__(self):
        keys = ("area", "volume_transport", "buoyancy_transport", "diffusive_flux")
        return "SectionFluxes(" + "; ".join(f"{nm}: " + ", ".join(f"{k}={self.total(k)[nm]:.6e}" for k in keys) for nm in self.names) + ")"


class SectionMaps:
    """Per-piece means (integral / area) of every channel: `values` (NPG_NSEC, npiece) in the order of SectionTransports.pieces(), `raw`
    the integrals themselves, `centroids` (npiece, 3), `s1`, `s2` the centroids' in-plane coordinates, `area`, `section` (npiece,) the
    index into `names`, `corners` (npiece, 3, 3).  `.of(name)` selects a section's pieces - ready for a tripcolor over (s1, s2)."""

    def __init__(self, names, plan, raw):
        self.names = tuple(names)
        self.raw = raw
        self.centroids, self.s1, self.s2, self.area = plan["centroids"], plan["s1"], plan["s2"], plan["area"]
        self.section, self.corners = plan["section"], plan["corners"]
        with np.errstate(invalid="ignore", divide="ignore"):
            self.values = np.where(raw[0] > 0.0, raw / raw[0], np.nan)

    def of(self, name):
        return self.section == self.names.index(name)


class SectionTransports:
    """SectionTransports(model, sections, mask=None): the integrals of the model's CURRENT state over sections (a Section or a list of
    at most 64, with distinct names).  mask (ncell,) bool: only these cells count.  The plan - which cells each plane cuts, the polygons
    clipped at the bin edges, the pieces sorted by bin - is made once on the host (`.info`: pieces, bins, cut_cells, max_per_bin,
    setup_seconds; `.pieces()`: the plan itself).  kappa_h and kappa_v are model.forcings' values at the six points of every piece; with
    the convection closure on, kappa_v is the background value plus the closure at the point's own d_z b'.
    `.compute(pieces=False)` runs two launches on the device and downloads 14 doubles per bin (and 14 per piece with pieces=True); two
    calls on the same state return the same bits.  Mesh-partitioned models, the replicated distributed layout and embedded 2-D meshes
    raise NotImplementedError."""

    def __init__(self, model, sections, mask=None):
        _refuse(model)
        self.model = model
        self.sections = (sections,) if isinstance(sections, Section) else tuple(sections)
        names = [s.name for s in self.sections]
        if len(set(names)) != len(names):
            raise ValueError(f"SectionTransports: duplicate section names in {names}")
        if not 1 <= len(names) <= 64:
            raise ValueError(f"SectionTransports: 1 .. 64 sections, got {len(names)}")
        self.names = tuple(names)
        fed = model.fe_data
        m = fed.mesh
        self.ctx = model.arch.ctx
        gmask = None if mask is None else np.asarray(mask)
        if gmask is not None and (gmask.dtype != bool or gmask.shape != (m.ncell,)):
            raise ValueError(f"SectionTransports: mask must be a bool array of shape ({m.ncell},), got {gmask.dtype} {gmask.shape}")
        self.fe = device_fe(model.arch, fed)
        self._X = L.as_f64(m.geo_coords[m.cell_geo])                                   # (ncell, 4, 3): the cells' own vertices
        self._keep = dict(frames=L.as_f64(np.stack([s.frame for s in self.sections])), n1=L.as_i32([s.shape[0] for s in self.sections]),
                          n2=L.as_i32([s.shape[1] for s in self.sections]), e1=L.as_f64(np.concatenate([s.edges1 for s in self.sections])),
                          e2=L.as_f64(np.concatenate([s.edges2 for s in self.sections])),
                          mask=None if gmask is None else np.ascontiguousarray(gmask, dtype=np.uint8))
        k = self._keep
        self.h = None
        h = C.c_void_p()
        t0 = time.perf_counter()
        L.check(L.lib().npg_sections_create(self.fe.h, L.ptr(self._X), len(self.sections), L.ptr(k["frames"]), L.ptr(k["n1"]), L.ptr(k["n2"]),
                                            L.ptr(k["e1"]), L.ptr(k["e2"]), None if k["mask"] is None else L.ptr(k["mask"]), C.byref(h)))
        setup = time.perf_counter() - t0
        self.h = h
        q = [C.c_int64() for _ in range(4)]
        L.check(L.lib().npg_sections_info(self.h, *[C.byref(v) for v in q]))
        self.npiece, self.nbin = int(q[0].value), int(q[1].value)
        self.info = dict(pieces=self.npiece, bins=self.nbin, cut_cells=int(q[2].value), max_per_bin=int(q[3].value), setup_seconds=setup)
        self._plan = None
        f = model.forcings
        self.set_coeff(L.NPG_SEC_KH, f.kappa_h)
        self.set_coeff(L.NPG_SEC_KV, f.kappa_v)
        cp = f.conv_param
        if cp.is_on:
            L.check(L.lib().npg_sections_set_closure(self.h, float(cp.kappa_c), float(cp.N2min), float(model.params.alpha), float(model.params.N2)))
        self._out = DeviceVector(self.ctx, self.nbin * NSEC)
        self._pieces_out = None

    def __del__(self):
        try:
            if self.h:
                L.lib().npg_sections_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def pieces(self):
        """the plan: dict of cell (npiece,), bin (npiece,) global bin index, section (npiece,), lam (npiece, 3, 4) the corners' barycentrics
        in their cell, area (npiece,), corners (npiece, 3, 3) and centroids (npiece, 3) in space, s1, s2 the centroids' in-plane
        coordinates, points (npiece, 6, 3) the quadrature points, bin_ptr (nbin + 1,).  Sorted by (bin, cell, index within the cell)."""
        if self._plan is None:
            n = self.npiece
            cell, bins = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
            lam, area = np.zeros((n, 3, 4)), np.zeros(n)
            L.check(L.lib().npg_sections_pieces(self.h, L.ptr(cell), L.ptr(bins), L.ptr(lam), L.ptr(area)))
            bin0 = np.concatenate([[0], np.cumsum([s.shape[0] * s.shape[1] for s in self.sections])])
            section = np.searchsorted(bin0, bins, side="right") - 1
            corners = np.einsum("pjm,pmi->pji", lam, self._X[cell])
            cen = corners.mean(axis=1)
            fr = self._keep["frames"][section].reshape(n, 4, 3)
            s1, s2 = np.einsum("pi,pi->p", cen - fr[:, 0], fr[:, 2]), np.einsum("pi,pi->p", cen - fr[:, 0], fr[:, 3])
            self._plan = dict(cell=cell, bin=bins, section=section, lam=lam, area=area, corners=corners, centroids=cen, s1=s1, s2=s2,
                              points=np.einsum("qj,pji->pqi", RULE_MU, corners),
                              bin_ptr=np.searchsorted(bins, np.arange(self.nbin + 1), side="left"))
        return self._plan

    def set_coeff(self, which, v):
        """replace coefficient `which` (L.NPG_SEC_KH, L.NPG_SEC_KV) by v: a number, a function of x, a table (npiece, 6), or None
        (remove it).  A refused table (wrong shape: ValueError; non-finite: DeviceError) leaves the handle as it was."""
        if v is None:
            L.check(L.lib().npg_sections_set_coeff(self.h, int(which), None))
            return
        if isinstance(v, np.ndarray):
            tab = np.asarray(v, dtype=np.float64)
        elif callable(v):
            pts = self.pieces()["points"]
            tab = np.broadcast_to(np.asarray(v(pts), dtype=np.float64), pts.shape[:2]).copy()
        else:
            tab = np.full((self.npiece, 6), float(v))
        if tab.shape != (self.npiece, 6):
            raise ValueError(f"SectionTransports.set_coeff: a table must have shape ({self.npiece}, 6), got {tab.shape}")
        tab = L.as_f64(tab.T)                                                          # [6][npiece]
        L.check(L.lib().npg_sections_set_coeff(self.h, int(which), L.ptr(tab)))

    def compute_raw(self, pieces=False):
        """(raw (nbin, NPG_NSEC), per-piece raw (NPG_NSEC, npiece) or None) of the current state"""
        m = self.model
        if pieces and self._pieces_out is None:
            self._pieces_out = DeviceVector(self.ctx, max(1, NSEC * self.npiece))
        L.check(L.lib().npg_sections_compute(self.h, m.inversion.solver.x.h, m.b_vec.h, self._out.h, self._pieces_out.h if pieces else None))
        raw = self._out.to_host().reshape(self.nbin, NSEC)
        per_piece = self._pieces_out.to_host()[:NSEC * self.npiece].reshape(NSEC, self.npiece) if pieces else None
        return raw, per_piece

    def compute(self, pieces=False) -> SectionFluxes:
        raw, per_piece = self.compute_raw(pieces)
        maps = SectionMaps(self.names, self.pieces(), per_piece) if pieces else None
        return SectionFluxes(self.sections, raw, self.model.params, maps)


class SectionRecorder:
    """SectionRecorder(st, every=1): an `on_plot(model, t)` hook (model.run calls it every n_plot steps) that appends (t, raw channels of
    every bin) on every `every`-th call.  `.as_arrays()` -> (t (n,), raw (n, nbin, NPG_NSEC)); `.fluxes()` the rows as SectionFluxes;
    `.save(path)` writes them with np.savez (keys t, raw, names, channels).  It reads the state and writes nothing: a run with the hook
    computes the same bits as one without."""

    def __init__(self, st, every=1):
        if int(every) < 1:
            raise ValueError(f"SectionRecorder: every must be >= 1, got {every}")
        self.st, self.every, self.calls = st, int(every), 0
        self.t, self.raw = [], []

    def __call__(self, model, t):
        self.calls += 1
        if (self.calls - 1) % self.every == 0:
            self.t.append(float(t))
            self.raw.append(self.st.compute_raw()[0])

    def as_arrays(self):
        return np.array(self.t, dtype=np.float64), np.array(self.raw, dtype=np.float64).reshape(len(self.raw), self.st.nbin, NSEC)

    def fluxes(self):
        return [SectionFluxes(self.st.sections, r, self.st.model.params) for r in self.raw]

    def save(self, path):
        t, raw = self.as_arrays()
        np.savez(path, t=t, raw=raw, names=np.array(self.st.names), channels=np.array(CHANNELS))
