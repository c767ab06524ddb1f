"""Boundary fluxes and maps: the quadrature integrals of the device-resident state over the mesh's boundary faces
(npg_boundary_compute) - where the model is forced and where it dissipates.  Per GROUP of faces (by default one per
physical surface of the mesh: surface, bottom, coastline): area, volume and advective buoyancy flux, pressure force (form drag) and
work, viscous traction (bottom drag) and work, the diffusive buoyancy flux, the wind work, the prescribed surface flux, and the area
means of p, b', d_z b' and the tangential flow; per face, on request, the same as maps.  The reference has no counterpart.

One pass over the boundary faces with the face rule of Mesh.surface_load lifted into each face's cell, NPG_NBND = 24 raw channels per
group (csrc/boundary_core.h lists them).  The fields are the finite-element fields themselves, so the integrals are exact where the
integrand is a polynomial of degree <= 4, and the prescribed-load channels are the very sums of the project's load vectors:

    alpha ch19 (surface)  = x_u' (the wind part of build_b_inversion)          ch20 = 1' surface_load(F)
    sum_groups ch5 = int div u,   sum_groups ch7 = int (u . grad b' + b' div u)      (divergence theorem on the discrete fields)

and the energy identity DESIGN.md 15 left open closes: for a converged inversion WITH wind,
dissipation = buoyancy production + wind work up to x' r with r the true residual."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .architectures import DeviceVector
from .fe import tri_quadrature_degree4
from .inputs import SurfaceFluxBC
from .inversion import device_fe

NBND = L.NPG_NBND
CHANNELS = ("one", "n_x", "n_y", "n_z", "z_n_z", "u_n", "b", "b_u_n", "p", "p_n_x", "p_n_y", "p_n_z", "p_u_n", "t_x", "t_y", "t_z", "u_t",
            "kappa_grad_b_n", "kv_n_z", "tau_u", "flux", "dz_b", "u_x", "u_y")
_OPP = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])          # the vertices of local face k, ascending


def _refuse(model):
    if getattr(model.fe_data.mesh, "dim", 3) != 3:
        raise NotImplementedError("BoundaryIntegrals is implemented for tetrahedral (3-D) meshes: the boundary of an embedded 2-D mesh is "
                                  "made of segments, not of faces")
    if getattr(model, "layout", None) is not None and (hasattr(model.layout, "cell_owner") or hasattr(model.layout, "locator_cells")):
        raise NotImplementedError("BoundaryIntegrals on a mesh-partitioned model is not implemented: every rank would integrate the faces "
                                  "of the cells it owns (the face_mask argument of npg_boundary_create) and the group sums would be added "
                                  "over the ranks - integrate the boundary of a single-device model")
    if getattr(model, "partition", None) is not None or getattr(model, "comm", None) is not None \
            or getattr(model.arch.ctx, "nranks", 1) > 1:
        raise NotImplementedError("BoundaryIntegrals of the replicated distributed layout is not implemented: use a single-device model")


def face_cells(mesh, faces):
    """(cell, local face) of boundary faces given as sorted topological vertex triples (nf, 3): the cell one of whose sides lambda_k = 0
    has exactly these vertices.  Vectorised: the (first, second) vertex pairs of all triples are numbered, which keeps every key below
    2^63 on any mesh.  A face that belongs to no cell, or to two, is a ValueError."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    nc, nv = mesh.ncell, int(mesh.nv)
    ct = mesh.cells[:, _OPP].reshape(-1, 3)                              # row 4 c + k; ascending because the cells are sorted
    pair = np.concatenate([ct[:, 0] * nv + ct[:, 1], faces[:, 0] * nv + faces[:, 1]])
    _, inv = np.unique(pair, return_inverse=True)
    key = inv.reshape(-1) * nv + np.concatenate([ct[:, 2], faces[:, 2]])
    ckey, fkey = key[:4 * nc], key[4 * nc:]
    order = np.argsort(ckey, kind="stable")
    cs = ckey[order]
    lo, hi = np.searchsorted(cs, fkey, side="left"), np.searchsorted(cs, fkey, side="right")
    if ((hi - lo) != 1).any():
        bad = int(np.nonzero((hi - lo) != 1)[0][0])
        raise ValueError(f"BoundaryIntegrals: boundary face {bad} (vertices {faces[bad].tolist()}) is a side of {int(hi[bad] - lo[bad])} "
                         f"cells - a boundary face belongs to exactly one")
    hit = order[lo]
    return hit // 4, hit % 4


def _at_points(v, xq):
    """a number or a function of x at the face points xq (nf, 9, 3) -> (nf, 9)"""
    if callable(v):
        return np.broadcast_to(np.asarray(v(xq), dtype=np.float64), xq.shape[:2]).copy()
    return np.full(xq.shape[:2], float(v))


def _is_zero(v):
    return not callable(v) and float(v) == 0.0


class BoundaryFluxes:
    """What BoundaryIntegrals.compute() returns.  `groups`: the group names; `raw[group]`: the NPG_NBND channels (numpy); and, with the
    model's parameters applied, dicts over the groups:
      area                      ch0                          volume_flux        ch5
      buoyancy_flux_advective   ch7                          pressure_force     ch9..11 (3,)            pressure_work   ch12
      viscous_force             alpha^2 eps^2 ch13..15 (3,)  viscous_work       alpha^2 eps^2 ch16      (the prefactor of Budgets.dissipation)
      wind_work                 alpha ch19                   diffusive_flux     ch17 + N2 ch18          prescribed_flux ch20
      mean_p, mean_b, mean_dz_b, mean_ux, mean_uy            ch8, ch6, ch21, ch22, ch23 over ch0 (NaN for a group without area)
    `.total(name)` adds a quantity over the groups.  `viscous_available` is False under the eddy closure - nu is then a function of the
    state, not of position alone, and channels 13..16 come back NaN.  `maps` (compute(faces=True)): BoundaryMaps."""

    def __init__(self, groups, raw, params, viscous_available=True, maps=None):
        self.groups = tuple(groups)
        raw = np.asarray(raw, dtype=np.float64).reshape(len(self.groups), NBND)
        self.raw = {g: raw[i] for i, g in enumerate(self.groups)}
        self.viscous_available = bool(viscous_available)
        self.maps = maps
        a, e, N2 = float(params.alpha), float(params.eps), float(params.N2)
        per = lambda fn: {g: fn(r) for g, r in self.raw.items()}
        mean = lambda k: per(lambda r: r[k] / r[0] if r[0] else np.nan)
        self.area = per(lambda r: r[0])
        self.volume_flux = per(lambda r: r[5])
        self.buoyancy_flux_advective = per(lambda r: r[7])
        self.pressure_force = per(lambda r: r[9:12].copy())
        self.pressure_work = per(lambda r: r[12])
        self.viscous_force = per(lambda r: a * a * e * e * r[13:16])
        self.viscous_work = per(lambda r: a * a * e * e * r[16])
        self.wind_work = per(lambda r: a * r[19])
        self.diffusive_flux = per(lambda r: r[17] + N2 * r[18])
        self.prescribed_flux = per(lambda r: r[20])
        self.mean_p, self.mean_b, self.mean_dz_b, self.mean_ux, self.mean_uy = mean(8), mean(6), mean(21), mean(22), mean(23)

    def total(self, name):
        """the sum over the groups of a per-group quantity (not meaningful for the means)"""
        if name.startswith("mean_"):
            raise ValueError(f"BoundaryFluxes.total: {name} is an area mean - add the raw channels and divide by the total area")
        return sum(getattr(self, name)[g] for g in self.groups)

    def __repr__(self):
        keys = ("area", "volume_flux", "buoyancy_flux_advective", "wind_work", "diffusive_flux", "prescribed_flux")
        return "BoundaryFluxes(" + "; ".join(f"{g}: " + ", ".join(f"{k}={getattr(self, k)[g]:.6e}" for k in keys) for g in self.groups) + ")"


class BoundaryMaps:
    """Per-face means (integral / area) of every channel: `values` (NPG_NBND, nface) in the order of BoundaryIntegrals.faces (NaN for a
    face that does not count), `raw` the integrals themselves, `centroids` (nface, 3), `normals` (nface, 3), `group` (nface,) the index
    into `groups`.  The conveniences return (centroids, values) of one group, ready for a tripcolor over the face centroids."""

    def __init__(self, groups, group, centroids, normals, raw, params):
        self.groups, self.group, self.centroids, self.normals, self.raw = tuple(groups), group, centroids, normals, raw
        with np.errstate(invalid="ignore", divide="ignore"):
            self.values = np.where(raw[0] > 0.0, raw / raw[0], np.nan)
        self._a2e2 = float(params.alpha) ** 2 * float(params.eps) ** 2

    def of(self, name):
        """the faces of group `name`"""
        return self.group == self.groups.index(name)

    def surface_pressure(self, group="surface"):
        """the pressure under the rigid lid: the sea-surface height of a PG model"""
        s = self.of(group)
        return self.centroids[s], self.values[8, s]

    def surface_velocity(self, group="surface"):
        s = self.of(group)
        return self.centroids[s], self.values[22:24, s].T

    def bottom_stress(self, group="bottom"):
        """alpha^2 eps^2 times the viscous traction the fluid feels at the bottom (NaN under the eddy closure)"""
        s = self.of(group)
        return self.centroids[s], self._a2e2 * self.values[13:16, s].T

    def bottom_pressure(self, group="bottom"):
        s = self.of(group)
        return self.centroids[s], self.values[8, s]


class BoundaryIntegrals:
    """BoundaryIntegrals(model, groups=None, mask=None): the integrals of the model's CURRENT state over its boundary faces.

    groups: {name: [physical tags]}; default one group per physical surface tag of the mesh that carries faces (bowl: bottom, surface;
    channel basin: bottom, coastline, surface), at most 8.  A face carrying tags of two groups is refused (ValueError); a face carrying
    none is left out.  `.faces` (nface, 3) are the faces that take part, as sorted topological vertex ids, sorted by (group, cell);
    `.face_cell`, `.face_local`, `.face_group`, `.centroids`, `.normals` (outward), `.area` follow that order, and so does `mask`
    (nface,) bool: only these faces count.
    Coefficients: model.forcings.nu / kappa_h / kappa_v (numbers or functions of x) are evaluated at the face points; tau_x / tau_y and
    the flux of a SurfaceFluxBC on the faces carrying the mesh's surface_tags only, zero elsewhere - as build_b_inversion and
    build_rhs_flux apply them.  With the convection closure on, kappa_v is the background value plus the closure at the point's own
    d_z b'.  With the EDDY closure on nu is a function of the state, not of position alone: channels 13..16 (viscous traction and work)
    are returned as NaN and BoundaryFluxes.viscous_available is False.
    `.compute(faces=False)` runs one pass on the device and downloads 24 doubles per group (and 24 per face with faces=True); two calls
    on the same state return the same bits.  Mesh-partitioned models, the replicated distributed layout and embedded 2-D meshes raise
    NotImplementedError."""

    def __init__(self, model, groups=None, mask=None):
        _refuse(model)
        self.model = model
        fed = model.fe_data
        m = fed.mesh
        self.ctx = model.arch.ctx
        phys = np.asarray(m._facets_phys, dtype=np.uint32)
        carries = lambda tags: np.bitwise_or.reduce([(phys >> np.uint32(m.tag_bit(t))) & 1 for t in tags]).astype(bool) if len(tags) \
            else np.zeros(len(phys), dtype=bool)
        if groups is None:
            groups = {nm: [nm] for nm in m.phys_names if carries([nm]).any()}
        groups = {str(k): list(v) for k, v in groups.items()}
        if not 1 <= len(groups) <= 8:
            raise ValueError(f"BoundaryIntegrals: 1 .. 8 groups, got {len(groups)}")
        self.groups = tuple(groups)
        member = np.stack([carries(tags) for tags in groups.values()])                 # (ngroup, all boundary faces)
        if (member.sum(axis=0) > 1).any():
            bad = int(np.nonzero(member.sum(axis=0) > 1)[0][0])
            raise ValueError(f"BoundaryIntegrals: boundary face {bad} carries tags of the groups "
                             f"{[g for g, mk in zip(self.groups, member[:, bad]) if mk]} - a face belongs to one group")
        sel = np.nonzero(member.any(axis=0))[0]
        group = member[:, sel].argmax(axis=0)
        faces, fgeo = m._facets[sel], m._facets_geo[sel]
        cell, local = face_cells(m, faces)
        order = np.lexsort((cell, group))                                              # by (group, cell)
        sel, group, faces, fgeo, cell, local = sel[order], group[order], faces[order], fgeo[order], cell[order], local[order]
        self.faces, self.face_cell, self.face_local, self.face_group = faces, cell, local, group
        nf = len(faces)
        X = m.geo_coords[fgeo]                                                         # (nf, 3, 3): the faces' own nodes
        cr = np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0])
        area2 = np.linalg.norm(cr, axis=1)
        n = cr / area2[:, None]
        Xc = m.geo_coords[m.cell_geo[cell]]                                            # the cells' own geometry: outward = away from the
        r = np.arange(nf)                                                              # cell's opposite vertex
        away = Xc[r[:, None], _OPP[local]].mean(axis=1) - Xc[r, local]
        n = np.where((np.einsum("fi,fi->f", n, away) < 0.0)[:, None], -n, n)
        self.centroids, self.normals, self.area = X.mean(axis=1), n, 0.5 * area2
        gmask = None if mask is None else np.asarray(mask, dtype=bool)
        if gmask is not None and gmask.shape != (nf,):
            raise ValueError(f"BoundaryIntegrals: mask must have shape ({nf},), got {gmask.shape}")
        self.nfaces_counted = int(nf if gmask is None else gmask.sum())
        self.fe = device_fe(model.arch, fed)
        self._keep = dict(cell=L.as_i32(cell), local=np.ascontiguousarray(local, dtype=np.uint8), group=np.ascontiguousarray(group, dtype=np.uint8),
                          xyz=L.as_f64(X.reshape(nf, 9).T), normal=L.as_f64(n.T), area2=L.as_f64(area2),
                          mask=None if gmask is None else np.ascontiguousarray(gmask, dtype=np.uint8))
        k = self._keep
        self.h = None
        h = C.c_void_p()
        L.check(L.lib().npg_boundary_create(self.fe.h, nf, L.ptr(k["cell"]), L.ptr(k["local"]), L.ptr(k["group"]), len(self.groups), L.ptr(k["xyz"]),
                                            L.ptr(k["normal"]), L.ptr(k["area2"]), None if k["mask"] is None else L.ptr(k["mask"]), C.byref(h)))
        self.h = h
        # the coefficients at the face points
        f = model.forcings
        lam, _ = tri_quadrature_degree4()
        self.points = np.einsum("qk,fki->fqi", lam, X)                                 # (nf, 9, 3), the points of surface_load
        on_surface = carries(m.surface_tags)[sel]
        self.viscous_available = not f.eddy_param.is_on
        self.full_stress = bool(callable(f.nu) or f.eddy_param.is_on)
        if self.viscous_available:
            self.set_coeff(L.NPG_BND_NU, f.nu)
        self.set_coeff(L.NPG_BND_KH, f.kappa_h)
        self.set_coeff(L.NPG_BND_KV, f.kappa_v)
        for which, v in ((L.NPG_BND_TAUX, f.tau_x), (L.NPG_BND_TAUY, f.tau_y)):
            if not _is_zero(v):
                self.set_coeff(which, v, on_surface)
        if isinstance(f.b_surface_bc, SurfaceFluxBC):
            self.set_coeff(L.NPG_BND_FLUX, f.b_surface_bc.flux, on_surface)
        cp = f.conv_param
        if cp.is_on:
            L.check(L.lib().npg_boundary_set_closure(self.h, float(cp.kappa_c), float(cp.N2min), float(model.params.alpha), float(model.params.N2)))
        self._out = DeviceVector(self.ctx, len(self.groups) * NBND)
        self._faces_out = None

    def __del__(self):
        try:
            if self.h:
                L.lib().npg_boundary_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def set_coeff(self, which, v, where=None):
        """replace coefficient `which` (L.NPG_BND_NU .. L.NPG_BND_FLUX) by v - a number, a function of x, a table (nface, 9) or None (remove
        it) - on the faces `where` (nface,) bool, zero elsewhere"""
        if v is None:
            L.check(L.lib().npg_boundary_set_coeff(self.h, int(which), None))
            return
        tab = np.asarray(v, dtype=np.float64) if isinstance(v, np.ndarray) else _at_points(v, self.points)
        if tab.shape != self.points.shape[:2]:
            raise ValueError(f"BoundaryIntegrals.set_coeff: a table must have shape {self.points.shape[:2]}, got {tab.shape}")
        if where is not None:
            tab = np.where(np.asarray(where, dtype=bool)[:, None], tab, 0.0)
        tab = L.as_f64(tab.T)                                                          # [9][nface]
        L.check(L.lib().npg_boundary_set_coeff(self.h, int(which), L.ptr(tab)))

    def compute_raw(self, faces=False):
        """(raw (ngroup, NPG_NBND), per-face raw (NPG_NBND, nface) or None) of the current state; under the eddy closure channels 13..16
        are NaN"""
        m = self.model
        nf = len(self.faces)
        if faces and self._faces_out is None:
            self._faces_out = DeviceVector(self.ctx, max(1, NBND * nf))
        L.check(L.lib().npg_boundary_compute(self.h, m.inversion.solver.x.h, m.b_vec.h, int(self.full_stress), self._out.h,
                                             self._faces_out.h if faces else None))
        raw = self._out.to_host().reshape(len(self.groups), NBND)
        per_face = self._faces_out.to_host()[:NBND * nf].reshape(NBND, nf) if faces else None
        if not self.viscous_available:
            raw[:, 13:17] = np.nan
            if per_face is not None:
                per_face[13:17] = np.nan
        return raw, per_face

    def compute(self, faces=False) -> BoundaryFluxes:
        raw, per_face = self.compute_raw(faces)
        prm = self.model.params
        maps = BoundaryMaps(self.groups, self.face_group, self.centroids, self.normals, per_face, prm) if faces else None
        return BoundaryFluxes(self.groups, raw, prm, self.viscous_available, maps)


class BoundaryRecorder:
    """BoundaryRecorder(model, groups=None, mask=None): an `on_plot(model, t)` hook (model.run calls it every n_plot steps) that appends
    (t, raw channels of every group) per call.  `.as_arrays()` -> (t (n,), raw (n, ngroup, NPG_NBND)); `.fluxes()` the rows as
    BoundaryFluxes; `.save(path)` writes them with np.savez (keys t, raw, groups, channels).  It reads the state and writes nothing:
    a run with the hook computes the same bits as one without."""

    def __init__(self, model, groups=None, mask=None):
        self.boundary = BoundaryIntegrals(model, groups, mask)
        self.t, self.raw = [], []

    def __call__(self, model, t):
        self.t.append(float(t))
        self.raw.append(self.boundary.compute_raw()[0])

    def as_arrays(self):
        B = self.boundary
        return np.array(self.t, dtype=np.float64), np.array(self.raw, dtype=np.float64).reshape(len(self.raw), len(B.groups), NBND)

    def fluxes(self):
        B = self.boundary
        return [BoundaryFluxes(B.groups, r, B.model.params, B.viscous_available) for r in self.raw]

    def save(self, path):
        t, raw = self.as_arrays()
        np.savez(path, t=t, raw=raw, groups=np.array(self.boundary.groups), channels=np.array(CHANNELS))
