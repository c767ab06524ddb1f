"""The flow mapped on buoyancy surfaces (npg_surfaces_*): where the surface B = B_k of the full buoyancy B = N2 z + b' lies
over a set of fixed columns (x_j, y_j), how thick the layer between two surfaces is, and the velocity, the slope and f d_z B on the
surface - the map a user of the channel-basin runs draws next to psi*(y, B).  The reference overlays contour lines of b on slices
(postprocess/slice.py, streamfunctions.py); from a sampled grid the same maps cost a full 3-D grid and lose the exact crossing of the P2
buoyancy.

Set-up tiles every column into the cells the vertical line passes through (host code, once); every call is then one scan of the
columns on the model's architecture - along a segment B is a quadratic in z, so a crossing is the root of a quadratic, not an
interpolation between samples - and one evaluation of u and grad B at the uppermost crossings.  The tiling also gives the exact depth
of the mesh under a point: `column_depth`."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .architectures import DeviceVector
from .sampling import _engine, _partitioned, locator

NSURF = L.NPG_NSURF
CROSSED, OUTCROPPED, GROUNDED, DRY = 0, 1, 2, 3


class SurfaceMaps:
    """What one call of BuoyancySurfaces.compute() found.  `shape` = the columns' shape: (nx, ny) for a grid, (n,) for points.

      .levels (nlev,)              the B_k
      .z, .z_low (nlev, *shape)    z of the uppermost and of the lowermost crossing of B = B_k in the column, NaN without one
      .ncross (nlev, *shape) int   the number of crossings
      .u, .grad_B (nlev, *shape, 3)   the velocity and grad B (N2 added to the z component) at the uppermost crossing
      .status (nlev, *shape)       0 crossed; 1 outcropped: no crossing and B_k > B at the top of the column; 2 grounded: no crossing
                                   otherwise; 3 dry: the column misses the mesh
      .z_top, .z_bot, .B_top, .B_bot (*shape)   the column's ends and B there, NaN where dry; .column_depth = z_top - z_bot, 0 where dry
      .thickness() (nlev - 1, *shape)   z of level k + 1 less z of level k, an outcropped level taken at z_top and a grounded one at z_bot
      .slope() (nlev, *shape, 2)   - grad_h B / d_z B
      .pv(f=None) (nlev, *shape)   f d_z B; f: a number, an array that broadcasts against (nlev, *shape), a function of the coordinates
                                   (..., 3), default the model's Coriolis parameter"""

    def __init__(self, levels, out, cols, shape, xy, f=None):
        nlev = len(levels)
        o = out.reshape((NSURF, nlev) + tuple(shape))
        self.levels, self.shape, self._xy, self._f = levels, tuple(shape), xy, f
        self.z, self.z_low, self.ncross = o[0], o[1], o[2].astype(np.int32)
        self.u = np.moveaxis(o[3:6], 0, -1)
        self.grad_B = np.moveaxis(o[6:9], 0, -1)
        c = cols.reshape((4,) + tuple(shape))
        self.z_top, self.z_bot, self.B_top, self.B_bot = c[0], c[1], c[2], c[3]

    @property
    def status(self):
        lev = self.levels.reshape((-1,) + (1,) * len(self.shape))
        st = np.where(lev > self.B_top[None], OUTCROPPED, GROUNDED)
        st = np.where(self.ncross > 0, CROSSED, st)
        return np.where(np.isnan(self.z_top)[None], DRY, st).astype(np.int8)

    @property
    def column_depth(self):
        return np.where(np.isnan(self.z_top), 0.0, self.z_top - self.z_bot)

    def thickness(self):
        st = self.status
        z = np.where(st == OUTCROPPED, self.z_top[None], np.where(st == GROUNDED, self.z_bot[None], self.z))
        return z[1:] - z[:-1]

    def slope(self):
        return -self.grad_B[..., :2] / self.grad_B[..., 2:3]

    def pv(self, f=None):
        f = self._f if f is None else f
        if f is None:
            raise ValueError("SurfaceMaps.pv: the model's parameters have no Coriolis parameter f - pass f= (a number, an array or a "
                             "function of the coordinates)")
        if callable(f):
            xy = np.broadcast_to(self._xy.reshape(self.shape + (2,)), self.z.shape + (2,))
            f = f(np.concatenate([xy, self.z[..., None]], axis=-1))
        return np.asarray(f, dtype=np.float64) * self.grad_B[..., 2]


class BuoyancySurfaces:
    """BuoyancySurfaces(model, b_levels, x=None, y=None, nx=256, ny=256, points=None): the surfaces B = b_levels[k] (finite, strictly
    increasing) over fixed columns on the model's architecture.  The columns are the tensor grid x (x) y - default nx and ny evenly
    spaced points over the locator's bounding box - or, points (n, 2) given, those.

      .compute() -> SurfaceMaps    of the model's CURRENT state
      .levels, .set_levels(b)      the B_k (read-only) and their replacement; the columns and their tiling stay
      .info -> dict                columns, segments, the most segments of one column, dry columns
      .segments()                  the tiling: col_ptr, cell, z_top, z_bot
      .z_top, .z_bot, .nseg        per column: the ends of its uppermost connected piece (NaN where dry) and its number of segments

    A column is the UPPERMOST connected piece of the vertical line inside the mesh: below an overhang it ends.  The bowls and the channel
    basin are height fields.  Mesh-partitioned models are refused: a column runs through the cells of several ranks."""

    def __init__(self, model, b_levels, x=None, y=None, nx=256, ny=256, points=None):
        if _partitioned(model):
            raise NotImplementedError("BuoyancySurfaces on a mesh-partitioned model is not implemented: a rank's locator and engine hold "
                                      "its own cells only, and a column runs through the cells of several ranks - map the surfaces of a "
                                      "single-device model")
        self.model, self.ctx = model, model.arch.ctx
        self.fe, self.loc = _engine(model), locator(model)     # kept alive for as long as the handle is
        self.set_levels(b_levels)
        if points is not None:
            xy = L.as_f64(points).reshape(-1, 2)
            self.x = self.y = None
            self.shape = (len(xy),)
        else:
            lo, hi = self.loc.bounding_box
            self.x = np.linspace(lo[0], hi[0], int(nx)) if x is None else L.as_f64(x).reshape(-1)
            self.y = np.linspace(lo[1], hi[1], int(ny)) if y is None else L.as_f64(y).reshape(-1)
            X, Y = np.meshgrid(self.x, self.y, indexing="ij")
            xy = L.as_f64(np.stack([X, Y], axis=-1).reshape(-1, 2))
            self.shape = (len(self.x), len(self.y))
        self.xy, self.ncol = xy, len(xy)
        h = C.c_void_p()
        L.check(L.lib().npg_surfaces_create(self.fe.h, self.loc.h, L.ptr(xy), self.ncol, C.byref(h)))
        self.h = h

    @property
    def levels(self):
        """the B_k, read-only (set_levels replaces them)"""
        return self._levels

    def set_levels(self, b_levels):
        """replace the levels; the columns and their tiling stay"""
        self._levels = L.as_f64(b_levels).reshape(-1).copy()
        self._levels.setflags(write=False)
        self._out = self._cols = None                          # sized by the number of levels: made again at the next compute
        return self

    def __del__(self):
        try:
            if self.h:
                L.lib().npg_surfaces_destroy(self.h)           # the handle goes before the locator and the engine it reads
                self.h = None
            self.loc = self.fe = None
        except Exception:
            pass

    @property
    def info(self):
        ns, mx, nd = C.c_int64(), C.c_int64(), C.c_int64()
        L.check(L.lib().npg_surfaces_info(self.h, C.byref(ns), C.byref(mx), C.byref(nd)))
        return dict(columns=self.ncol, segments=ns.value, max_per_column=mx.value, dry=nd.value)

    def _columns(self):
        zt, zb, ns = np.empty(self.ncol), np.empty(self.ncol), np.empty(self.ncol, dtype=np.int32)
        L.check(L.lib().npg_surfaces_columns(self.h, L.ptr(zt), L.ptr(zb), L.ptr(ns)))
        return zt.reshape(self.shape), zb.reshape(self.shape), ns.reshape(self.shape)

    z_top = property(lambda self: self._columns()[0])
    z_bot = property(lambda self: self._columns()[1])
    nseg = property(lambda self: self._columns()[2])

    def segments(self):
        """the tiling itself: (col_ptr (ncol + 1,), cell, z_top, z_bot) - column j owns the segments col_ptr[j] .. col_ptr[j + 1), top to
        bottom, and the z_top of each is the z_bot of the one above it"""
        ptr = np.concatenate([[0], np.cumsum(self.nseg.ravel(), dtype=np.int64)])
        cell, zt, zb = np.empty(ptr[-1], dtype=np.int32), np.empty(ptr[-1]), np.empty(ptr[-1])
        L.check(L.lib().npg_surfaces_segments(self.h, L.ptr(cell), L.ptr(zt), L.ptr(zb)))
        return ptr, cell, zt, zb

    def compute_raw(self):
        """(out (NPG_NSURF, nlev, ncol), cols (4, ncol)) as npg_surfaces_compute writes them"""
        nlev = len(self.levels)
        if self.ncol == 0 and nlev >= 1:
            return np.empty((NSURF, nlev, 0)), np.empty((4, 0))
        if self._out is None:
            self._out = DeviceVector(self.ctx, max(1, NSURF * nlev * self.ncol))
            self._cols = DeviceVector(self.ctx, 4 * self.ncol)
        m = self.model
        L.check(L.lib().npg_surfaces_compute(self.h, m.inversion.solver.x.h, m.b_vec.h, float(m.params.N2), L.ptr(self.levels), nlev,
                                             self._out.h, self._cols.h))
        return self._out.to_host()[:NSURF * nlev * self.ncol].reshape(NSURF, nlev, self.ncol), self._cols.to_host().reshape(4, self.ncol)

    def compute(self) -> SurfaceMaps:
        out, cols = self.compute_raw()
        return SurfaceMaps(self.levels, out, cols, self.shape, self.xy, getattr(self.model.params, "f", None))


def column_depth(model, x, y):
    """The depth of the mesh under (x, y), exactly: z_top - z_bot of the column's uppermost connected piece from the tiling of the
    cells (no probing, no bisection - `find_H` is the reference's way); 0 where the column is dry.  x, y: numbers or arrays of one
    shape."""
    x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    S = BuoyancySurfaces(model, [0.0], points=np.stack([x.ravel(), y.ravel()], axis=-1))
    zt, zb = S.z_top, S.z_bot
    H = np.where(np.isnan(zt), 0.0, zt - zb).reshape(x.shape)
    return float(H) if H.ndim == 0 else H


class SurfaceRecorder:
    """SurfaceRecorder(surfaces): an `on_plot(model, t)` hook that appends (t, SurfaceMaps) per call, as ClassRecorder does for the class
    tables.  `.as_arrays()` -> (t (n,), z (n, nlev, *shape), ncross (n, nlev, *shape)); `.save(path)` writes them with np.savez (keys t,
    z, z_low, ncross, u, grad_B, levels, xy, z_top, z_bot)."""

    def __init__(self, surfaces: BuoyancySurfaces):
        self.surfaces = surfaces
        self.t, self.maps = [], []

    def __call__(self, model, t):
        self.t.append(float(t))
        self.maps.append(self.surfaces.compute())

    def as_arrays(self):
        S = self.surfaces
        full = (len(self.maps), len(S.levels)) + S.shape
        return (np.array(self.t, dtype=np.float64), np.array([m.z for m in self.maps], dtype=np.float64).reshape(full),
                np.array([m.ncross for m in self.maps], dtype=np.int32).reshape(full))

    def save(self, path):
        t, z, ncross = self.as_arrays()
        S = self.surfaces
        full = z.shape
        zt, zb, _ = S._columns()
        np.savez(path, t=t, z=z, ncross=ncross, z_low=np.array([m.z_low for m in self.maps], dtype=np.float64).reshape(full),
                 u=np.array([m.u for m in self.maps], dtype=np.float64).reshape(full + (3,)),
                 grad_B=np.array([m.grad_B for m in self.maps], dtype=np.float64).reshape(full + (3,)),
                 levels=S.levels, xy=S.xy, z_top=zt, z_bot=zb)
