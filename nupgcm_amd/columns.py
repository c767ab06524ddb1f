"""Column integrals (npg_columns_*): the depth-integrated flow and the terms of its vorticity balance over fixed columns
(x_j, y_j) - the barotropic transport (U, V) and its streamfunction, the baroclinic potential energy gamma = - int z B dz, JEBAR
= - J(1/H, gamma), the bottom pressure torque and the depth-integrated pressure gradient.  The reference's author computes them from
nan_eval samples on a sigma grid, a trapezoid in the vertical and finite differences in x and y (scratch/postprocess.jl: compute_U_V,
compute_Psi, compute_gamma, compute_JEBAR).

Here the vertical integral is exact: a column is tiled into the cells it passes through (the tiling of BuoyancySurfaces), along a
segment every integrand is a polynomial in z of degree <= 5, and a 3-point Gauss-Legendre rule integrates it exactly.  grad H of the
piecewise-linear bottom is the slope of the face the column leaves through, and grad gamma follows from Leibniz's rule per column, so
JEBAR and the bottom pressure torque are pointwise maps of the discrete state without a horizontal difference."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .architectures import DeviceVector
from .sampling import _engine, _partitioned, locator

NCOLI, NCOLE = L.NPG_NCOLI, L.NPG_NCOLE


class ColumnMaps:
    """What one call of ColumnIntegrals.compute() found.  `shape` = the columns' shape: (nx, ny) for a grid, (n,) for points.  NaN where
    the column is dry.

      .z_top, .z_bot, .H (*shape)     the column's ends and H = z_top - z_bot (column_depth's bits);  .thickness = int dz, the sum of
                                      the segments' lengths (H to rounding)
      .grad_z_top, .grad_z_bot, .grad_H (*shape, 2)   the slopes of the faces at the ends; grad H = grad z_top - grad z_bot
      .U (*shape, 3)                  int u dz
      .ke                             int (u_x^2 + u_y^2) / 2 dz
      .buoyancy_transport (*shape, 3) int u b' dz
      .b_int, .p_int                  int b' dz, int p dz
      .grad_p_int (*shape, 2)         int grad_h p dz
      .p_bot, .b_bot, .N2_bot         p, b' and N2 + d_z b' at the bottom;  .grad_p_bot (*shape, 3)
      .p_top, .b_top, .u_top (*shape, 2)   at the top
      .gamma(full=True)               - int z B dz; B = N2 z + b' (full) or b' alone
      .grad_gamma(full=True) (*shape, 2)
      .jebar(full=True)               (H_x gamma_y - H_y gamma_x) / H^2 = - J(1/H, gamma)
      .bottom_pressure_torque()       d_x p d_y H - d_y p d_x H at the bottom
      .stress_residual(f) (*shape, 2) f z^ x U + int grad_h p dz: what friction and the wind stress balance; f a number or f(x, y)
      .streamfunction()               gridded columns only: Psi = - int U dy, cumulative trapezoid from y[0], dry columns as 0, then NaN"""

    def __init__(self, out, z_top, z_bot, shape, xy, N2, x=None, y=None):
        self.shape, self._xy, self.N2, self.x, self.y = tuple(shape), xy, float(N2), x, y
        o = out.reshape((NCOLI + NCOLE,) + self.shape)
        self.raw = o
        vec = lambda *ch: np.stack([o[k] for k in ch], axis=-1)
        self.thickness, self.z_top, self.z_bot = o[0], z_top.reshape(self.shape), z_bot.reshape(self.shape)
        self.H = self.z_top - self.z_bot
        self.U, self.b_int, self.p_int, self.ke = vec(1, 2, 3), o[4], o[6], o[13]
        self.zb_int, self.grad_p_int, self.grad_b_int, self.z_grad_b_int = o[5], vec(7, 8), vec(9, 10), vec(11, 12)
        self.buoyancy_transport = vec(14, 15, 16)
        self.p_bot, self.b_bot, self.N2_bot, self.grad_p_bot = o[17], o[18], self.N2 + o[19], vec(20, 21, 22)
        self.grad_z_bot = vec(23, 24)
        self.p_top, self.b_top, self.u_top, self.grad_z_top = o[25], o[26], vec(27, 28), vec(29, 30)
        self.grad_H = self.grad_z_top - self.grad_z_bot

    def gamma(self, full=True):
        g = -self.zb_int
        if full:
            g = g - self.N2 * (self.z_top ** 3 - self.z_bot ** 3) / 3.0
        return g

    def grad_gamma(self, full=True):
        """Leibniz: d gamma = - int z d b' dz - z_top B(z_top) d z_top + z_bot B(z_bot) d z_bot (b' is continuous across the faces inside
        the column, so only the two ends contribute)"""
        Bt, Bb = self.b_top, self.b_bot
        if full:
            Bt, Bb = Bt + self.N2 * self.z_top, Bb + self.N2 * self.z_bot
        return -self.z_grad_b_int - (self.z_top * Bt)[..., None] * self.grad_z_top + (self.z_bot * Bb)[..., None] * self.grad_z_bot

    def jebar(self, full=True):
        g = self.grad_gamma(full)
        return (self.grad_H[..., 0] * g[..., 1] - self.grad_H[..., 1] * g[..., 0]) / self.H ** 2

    def bottom_pressure_torque(self):
        return self.grad_p_bot[..., 0] * self.grad_H[..., 1] - self.grad_p_bot[..., 1] * self.grad_H[..., 0]

    def stress_residual(self, f):
        if callable(f):
            xy = self._xy.reshape(self.shape + (2,))
            f = f(xy[..., 0], xy[..., 1])
        f = np.asarray(f, dtype=np.float64)
        return np.stack([-f * self.U[..., 1] + self.grad_p_int[..., 0], f * self.U[..., 0] + self.grad_p_int[..., 1]], axis=-1)

    def streamfunction(self):
        if self.y is None:
            raise ValueError("ColumnMaps.streamfunction: Psi = - int U dy needs gridded columns (x, y), not points")
        U = self.U[..., 0]
        dry = np.isnan(U)
        Uf = np.where(dry, 0.0, U)
        psi = -np.concatenate([np.zeros((Uf.shape[0], 1)), np.cumsum(0.5 * (Uf[:, 1:] + Uf[:, :-1]) * np.diff(self.y), axis=1)], axis=1)
        psi[dry] = np.nan
        return psi


class ColumnIntegrals:
    """ColumnIntegrals(model, x=None, y=None, nx=256, ny=256, points=None): the exact vertical integrals of the model's state over fixed
    columns on the model's architecture.  The columns are those of BuoyancySurfaces: the tensor grid x (x) y - default nx and ny evenly
    spaced points over the locator's bounding box - or, points (n, 2) given, those.

      .compute() -> ColumnMaps       of the model's CURRENT state (model.inversion.solver.x and model.b_vec: TimeAverages.applied works)
      .compute_raw(segments=False)   out (NPG_NCOLI + NPG_NCOLE, ncol) as npg_columns_compute writes it; segments: and the terms
                                     (NPG_NCOLI, nseg) the columns are folded from
      .info -> dict                  columns, segments, the most segments of one column, dry columns
      .segments()                    the tiling: col_ptr, cell, z_top, z_bot
      .z_top, .z_bot, .nseg          per column

    Mesh-partitioned models are refused: a column runs through the cells of several ranks."""

    def __init__(self, model, x=None, y=None, nx=256, ny=256, points=None):
        if _partitioned(model):
            raise NotImplementedError("ColumnIntegrals on a mesh-partitioned model is not implemented: a rank's locator and engine hold "
                                      "its own cells only, and a column runs through the cells of several ranks - integrate the columns "
                                      "of a single-device model")
        self.h = None
        self.model, self.ctx = model, model.arch.ctx
        self.fe, self.loc = _engine(model), locator(model)     # kept alive for as long as the handle is
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
        self._out = self._seg = None
        h = C.c_void_p()
        L.check(L.lib().npg_columns_create(self.fe.h, self.loc.h, L.ptr(xy), self.ncol, C.byref(h)))
        self.h = h

    def __del__(self):
        try:
            if self.h:
                L.lib().npg_columns_destroy(self.h)            # the handle goes before the locator and the engine it reads
                self.h = None
            self.loc = self.fe = None
        except Exception:
            pass

    @property
    def info(self):
        ns, mx, nd = C.c_int64(), C.c_int64(), C.c_int64()
        L.check(L.lib().npg_columns_info(self.h, C.byref(ns), C.byref(mx), C.byref(nd)))
        return dict(columns=self.ncol, segments=ns.value, max_per_column=mx.value, dry=nd.value)

    def _columns(self):
        zt, zb, ns = np.empty(self.ncol), np.empty(self.ncol), np.empty(self.ncol, dtype=np.int32)
        L.check(L.lib().npg_columns_columns(self.h, L.ptr(zt), L.ptr(zb), L.ptr(ns)))
        return zt.reshape(self.shape), zb.reshape(self.shape), ns.reshape(self.shape)

    z_top = property(lambda self: self._columns()[0])
    z_bot = property(lambda self: self._columns()[1])
    nseg = property(lambda self: self._columns()[2])

    def segments(self):
        """the tiling itself: (col_ptr (ncol + 1,), cell, z_top, z_bot) - column j owns the segments col_ptr[j] .. col_ptr[j + 1), top to
        bottom, and the z_top of each is the z_bot of the one above it"""
        ptr = np.concatenate([[0], np.cumsum(self.nseg.ravel(), dtype=np.int64)])
        cell, zt, zb = np.empty(ptr[-1], dtype=np.int32), np.empty(ptr[-1]), np.empty(ptr[-1])
        L.check(L.lib().npg_columns_segments(self.h, L.ptr(cell), L.ptr(zt), L.ptr(zb)))
        return ptr, cell, zt, zb

    def compute_raw(self, segments=False):
        if self._out is None:
            self._out = DeviceVector(self.ctx, (NCOLI + NCOLE) * self.ncol)
        nseg = self.info["segments"]
        seg = None
        if segments and nseg:
            if self._seg is None:
                self._seg = DeviceVector(self.ctx, NCOLI * nseg)
            seg = self._seg
        m = self.model
        L.check(L.lib().npg_columns_compute(self.h, m.inversion.solver.x.h, m.b_vec.h, self._out.h, seg.h if seg is not None else None))
        out = self._out.to_host().reshape(NCOLI + NCOLE, self.ncol)
        if not segments:
            return out
        return out, (seg.to_host().reshape(NCOLI, nseg) if seg is not None else np.empty((NCOLI, 0)))

    def compute(self) -> ColumnMaps:
        zt, zb, _ = self._columns()
        return ColumnMaps(self.compute_raw(), zt, zb, self.shape, self.xy, self.model.params.N2, self.x, self.y)


class ColumnRecorder:
    """ColumnRecorder(columns): an `on_plot(model, t)` hook that appends (t, ColumnMaps) per call, as SurfaceRecorder does for the maps on
    buoyancy surfaces.  `.as_arrays()` -> (t (n,), raw (n, NPG_NCOLI + NPG_NCOLE, *shape)); `.save(path)` writes them with np.savez (keys
    t, raw, xy, z_top, z_bot, N2) and `ColumnRecorder.load(path)` -> (t, [ColumnMaps])."""

    def __init__(self, columns: ColumnIntegrals):
        self.columns = columns
        self.t, self.maps = [], []

    def __call__(self, model, t):
        self.t.append(float(t))
        self.maps.append(self.columns.compute())

    def as_arrays(self):
        shape = (len(self.maps), NCOLI + NCOLE) + self.columns.shape
        return np.array(self.t, dtype=np.float64), np.array([m.raw for m in self.maps], dtype=np.float64).reshape(shape)

    def save(self, path):
        t, raw = self.as_arrays()
        S = self.columns
        zt, zb, _ = S._columns()
        grid = {} if S.x is None else dict(x=S.x, y=S.y)
        np.savez(path, t=t, raw=raw, xy=S.xy, z_top=zt, z_bot=zb, N2=float(S.model.params.N2), **grid)

    @staticmethod
    def load(path):
        f = np.load(path)
        shape = f["z_top"].shape
        x, y = (f["x"], f["y"]) if "x" in f.files else (None, None)
        return f["t"], [ColumnMaps(r.reshape(NCOLI + NCOLE, -1), f["z_top"], f["z_bot"], shape, f["xy"], float(f["N2"]), x, y) for r in f["raw"]]
