"""Sampling the device-resident state at points - nan_eval, plot_slice's and plot_profiles' grids (src/plotting.jl:9-90,
279-300) and the evenly spaced grid the reference's post-processing starts from (postprocess/utils.py:33-83,
postprocess/streamfunctions.py:14-45).

The state never leaves the device to be looked at: a `PointLocator` (npg_locator: uniform bins over the mesh's bounding box)
finds, for every point, the cell that contains it and its barycentric coordinates; `npg_fe_sample` evaluates u, p, b' or
grad b' there from the solver vectors through the engine's DoF tables.  Outside the mesh every value is NaN, as nan_eval returns
it.  Locating and evaluating are separate steps: the `Located` points of a fixed slice are the reference's plotting `cache`
(plot_slice(cache, u, b)) - located once, re-evaluated every n_plot steps.  Drawing the pictures (matplotlib) is not part of this
package; `model.on_plot` (model.run) is where a caller hangs it.

What the reference does with the evenly spaced grid is reduce it (postprocess/streamfunctions.py, stratification.py): `GridDiagnostics`
does those reductions where the state lives - one fused pass (npg_fe_grid_integrals) generates, locates and evaluates every grid
point and accumulates the vertical and the zonal trapezoids, and only the 2-D integrals cross to the host.  The same diagnostics
from a `GridSamples` on the host (zonal_width, zonal_mean, overturning_streamfunction, average_stratification) are the reference's
functions restated."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .architectures import DeviceVector
from .inversion import device_fe

_FIELDS = {"u": (L.NPG_SAMPLE_U, 3), "p": (L.NPG_SAMPLE_P, 1), "b": (L.NPG_SAMPLE_B, 1), "grad_b": (L.NPG_SAMPLE_GRAD_B, 3)}
_trapz = getattr(np, "trapezoid", None) or np.trapz
CHUNK = 1 << 21          # points located / evaluated per call by sample_to_grid: ~150 MB of device memory at a time


def _partitioned(model):
    """The dispatch of every entry point: False for a single-device model, True for a mesh-partitioned one
    (partition.PartitionedModel), whose ranks then call the entry point COLLECTIVELY - the same arguments on every rank, the same
    complete result on every rank.  The replicated layout of distributed.py and 2-D meshes are refused."""
    if getattr(model.fe_data.mesh, "dim", 3) != 3:
        raise NotImplementedError("sampling is implemented for tetrahedral (3-D) meshes")
    if getattr(model, "layout", None) is not None and hasattr(model.layout, "locator_cells"):
        return True
    if getattr(model, "partition", None) is not None or getattr(model, "comm", None) is not None \
            or getattr(model.arch.ctx, "nranks", 1) > 1:
        raise NotImplementedError("sampling the replicated distributed layout is not implemented: use the mesh-partitioned model "
                                  "(partition.partitioned_model), whose ranks sample collectively, or a single-device model")
    return False


def _engine(model):
    """the assembly engine whose DoF tables the samples are evaluated through: the rank's own on a partitioned model"""
    return model.fe if _partitioned(model) else device_fe(model.arch, model.fe_data)


def _allreduce(ctx, vec):
    L.check(L.lib().npg_comm_allreduce_long(ctx.h, vec.h))


class Located:
    """n located points on the device (npg_located): the cell id of each (-1 outside the mesh) and its barycentric coordinates
    there.  The reference's evaluation `cache`.
    On a partitioned model every rank holds its own: `cells` and `lambdas` are RANK-LOCAL (the index of the cell in the rank's
    engine where this rank reports the point; -1 / NaN elsewhere - outside the mesh or another rank's point), `valid` is the mask
    merged over the ranks."""

    def __init__(self, ctx, n, collective=False):
        h = C.c_void_p()
        L.check(L.lib().npg_located_create(ctx.h, int(n), C.byref(h)))
        self.h, self.ctx, self.n = h, ctx, int(n)
        self.collective, self._valid = bool(collective), None

    @classmethod
    def from_host(cls, ctx, cells, lambdas):
        """points located by the caller: cells (n,) int, lambdas (n, 4).  Cell ids are checked when they are used."""
        c, lam = L.as_i32(cells), L.as_f64(lambdas)
        if lam.shape != (c.size, 4):
            raise ValueError(f"Located.from_host: lambdas must be ({c.size}, 4), got {lam.shape}")
        out = cls(ctx, c.size)
        L.check(L.lib().npg_located_upload(out.h, L.ptr(c), L.ptr(lam)))
        return out

    def __del__(self):
        try:
            if self.h:
                L.lib().npg_located_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def __len__(self):
        return self.n

    @property
    def cells(self):
        """cell ids, -1 outside the mesh.  Partitioned model: rank-local (see the class)"""
        c = np.empty(self.n, dtype=np.int32)
        L.check(L.lib().npg_located_download(self.h, L.ptr(c), None))
        return c

    @property
    def lambdas(self):
        """barycentric coordinates (n, 4), NaN outside the mesh.  Partitioned model: rank-local (see the class)"""
        lam = np.empty((self.n, 4))
        L.check(L.lib().npg_located_download(self.h, None, L.ptr(lam)))
        return lam

    @property
    def valid(self):
        """mask of the points that lie in the mesh (downloaded on request).  Partitioned model: the mask merged over the ranks - the
        FIRST read is collective (every rank must make it), later reads return the kept mask"""
        if not self.collective:
            return self.cells >= 0
        if self._valid is None:
            cnt = DeviceVector(self.ctx, max(1, self.n))
            if self.n:
                L.check(L.lib().npg_sample_mask(self.h, 0, cnt.h))
                _allreduce(self.ctx, cnt)
            self._valid = cnt.to_host()[:self.n] > 0.0
        return self._valid


class PointLocator:
    """PointLocator(model, nbins=0): the point search of one mesh on the model's architecture.  nbins = 0 chooses about one bin
    per cell.  `.locate(points)` -> Located.
    On a partitioned model the rank's locator holds the cells it owns and their witness layer (RankLayout.locator_cells) over the
    bounding box and the bin size of the WHOLE mesh; a point is found where the elected cell is owned by this rank, so over the
    ranks it is found exactly once."""

    def __init__(self, model, nbins=0):
        self.collective = _partitioned(model)
        m = model.fe_data.mesh
        self.ctx, self.fe = model.arch.ctx, _engine(model)
        # each cell's OWN first vertex: across a periodic seam a cell lies where its geometry says, not where its vertices' masters do
        anchor = L.as_f64(m.geo_coords[m.cell_geo[:, 0]])
        h = C.c_void_p()
        if self.collective:
            lay = model.layout
            cells, owned = lay.locator_cells(model.fe_data)
            pos = np.minimum(np.searchsorted(lay.cells, cells), len(lay.cells) - 1)
            engine = np.where(lay.cells[pos] == cells, pos, -1).astype(np.int32)     # witness cells the rank does not keep: -1
            G = L.as_f64(m.grad_lambda).reshape(m.ncell, 12)
            geo12 = L.as_f64(np.concatenate([anchor[cells], G[cells, 3:]], axis=1))
            box = np.zeros(6)
            L.check(L.lib().npg_locator_box(L.ptr(G), L.ptr(anchor), int(m.ncell), L.ptr(box)))   # the box of the serial locator
            gid, own8 = L.as_i64(cells), np.ascontiguousarray(owned, dtype=np.uint8)
            L.check(L.lib().npg_locator_create_cells(self.ctx.h, L.ptr(geo12), L.ptr(engine), L.ptr(gid), L.ptr(own8), len(cells),
                                                     L.ptr(box), int(nbins) or int(m.ncell), C.byref(h)))
        else:
            L.check(L.lib().npg_locator_create(self.fe.h, L.ptr(anchor), int(nbins), C.byref(h)))
        self.h = h

    def __del__(self):
        try:
            if self.h:
                L.lib().npg_locator_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def info(self):
        """bins per axis, bounding box (lo, hi), total candidate entries, mean and max candidates per bin"""
        dims, box = np.zeros(3, dtype=np.int64), np.zeros(6)
        ne, mx = C.c_int64(), C.c_int64()
        L.check(L.lib().npg_locator_info(self.h, L.ptr(dims), L.ptr(box), C.byref(ne), C.byref(mx)))
        out = dict(dims=tuple(int(v) for v in dims), lo=box[:3].copy(), hi=box[3:].copy(), entries=ne.value,
                   mean_per_bin=ne.value / float(np.prod(dims)), max_per_bin=mx.value)
        if self.collective:          # this rank's share: cell records held, the owned ones among them, device bytes of records and bins
            nr, no, nb = C.c_int64(), C.c_int64(), C.c_int64()
            L.check(L.lib().npg_locator_cells(self.h, C.byref(nr), C.byref(no), C.byref(nb)))
            out.update(cells=nr.value, owned=no.value, witness=nr.value - no.value, bytes=nb.value)
        return out

    @property
    def bounding_box(self):
        i = self.info()
        return i["lo"], i["hi"]

    def locate(self, points) -> Located:
        pts = L.as_f64(points).reshape(-1, 3)
        out = Located(self.ctx, len(pts), self.collective)
        if len(pts):
            pv = DeviceVector.from_host(self.ctx, pts.ravel())
            L.check(L.lib().npg_locator_find(self.h, pv.h, len(pts), out.h))
        return out


def locator(model) -> PointLocator:
    """the model's point locator, built on first use (a partitioned model: the rank's, from its layout)"""
    loc = model.__dict__.get("_point_locator")
    if loc is None:
        loc = model.__dict__["_point_locator"] = PointLocator(model)
    return loc


def _evaluate(model, field, located: Located):
    code, nc = _FIELDS[field]
    fe = _engine(model)
    vec = model.b_vec if field in ("b", "grad_b") else model.inversion.solver.x
    if located.n == 0:
        return np.empty((0, nc) if nc > 1 else (0,))
    if _partitioned(model):
        # every rank evaluates the points it reports and contributes zeros elsewhere; a count per point is summed alongside.  One
        # contributor per point: the sum is that rank's value, exactly.  Merged on the device, downloaded once.
        n = located.n
        buf = DeviceVector(model.arch.ctx, n * (nc + 1))
        out = buf.view(0, n * nc)
        L.check(L.lib().npg_fe_sample(fe.h, code, vec.h, located.h, out.h))
        L.check(L.lib().npg_sample_mask(located.h, nc, buf.h))
        _allreduce(model.arch.ctx, buf)
        L.check(L.lib().npg_sample_unmask(n, nc, buf.h))
    else:
        out = DeviceVector(model.arch.ctx, max(1, located.n * nc))
        L.check(L.lib().npg_fe_sample(fe.h, code, vec.h, located.h, out.h))
    a = out.to_host()
    return a.reshape(-1, nc) if nc > 1 else a


def nan_eval(model, field, points, cache: Located = None, perturbation=False):
    """nan_eval(u, x) of src/plotting.jl:9-31 for the model's fields: field "u" (n, 3), "p" (n,), "b" (n,), "grad_b" (n, 3) at
    points (n, 3), NaN outside the mesh.  "b" is the full buoyancy N2 z + b' and "grad_b" its gradient (N2 added to the z
    component), as save_vtk / plot_slice show it; perturbation=True returns b' / grad b' alone.  cache: the `Located` of an earlier
    call on the same points (returned by PointLocator.locate) - the points are then not searched again.
    Collective on a partitioned model (every rank: the same points, the same complete result)."""
    _partitioned(model)
    if field not in _FIELDS:
        raise ValueError(f"nan_eval: field must be one of {sorted(_FIELDS)}, got {field!r}")
    pts = L.as_f64(points).reshape(-1, 3)
    if cache is None:
        cache = locator(model).locate(pts)
    elif cache.n != len(pts):
        raise ValueError(f"nan_eval: the cache holds {cache.n} points, got {len(pts)}")
    v = _evaluate(model, field, cache)
    if not perturbation and model.params.N2 != 0.0:
        if field == "b":
            v = v + model.params.N2 * pts[:, 2]            # NaN + finite = NaN: outside stays outside
        elif field == "grad_b":
            v[:, 2] += model.params.N2
    return v


def sample_slice(model, x=None, y=None, z=None, bbox=(-1, -1, 1, 1), n=256, cache=None):
    """The grid of plot_slice (src/plotting.jl:61-80): one of x, y, z fixes the plane, bbox = (a_min, b_min, a_max, b_max) bounds the
    two remaining axes (in the order x, y, z), n points each way.  Returns a dict: `axes` (the two coordinate arrays), `dir`,
    u (n, n, 3), b (n, n) (full buoyancy) and `cache`, which a later call takes back as cache= to skip the point search."""
    a = np.linspace(bbox[0], bbox[2], n)
    b = np.linspace(bbox[1], bbox[3], n)
    A, B = np.meshgrid(a, b, indexing="ij")
    if x is not None:
        d, pts = "x", np.stack([np.full_like(A, float(x)), A, B], axis=-1)
    elif y is not None:
        d, pts = "y", np.stack([A, np.full_like(A, float(y)), B], axis=-1)
    elif z is not None:
        d, pts = "z", np.stack([A, B, np.full_like(A, float(z))], axis=-1)
    else:
        raise ValueError("One of x, y, or z must be specified for slice.")
    pts = pts.reshape(-1, 3)
    if cache is None:
        cache = locator(model).locate(pts)
    return dict(dir=d, axes=(a, b), points=pts, cache=cache,
                u=nan_eval(model, "u", pts, cache).reshape(n, n, 3), b=nan_eval(model, "b", pts, cache).reshape(n, n))


def find_H(model, x, y, tol=1e-8, n_probe=256):
    """Depth of the water column at (x, y) - find_H, src/plotting.jl:38-57: the lowest valid point of a probe of n_probe points
    between the bottom of the bounding box and z = 0, refined by bisection on validity to tol.  0 if the column is dry."""
    loc = locator(model)
    zlo = float(loc.bounding_box[0][2])
    zs = np.linspace(zlo, 0.0, n_probe)
    ok = loc.locate(np.column_stack([np.full(n_probe, float(x)), np.full(n_probe, float(y)), zs])).valid
    if not ok.any():
        return 0.0
    k = int(np.argmax(ok))
    if k == 0:
        return -zlo
    z_in, z_out = zs[k], zs[k - 1]
    while abs(z_in - z_out) > tol:
        zm = 0.5 * (z_in + z_out)
        if loc.locate([[x, y, zm]]).valid[0]:
            z_in = zm
        else:
            z_out = zm
    return -z_in


def sample_profiles(model, x, y, n=256):
    """The column of plot_profiles (src/plotting.jl:279-300): n points from z = -H to 0 at (x, y) with H from find_H.  Returns a
    dict: H, z (n,), u (n, 3), b (n,) (full buoyancy) and the `cache` of the column's points."""
    H = find_H(model, x, y)
    z = np.linspace(-H, 0.0, n)
    pts = np.column_stack([np.full(n, float(x)), np.full(n, float(y)), z])
    cache = locator(model).locate(pts)
    return dict(H=H, z=z, points=pts, cache=cache, u=nan_eval(model, "u", pts, cache), b=nan_eval(model, "b", pts, cache))


class GridSamples:
    """An evenly spaced grid over the mesh's bounding box (postprocess/utils.py:33-45) and what was sampled on it: x, y, z axes,
    valid (nx, ny, nz) bool, fields[name] of shape (nx, ny, nz[, 3]) with NaN outside."""

    def __init__(self, x, y, z, valid, fields):
        self.x, self.y, self.z, self.valid, self.fields = x, y, z, valid, fields
        self.nx, self.ny, self.nz = len(x), len(y), len(z)

    def __getitem__(self, name):
        return self.fields[name]


def sample_to_grid(model, nx=256, ny=256, nz=256, fields=("u", "b"), chunk=CHUNK):
    """sample_to_grid of postprocess/utils.py:48-78 without the VTK round trip: nx x ny x nz evenly spaced points over the mesh's
    bounding box, located and evaluated on the device.  The grid is worked through in chunks of `chunk` points (default 2^21), so the
    extra device memory stays near 72 bytes per chunk point (coordinates, cell ids, lambdas, one field) - about 150 MB - whatever
    the grid; the result lives on the host.  On a partitioned model (collective) every chunk is merged over the ranks before the
    next one starts: one more vector of (components + 1) doubles per chunk point, 32 bytes for u."""
    _partitioned(model)
    loc = locator(model)
    lo, hi = loc.bounding_box
    x, y, z = (np.linspace(lo[a], hi[a], k) for a, k in enumerate((nx, ny, nz)))
    n = nx * ny * nz
    valid = np.empty(n, dtype=bool)
    out = {f: np.empty((n, _FIELDS[f][1]) if _FIELDS[f][1] > 1 else n) for f in fields}
    per_x = ny * nz
    step = max(1, int(chunk) // per_x)                     # whole x-planes per chunk
    Y, Z = np.meshgrid(y, z, indexing="ij")
    for i0 in range(0, nx, step):
        i1 = min(nx, i0 + step)
        pts = np.empty((i1 - i0, per_x, 3))
        pts[:, :, 0] = x[i0:i1, None]
        pts[:, :, 1] = Y.ravel()
        pts[:, :, 2] = Z.ravel()
        pts = pts.reshape(-1, 3)
        c = loc.locate(pts)
        sl = slice(i0 * per_x, i1 * per_x)
        valid[sl] = c.valid
        for f in fields:
            out[f][sl] = nan_eval(model, f, pts, c)
    shp = (nx, ny, nz)
    return GridSamples(x, y, z, valid.reshape(shp), {f: v.reshape(shp + v.shape[1:]) for f, v in out.items()})


def depth(samples: GridSamples):
    """depth of postprocess/utils.py:81-83: the vertical trapezoid of the valid mask, (nx, ny)"""
    return _trapz(samples.valid.astype(float), x=samples.z, axis=2)


def barotropic_streamfunction(samples: GridSamples):
    """calculate_barotropic_streamfunction of postprocess/streamfunctions.py:14-45 on sampled u: U = vertical trapezoid of u_x (zero
    outside the mesh, as VTK's sampling leaves it), Psi(x, y) = int_y^ymax U dy'; both NaN where the depth is 0.  Returns (Psi, U)."""
    ux = np.nan_to_num(samples["u"][..., 0], nan=0.0)
    U = _trapz(ux, x=samples.z, axis=2)
    H = depth(samples)
    dy = np.diff(samples.y)
    cum = np.concatenate([np.zeros((U.shape[0], 1)), np.cumsum(0.5 * (U[:, 1:] + U[:, :-1]) * dy, axis=1)], axis=1)
    Psi = cum[:, -1:] - cum
    U[H == 0] = np.nan
    Psi[H == 0] = np.nan
    return Psi, U


def _cumtrapz(f, x, axis):
    """cumulative_trapezoid(f, x, axis=axis, initial=0)"""
    f = np.moveaxis(f, axis, -1)
    c = np.concatenate([np.zeros(f.shape[:-1] + (1,)), np.cumsum(0.5 * (f[..., 1:] + f[..., :-1]) * np.diff(x), axis=-1)], axis=-1)
    return np.moveaxis(c, -1, axis)


def _y_range(y, ymin, ymax):
    """the rows iymin : iymax + 1 of average_stratification (postprocess/stratification.py:49-52)"""
    return slice(int(np.searchsorted(y, ymin)), int(np.searchsorted(y, ymax)) + 1)


def _ratio(a, b):
    return np.divide(a, b, where=b != 0, out=np.full_like(a, np.nan))


def zonal_width(samples: GridSamples):
    """zonal_width of postprocess/utils.py:85-87: the zonal trapezoid of the valid mask, (ny, nz)"""
    return _trapz(samples.valid.astype(float), x=samples.x, axis=0)


def zonal_mean(field, samples: GridSamples, width=None):
    """zonal_mean of postprocess/utils.py:90-94: the zonal trapezoid of a sampled scalar field (nx, ny, nz) (zero outside the mesh)
    over the zonal width; NaN where the width is 0"""
    width = zonal_width(samples) if width is None else width
    return _ratio(_trapz(np.nan_to_num(field, nan=0.0), x=samples.x, axis=0), width)


def overturning_streamfunction(samples: GridSamples):
    """calculate_overturning_streamfunction of postprocess/streamfunctions.py:47-80 on sampled u and b: v_int = zonal trapezoid of
    u_y, psi_bar(y, z) = -1/alpha int_{-H}^{z} v_int dz' with alpha = -z.min(), both NaN where the zonal width is 0; b_bar the zonal
    mean of the full buoyancy.  Returns (psi_bar, v_int, b_bar)."""
    width = zonal_width(samples)
    v_int = _trapz(np.nan_to_num(samples["u"][..., 1], nan=0.0), x=samples.x, axis=0)
    b_bar = zonal_mean(samples["b"], samples, width)
    psi_bar = -1.0 / (-samples.z.min()) * _cumtrapz(v_int, samples.z, axis=1)
    v_int[width == 0] = np.nan
    psi_bar[width == 0] = np.nan
    return psi_bar, v_int, b_bar


def average_stratification(samples: GridSamples, ymin=-1, ymax=1, alpha=1.0):
    """average_stratification of postprocess/stratification.py:45-62 on sampled grad b (ask sample_to_grid for fields=("u", "b",
    "grad_b")): alpha d_z b, negative values and points outside the mesh set to 0, averaged horizontally over the rows ymin <= y <=
    ymax (searchsorted bounds, as the reference takes them).  Returns the profile (nz,); NaN at levels without a valid point.  d_z b is
    the pointwise derivative nan_eval(model, "grad_b") returns; alpha = params.alpha gives the reference's alpha*b_z."""
    sl = _y_range(samples.y, ymin, ymax)
    bz = np.where(samples.valid, np.nan_to_num(samples["grad_b"][..., 2], nan=0.0), 0.0)[:, sl, :]
    bz = alpha * np.maximum(bz, 0.0)
    mask = samples.valid[:, sl, :].astype(float)
    area = _trapz(_trapz(mask, x=samples.x, axis=0), x=samples.y[sl], axis=0)
    return _ratio(_trapz(_trapz(bz, x=samples.x, axis=0), x=samples.y[sl], axis=0), area)


class GridIntegrals:
    """What GridDiagnostics.compute() returns: the axes x, y, z and, finished on the host from the device's 2-D integrals,
      count_z (nx, ny), count_x (ny, nz)   valid points per column / per zonal line (integers)
      H, U, V, Psi (nx, ny)                depth, vertical integrals of u_x and u_y, barotropic streamfunction Psi = int_y^ymax U dy'
                                           (calculate_barotropic_streamfunction); U, V, Psi are NaN where H = 0
      width, v_int, w_int, b_bar, psi_bar (ny, nz)   zonal width, zonal integrals of u_y and u_z, zonal-mean full buoyancy and the
                                           overturning streamfunction (calculate_overturning_streamfunction); NaN where width = 0
      N2_bar(ymin, ymax) (nz,)             the horizontally averaged stratification (average_stratification)
    col (4, nx, ny) and zon (6, ny, nz) are the raw integrals (zeros, not NaN, where nothing is valid)."""

    def __init__(self, x, y, z, col, zon, alpha):
        self.x, self.y, self.z, self.col, self.zon, self.alpha = x, y, z, col, zon, float(alpha)
        self.count_z, self.count_x = np.rint(col[0]).astype(np.int64), np.rint(zon[0]).astype(np.int64)
        self.H, self.width = col[1].copy(), zon[1].copy()
        dry, closed = self.H == 0, self.width == 0
        U, V = col[2].copy(), col[3].copy()
        Psi = _trapz(U, x=y, axis=1)[:, None] - _cumtrapz(U, y, axis=1)
        v_int, w_int = zon[2].copy(), zon[3].copy()
        psi_bar = -1.0 / (-z.min()) * _cumtrapz(v_int, z, axis=1)
        for a in (U, V, Psi):
            a[dry] = np.nan
        for a in (v_int, w_int, psi_bar):
            a[closed] = np.nan
        self.U, self.V, self.Psi, self.v_int, self.w_int, self.psi_bar = U, V, Psi, v_int, w_int, psi_bar
        self.b_bar = _ratio(zon[4], self.width)

    def N2_bar(self, ymin=-1, ymax=1):
        """average_stratification (postprocess/stratification.py:45-62): params.alpha times the horizontal mean over ymin <= y <= ymax
        (searchsorted bounds) of max(d_z b, 0), b the full buoyancy; NaN at levels without a valid point.  d_z b is the POINTWISE
        derivative of the finite-element buoyancy, the one nan_eval(model, "grad_b") returns - not the nodally recovered field that
        save_vtk writes as alpha*b_z and the reference samples."""
        sl = _y_range(self.y, ymin, ymax)
        area = _trapz(self.zon[1][sl], x=self.y[sl], axis=0)
        return _ratio(self.alpha * _trapz(self.zon[5][sl], x=self.y[sl], axis=0), area)


class GridDiagnostics:
    """GridDiagnostics(model, nx=256, ny=256, nz=256, x=None, y=None, z=None): the streamfunctions, zonal means and the averaged
    stratification of the model's CURRENT state on the grid x (x) y (x) z - by default the np.linspace grid over the mesh's bounding
    box that sample_to_grid uses; an axis given explicitly (strictly increasing, at least 2 points; need not be uniform) replaces it.
    The axes are uploaded once and the output vectors are kept: `.compute()` runs one fused pass on the device
    (npg_fe_grid_integrals) and downloads 4 nx ny + 6 ny nz doubles.  Call it again after more timesteps - it is what an on_plot hook
    calls.
    On a partitioned model `compute()` is collective: each rank integrates the grid points it owns and the 2-D integrals are summed
    over the ranks in rank order - the same bits on every rank and every call; the counts are exact, the integrals differ from the
    single-device ones by the re-association of each sum into per-rank partial sums."""

    def __init__(self, model, nx=256, ny=256, nz=256, x=None, y=None, z=None):
        self.collective = _partitioned(model)
        self.model, self.loc = model, locator(model)
        lo, hi = self.loc.bounding_box
        given = (x, y, z)
        self.x, self.y, self.z = (np.linspace(lo[a], hi[a], int(k)) if given[a] is None else L.as_f64(given[a]).ravel().copy()
                                  for a, k in enumerate((nx, ny, nz)))
        self.nx, self.ny, self.nz = len(self.x), len(self.y), len(self.z)
        ctx = model.arch.ctx
        self.fe = _engine(model)
        self._axes = DeviceVector.from_host(ctx, np.concatenate([self.x, self.y, self.z]))
        ncol, nzon = max(1, 4 * self.nx * self.ny), max(1, 6 * self.ny * self.nz)
        if self.collective:
            self._out = DeviceVector(ctx, ncol + nzon)      # [col | zon]: one vector, so that the ranks' sum is one collective
            self._col, self._zon = self._out.view(0, ncol), self._out.view(ncol, nzon)
        else:
            self._col, self._zon = DeviceVector(ctx, ncol), DeviceVector(ctx, nzon)

    def compute(self) -> GridIntegrals:
        m = self.model
        L.check(L.lib().npg_fe_grid_integrals(self.fe.h, self.loc.h, m.inversion.solver.x.h, m.b_vec.h, float(m.params.N2),
                                              self._axes.h, self.nx, self.ny, self.nz, self._col.h, self._zon.h))
        if self.collective:
            _allreduce(m.arch.ctx, self._out)               # each rank integrated the points it owns: summed in rank order
        col = self._col.to_host().reshape(4, self.nx, self.ny)
        zon = self._zon.to_host().reshape(6, self.ny, self.nz)
        return GridIntegrals(self.x, self.y, self.z, col, zon, m.params.alpha)
