"""The flow in buoyancy coordinates: the device-resident state binned into (latitude band, buoyancy class) (npg_classes_compute,
DESIGN.md 17) - how much water lies in each buoyancy class and at what depth, how much of it moves north in each latitude band (the
residual overturning psi*(y, B)), how much crosses each class.  The reference's post-processing overlays isopycnals on a z-coordinate
psi (postprocess/streamfunctions.py) and stops there.

Definition.  Every cell is sampled at `ns` barycentric points lam[ns][4] with weights w[ns] > 0, sum w = 1 - NOT the engine's
quadrature: Keast's 11-point rule has a negative weight, and a census must not put negative volume into a class.  The default rule is
the centroids of the 8^level equal-volume sub-tetrahedra of `level` red refinements, all weights equal (embedded 2-D meshes: the
centroids of the 4^level sub-triangles, lambda_4 = 0).  A sample of cell c carries the measure w[s] wdet(c) sum_q qw[q]; the rule is
exact for functions linear in the cell and a positive Riemann sum that `level` refines for everything else.  At a sample, all from
one lambda with the closed-form shape functions and the nodal values (Dirichlet nodes count):

    y = sum lambda_i y_i,  z = sum lambda_i z_i  (the cell's own vertices),   B = N2 z + b',   u,   grad B = grad b' + N2 e_z

Bins.  b_edges[nb] and y_edges[ny] are finite and strictly increasing (nb = 0 and ny = 0 are allowed); the class of a sample is
np.searchsorted(b_edges, B, side="right") (0 .. nb), its band the same of y_edges and y: the end bins are open, so every finite sample
is counted exactly once.  A sample whose B or y is not finite goes to no bin and is counted in `dropped`.  The table is
(ny + 1, nb + 1, NPG_NCLS), term = measure x integrand, raw integrals (prefactors are the caller's):

    0  1 (volume census)    1  u_x    2  u_y (residual overturning)    3  u_z    4  z    5  B    6  d_z B    7  u . grad B

Determinism.  Two calls on the same state give the same bits.  The destination of a term depends on the data, so the sums are made
order-independent: a first pass forms S_c = sum |term_c| (fixed order), the terms are rounded to integers in units of 2^(e - 61),
frexp(S_c) = (m, e), added as 64-bit integers (associative: any order, any atomics) and divided by the scale at the end.  The
quantisation is at most half a unit per sample: n_bin 2^-61 S_c per bin."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .architectures import DeviceVector
from .integrals import _layout
from .inversion import device_fe

NCLS = L.NPG_NCLS
CHANNELS = ("one", "u_x", "u_y", "u_z", "z", "B", "dz_B", "u_grad_B")


def _red_children(T):
    """the 8 equal-volume children of the red refinement of simplices T (n, 4, 4) (rows = vertices in barycentric coordinates)"""
    v = [T[:, i] for i in range(4)]
    m = {(i, j): 0.5 * (v[i] + v[j]) for i in range(4) for j in range(i + 1, 4)}
    kids = [(v[0], m[0, 1], m[0, 2], m[0, 3]), (m[0, 1], v[1], m[1, 2], m[1, 3]), (m[0, 2], m[1, 2], v[2], m[2, 3]),
            (m[0, 3], m[1, 3], m[2, 3], v[3]),
            # the inner octahedron cut along the diagonal m02 - m13
            (m[0, 1], m[0, 2], m[0, 3], m[1, 3]), (m[0, 1], m[0, 2], m[1, 2], m[1, 3]),
            (m[0, 2], m[0, 3], m[1, 3], m[2, 3]), (m[0, 2], m[1, 2], m[1, 3], m[2, 3])]
    return np.concatenate([np.stack(k, axis=1) for k in kids])


def _red_children_2d(T):
    """the 4 congruent children of triangles T (n, 3, 4) on the face lambda_4 = 0"""
    a, b, c = T[:, 0], T[:, 1], T[:, 2]
    ab, ac, bc = 0.5 * (a + b), 0.5 * (a + c), 0.5 * (b + c)
    return np.concatenate([np.stack(k, axis=1) for k in ((a, ab, ac), (ab, b, bc), (ac, bc, c), (ab, bc, ac))])


def default_rule(level=1, dim=3):
    """(lam (ns, 4), w (ns,)): the centroids of the 8^level (dim = 3) or 4^level (dim = 2, lambda_4 = 0) equal sub-simplices of
    `level` red refinements of the reference cell, equal weights; level = 0 is the cell centroid"""
    level = int(level)
    if level < 0 or (8 if dim == 3 else 4) ** level > 4096:
        raise ValueError(f"BuoyancyClasses: level {level} gives fewer than 1 or more than 4096 samples per cell")
    T = np.eye(4)[None, :dim + 1]
    for _ in range(level):
        T = _red_children(T) if dim == 3 else _red_children_2d(T)
    lam = np.ascontiguousarray(T.mean(axis=1))
    return lam, np.full(len(lam), 1.0 / len(lam))


class ClassTable:
    """What BuoyancyClasses.compute() returns: `raw` (ny + 1, nb + 1, NPG_NCLS), `b_edges`, `y_edges`, and
      volume                   ch0 per (band, class)
      census()                 V(B < beta_k): ch0 summed over the bands, cumulative over the classes (nb + 1 values; the last = the volume)
      residual_overturning()   psi*[j, k] = sum_{k' <= k} ch2[j, k'] / (y_{j+1} - y_j) for the INTERIOR bands (ny - 1, nb + 1): the northward
                               transport below B = beta_k per unit latitude
      mean_depth, mean_buoyancy, stratification     ch4, ch5, ch6 / volume, NaN where the volume is 0
      advective_tendency       ch7"""

    def __init__(self, raw, b_edges, y_edges):
        self.raw, self.b_edges, self.y_edges = raw, b_edges, y_edges
        self.volume = raw[..., 0]
        self.advective_tendency = raw[..., 7]

    def _per_volume(self, k):
        V = self.volume
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(V != 0.0, self.raw[..., k] / V, np.nan)

    @property
    def mean_depth(self):
        return self._per_volume(4)

    @property
    def mean_buoyancy(self):
        return self._per_volume(5)

    @property
    def stratification(self):
        return self._per_volume(6)

    def census(self):
        return np.cumsum(self.volume.sum(axis=0))

    def residual_overturning(self):
        if len(self.y_edges) < 2:
            return np.zeros((0, self.raw.shape[1]))
        return np.cumsum(self.raw[1:-1, :, 2], axis=1) / np.diff(self.y_edges)[:, None]

    def __repr__(self):
        return f"ClassTable({self.raw.shape[0]} bands x {self.raw.shape[1]} classes, volume {self.volume.sum():.6e})"


class BuoyancyClasses:
    """BuoyancyClasses(model, b_edges, y_edges=(), level=1, mask=None, rule=None): the joint (latitude band, buoyancy class) table of
    the model's CURRENT state (3-D and embedded 2-D meshes).  rule = (lam (ns, 4), w (ns,)) replaces the default rule of `level`.
    mask (ncell,) bool: only these cells count.  `.compute(total=True)` bins the full buoyancy B = N2 z + b' (total=False: N2 = 0, the
    perturbation) and returns a ClassTable; it raises when samples were dropped (non-finite B or y).  `.compute_raw(total=True)`
    returns (table (ny + 1, nb + 1, NPG_NCLS), dropped, S (NPG_NCLS,)) and does not raise.  Two calls on the same state return the same
    bits.
    On a partition.PartitionedModel construction and `compute()` are COLLECTIVE, exactly as MeshIntegrals: every rank bins the cells
    it owns (and-ed with the GLOBAL `mask`) with its own scales, and the table and the info vector are added over the ranks in rank
    order (npg_comm_allreduce_long: the same bits on every rank)."""

    def __init__(self, model, b_edges, y_edges=(), level=1, mask=None, rule=None):
        self.model = model
        fed = model.fe_data
        m = fed.mesh
        self.layout = _layout(model)
        self.ctx = model.arch.ctx
        self.b_edges = L.as_f64(np.asarray(b_edges, dtype=np.float64).reshape(-1))
        self.y_edges = L.as_f64(np.asarray(y_edges, dtype=np.float64).reshape(-1))
        X = m.geo_coords[m.cell_geo]
        if rule is None:
            rule = default_rule(level, X.shape[1] - 1)
        lam, w = L.as_f64(rule[0]), L.as_f64(rule[1])
        if lam.ndim != 2 or lam.shape[1] != 4 or w.shape != (len(lam),):
            raise ValueError(f"BuoyancyClasses: the rule must be (lam (ns, 4), w (ns,)), got {lam.shape} and {w.shape}")
        self.rule = (lam, w)
        y, z = L.as_f64(X[:, :, 1]), L.as_f64(X[:, :, 2])
        if y.shape[1] == 3:                    # embedded 2-D mesh: the device's fourth vertex (lambda_4 = 0) never weighs in
            y, z = (L.as_f64(np.concatenate([a, np.zeros((len(a), 1))], axis=1)) for a in (y, z))
        gmask = None if mask is None else np.asarray(mask, dtype=bool)
        if gmask is not None and gmask.shape != (m.ncell,):
            raise ValueError(f"BuoyancyClasses: mask must have shape ({m.ncell},), got {gmask.shape}")
        if self.layout is not None:
            lay = self.layout
            own = lay.cell_owner == lay.rank
            assert np.isin(np.nonzero(own)[0], lay.cells, assume_unique=True).all(), "an owned cell is kept by no rank"
            self.fe = model.fe
            y, z = L.as_f64(y[lay.cells]), L.as_f64(z[lay.cells])
            cmask = own[lay.cells] if gmask is None else own[lay.cells] & gmask[lay.cells]
        else:
            self.fe = device_fe(model.arch, fed)
            cmask = gmask
        self.ncells_counted = int(len(z) if cmask is None else cmask.sum())         # this rank's share
        self._mask8 = None if cmask is None else np.ascontiguousarray(cmask, dtype=np.uint8)
        self.shape = (len(self.y_edges) + 1, len(self.b_edges) + 1, NCLS)
        self.h = None
        h = C.c_void_p()
        L.check(L.lib().npg_classes_create(self.fe.h, L.ptr(y), L.ptr(z), None if self._mask8 is None else L.ptr(self._mask8),
                                           L.ptr(lam), L.ptr(w), len(w), L.ptr(self.y_edges), len(self.y_edges), L.ptr(self.b_edges),
                                           len(self.b_edges), C.byref(h)))
        self.h = h
        self._table = DeviceVector(self.ctx, int(np.prod(self.shape)))
        self._info = DeviceVector(self.ctx, 1 + NCLS)

    def __del__(self):
        try:
            if self.h:
                L.lib().npg_classes_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def compute_raw(self, total=True):
        """(table (ny + 1, nb + 1, NPG_NCLS), dropped, S (NPG_NCLS,)) of the current state"""
        m = self.model
        N2 = float(m.params.N2) if total else 0.0
        L.check(L.lib().npg_classes_compute(self.h, m.inversion.solver.x.h, m.b_vec.h, N2, self._table.h, self._info.h))
        if self.layout is not None:
            L.check(L.lib().npg_comm_allreduce_long(self.ctx.h, self._table.h))    # summed in rank order
            L.check(L.lib().npg_comm_allreduce_long(self.ctx.h, self._info.h))
        info = self._info.to_host()
        return self._table.to_host().reshape(self.shape), int(info[0]), info[1:]

    def compute(self, total=True) -> ClassTable:
        raw, dropped, _ = self.compute_raw(total)
        if dropped > 0:
            raise FloatingPointError(f"BuoyancyClasses.compute: {dropped} samples were dropped (B or y is not finite there)")
        return ClassTable(raw, self.b_edges, self.y_edges)


class ClassRecorder:
    """ClassRecorder(model, b_edges, y_edges=(), level=1, mask=None, total=True): an `on_plot(model, t)` hook that appends (t, raw
    table) per call.  `.as_arrays()` -> (t (n,), raw (n, ny + 1, nb + 1, NPG_NCLS)); `.save(path)` writes them with np.savez (keys t,
    raw, b_edges, y_edges, channels).  Collective on a partitioned model (every rank records the same series)."""

    def __init__(self, model, b_edges, y_edges=(), level=1, mask=None, total=True):
        self.classes = BuoyancyClasses(model, b_edges, y_edges, level=level, mask=mask)
        self.total = total
        self.t, self.raw = [], []

    def __call__(self, model, t):
        self.t.append(float(t))
        self.raw.append(self.classes.compute(self.total).raw)

    def as_arrays(self):
        return np.array(self.t, dtype=np.float64), np.array(self.raw, dtype=np.float64).reshape((len(self.raw),) + self.classes.shape)

    def tables(self):
        """the recorded rows as ClassTable"""
        K = self.classes
        return [ClassTable(r, K.b_edges, K.y_edges) for r in self.raw]

    def save(self, path):
        t, raw = self.as_arrays()
        K = self.classes
        np.savez(path, t=t, raw=raw, b_edges=K.b_edges, y_edges=K.y_edges, channels=np.array(CHANNELS))
