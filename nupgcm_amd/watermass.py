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
quantisation is at most half a unit per sample: n_bin 2^-61 S_c per bin.

Mixing (npg_classes_mixing).  The same handle bins what the mixing does to each class.  For FE fields div(kappa grad B)
is a distribution (gradients jump across faces), so the transformation is built from the quantity that is a function in every cell:

    D(B0) = int_{B < B0} kappa_h (d_x B^2 + d_y B^2) + kappa_v (d_z B)^2 dV,     Phi(B0) = dD / dB0 >= 0,     E(B0) = dPhi / dB0

Phi is the down-gradient diffusive buoyancy flux through the surface B = B0 and E the diapycnal volume transport towards higher
buoyancy, which in a steady state balances psi*.  Boundary terms (a surface buoyancy flux) are NOT part of it.  At a sample kappa_h
and the BACKGROUND kappa_v0 are the user's forcing functions evaluated at the physical sample point (not the engine's current
tables), and kappa_v = kappa_v0 + kappa_c (1 + tanh(-alpha (N2 + d_z b') / N2min)) / 2 is the convection closure evaluated from the
sample's own d_z b' when it is on.  The table is (ny + 1, nb + 1, NPG_NMIX), term = measure x integrand, raw integrals:

    0  1 (the census again)    1  kappa_h (d_x B^2 + d_y B^2)    2  kappa_v (d_z B)^2    3  kappa_v d_z B
    4  kappa_v                 5  kappa_h                        6  |grad B|^2           7  kappa_v - kappa_v0 (the closure's part)"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .architectures import DeviceVector
from .integrals import _layout
from .inversion import device_fe

NCLS = L.NPG_NCLS
CHANNELS = ("one", "u_x", "u_y", "u_z", "z", "B", "dz_B", "u_grad_B")
NMIX = L.NPG_NMIX
MIXING_CHANNELS = ("one", "kappa_h_gradh_B_sq", "kappa_v_dz_B_sq", "kappa_v_dz_B", "kappa_v", "kappa_h", "grad_B_sq", "kappa_conv")


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


def _quotient(num, den):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den != 0.0, num / den, np.nan)


class MixingTable:
    """What BuoyancyClasses.mixing() returns: `raw` (ny + 1, nb + 1, NPG_NMIX), `b_edges`, `y_edges`, and
      volume                   ch0 per (band, class)
      dissipation              ch1 + ch2: int kappa_h |grad_h B|^2 + kappa_v (d_z B)^2 over the class
      diffusive_flux()         Phi[j, k - 1] = dissipation[j, k] / (beta_k - beta_{k-1}) for the INTERIOR classes k = 1 .. nb - 1
                               (ny + 1, nb - 1; empty when nb < 2): the down-gradient buoyancy flux through the surfaces of class k
      transformation()         (Phi_{k+1} - Phi_k) / ((Delta_k + Delta_{k+1}) / 2) at the edges between two interior classes
                               (ny + 1, nb - 2): the diapycnal volume transport, positive towards higher buoyancy
      effective_diffusivity    dissipation / ch6: the diffusivity the class's own gradients feel
      mean_kappa_v, mean_kappa_h     ch4, ch5 / volume
      convective_fraction      ch7 / ch4: how much of the class's vertical diffusivity is convective adjustment
    Every quotient is NaN where its denominator is 0.  Boundary terms (a surface flux) are not part of Phi."""

    def __init__(self, raw, b_edges, y_edges):
        self.raw, self.b_edges, self.y_edges = raw, b_edges, y_edges
        self.volume = raw[..., 0]
        self.dissipation = raw[..., 1] + raw[..., 2]

    @property
    def effective_diffusivity(self):
        return _quotient(self.dissipation, self.raw[..., 6])

    @property
    def mean_kappa_v(self):
        return _quotient(self.raw[..., 4], self.volume)

    @property
    def mean_kappa_h(self):
        return _quotient(self.raw[..., 5], self.volume)

    @property
    def convective_fraction(self):
        return _quotient(self.raw[..., 7], self.raw[..., 4])

    def diffusive_flux(self):
        nb = len(self.b_edges)
        if nb < 2:
            return np.zeros((self.raw.shape[0], 0))
        return self.dissipation[:, 1:nb] / np.diff(self.b_edges)[None, :]

    def transformation(self):
        nb = len(self.b_edges)
        if nb < 3:
            return np.zeros((self.raw.shape[0], 0))
        delta = np.diff(self.b_edges)
        return np.diff(self.diffusive_flux(), axis=1) / (0.5 * (delta[:-1] + delta[1:]))[None, :]

    def __repr__(self):
        return f"MixingTable({self.raw.shape[0]} bands x {self.raw.shape[1]} classes, dissipation {self.dissipation.sum():.6e})"


class BuoyancyClasses:
    """BuoyancyClasses(model, b_edges, y_edges=(), level=1, mask=None, rule=None): the joint (latitude band, buoyancy class) table of
    the model's CURRENT state (3-D and embedded 2-D meshes).  rule = (lam (ns, 4), w (ns,)) replaces the default rule of `level`.
    mask (ncell,) bool: only these cells count.  `.compute(total=True)` bins the full buoyancy B = N2 z + b' (total=False: N2 = 0, the
    perturbation) and returns a ClassTable; it raises when samples were dropped (non-finite B or y).  `.compute_raw(total=True)`
    returns (table (ny + 1, nb + 1, NPG_NCLS), dropped, S (NPG_NCLS,)) and does not raise.  Two calls on the same state return the same
    bits.
    On a partition.PartitionedModel construction and `compute()` are COLLECTIVE, exactly as MeshIntegrals: every rank bins the cells
    it owns (and-ed with the GLOBAL `mask`) with its own scales, and the table and the info vector are added over the ranks in rank
    order (npg_comm_allreduce_long: the same bits on every rank).
    `.mixing(total=True)` bins the diffusivity-weighted channels of the same samples and returns a MixingTable (it raises on dropped
    samples); `.mixing_raw(total=True)` returns (table (ny + 1, nb + 1, NPG_NMIX), dropped, S) - collective in the same way.  On first
    use model.forcings.kappa_h / kappa_v (numbers or functions of x) are evaluated at the physical sample points of this handle's
    cells (`.set_diffusivity(kappa_h, kappa_v0)` replaces them); the closure's arguments are those of model.forcings.conv_param,
    params.alpha and params.N2 when it is on (`closure=(kappa_c, N2min, alpha, N2c)` overrides them, kappa_c = 0: off)."""

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
            self._cells = lay.cells
        else:
            self.fe = device_fe(model.arch, fed)
            cmask = gmask
            self._cells = None
        self._kappa_set = False
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

    def sample_points(self):
        """(ncell, ns, 3): the physical sample points of this handle's cells (this rank's on a partitioned model) - the rule's lam
        times the cells' own vertices"""
        m = self.model.fe_data.mesh
        X = m.geo_coords[m.cell_geo]
        if self._cells is not None:
            X = X[self._cells]
        return np.einsum("sk,cki->csi", self.rule[0][:, :X.shape[1]], X)

    def set_diffusivity(self, kappa_h=None, kappa_v0=None):
        """kappa_h and the background kappa_v0 of mixing(): numbers or functions of x (arrays (..., 3) -> (...)), as set_coeff accepts
        them; None: model.forcings.kappa_h / kappa_v.  A function is evaluated at sample_points(), a number is passed as the scalar.  A
        second call replaces the first."""
        f = self.model.forcings
        xs = None
        args = []
        for v in (f.kappa_h if kappa_h is None else kappa_h, f.kappa_v if kappa_v0 is None else kappa_v0):
            if callable(v):
                xs = self.sample_points() if xs is None else xs
                args += [L.as_f64(np.broadcast_to(np.asarray(v(xs), dtype=np.float64), xs.shape[:2])), 0.0]
            else:
                args += [None, float(v)]
        L.check(L.lib().npg_classes_set_diffusivity(self.h, None if args[0] is None else L.ptr(args[0]), args[1],
                                                    None if args[2] is None else L.ptr(args[2]), args[3]))
        self._kappa_set = True

    def mixing_raw(self, total=True, closure=None):
        """(table (ny + 1, nb + 1, NPG_NMIX), dropped, S (NPG_NMIX,)) of the current state"""
        m = self.model
        if not self._kappa_set:
            self.set_diffusivity()
        if closure is None:
            cp = m.forcings.conv_param
            closure = (cp.kappa_c, cp.N2min, m.params.alpha, m.params.N2) if cp.is_on else (0.0, 0.0, 0.0, 0.0)
        N2 = float(m.params.N2) if total else 0.0
        L.check(L.lib().npg_classes_mixing(self.h, m.b_vec.h, N2, *(float(v) for v in closure), self._table.h, self._info.h))
        if self.layout is not None:
            L.check(L.lib().npg_comm_allreduce_long(self.ctx.h, self._table.h))    # summed in rank order
            L.check(L.lib().npg_comm_allreduce_long(self.ctx.h, self._info.h))
        info = self._info.to_host()
        return self._table.to_host().reshape(self.shape), int(info[0]), info[1:]

    def mixing(self, total=True, closure=None) -> MixingTable:
        raw, dropped, _ = self.mixing_raw(total, closure)
        if dropped > 0:
            raise FloatingPointError(f"BuoyancyClasses.mixing: {dropped} samples were dropped (B or y is not finite there)")
        return MixingTable(raw, self.b_edges, self.y_edges)


class ClassRecorder:
    """ClassRecorder(model, b_edges, y_edges=(), level=1, mask=None, total=True): an `on_plot(model, t)` hook that appends (t, raw
    table) per call.  `.as_arrays()` -> (t (n,), raw (n, ny + 1, nb + 1, NPG_NCLS)); `.save(path)` writes them with np.savez (keys t,
    raw, b_edges, y_edges, channels).  Collective on a partitioned model (every rank records the same series).
    mixing=True: every call also appends the mixing table of the same handle (`.mixing_raw`, `.mixing_tables()`), and `save` adds the
    keys mixing_raw (n, ny + 1, nb + 1, NPG_NMIX) and mixing_channels."""

    def __init__(self, model, b_edges, y_edges=(), level=1, mask=None, total=True, mixing=False):
        self.classes = BuoyancyClasses(model, b_edges, y_edges, level=level, mask=mask)
        self.total = total
        self.t, self.raw = [], []
        self.mixing = bool(mixing)
        self.mixing_raw = []

    def __call__(self, model, t):
        self.t.append(float(t))
        self.raw.append(self.classes.compute(self.total).raw)
        if self.mixing:
            self.mixing_raw.append(self.classes.mixing(self.total).raw)

    def as_arrays(self):
        return np.array(self.t, dtype=np.float64), np.array(self.raw, dtype=np.float64).reshape((len(self.raw),) + self.classes.shape)

    def tables(self):
        """the recorded rows as ClassTable"""
        K = self.classes
        return [ClassTable(r, K.b_edges, K.y_edges) for r in self.raw]

    def mixing_tables(self):
        """the recorded mixing rows as MixingTable (mixing=True)"""
        K = self.classes
        return [MixingTable(r, K.b_edges, K.y_edges) for r in self.mixing_raw]

    def save(self, path):
        t, raw = self.as_arrays()
        K = self.classes
        extra = {}
        if self.mixing:
            extra = dict(mixing_raw=np.array(self.mixing_raw, dtype=np.float64).reshape((len(self.mixing_raw),) + K.shape),
                         mixing_channels=np.array(MIXING_CHANNELS))
        np.savez(path, t=t, raw=raw, b_edges=K.b_edges, y_edges=K.y_edges, channels=np.array(CHANNELS), **extra)
