"""Gradients of the device-resident state recovered at the mesh's P2 nodes (npg_nodal_*): d_j u_a, grad b' and grad p as
nodal FIELDS, and what is made of them - vorticity, divergence, the stratification N2 + d_z b', the planetary PV f (N2 + d_z b') and the
closure fields of save_vtk.  Every other diagnostic reduces the state to sums, tables, maps on columns or values at sampled points; this
one returns a derivative of the state on the mesh.

Definition (csrc/nodal_core.h; the bits are part of the interface).  A node n has incidences (c, i): cell c holds it as local node i,
taken in ascending c.  Per cell and field the gradient at the cell's four vertices is formed exactly as the point sampler forms it
there; the mid-node of the edge (a, b) takes 0.5 (g_a + g_b) - the gradient of a P2 function is affine in lambda, so this is the
gradient at the midpoint.  Per node S = sum_c w_c g_c and W = sum_c w_c, from 0.0 in incidence order, and the result is S / W with
w_c = wdet(c) (weight="volume") or 1.0 (weight="count").  The cells carry their own geometry, so a periodic seam needs nothing special.
A BOUNDARY node has cells on one side only: its value is a one-sided average, first-order accurate where an interior node's is second.

Two launches on the device (cells into a scratch of at most 51 doubles per cell, then nodes), no atomics: two calls give the same bits,
and GPU() and CPU() give the same bits."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .architectures import DeviceVector
from .inversion import device_fe

FIELDS = {"u": L.NPG_NODAL_U, "b": L.NPG_NODAL_B, "p": L.NPG_NODAL_P}
WEIGHTS = {"volume": 0, "count": 1}


def _refuse(model):
    if model.fe_data.mesh.cell_nodes.shape[1] != 10:
        raise NotImplementedError("NodalFields is implemented for tetrahedral (3-D) meshes, not for embedded 2-D meshes")
    if getattr(model, "layout", None) is not None and (hasattr(model.layout, "cell_owner") or hasattr(model.layout, "locator_cells")):
        raise NotImplementedError("NodalFields on a mesh-partitioned model is not implemented (a node on a cut has incidences on several "
                                  "ranks): recover the gradients of a single-device model")
    if getattr(model, "partition", None) is not None or getattr(model, "comm", None) is not None \
            or getattr(model.arch.ctx, "nranks", 1) > 1:
        raise NotImplementedError("NodalFields of the replicated distributed layout is not implemented: use a single-device model")


def incidence_table(cell_nodes, nn, nodes=None, ordered=False):
    """(node ids, ptr int64 (nsel + 1), inc int32): the incidences 16 cell + local of the selected nodes, ascending in the cell.
    ordered: the rows sorted by valence (stably: mesh order within a valence) - the lanes of a wave then walk lists of one length (a
    vertex has some 24 cells around it, a mid-node 5), but neighbouring rows no longer share cells: measured slower, so
    mesh order is the default.  A node's own list, and so its bits, are the same in either order"""
    nc, nl = cell_nodes.shape
    flat = np.asarray(cell_nodes).ravel()
    order = np.argsort(flat, kind="stable")                            # by node; within a node by 10 c + i, so by c
    code = (16 * (order // nl) + order % nl).astype(np.int64)
    count = np.bincount(flat, minlength=nn)
    sel = np.arange(nn) if nodes is None else np.nonzero(nodes)[0]
    if nodes is not None:
        code = code[nodes[flat[order]]]
    ptr = np.concatenate([[0], np.cumsum(count[sel])])
    if ordered and len(sel):
        perm = np.argsort(count[sel], kind="stable")
        n = count[sel][perm]
        new = np.concatenate([[0], np.cumsum(n)])
        code = code[np.repeat(ptr[:-1][perm] - new[:-1], n) + np.arange(new[-1])]
        sel, ptr = sel[perm], new
    return sel, L.as_i64(ptr), L.as_i32(code)


def mask_of(fields):
    """the fields_mask of a tuple of names out of "u", "b", "p" """
    if isinstance(fields, str):
        fields = (fields,)
    fields = tuple(fields)
    bad = [f for f in fields if f not in FIELDS]
    if bad or not fields:
        raise ValueError(f"NodalFields: fields must be a non-empty choice of {tuple(FIELDS)}, got {fields!r}")
    mask = 0
    for f in fields:
        mask |= FIELDS[f]
    return mask


def channels_of(mask):
    """(the channel of the full layout 0..16 behind every row of a compute with this mask)"""
    ch = []
    if mask & L.NPG_NODAL_U:
        ch += list(range(0, 9))
    if mask & L.NPG_NODAL_B:
        ch += list(range(9, 12))
    if mask & L.NPG_NODAL_P:
        ch += list(range(12, 15))
    return ch + [15, 16]


class NodalGradients:
    """What NodalFields.compute() returns, on all nn P2 nodes of the mesh; NaN at nodes outside the mask and in the fields not asked for:
      .grad_u (nn, 3, 3)  grad_u[n, a, j] = d u_a / d x_j        .grad_b (nn, 3)  grad b'        .grad_p (nn, 3)
      .weight (nn,)  W = the summed weights                      .valence (nn,)   the number of cells around the node
      .vorticity() (nn, 3)   .divergence() (nn,)
      .N2() = N2 + d_z b'    .alpha_bz() = alpha N2()    .pv(f=None) = f N2()  (f: a number, an array over the nodes or a function of the
      coordinates; default the model's params.f)    .closures() = (alpha*b_z, nu, kappa_v) by the formulas save_vtk writes
    `raw` (17, nn) holds the channels in the library's order."""

    def __init__(self, raw, model):
        self.raw = raw
        self._model = model
        self.grad_u = np.moveaxis(raw[0:9].reshape(3, 3, -1), -1, 0)
        self.grad_b = raw[9:12].T
        self.grad_p = raw[12:15].T
        self.weight, self.valence = raw[15], raw[16]

    def vorticity(self):
        g = self.grad_u
        return np.stack([g[:, 2, 1] - g[:, 1, 2], g[:, 0, 2] - g[:, 2, 0], g[:, 1, 0] - g[:, 0, 1]], axis=1)

    def divergence(self):
        g = self.grad_u
        return (g[:, 0, 0] + g[:, 1, 1]) + g[:, 2, 2]

    def N2(self):
        return float(self._model.params.N2) + self.grad_b[:, 2]

    def alpha_bz(self):
        return float(self._model.params.alpha) * self.N2()

    def pv(self, f=None):
        f = getattr(self._model.params, "f", None) if f is None else f
        if f is None:
            raise ValueError("NodalGradients.pv: the model's parameters have no Coriolis parameter f - pass f= (a number, an array over "
                             "the nodes or a function of the coordinates)")
        if callable(f):
            f = f(self._model.fe_data.mesh.node_coords)
        return np.asarray(f, dtype=np.float64) * self.N2()

    def closures(self):
        from .io import _closures_of
        return _closures_of(self._model, self.alpha_bz())


class NodalFields:
    """NodalFields(model, weight="volume", nodes=None, ordered=False): the gradients of the model's CURRENT state at the mesh's P2 nodes.

    weight: "volume" (a cell counts with its volume) or "count" (every cell counts 1: what save_vtk's closure fields use).  nodes: a bool
    mask over the mesh's P2 nodes (as TimeAverages takes it) - only these are computed and downloaded.
    `.compute(fields=("u", "b", "p"))` -> NodalGradients; the groups not asked for cost neither scratch nor download.
    `.compute_device(fields)` -> the raw DeviceVector [channel][nsel] (rows: `channels_of(mask_of(fields))`, columns: `.sel`) for
    consumers that stay on the device; it is the handle's own vector, overwritten by the next call with the same fields.
    `.sel` (nsel,) the node of every row, in mesh order (ordered=True sorts the rows by valence so that the lanes of a wave walk
    incidence lists of one length - kept for timing what that is worth: it measured slower; the results are the same bits), `.valence`
    (nsel,) in that order, `.max_valence`, `.nbytes` (device memory held).
    Refused, leaving the model untouched: embedded 2-D meshes, mesh-partitioned and replicated-distributed models (NotImplementedError);
    a mask of the wrong shape or dtype, an unknown weight or field name (ValueError)."""

    def __init__(self, model, weight="volume", nodes=None, ordered=False):
        _refuse(model)
        if weight not in WEIGHTS:
            raise ValueError(f"NodalFields: weight must be 'volume' or 'count', got {weight!r}")
        m = model.fe_data.mesh
        if nodes is not None:
            nodes = np.asarray(nodes)
            if nodes.shape != (m.nn,) or nodes.dtype != bool:
                raise ValueError(f"NodalFields: nodes must be a bool array of shape ({m.nn},), got {nodes.dtype} {nodes.shape}")
            nodes = nodes.copy()
        self.model, self.weighting, self.nodes, self.nn = model, weight, nodes, m.nn
        self.ctx = model.arch.ctx
        self.fe = device_fe(model.arch, model.fe_data)
        self.sel, ptr, inc = incidence_table(m.cell_nodes, m.nn, nodes, ordered)
        self._table = (ptr, inc)
        self.valence = np.diff(ptr)
        self.max_valence = int(self.valence.max(initial=0))
        self._out = {}
        self.h = None
        h = C.c_void_p()
        L.check(L.lib().npg_nodal_create(self.fe.h, len(self.sel), L.ptr(ptr), L.ptr(inc), WEIGHTS[weight], C.byref(h)))
        self.h = h

    def __del__(self):
        try:
            if self.h:
                L.lib().npg_nodal_destroy(self.h)
                self.h = None
        except Exception:
            pass

    @property
    def nbytes(self):
        s = C.c_int64()
        L.check(L.lib().npg_nodal_info(self.h, None, None, None, C.byref(s)))
        return 8 * s.value + sum(a.nbytes for a in self._table) + 8 * sum(v.n for v in self._out.values())

    def compute_device(self, fields=("u", "b", "p")):
        mask = mask_of(fields)
        if mask not in self._out:
            self._out[mask] = DeviceVector(self.ctx, len(channels_of(mask)) * len(self.sel))
        out = self._out[mask]
        L.check(L.lib().npg_nodal_compute(self.h, self.model.inversion.solver.x.h, self.model.b_vec.h, mask, out.h))
        return out

    def compute_raw(self, fields=("u", "b", "p")):
        """(17, nn): the library's channels in mesh node order, NaN where nothing was computed"""
        mask = mask_of(fields)
        ch = channels_of(mask)
        raw = np.full((L.NPG_NODAL_NCH, self.nn), np.nan)
        if len(self.sel):
            raw[np.ix_(ch, self.sel)] = self.compute_device(fields).to_host().reshape(len(ch), len(self.sel))
        return raw

    def compute(self, fields=("u", "b", "p")):
        return NodalGradients(self.compute_raw(fields), self.model)
