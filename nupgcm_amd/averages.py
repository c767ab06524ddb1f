"""Time means and eddy covariances of the running state, accumulated on the device (npg_tavg_*).  Every other diagnostic
reads the instantaneous state; with a time-dependent forcing the annual mean, a monthly climatology, the eddy buoyancy flux <u'b'>, the
eddy kinetic energy and the buoyancy variance need every step - and a download of [u; p] and b per step puts a synchronisation and a
host pass into a loop that otherwise never leaves the device.

TimeAverages(model, ...) is set as `model.averages`; run() calls accumulate(model, t_{n+1}, dt) once per step, after the blow-up guard.
Opt-in like model.tracers and model.surface_forcing: a model without one computes what it always did.

The recurrence is the weighted running mean and co-moments of West / Welford, fixed so that the result is testable to the bit: per
accumulator set (a "bin": W = 0, mu = 0, C = 0) and per sample of weight w > 0 the host forms W' = W + w, r = w / W', q = w (W / W')
in fp64 and the device does, with the OLD means,  delta_a = a - mu_a;  C_ab += (q delta_a) delta_b;  mu_a += r delta_a.
Covariance = C / W, eddy flux <u'b'> = C_ub / W, EKE = (C_uu + C_vv + C_ww) / 2W.  The means are whole vectors in the solvers' own DoF
order: a mean state is an ordinary pair of device vectors that every existing diagnostic can read (`applied`).  The co-moments live on
the P2 mesh nodes; a Dirichlet DoF is constant in time (delta = 0), a mid-node of a P1 buoyancy takes half the sum of its edge's
vertices.  Pressure has a mean only.

Out of scope: tracer concentrations, pressure covariances, third moments, a sliding window, and the partitioned layouts (a later change
gives every rank its owned nodes)."""
from __future__ import annotations

import contextlib
import ctypes as C
import math

import numpy as np

from . import _lib as L
from .architectures import DeviceVector

PAIRS = ("uu", "uv", "uw", "vv", "vw", "ww", "ub", "vb", "wb", "bb")
_PA = (0, 0, 0, 1, 1, 2, 0, 1, 2, 3)
_PB = (0, 1, 2, 1, 2, 2, 3, 3, 3, 3)


def node_table(fe_data, nodes=None, ordered=True):
    """(node ids, iu (3, n), ib (2, n)) of the selected P2 mesh nodes: the positions of a node's velocity components in x_inv and two
    positions in b (equal for a P2 node or a vertex; the edge's vertices for a mid-node of a P1 buoyancy); -1 = Dirichlet.
    ordered: by the position of the node's first free velocity DoF in x_inv - a wave of consecutive table rows then gathers
    neighbouring entries (DoFHandler keeps a node's components adjacent); nodes without one come last, by buoyancy position."""
    m, t = fe_data.mesh, fe_data.tables
    sel = np.arange(m.nn) if nodes is None else np.nonzero(nodes)[0]
    iu = np.asarray(t.u_pos, dtype=np.int64)[sel].T                                         # (3, n)
    if fe_data.spaces.b_order == 2:
        ib = np.stack([t.b_pos[sel], t.b_pos[sel]])
    else:
        ends = np.where((sel < m.nv)[:, None], np.stack([sel, sel], axis=1), m.edges[np.maximum(sel - m.nv, 0)])
        ib = t.b_pos[ends].T                                                                # (2, n)
    if ordered and len(sel):
        free = iu >= 0
        first = np.where(free.any(axis=0), iu[free.argmax(axis=0), np.arange(len(sel))], np.iinfo(np.int64).max)
        order = np.lexsort((ib[0], first))
        sel, iu, ib = sel[order], iu[:, order], ib[:, order]
    return sel, L.as_i32(iu), L.as_i32(ib)


def phase_bin(t, phases, period, t0=0.0):
    """the climatology's bin of time t: min(P - 1, floor(P (((t - t0) mod T) / T))), in fp64"""
    if phases == 1:
        return 0
    return min(phases - 1, int(math.floor(phases * (((float(t) - t0) % period) / period))))


class Covariance:
    """co-moments over the weight on the mesh's P2 nodes (NaN at nodes outside the mask): .uu .uv .uw .vv .vw .ww .ub .vb .wb .bb,
    .eddy_flux (nnode, 3) = <u'b'>, .eke = (uu + vv + ww) / 2, .b_variance = bb; .weight = W"""

    def __init__(self, comom, weight, sel, nn):
        self.weight = float(weight)
        for k, name in enumerate(PAIRS):
            full = np.full(nn, np.nan)
            if self.weight > 0.0:
                full[sel] = comom[k] / self.weight
            setattr(self, name, full)
        self.eddy_flux = np.stack([self.ub, self.vb, self.wb], axis=1)
        self.eke = (self.uu + self.vv + self.ww) / 2.0
        self.b_variance = self.bb


class TimeAverages:
    """TimeAverages(model, covariances=True, phases=1, period=None, t0=0.0, weight="dt", every=1, nodes=None), set as `model.averages`.

    weight: "dt" - the level t_{n+1} is weighted by the dt of the step that produced it (what an adaptive BDF1 needs) - or "steps"
    (weight 1).  every = k samples every k-th call with the weights since the last sample summed.  phases = P with period = T keeps P
    independent bins, a climatology: the bin of time t is phase_bin(t, P, T, t0).  nodes: a bool mask over the mesh's P2 nodes that
    restricts the CO-MOMENTS to those nodes (the means are always whole vectors) - it bounds the memory of a phase-binned run.
    `.accumulate(model, t, dt)` is what run() calls.  `.weight(bin)`, `.mean_state(bin)` -> (x_inv, b) DeviceVectors in the solvers'
    order (one bin: the accumulators themselves - read them, do not write; bin=None over several bins: new vectors,
    sum_k (W_k / W) mu_k by npg_vec_lincomb), `.mean()` -> host u, p, b in native order as State gives them, `.covariance(bin)` ->
    Covariance (bins merged on the host by Chan's pairwise formula in fp64), `.applied(model, bin)`: a context in which the model's
    state vectors hold the mean flow, `.reset()`, `.save(path)`, `.load(path)`, `.nbytes` (device memory held), `.detach()`.
    Refused: mesh-partitioned and replicated-distributed models (NotImplementedError); a mask of the wrong shape, non-positive every,
    phases or period, phases > 1 without a period, a non-finite or negative weight (ValueError).  A failed constructor leaves the model
    as it was.  Embedded 2-D meshes work: nothing here depends on the cell shape.  ordered=False keeps the node table in mesh order
    (for timing what the ordering is worth; the results are the same bits)."""

    def __init__(self, model, covariances=True, phases=1, period=None, t0=0.0, weight="dt", every=1, nodes=None, ordered=True):
        _refuse_model(model)
        if weight not in ("dt", "steps"):
            raise ValueError(f"TimeAverages: weight must be 'dt' or 'steps', got {weight!r}")
        for name, v in (("every", every), ("phases", phases)):
            if isinstance(v, bool) or int(v) != v or int(v) < 1:
                raise ValueError(f"TimeAverages: {name} must be a positive integer, got {v!r}")
        if period is not None and not (math.isfinite(float(period)) and float(period) > 0.0):
            raise ValueError(f"TimeAverages: the period must be positive and finite, got {period!r}")
        if int(phases) > 1 and period is None:
            raise ValueError("TimeAverages: phases > 1 needs a period")
        if not math.isfinite(float(t0)):
            raise ValueError(f"TimeAverages: t0 must be finite, got {t0!r}")
        fed = model.fe_data
        nn = fed.mesh.nn
        if nodes is not None:
            nodes = np.asarray(nodes)
            if nodes.shape != (nn,) or nodes.dtype != bool:
                raise ValueError(f"TimeAverages: nodes must be a bool array of shape ({nn},), got {nodes.dtype} {nodes.shape}")
            nodes = nodes.copy()
        self.model = model
        self.ctx = model.arch.ctx
        self.covariances, self.phases, self.every, self.weighting = bool(covariances), int(phases), int(every), weight
        self.period, self.t0 = None if period is None else float(period), float(t0)
        self.nodes, self.nnode_mesh = nodes, nn
        self.n_inv, self.n_b = model.inversion.solver.x.n, model.b_vec.n
        self.sel, iu, ib = node_table(fed, nodes, ordered) if self.covariances else (np.zeros(0, dtype=np.int64), L.as_i32(np.zeros((3, 0))),
                                                                                     L.as_i32(np.zeros((2, 0))))
        self._table = (iu, ib)
        self.h = None
        h = C.c_void_p()
        L.check(L.lib().npg_tavg_create(self.ctx.h, self.n_inv, self.n_b, len(self.sel), L.ptr(iu), L.ptr(ib), C.byref(h)))
        self.h = h
        self.mean_x = [DeviceVector(self.ctx, self.n_inv) for _ in range(self.phases)]
        self.mean_b = [DeviceVector(self.ctx, self.n_b) for _ in range(self.phases)]
        self.comom = [DeviceVector(self.ctx, len(PAIRS) * len(self.sel)) if self.covariances else None for _ in range(self.phases)]
        self.reset()
        model.averages = self                    # from here on the model changes

    def __del__(self):
        try:
            if self.h:
                L.lib().npg_tavg_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def detach(self):
        if getattr(self.model, "averages", None) is self:
            self.model.averages = None
        return self

    def reset(self):
        """every bin back to W = 0, mu = 0, C = 0; the pending weight of `every` dropped"""
        for v in self.mean_x + self.mean_b + [c for c in self.comom if c is not None]:
            v.fill(0.0)
        self.W = np.zeros(self.phases)
        self.pending, self.calls, self.nsamples = 0.0, 0, 0
        return self

    @property
    def nbytes(self):
        vecs = self.mean_x + self.mean_b + [c for c in self.comom if c is not None]
        return 8 * sum(v.n for v in vecs) + sum(a.nbytes for a in self._table)

    # ---- accumulation ------------------------------------------------------------------------------------------------------------
    def bin_of(self, t):
        return phase_bin(t, self.phases, self.period, self.t0)

    def accumulate(self, model, t, dt):
        """fold the model's state, the level at time t reached by a step dt, into the bin of t"""
        w = float(dt) if self.weighting == "dt" else 1.0
        return self.add_sample(model.inversion.solver.x, model.b_vec, w, t)

    def add_sample(self, x_inv, b, w, t=0.0):
        """one call of the sampling rule with the state (x_inv, b), weight w and time t: every `every`-th call is a sample, carrying
        the weights since the last one"""
        w = float(w)
        if not (math.isfinite(w) and w >= 0.0):
            raise ValueError(f"TimeAverages: a weight must be finite and >= 0, got {w}")
        if not math.isfinite(float(t)):
            raise ValueError(f"TimeAverages: t must be finite, got {t}")
        self.pending += w
        self.calls += 1
        if self.calls % self.every != 0 or self.pending == 0.0:
            return self
        if not math.isfinite(self.pending):
            raise ValueError("TimeAverages: the summed weight is not finite")
        k = self.bin_of(t)
        W = float(self.W[k])
        W1 = W + self.pending
        r, q = self.pending / W1, self.pending * (W / W1)
        L.check(L.lib().npg_tavg_accumulate(self.h, r, q, x_inv.h, b.h, self.mean_x[k].h, self.mean_b[k].h,
                                            self.comom[k].h if self.covariances else None))
        self.W[k] = W1
        self.pending = 0.0
        self.nsamples += 1
        return self

    # ---- results -----------------------------------------------------------------------------------------------------------------
    def weight(self, bin=None):
        """W of one bin, or of all of them"""
        return float(self.W.sum()) if bin is None else float(self.W[self._bin(bin)])

    def _bin(self, bin):
        if not 0 <= int(bin) < self.phases:
            raise ValueError(f"TimeAverages: bin {bin} is outside the {self.phases} bins")
        return int(bin)

    def mean_state(self, bin=None):
        """(x_inv, b) of the time mean as DeviceVectors in the solvers' order"""
        if bin is not None or self.phases == 1:
            k = 0 if bin is None else self._bin(bin)
            return self.mean_x[k], self.mean_b[k]
        W = self.weight()
        live = [k for k in range(self.phases) if self.W[k] > 0.0]
        coef = [self.W[k] / W for k in live]
        return (_lincomb(self.ctx, self.n_inv, coef, [self.mean_x[k] for k in live]),
                _lincomb(self.ctx, self.n_b, coef, [self.mean_b[k] for k in live]))

    def mean(self, bin=None):
        """host (u, p, b) of the time mean in native order, as State gives the instantaneous ones"""
        d = self.model.fe_data.dofs
        x, b = self.mean_state(bin)
        xh = x.to_host(d.inv_p_inversion)
        return xh[:d.nu], xh[d.nu:], b.to_host(d.inv_p_b)

    def _node_means(self, k):
        """(4, nsel): the bin's means of u, v, w, b at the table's nodes, as far as they enter a delta (a Dirichlet DoF: 0)"""
        iu, ib = self._table
        x, b = self.mean_x[k].to_host(), self.mean_b[k].to_host()
        at = lambda a, i: np.where(i >= 0, a[np.maximum(i, 0)], 0.0) if len(a) else np.zeros(i.shape)
        return np.vstack([at(x, iu), np.where(ib[0] == ib[1], at(b, ib[0]), 0.5 * (at(b, ib[0]) + at(b, ib[1])))[None]])

    def covariance(self, bin=None):
        """Covariance of one bin, or (bin=None) of all bins merged pairwise:  C = C_A + C_B + (W_A W_B / W) dmu_a dmu_b"""
        if not self.covariances:
            raise ValueError("TimeAverages: created with covariances=False")
        nsel = len(self.sel)
        get = lambda k: self.comom[k].to_host().reshape(len(PAIRS), nsel)
        if bin is not None or self.phases == 1:
            k = 0 if bin is None else self._bin(bin)
            return Covariance(get(k), self.W[k], self.sel, self.nnode_mesh)
        Wa, Ca, Ma = 0.0, np.zeros((len(PAIRS), nsel)), np.zeros((4, nsel))
        for k in range(self.phases):
            Wb = float(self.W[k])
            if Wb == 0.0:
                continue
            Cb, Mb = get(k), self._node_means(k)
            W = Wa + Wb
            d = Mb - Ma
            f = Wa * (Wb / W)
            for p, (a, b) in enumerate(zip(_PA, _PB)):
                Ca[p] = Ca[p] + Cb[p] + (f * d[a]) * d[b]
            Ma = Ma + (Wb / W) * d
            Wa = W
        return Covariance(Ca, Wa, self.sel, self.nnode_mesh)

    @contextlib.contextmanager
    def applied(self, model=None, bin=None):
        """a context in which model.inversion.solver.x and model.b_vec hold the mean state: MeshIntegrals, GridDiagnostics,
        BuoyancyClasses, BuoyancySurfaces and the samplers see the mean flow.  On exit - also on an exception - the saved bits are
        restored.  Closure tables held by the engine (convective kappa_v, eddy nu) stay those of the CURRENT state."""
        model = self.model if model is None else model
        x, b = model.inversion.solver.x, model.b_vec
        mx, mb = self.mean_state(bin)
        saved = (x.copy(), b.copy())
        try:
            x.copy_from(mx)
            b.copy_from(mb)
            yield self
        finally:
            x.copy_from(saved[0])
            b.copy_from(saved[1])

    # ---- save / load -------------------------------------------------------------------------------------------------------------
    def _config(self):
        return dict(covariances=self.covariances, phases=self.phases, period=np.nan if self.period is None else self.period, t0=self.t0,
                    weighting=self.weighting, every=self.every, n_inv=self.n_inv, n_b=self.n_b)

    def save(self, path):
        """the configuration, W per bin, the means, the co-moments (table order, with the table's node ids) and the pending weight"""
        with open(path, "wb") as f:
            np.savez(f, W=self.W, pending=self.pending, calls=self.calls, nsamples=self.nsamples, sel=self.sel,
                     mean_x=np.stack([v.to_host() for v in self.mean_x]), mean_b=np.stack([v.to_host() for v in self.mean_b]),
                     comom=np.stack([c.to_host() for c in self.comom]) if self.covariances else np.zeros((self.phases, 0)),
                     **{"cfg_" + k: v for k, v in self._config().items()})
        return self

    def load(self, path):
        """take over the accumulators of a save() made with the same configuration: a run continued from here has the bits of the
        uninterrupted one"""
        with np.load(path) as z:
            for k, v in self._config().items():
                got = z["cfg_" + k][()]
                same = (isinstance(v, float) and math.isnan(v) and np.isnan(got)) or got == v
                if not same:
                    raise ValueError(f"TimeAverages.load: {path} was saved with {k} = {got}, this object has {v}")
            if not np.array_equal(z["sel"], self.sel):
                raise ValueError(f"TimeAverages.load: {path} was saved with another node mask")
            for k in range(self.phases):
                self.mean_x[k].upload(z["mean_x"][k])
                self.mean_b[k].upload(z["mean_b"][k])
                if self.covariances:
                    self.comom[k].upload(z["comom"][k])
            self.W = np.array(z["W"], dtype=np.float64)
            self.pending, self.calls, self.nsamples = float(z["pending"]), int(z["calls"]), int(z["nsamples"])
        return self


def _lincomb(ctx, n, coef, xs):
    """a new vector sum_k coef[k] xs[k]; npg_vec_lincomb takes eight terms, more are folded in groups"""
    out = DeviceVector(ctx, n)
    if not xs:
        return out.fill(0.0)
    if len(xs) <= 8:
        return out.lincomb(coef, xs)
    parts = [_lincomb(ctx, n, coef[i:i + 8], xs[i:i + 8]) for i in range(0, len(xs), 8)]
    return _lincomb(ctx, n, [1.0] * len(parts), parts)


def _refuse_model(model):
    if getattr(model, "layout", None) is not None and (hasattr(model.layout, "cell_owner") or hasattr(model.layout, "locator_cells")):
        raise NotImplementedError("TimeAverages on a mesh-partitioned model is not implemented (every rank would accumulate the nodes "
                                  "it owns): average a single-device model")
    if getattr(model, "partition", None) is not None or getattr(model, "comm", None) is not None \
            or getattr(model.arch.ctx, "nranks", 1) > 1:
        raise NotImplementedError("TimeAverages of the replicated distributed layout is not implemented: use a single-device model")
