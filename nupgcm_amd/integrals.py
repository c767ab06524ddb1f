"""Energy and buoyancy budgets: the quadrature integrals of the device-resident state over the mesh (npg_integrals_compute,
DESIGN.md 15) - domain volume, mean and variance of b', kinetic energy, buoyancy production, viscous dissipation, potential energy,
advective tendency, diffusive variance destruction and flux, the L2 norm of div u.  The reference has no counterpart: its run log
prints maxima and its post-processing stops at streamfunctions.

One pass over the cells with the engine's own quadrature rule, NPG_NINT = 15 raw channels, one download of 15 doubles per call.  The
integrals are EXACT for the finite-element fields (the rule integrates degree 4), so the discrete identities hold to rounding:

    alpha^2 eps^2 ch6 (ch7 in the full-stress form) = x' A x          (Coriolis and the u-p / p-u blocks are skew)
    ch5 / alpha                                     = x_u' (B b + lift)
    ch2 = b' M b,   ch11 = b' (Kh + Kv) b           (no Dirichlet b)

and, for a converged inversion without wind, dissipation = buoyancy production up to x' r with r the true residual."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .architectures import DeviceVector
from .inversion import device_fe

NINT = L.NPG_NINT
CHANNELS = ("one", "b", "b2", "ke_h", "ke_v", "w_b", "nu_grad_u2", "nu_2sigma2", "z_b", "u_grad_b", "w", "kappa_grad_b2", "kv_dz_b",
            "kv", "div_u2")


def _layout(model):
    """the RankLayout of a mesh-partitioned model (partition.PartitionedModel), else None; the replicated layout of distributed.py is
    refused, as sampling refuses it"""
    lay = getattr(model, "layout", None)
    if lay is not None and hasattr(lay, "cell_owner"):
        return lay
    if getattr(model, "partition", None) is not None or getattr(model, "comm", None) is not None \
            or getattr(model.arch.ctx, "nranks", 1) > 1:
        raise NotImplementedError("mesh integrals of the replicated distributed layout are not implemented: use the mesh-partitioned "
                                  "model (partition.partitioned_model) or a single-device model")
    return None


class Budgets:
    """What MeshIntegrals.compute() returns: `raw` (the NPG_NINT channels, numpy) and, with the model's parameters applied,
      volume                 ch0                                 b_mean       ch1 / V
      b_variance             ch2 / V - b_mean^2                  ke_h, ke_v   ch3, ch4
      buoyancy_production    ch5 / alpha                         dissipation  alpha^2 eps^2 ch6 (ch7: full-stress form)
      potential_energy       -(ch8 + N2 int z^2)                 advective_tendency   ch9
      variance_destruction   ch11                                diffusive_flux       N2 ch13 + ch12
      div2                   ch14"""

    def __init__(self, raw, params, full_stress, z2):
        self.raw = raw
        a, e, N2 = float(params.alpha), float(params.eps), float(params.N2)
        V = raw[0]
        self.volume = V
        self.b_mean = raw[1] / V if V else np.nan
        self.b_variance = raw[2] / V - self.b_mean ** 2 if V else np.nan
        self.ke_h, self.ke_v = raw[3], raw[4]
        self.buoyancy_production = raw[5] / a
        self.dissipation = a * a * e * e * (raw[7] if full_stress else raw[6])
        self.potential_energy = -(raw[8] + N2 * z2)
        self.advective_tendency = raw[9]
        self.variance_destruction = raw[11]
        self.diffusive_flux = N2 * raw[13] + raw[12]
        self.div2 = raw[14]

    def __repr__(self):
        keys = ("volume", "b_mean", "b_variance", "ke_h", "ke_v", "buoyancy_production", "dissipation", "potential_energy",
                "advective_tendency", "variance_destruction", "diffusive_flux", "div2")
        return "Budgets(" + ", ".join(f"{k}={getattr(self, k):.6e}" for k in keys) + ")"


class MeshIntegrals:
    """MeshIntegrals(model, mask=None): the integrals of the model's CURRENT state over its mesh (3-D and embedded 2-D).  The handle
    (npg_integrals) keeps the z of every cell's own vertices, the mask and the partial sums; `.compute()` runs one pass on the device
    and downloads NPG_NINT doubles - cheap enough for an on_plot hook (BudgetRecorder).  mask (ncell,) bool: only these cells count.
    Two calls on the same state return the same bits.
    On a partition.PartitionedModel construction and `compute()` are COLLECTIVE: every rank integrates the cells it owns
    (RankLayout.cell_owner == rank; an owned cell is always among the rank's engine cells - the assertion locator_cells makes) and
    the NPG_NINT sums are added over the ranks in rank order (npg_comm_allreduce_long: the same bits on every rank).  An owned cell
    reads DoFs other ranks own: the ghost values are current after every solve (PartitionedSolverToolkit.refresh_ghosts), which is
    what compute() relies on - call it after a solve or a run step, not on hand-written owned slices.  `mask` then is over the GLOBAL
    cells and is applied on top of the ownership."""

    def __init__(self, model, mask=None):
        self.model = model
        fed = model.fe_data
        m = fed.mesh
        self.layout = _layout(model)
        self.ctx = model.arch.ctx
        z = L.as_f64(m.geo_coords[m.cell_geo][:, :, 2])
        if z.shape[1] == 3:                    # embedded 2-D mesh: the device's fourth vertex (lambda_4 = 0) never weighs in
            z = L.as_f64(np.concatenate([z, np.zeros((len(z), 1))], axis=1))
        gmask = None if mask is None else np.asarray(mask, dtype=bool)
        if gmask is not None and gmask.shape != (m.ncell,):
            raise ValueError(f"MeshIntegrals: mask must have shape ({m.ncell},), got {gmask.shape}")
        if self.layout is not None:
            lay = self.layout
            own = lay.cell_owner == lay.rank
            assert np.isin(np.nonzero(own)[0], lay.cells, assume_unique=True).all(), "an owned cell is kept by no rank"
            self.fe = model.fe
            z = L.as_f64(z[lay.cells])
            cmask = own[lay.cells] if gmask is None else own[lay.cells] & gmask[lay.cells]
        else:
            self.fe = device_fe(model.arch, fed)
            cmask = gmask
        self.ncells_counted = int(len(z) if cmask is None else cmask.sum())         # this rank's share
        self._mask8 = None if cmask is None else np.ascontiguousarray(cmask, dtype=np.uint8)
        h = C.c_void_p()
        L.check(L.lib().npg_integrals_create(self.fe.h, L.ptr(z), None if self._mask8 is None else L.ptr(self._mask8), C.byref(h)))
        self.h = h
        self._out = DeviceVector(self.ctx, NINT)
        f = model.forcings
        self.full_stress = bool(callable(f.nu) or f.eddy_param.is_on)
        # int z^2 over the (masked) whole mesh, once, from the same rule: the background part of the potential energy
        k = m.cell_geo.shape[1]
        zq = np.einsum("qk,ck->cq", m.q_lam[:, :k], m.geo_coords[m.cell_geo][:, :, 2])
        t = (m.q_w[None, :] * m.detJ[:, None] * zq * zq).sum(axis=1)
        self.z2 = float(t.sum() if gmask is None else t[gmask].sum())

    def __del__(self):
        try:
            if self.h:
                L.lib().npg_integrals_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def compute_raw(self):
        """the NPG_NINT raw channels of the current state (numpy)"""
        m = self.model
        L.check(L.lib().npg_integrals_compute(self.h, m.inversion.solver.x.h, m.b_vec.h, int(self.full_stress), self._out.h))
        if self.layout is not None:
            L.check(L.lib().npg_comm_allreduce_long(self.ctx.h, self._out.h))      # summed in rank order
        return self._out.to_host()

    def compute(self) -> Budgets:
        return Budgets(self.compute_raw(), self.model.params, self.full_stress, self.z2)


class BudgetRecorder:
    """BudgetRecorder(model): an `on_plot(model, t)` hook (model.run calls it every n_plot steps) that appends (t, raw channels) per
    call.  `.as_arrays()` -> (t (n,), raw (n, NPG_NINT)); `.save(path)` writes them with np.savez (keys t, raw, channels).  The series
    is the caller's to difference: the library keeps no time derivatives.  Collective on a partitioned model (every rank records the
    same series)."""

    def __init__(self, model, mask=None):
        self.integrals = MeshIntegrals(model, mask)
        self.t, self.raw = [], []

    def __call__(self, model, t):
        self.t.append(float(t))
        self.raw.append(self.integrals.compute_raw())

    def as_arrays(self):
        return np.array(self.t, dtype=np.float64), np.array(self.raw, dtype=np.float64).reshape(len(self.raw), NINT)

    def budgets(self):
        """the recorded rows as Budgets"""
        I = self.integrals
        return [Budgets(r, I.model.params, I.full_stress, I.z2) for r in self.raw]

    def save(self, path):
        t, raw = self.as_arrays()
        np.savez(path, t=t, raw=raw, channels=np.array(CHANNELS))
