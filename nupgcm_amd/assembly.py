"""DeviceFE: the element-local assembly engine of one (FEData, GPU) pair - wraps the npg_fe_* entry points.

Replaces the Gridap `assemble_vector` / `assemble_matrix` call sites of the hot path (src/model.jl:271-273,
src/evolution.jl:257-258,277, src/inversion.jl:145,163-166,210) with HIP kernels; user closures (nu, kappa, f) are
evaluated by the host at the quadrature points once and shipped as tables, so the device never runs user code."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .architectures import DeviceCSR, DeviceVector


def eval_at_quad_points(mesh, v):
    """table (ncell, nq) of a coefficient given as a number or as a function of x (arrays (..., 3) -> (...))"""
    xq = mesh.quad_points()
    if callable(v):
        return np.ascontiguousarray(np.broadcast_to(np.asarray(v(xq), dtype=float), xq.shape[:2]))
    return np.full(xq.shape[:2], float(v))


# the LogSumExp parameters of the eddy closure (nu_eddy, src/inputs.jl:130-137): the one place the model's refresh (update_nu_eddy) and
# the linearised model's loads (tangent_eddy, tangent_eddy_adjoint: linearized.py passes them explicitly) take them from
EDDY_SMOOTHING, EDDY_NU_MIN = 10.0, 1.0


class DeviceFE:
    def __init__(self, ctx, fe_data):
        self.ctx, self.fe_data = ctx, fe_data
        m, s, t = fe_data.mesh, fe_data.spaces, fe_data.tables
        nloc_b = 10 if s.b_order == 2 else 4
        Nb, dNb = (m.N2, m.dN2) if s.b_order == 2 else (m.N1, m.dN1)
        self._keep = dict(
            G=L.as_f64(m.grad_lambda), wdet=L.as_f64(m.detJ), qw=L.as_f64(m.q_w), N2=L.as_f64(m.N2), dN2=L.as_f64(m.dN2),
            Nb=L.as_f64(Nb), dNb=L.as_f64(dNb), N1=L.as_f64(m.N1), cu=L.as_i32(t.cell_u), cp=L.as_i32(t.cell_p),
            cb=L.as_i32(t.cell_b), ud=L.as_f64(t.u_diri), bd=L.as_f64(t.b_diri))
        k = self._keep
        d = L.FeDesc(ncell=m.ncell, nq=len(m.q_w), nloc_b=nloc_b, grad_lambda=k["G"].ctypes.data,
                     wdet=k["wdet"].ctypes.data, qw=k["qw"].ctypes.data, N2=k["N2"].ctypes.data, dN2=k["dN2"].ctypes.data,
                     Nb=k["Nb"].ctypes.data, dNb=k["dNb"].ctypes.data, N1=k["N1"].ctypes.data, cell_u=k["cu"].ctypes.data,
                     cell_p=k["cp"].ctypes.data, cell_b=k["cb"].ctypes.data, u_diri=k["ud"].ctypes.data,
                     n_u_diri=k["ud"].size, b_diri=k["bd"].ctypes.data, n_b_diri=k["bd"].size,
                     n_inv=fe_data.dofs.nu + fe_data.dofs.np, n_b=fe_data.dofs.nb)
        h = C.c_void_p()
        L.check(L.lib().npg_fe_create(ctx.h, C.byref(d), C.byref(h)))
        self.h = h
        self._patterns = {}
        self._f_probe = None

    def __del__(self):
        try:
            if self.h:
                L.lib().npg_fe_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def set_precision(self, precision):
        """arithmetic of the element-local work: "fp64" (default, = Gridap) or "fp32" (mixed mode of configs[4]: fp32 local
        products, fp64 accumulation and solves) - npg_fe_set_precision"""
        code = {"fp64": L.NPG_FE_FP64, "fp32": L.NPG_FE_FP32}[precision]
        L.check(L.lib().npg_fe_set_precision(self.h, code))
        return self

    @property
    def precision(self):
        return "fp32" if L.lib().npg_fe_get_precision(self.h) == L.NPG_FE_FP32 else "fp64"

    def set_coeff(self, name, v):
        # the Coriolis table only ever changes through this call: setting the SAME function object again (every re-assembly of
        # the eddy closure does, src/inversion.jl:149-170) would re-evaluate it at every quadrature point on the host for
        # nothing - 0.4 s of the 0.6 s a re-assembly took at 3.9 M unknowns.  (nu / kappa tables are also rewritten on the
        # device by the closures, so they are always re-set.)
        # The skip is keyed on VALUES, not on the object: the function is sampled at a few fixed cells and the samples must equal
        # the ones taken when the table was built - a callable whose captured state changed (params.beta mutated, a lambda
        # closing over a params object) re-evaluates.  force=True (keyword of set_coeff_force) always re-evaluates.
        if name == "f" and callable(v) and getattr(self, "_f_src", None) is v and self._f_probe is not None:
            if np.array_equal(self._probe(v), self._f_probe):
                return
        tab = L.as_f64(eval_at_quad_points(self.fe_data.mesh, v))
        L.check(L.lib().npg_fe_set_coeff(self.h, name.encode(), L.ptr(tab)))
        if name == "f":
            self._f_src = v if callable(v) else None
            self._f_probe = self._probe(v) if callable(v) else None

    def _probe(self, fn):
        """the function at the quadrature points of up to 64 cells spread over the mesh (the table's own values there)"""
        if getattr(self, "_probe_x", None) is None:          # (the points are taken once: evaluating them all is what the skip saves)
            xq = self.fe_data.mesh.quad_points()
            self._probe_x = xq[np.linspace(0, len(xq) - 1, num=min(64, len(xq)), dtype=np.int64)].copy()
        return np.asarray(fn(self._probe_x), dtype=np.float64).copy()

    def new_matrix(self, kind, structural=False):
        """zero-valued DeviceCSR with the pattern of 'A', 'B' or 'b' (buoyancy-buoyancy)"""
        key = (kind, structural)
        if key not in self._patterns:
            fd = self.fe_data
            rp, ci, shape = {"A": fd.pattern_A, "B": fd.pattern_B}[kind](structural) if kind != "b" else fd.pattern_b()
            self._patterns[key] = DeviceCSR.from_pattern(self.ctx, shape[0], shape[1], rp, ci)
        return self._patterns[key].clone()       # the cached matrix only ever serves as the pattern owner

    def assemble(self, which, A: DeviceCSR, scale=1.0, full_stress=False, lift: DeviceVector = None):
        L.check(L.lib().npg_fe_assemble_matrix(self.h, which, float(scale), int(bool(full_stress)), A.h,
                                               None if lift is None else lift.h))
        return A

    def rhs_diff(self, N2, out: DeviceVector):
        L.check(L.lib().npg_fe_assemble_rhs_diff(self.h, float(N2), out.h))
        return out

    def advection_rhs(self, scheme, dt, N2, b, b_prev, x_inv, x_inv_prev, out):
        L.check(L.lib().npg_fe_advection_rhs(self.h, scheme, float(dt), float(N2), b.h, b_prev.h, x_inv.h, x_inv_prev.h,
                                             out.h))
        return out

    def tangent_rhs(self, N2, b_base, x_base, db, dx, out):
        """out_i = int (u_base . grad db + du . grad b_base + du_z N2) phi_i: the tangent of the advection load (npg_fe_tangent_rhs);
        the base state carries the engine's Dirichlet values, the perturbation none"""
        L.check(L.lib().npg_fe_tangent_rhs(self.h, float(N2), b_base.h, x_base.h, db.h, dx.h, out.h))
        return out

    def tangent_adjoint(self, N2, b_base, x_base, lam, out_b, out_x):
        """(out_b, out_x) with <lam, tangent_rhs(db, dx)> = <out_b, db> + <out_x, dx>: the adjoint of the tangent load at the same
        base state (npg_fe_tangent_adjoint); the pressure rows of out_x are 0"""
        L.check(L.lib().npg_fe_tangent_adjoint(self.h, float(N2), b_base.h, x_base.h, lam.h, out_b.h, out_x.h))
        return out_b, out_x

    def tangent_diffusion(self, kappa_c, N2min, alpha, N2, b_base, db, out):
        """out = D_v db: the derivative of the vertical diffusion with the convection closure at b_base, over the background kappa_v
        (npg_fe_tangent_diffusion); kappa_c = 0 gives the background K_v product"""
        L.check(L.lib().npg_fe_tangent_diffusion(self.h, float(kappa_c), float(N2min), float(alpha), float(N2), b_base.h, db.h, out.h))
        return out

    def tangent_eddy(self, a2e2, full_stress, N2min, alpha, N2, b_base, x_base, db, out_x, smoothing=EDDY_SMOOTHING, nu_min=EDDY_NU_MIN):
        """out_x = r_x(db) = -(dA/dnu)[nu'(s) alpha d_z db] x_base: what the eddy closure adds to the right-hand side of the tangent
        inversion (npg_fe_tangent_eddy); the pressure rows are 0"""
        L.check(L.lib().npg_fe_tangent_eddy(self.h, float(a2e2), int(bool(full_stress)), float(N2min), float(alpha), float(N2),
                                            float(smoothing), float(nu_min), b_base.h, x_base.h, db.h, out_x.h))
        return out_x

    def tangent_eddy_adjoint(self, a2e2, full_stress, N2min, alpha, N2, b_base, x_base, mu, out_b, smoothing=EDDY_SMOOTHING, nu_min=EDDY_NU_MIN):
        """out_b = g(mu) with <mu, tangent_eddy(db)> = <out_b, db> (npg_fe_tangent_eddy_adjoint)"""
        L.check(L.lib().npg_fe_tangent_eddy_adjoint(self.h, float(a2e2), int(bool(full_stress)), float(N2min), float(alpha), float(N2),
                                                    float(smoothing), float(nu_min), b_base.h, x_base.h, mu.h, out_b.h))
        return out_b

    def get_coeff(self, name):
        """the coefficient table `name` as it stands, (ncell, nq): the read-back of set_coeff (npg_fe_get_coeff)"""
        out = np.empty(self.fe_data.mesh.quad_points().shape[:2], dtype=np.float64)
        L.check(L.lib().npg_fe_get_coeff(self.h, name.encode(), L.ptr(out)))
        return out

    def evolution_rhs(self, scheme, dt, N2, theta, b, b_prev, x_inv, x_inv_prev, rhs_diff, rhs_flux, rhs_M, rhs_h, rhs_v,
                      y):
        hh = [None if v is None else v.h for v in (rhs_diff, rhs_flux, rhs_M, rhs_h, rhs_v)]
        L.check(L.lib().npg_fe_evolution_rhs(self.h, scheme, float(dt), float(N2), float(theta), b.h, b_prev.h, x_inv.h,
                                             x_inv_prev.h, *hh, y.h))
        return y

    def update_kappa_convection(self, kappa_c, N2min, alpha, N2, b):
        L.check(L.lib().npg_fe_update_kappa_convection(self.h, None, float(kappa_c), float(N2min), float(alpha),
                                                       float(N2), b.h))

    def update_nu_eddy(self, N2min, alpha, N2, b, smoothing=EDDY_SMOOTHING, nu_min=EDDY_NU_MIN):
        L.check(L.lib().npg_fe_update_nu_eddy(self.h, float(N2min), float(alpha), float(N2), float(smoothing),
                                              float(nu_min), b.h))

    def restrict_coeff(self, fine: "DeviceFE", name="nu"):
        """this (coarse) engine's coefficient table <- the child-volume average of `fine`'s (npg_fe_restrict_coeff)"""
        L.check(L.lib().npg_fe_restrict_coeff(self.h, fine.h, name.encode()))

    def coeff_cell_mean(self, name, out: DeviceVector):
        """out[c] = quadrature mean of coefficient `name` over cell c (npg_fe_coeff_cell_mean)"""
        L.check(L.lib().npg_fe_coeff_cell_mean(self.h, name.encode(), out.h))
        return out

    def cfl_ratio(self, x_inv, u_min=0.01, h_cells=None):
        out = C.c_double()
        hc = None if h_cells is None else L.as_f64(h_cells)
        L.check(L.lib().npg_fe_cfl_ratio(self.h, None if hc is None else L.ptr(hc), float(u_min), x_inv.h,
                                         C.byref(out)))
        return out.value
