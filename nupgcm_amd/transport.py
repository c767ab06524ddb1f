"""The tracers' transport operator as a matrix (npg_tracers_transport_*): equilibria and implicit-advection steps of the
passive tracers with a frozen or mean flow.  The reference has no counterpart.

With kappa^ = alpha^2 eps^2 / mu_rho (evolution_parameter without dt), the tracer Gamma z + c and c_D the FE function of its Dirichlet
values,

    C_ij  = sum_{cells, q} W phi_i ( u . grad phi_j )                                   u(q) = scale sum_a N2[q][a] u_a
    T_k   = C + kappa^ (Kh + Kv) + lambda_k M                                           free rows and columns, buoyancy pattern
    g_k,i = int ( S_k - u_z Gamma_k - u . grad c_D,k - lambda_k c_D,k ) phi_i
            - kappa^ int ( kappa_h grad_h c_D,k . grad_h phi_i + kappa_v d_z c_D,k d_z phi_i ) + kappa^ Gamma_k rhs_diff1_i + flux_k,i
    equilibrium:    T_k c = g_k                                                         Jacobi-preconditioned restarted GMRES
    implicit step:  (M + cdt T_k) c^{n+1} = M (c1 c^n + c2 c^{n-1}) + cdt g_k           the constants of the model's BDF schemes

PassiveTracers steps a tracer with the running model and every advective term explicit; an ideal age or a dye's steady plume is 10^5
or more such steps away.  Here the flow is frozen (the model's current [u; p], or a mean from TimeAverages.mean_state()[0]), the
advection is a matrix, and the steady state is one linear solve per tracer.  The Galerkin operator is not stabilised: set_flow refuses
a flow so strong for the mesh that a diagonal entry of T_k is not positive, and peclet() reports the cell Peclet numbers."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .architectures import DeviceVector
from .assembly import eval_at_quad_points
from .iterative_solvers import Diagonal, GmresWorkspace
from .tracers import PassiveTracers


class TracerTransport:
    """TracerTransport(model, tracers, flow=None, scale=1.0, decay=None, memory=30): `tracers` as PassiveTracers takes them, `decay` one
    rate lambda_k >= 0 per tracer (default 0), `flow` a [u; p] DeviceVector (default: model.inversion.solver.x).  The operator is
    frozen: it holds the engine's Kh, Kv and kappa tables as they are at set_flow().  `c`, `c_prev` are stacked device vectors (tracer k
    at k * n_b); `stats[k]` and `residual[k] = (||P r||, ||P r0||)` describe the last equilibrium() of tracer k.
    Creating or using one changes nothing else: u, p, b' and an attached PassiveTracers keep their bits."""

    def __init__(self, model, tracers, flow=None, scale=1.0, decay=None, memory=30, isoneutral=None):
        if isoneutral is not None:
            raise NotImplementedError("TracerTransport: isoneutral= is not supported: a frozen K_iso and its lift are not built")
        if getattr(model, "comm", None) is not None or getattr(model, "layout", None) is not None \
                or getattr(model.arch.ctx, "nranks", 1) > 1:
            raise NotImplementedError("TracerTransport: distributed and mesh-partitioned models are not supported")
        if model.evolution is None:
            raise ValueError("TracerTransport: the model has no EvolutionToolkit")
        self.model = model
        # the handle, the Dirichlet values, Gamma, S, the initial values and the flux loads: PassiveTracers' own set-up, not attached
        tr = self._tr = PassiveTracers(model, tracers)
        self.h, self.fe, self.ctx = tr.h, tr.fe, tr.ctx
        self.names, self.specs, self.ntracer, self.nb = tr.names, tr.specs, tr.ntracer, tr.nb
        K, nb = self.ntracer, self.nb
        self.decay = np.zeros(K) if decay is None else np.array(decay, dtype=float).reshape(-1)
        if self.decay.shape != (K,):
            raise ValueError(f"TracerTransport: decay must hold one rate per tracer ({K}), got {self.decay.shape}")
        if not (np.isfinite(self.decay).all() and (self.decay >= 0).all()):
            raise ValueError(f"TracerTransport: decay rates must be finite and >= 0, got {self.decay}")
        p = model.params
        self.kappa_hat = p.alpha ** 2 * p.eps ** 2 / p.mu_rho
        self.memory = int(memory)
        self.c, self.c_prev, self.flux = tr.c, tr.c_prev, tr.flux
        self.g = DeviceVector(self.ctx, K * nb)
        self.y = DeviceVector(self.ctx, K * nb)
        self.r = DeviceVector(self.ctx, nb)
        self.rhs_diff1 = DeviceVector(self.ctx, nb) if np.any(tr.gamma != 0.0) else None
        self.C = self.fe.new_matrix("b")
        self._T, self._P, self._A = {}, {}, {}
        self.ws = GmresWorkspace(self.ctx, nb, self.memory)
        self.ws.set_basis(64)
        self.stats, self.residual = [None] * K, [None] * K
        self.flow, self.scale = None, float(scale)
        self.set_flow(flow, scale)

    # ---- the operator ---------------------------------------------------------------------------------------------------------------
    def set_flow(self, x_inv=None, scale=1.0):
        """velocity tables -> C -> T = C + kappa^ (Kh + Kv) (+ lambda_k M) with their Jacobi vectors -> the K loads.  ValueError when a
        T_k has a non-positive diagonal entry (the flow is too strong for this mesh)."""
        ev, lib = self.model.evolution, L.lib()
        x = x_inv if x_inv is not None else (self.flow if self.flow is not None else self.model.inversion.solver.x)
        L.check(lib.npg_tracers_transport_update(self.h, x.h, float(scale)))
        self.flow, self.scale = x, float(scale)
        L.check(lib.npg_tracers_transport_matrix(self.h, self.C.h))
        self._T, self._P, self._A = {}, {}, {}
        for lam in sorted(set(self.decay.tolist())):
            T = self.fe.new_matrix("b").combine(1.0, self.C, self.kappa_hat, ev.Kh, ev.Kv)
            if lam != 0.0:
                T.axpy(lam, ev.M)
            P = Diagonal(T.inv_diag())
            d = P.diag.to_host()
            if not (np.isfinite(d).all() and (d > 0).all()):
                with np.errstate(divide="ignore", invalid="ignore"):
                    worst = float(np.nanmin(np.where(np.isfinite(d) & (d != 0), 1.0 / d, 0.0)))
                self._T, self._P = {}, {}                   # (no operator until a set_flow succeeds)
                raise ValueError(f"TracerTransport.set_flow: T has a non-positive diagonal entry (smallest {worst:.3e}) at scale {scale:g}, "
                                 f"decay {lam:g}: the flow is too strong for this mesh (largest cell Peclet number "
                                 f"{self.peclet().max():.3e})")
            self._T[lam], self._P[lam] = T, P
        if self.rhs_diff1 is not None:
            self.fe.rhs_diff(1.0, self.rhs_diff1)
        dec = L.as_f64(self.decay)
        L.check(lib.npg_tracers_transport_load(self.h, self.kappa_hat, L.ptr(dec), None if self.rhs_diff1 is None else self.rhs_diff1.h,
                                               None if self.flux is None else self.flux.h, self.g.h))
        return self

    def tables(self):
        """(ux, uy, uz) of the last set_flow on the host, (ncell, nq) each"""
        m = self.model.fe_data.mesh
        out = [np.empty((len(m.q_w), m.ncell)) for _ in range(3)]
        L.check(L.lib().npg_tracers_transport_tables(self.h, *(L.ptr(a) for a in out)))
        return tuple(np.ascontiguousarray(a.T) for a in out)

    def info(self):
        """dict(state, umax) of the velocity tables (state: L.NPG_TRANSPORT_OFF / _UPDATED)"""
        st, um = C.c_int(), C.c_double()
        L.check(L.lib().npg_tracers_transport_info(self.h, C.byref(st), C.byref(um)))
        return dict(state=st.value, umax=um.value)

    def peclet(self):
        """per cell, the maximum over the quadrature points of |u| h / (kappa^ kappa_h), h the cell's longest edge"""
        m = self.model.fe_data.mesh
        ux, uy, uz = self.tables()
        X = m.coords[m.cells]
        h = np.linalg.norm(X[:, :, None, :] - X[:, None, :, :], axis=-1).max(axis=(1, 2))
        kh = eval_at_quad_points(m, self.model.forcings.kappa_h)
        return (np.sqrt(ux ** 2 + uy ** 2 + uz ** 2) * h[:, None] / (self.kappa_hat * kh)).max(axis=1)

    def index(self, k):
        return self.names.index(k) if isinstance(k, str) else int(k)

    def operator(self, k):
        return self._T[float(self.decay[self.index(k)])]

    def load(self, k):
        k = self.index(k)
        return self.g.view(k * self.nb, self.nb)

    def view(self, k, which="c"):
        k = self.index(k)
        return getattr(self, which).view(k * self.nb, self.nb)

    def values(self, k):
        """tracer k (index or name) on the host, free values in native order - as PassiveTracers.values"""
        return self.view(k).to_host(self.model.fe_data.dofs.inv_p_b)

    # ---- equilibrium ------------------------------------------------------------------------------------------------------------------
    def _pnorm(self, P, r):
        self.y.view(0, self.nb).mul(P.diag, r)
        return self.y.view(0, self.nb).norm()

    def equilibrium(self, atol=0.0, rtol=1e-8, itmax=0, guess=None, max_passes=3):
        """T_k c = g_k for every tracer: Jacobi-preconditioned GMRES(memory) warm-started from `guess` (stacked, K n_b) or the current c;
        the true residual g - T c is formed after each solve and the solver is re-entered, warm-started, while
        ||P r|| > atol + rtol ||P r0||, for at most max_passes passes."""
        fed = self.model.fe_data
        if not np.any(fed.tables.b_pos < 0):
            for k in range(self.ntracer):
                if self.decay[k] == 0.0:
                    raise ValueError(f"TracerTransport.equilibrium: tracer '{self.names[k]}' has no decay on a mesh without buoyancy Dirichlet "
                                     "nodes: the problem is singular")
        if guess is not None:
            self.c.copy_from(guess)
        nb = self.nb
        for k in range(self.ntracer):
            T, P = self.operator(k), self._P[float(self.decay[k])]
            g, c = self.load(k), self.view(k)
            self.r.copy_from(g)
            T.mul(c, self.r, alpha=-1.0, beta=1.0)
            r0 = self._pnorm(P, self.r)
            target = atol + rtol * r0
            total = None
            for passes in range(1, max(1, int(max_passes)) + 1):
                # (the solver's own relative test is against the residual it starts from: hand it the absolute target)
                st = self.ws.solve(T, g, c, P, atol=target, rtol=0.0, itmax=itmax)
                total = dict(st, niter=st["niter"] + (total["niter"] if total else 0))
                self.r.copy_from(g)
                T.mul(c, self.r, alpha=-1.0, beta=1.0)
                rn = self._pnorm(P, self.r)
                if rn <= target:
                    break
            total["solved"] = int(bool(total["solved"]) and rn <= target)
            total["passes"] = passes
            self.stats[k], self.residual[k] = total, (rn, r0)
        return self

    # ---- implicit steps with the frozen flow ------------------------------------------------------------------------------------------------
    def step_system(self, k, dt, scheme="BDF1"):
        """(A_k, P_k, cdt, c1, c2) of an implicit step: A_k = M + cdt T_k and its Jacobi vector, cached per (cdt, lambda_k)"""
        if scheme not in ("BDF1", "BDF2"):
            raise ValueError(f"TracerTransport.step: scheme must be 'BDF1' or 'BDF2', got {scheme!r}")
        c1, c2, cdt = (4.0 / 3.0, -1.0 / 3.0, 2.0 / 3.0 * dt) if scheme == "BDF2" else (1.0, 0.0, float(dt))
        lam = float(self.decay[self.index(k)])
        if (cdt, lam) not in self._A:
            A = self.model.evolution.M.clone().axpy(cdt, self._T[lam])
            self._A[(cdt, lam)] = (A, Diagonal(A.inv_diag()))
        A, P = self._A[(cdt, lam)]
        return A, P, cdt, c1, c2

    def step(self, dt, scheme="BDF1", atol=0.0, rtol=1e-10, itmax=0):
        """(M + cdt T_k) c^{n+1} = M (c1 c^n + c2 c^{n-1}) + cdt g_k for every tracer, then c_prev <- c^n"""
        nb, M = self.nb, self.model.evolution.M
        old = self.c.copy()
        self.step_stats = []
        for k in range(self.ntracer):
            A, P, cdt, c1, c2 = self.step_system(k, dt, scheme)
            c, cp, g, y = self.view(k), self.view(k, "c_prev"), self.load(k), self.y.view(k * nb, nb)
            self.r.lincomb([c1, c2], [c, cp])
            y.copy_from(g)
            M.mul(self.r, y, alpha=1.0, beta=cdt)
            self.step_stats.append(self.ws.solve(A, y, c, P, atol=atol, rtol=rtol, itmax=itmax))
        self.c_prev.copy_from(old)
        return self
