"""The model linearised about a frozen state: its tangent tendency as a matrix-free operator on the device, a
backward-Euler step of the tangent model, and the least-damped or growing eigenmodes of a circulation.

With fixed nu and kappa the weak-form tendency of the free buoyancy DoFs is

    M d_t b = F(b) = -adv(x(b), b) - c (Kh + Kv) b + c rhs_diff + rhs_flux - lifts,      c = alpha^2 eps^2 / mu_rho,

adv(x, b)_i = int (u . grad b + w N2) phi_i with the Dirichlet values of both fields, x(b) = A^-1 (B b + b0) the inversion - affine in
b, so F is exactly quadratic.  Its Jacobian at a base state (b_base, x_base) is

    J db = -T(b_base, x_base; db, L db) - c (Kh + Kv) db,      T_i = int (u_base . grad db + du . grad b_base + du_z N2) phi_i,

L db the solution of A dx = B db - no b0: neither wind nor Dirichlet lift.  T is npg_fe_tangent_rhs (csrc/linearized.hip,
csrc/tangent_core.h); every application of J costs one inversion.

LinearizedModel is PASSIVE: it owns its work vectors, its Krylov workspaces, its left-hand side and preconditioner; it reads the model's
A, P, B, M, Kh, Kv and writes nothing the model owns - u, p, b' and the solvers' warm starts keep their bits.

With the convection or the eddy closure on, kappa_v and nu depend on b and F is no longer quadratic.  closures="tangent"
differentiates them: -c (Kv b + rhs_v) + c rhs_diff = -(c / alpha) int kappa_v(s) s d_z phi_i with s = alpha (N2 + d_z b) has the
derivative -c D_v db, (D_v db)_i = int (kappa_v + s kappa_v') d_z db d_z phi_i (npg_fe_tangent_diffusion), and the inversion
A(nu(b)) x = B b + b0 the tangent A(nu_base) dx = B db + r_x(db), r_x = -(dA / dnu)[nu' alpha d_z db] x_base (npg_fe_tangent_eddy; its
adjoint g: npg_fe_tangent_eddy_adjoint), on an own copy of A assembled at nu(b_base):

    J db   = -T(b_base, x_base; db, dx) - c Kh db - c D_v db,      dx = A(nu_base)^-1 (B db + r_x(db))
    J' lam = -g_b - (B' y + g(y)) - c Kh lam - c D_v lam,           y = A(nu_base)^-T g_x .

closures="frozen" accepts such a model and uses its Kv and A as they stand: an operator of the same shape that is NOT the Jacobian
(on the golden bowl it misses 72 % of max |J db| with the convection closure on).

All solves inside use atol = 0 and the given rtol.  The model's own atol = 1e-6 is an absolute threshold on the 1/h^d-scaled residual: for
a small db it would accept dx = 0 and make the "linear" operator nonlinear."""
from __future__ import annotations

import numpy as np

from .architectures import CPU, DeviceCSR, DeviceVector
from .assembly import EDDY_NU_MIN, EDDY_SMOOTHING
from .averages import TimeAverages
from .evolution import collect_evolution_LHS_into, evolution_parameter
from .iterative_solvers import LU, CgWorkspace, Diagonal, GmresWorkspace, IterativeSolverToolkit, iterative_solve
from .timesteppers import BDF1


def _bdf1(dt):
    return BDF1(t_start=0.0, t_stop=float(dt), dt=float(dt))


class EigenModes:
    """What LinearizedModel.eigenmodes returns: `n` eigenpairs J v = sigma M v.

    sigma      complex (n,), sorted by descending real part
    vectors    complex (n, nb), native free-DoF order, each of unit M-norm (v^H M v = 1) with its largest entry real
    residuals  ||J v - sigma M v||_2 / (|sigma| ||M v||_2), recomputed with LinearizedModel.apply on the real and imaginary parts
               after convergence (not the Arnoldi estimate)
    converged  bool (n,): the residual is within the tolerance asked for
    n_applies, n_inversions, n_inner   applications of J, inversions and inner GMRES iterations the call spent
    dt         the shift-and-invert step: the modes are the ones nearest the shift 1 / dt
    side       "right" (J v = sigma M v) or "left" (J' w = sigma M w, i.e. w' J = sigma w' M - no conjugate; the residuals are then
               those of the transposed pencil, recomputed with LinearizedModel.apply_adjoint)"""

    def __init__(self, sigma, vectors, residuals, converged, n_applies, n_inversions, dt, n_inner=0, n_restarts=0, side="right"):
        if side not in ("left", "right"):
            raise ValueError(f"EigenModes: side must be 'left' or 'right', got {side!r}")
        self.side = side
        self.sigma = np.asarray(sigma, dtype=complex)
        self.vectors = np.asarray(vectors, dtype=complex)
        self.residuals = np.asarray(residuals, dtype=float)
        self.converged = np.asarray(converged, dtype=bool)
        self.n_applies, self.n_inversions, self.n_inner, self.n_restarts = int(n_applies), int(n_inversions), int(n_inner), int(n_restarts)
        self.dt = float(dt)

    def __len__(self):
        return len(self.sigma)

    def as_b(self, i, part="real"):
        """the real or imaginary part of mode i as free values in native order: what set_b (and, through it, save_vtk) accepts"""
        if part not in ("real", "imag"):
            raise ValueError(f"EigenModes.as_b: part must be 'real' or 'imag', got {part!r}")
        v = self.vectors[int(i)]
        return np.ascontiguousarray(v.real if part == "real" else v.imag)

    def save(self, path):
        np.savez(path, sigma=self.sigma, vectors=self.vectors, residuals=self.residuals, converged=self.converged,
                 counts=np.array([self.n_applies, self.n_inversions, self.n_inner, self.n_restarts], dtype=np.int64), dt=self.dt,
                 side=self.side)
        return path

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            c = z["counts"]
            side = str(z["side"]) if "side" in z.files else "right"          # a file from before the left modes
            return cls(z["sigma"], z["vectors"], z["residuals"], z["converged"], c[0], c[1], float(z["dt"]), c[2], c[3], side)

    def __repr__(self):
        return f"EigenModes: {len(self)} {self.side} modes nearest 1/dt = {1.0 / self.dt:.3e}, sigma = {self.sigma}"


class LinearizedModel:
    """LinearizedModel(model, base=None, rtol=1e-10, closures=None): the tangent model about a frozen base state.

    base = None: copies of the model's current b_vec and inversion.solver.x; a TimeAverages: copies of its means; a pair (b, x_inv) of
    DeviceVectors in the solvers' order: copies of them.  rtol: the relative tolerance of every solve inside (atol = 0).
    closures: what to do with a model whose convection or eddy closure is on.  None refuses it.  "frozen" uses the model's Kv and A as
    they stand and differentiates nothing - not the Jacobian.  "tangent" differentiates both closures: Kv.mul is replaced by
    npg_fe_tangent_diffusion (the preconditioner of implicit_step stays (M + dt c (Kh + Kv)) on the model's positive Kv); with the eddy
    closure an own A is assembled at nu(b_base) - the engine's nu table is read back and restored, bit for bit - with an own
    preconditioner of the model's kind (Diagonal is shared, CPU(): LU, the dense inverse is rebuilt, a multigrid handle is reused as it
    is), and x_base is solved once more under it so that the base state is consistent: counted in n_inversions - unless the given
    x_base already meets rtol under the own A (a base handed over from another LinearizedModel), in which case it stands, nothing is
    solved and nothing is counted.  kappa_eff =
    kappa_v + s kappa_v' is negative inside a steep tanh transition: the tangent operator may then have growing modes that the frozen
    one lacks, and implicit_step with dt beyond their growth time does not converge.  A model without closures runs the code it ran,
    whatever `closures` says."""

    def __init__(self, model, base=None, rtol=1e-10, closures=None):
        if closures not in (None, "frozen", "tangent"):
            raise ValueError(f"LinearizedModel: closures must be None, 'frozen' or 'tangent', got {closures!r}")
        if getattr(model, "comm", None) is not None or getattr(model, "layout", None) is not None \
                or getattr(model.arch.ctx, "nranks", 1) > 1 or hasattr(model.inversion.solver, "solve"):
            raise NotImplementedError("LinearizedModel: mesh-partitioned and distributed models are not supported")
        if model.evolution is None:
            raise ValueError("LinearizedModel: the model has no EvolutionToolkit")
        frc = model.forcings
        if (frc.conv_param.is_on or frc.eddy_param.is_on) and closures is None:
            raise NotImplementedError("LinearizedModel: the convection and eddy closures are not supported: their coefficients depend on b "
                                      "and are not differentiated (pass closures='tangent' to differentiate them, or closures='frozen' "
                                      "to keep the model's K_v and A as they stand)")
        if getattr(model, "surface_forcing", None) is not None or getattr(model, "interior_forcing", None) is not None:
            raise NotImplementedError("LinearizedModel: an attached surface_forcing or interior_forcing is not supported: their S / R "
                                      "matrices are not part of the tangent operator yet")
        if not (np.isfinite(rtol) and 0.0 < rtol < 1.0):
            raise ValueError(f"LinearizedModel: rtol must lie in (0, 1), got {rtol}")
        self.model, self.arch, self.ctx = model, model.arch, model.arch.ctx
        self.fe = model.evolution.fe
        self.rtol = float(rtol)
        d = model.fe_data.dofs
        self.nb, self.n_inv = d.nb, d.nu + d.np
        self.N2 = float(model.params.N2)
        self.c = evolution_parameter(model.params, _bdf1(1.0))
        if base is None:
            b, x = model.b_vec, model.inversion.solver.x
        elif isinstance(base, TimeAverages):
            x, b = base.mean_state()
        else:
            try:
                b, x = base
            except (TypeError, ValueError):
                raise TypeError("LinearizedModel: base must be None, a TimeAverages or a pair (b, x_inv) of DeviceVectors") from None
            if not (isinstance(b, DeviceVector) and isinstance(x, DeviceVector)):
                raise TypeError("LinearizedModel: base must be None, a TimeAverages or a pair (b, x_inv) of DeviceVectors")
        if len(b) != self.nb or len(x) != self.n_inv:
            raise ValueError(f"LinearizedModel: the base state must hold {self.nb} buoyancy and {self.n_inv} flow entries, "
                             f"got {len(b)} and {len(x)}")
        self.b_base, self.x_base = b.copy(), x.copy()
        self.closures = closures
        # the closures whose derivatives enter the operators (closures="tangent"); None: the coefficient is used as the model holds it
        self._conv = frc.conv_param if closures == "tangent" and frc.conv_param.is_on else None
        self._eddy = frc.eddy_param if closures == "tangent" and frc.eddy_param.is_on else None
        # a second solver on the model's A and P: its own x, y and workspace; the model's kwargs with atol = 0 and rtol
        ms = model.inversion.solver
        kw = dict(ms.kwargs)
        kw.update(atol=0.0, rtol=self.rtol)
        mem = getattr(ms.workspace, "memory", 20)
        A, P = ms.A, ms.P
        if self._eddy is not None:
            A, P = self._own_inversion_matrix(ms)
        self._A_plain = A if self._eddy is not None else None
        if isinstance(P, (Diagonal, LU)) or P is None:
            ws = GmresWorkspace(self.ctx, self.n_inv, memory=mem)
        else:
            from .multigrid import FgmresWorkspace
            ws = FgmresWorkspace(self.ctx, self.n_inv, memory=mem)
        self.inv_solver = IterativeSolverToolkit(A, P, DeviceVector(self.ctx, self.n_inv), ws, kw, "Linearised inversion")
        self.B = model.inversion.B
        ev = model.evolution
        self.M, self.Kh, self.Kv = ev.M, ev.Kh, ev.Kv
        self._dx = DeviceVector(self.ctx, self.n_inv)
        self._w = [DeviceVector(self.ctx, self.nb) for _ in range(4)]
        self._lhs_dt = None
        self._lhs = self._lhs_P = self._lhs_ws = self._lhs_y = None
        self._gm = None
        self.n_inversions = self.n_applies = self.n_inner = self.n_inversion_iterations = 0
        # the transposed inversion (A', B', their solver) and the adjoint's work vectors: built by the first adjoint call
        self.adj_solver = self.B_T = None
        self._adj = None
        self.n_adjoint_inversions = self.n_adjoint_applies = 0
        self._dv = None
        if self._eddy is not None:
            self._rx = DeviceVector(self.ctx, self.n_inv)
            self._solve_base_flow()

    # ---- the closures ----------------------------------------------------------------------------------------------------
    def _own_inversion_matrix(self, ms):
        """A at nu(b_base) in the full-stress form the model's own refresh assembles, into a matrix of this object's, and a
        preconditioner of the model's kind for it.  The engine's nu table is read back first and put back afterwards: the same bits."""
        from . import _lib as L
        from .inversion import assemble_A_inversion
        from .multigrid import DenseInversePreconditioner
        fe, prm, ep = self.fe, self.model.params, self._eddy
        keep = fe.get_coeff("nu")
        try:
            fe.update_nu_eddy(ep.N2min, prm.alpha, prm.N2, self.b_base, **self._eddy_kw())
            A = assemble_A_inversion(fe, prm, fe.new_matrix("A", structural=True), True)
        finally:
            L.check(L.lib().npg_fe_set_coeff(fe.h, b"nu", L.ptr(keep)))
        P = ms.P
        if isinstance(self.arch, CPU):
            P = LU(A)               # InversionToolkit picks Diagonal there when the eddy closure is on: every solve would factorise
        elif isinstance(P, DenseInversePreconditioner):
            P = DenseInversePreconditioner(self.arch, A, storage=P.storage)
        # Diagonal(1 / h^dim) does not depend on A; a multigrid handle is the model's as it is - inexact for A(nu(b_base)), behind FGMRES
        return A, P

    def _solve_base_flow(self):
        """x_base <- A(nu(b_base))^-1 (B b_base + b0) from the given x_base as a guess: the flow that belongs to b_base under the
        closure, which r_x and the tangent load are taken at.  Counted in n_inversions.

        The Krylov solvers stop relative to the residual they START from: a guess that is already the solution (a base state taken
        from another LinearizedModel) would ask them for rtol below rounding.  So the residual r of the guess is formed first; the
        guess stands when ||r|| <= rtol ||y||, and otherwise the correction A e = r is solved from zero down to rtol ||y||."""
        s = self.inv_solver
        s.y.copy_from(self.model.inversion.b)
        self.B.mul(self.b_base, s.y, alpha=1.0, beta=1.0)
        if isinstance(s.P, LU):
            iterative_solve(s)
            self.n_inversions += 1
            self.x_base.copy_from(s.x)
            return
        ynorm = s.y.norm()
        s.A.mul(self.x_base, s.y, alpha=-1.0, beta=1.0)
        rnorm = s.y.norm()
        if rnorm <= self.rtol * ynorm:
            return
        s.x.fill(0.0)
        keep = s.kwargs["rtol"]
        s.kwargs["rtol"] = min(0.5, self.rtol * ynorm / rnorm)
        try:
            iterative_solve(s)
        finally:
            s.kwargs["rtol"] = keep
        st = s.workspace.stats or {}
        if not st.get("solved", 1):
            raise RuntimeError(f"LinearizedModel: the inversion of the base state did not reach rtol = {self.rtol:g} (atol = 0): {st}")
        self.n_inversion_iterations += int(st.get("niter", 0))
        self.n_inversions += 1
        self.x_base.axpby(1.0, s.x, 1.0)

    def _eddy_args(self):
        prm, ep = self.model.params, self._eddy
        return prm.alpha ** 2 * prm.eps ** 2, True, ep.N2min, prm.alpha, self.N2

    @staticmethod
    def _eddy_kw():
        """the LogSumExp parameters, passed explicitly to the update behind the own A and to both loads: the model's (assembly.py)"""
        return dict(smoothing=EDDY_SMOOTHING, nu_min=EDDY_NU_MIN)

    def _vertical_diffusion(self, v, out):
        """out <- out - c D_v v: the model's K_v, or with closures="tangent" and convection on the derivative of kappa_v(b) d_z b"""
        if self._conv is None:
            self.Kv.mul(v, out, alpha=-self.c, beta=1.0)
        else:
            cp, prm = self._conv, self.model.params
            if self._dv is None:
                self._dv = DeviceVector(self.ctx, self.nb)
            self.fe.tangent_diffusion(cp.kappa_c, cp.N2min, prm.alpha, self.N2, self.b_base, v, self._dv)
            out.axpby(-self.c, self._dv, 1.0)
        return out

    # ---- the operator ---------------------------------------------------------------------------------------------------------------
    def invert(self, db: DeviceVector, dx: DeviceVector = None):
        """dx = L db: A dx = B db from a zero guess - no b0, hence no wind and no Dirichlet lift.  Returns dx (default: an own vector)."""
        s = self.inv_solver
        dx = self._dx if dx is None else dx
        if self._eddy is None:
            self.B.mul(db, s.y, alpha=1.0, beta=0.0)
        else:                       # A(nu_base) dx = B db + r_x(db): the derivative of nu moves the base flow
            self.fe.tangent_eddy(*self._eddy_args(), self.b_base, self.x_base, db, self._rx, **self._eddy_kw())
            s.y.copy_from(self._rx)
            self.B.mul(db, s.y, alpha=1.0, beta=1.0)
        s.x.fill(0.0)
        iterative_solve(s)
        st = s.workspace.stats or {}
        if not st.get("solved", 1):
            raise RuntimeError(f"LinearizedModel.invert: the inversion did not reach rtol = {self.rtol:g} (atol = 0): {st}")
        self.n_inversion_iterations += int(st.get("niter", 0))
        self.n_inversions += 1
        dx.copy_from(s.x)
        return dx

    def apply(self, db: DeviceVector, out: DeviceVector = None):
        """out = J db in weak form (the vectors hold free DoFs only: there are no Dirichlet rows to mask)"""
        out = DeviceVector(self.ctx, self.nb) if out is None else out
        if out is db:
            raise ValueError("LinearizedModel.apply: out must not be db")
        dx = self.invert(db)
        self.fe.tangent_rhs(self.N2, self.b_base, self.x_base, db, dx, out)
        self.Kh.mul(db, out, alpha=-self.c, beta=-1.0)
        self._vertical_diffusion(db, out)
        self.n_applies += 1
        return out

    # ---- the adjoint operator ------------------------------------------------------------------------------------------
    def _adjoint(self):
        """A', B' and a second solver on them, built once: own x, y and workspace, atol = 0 and the model's rtol; the preconditioner
        follows the model's - Diagonal is symmetric and serves as it is, LU and the dense inverse are rebuilt from A'"""
        if self._adj is not None:
            return self._adj
        from .multigrid import DenseInversePreconditioner, FgmresWorkspace
        ms = self.model.inversion.solver
        P = ms.P
        if not (P is None or isinstance(P, (Diagonal, LU, DenseInversePreconditioner))):
            raise NotImplementedError(f"LinearizedModel: the adjoint supports the inversion preconditioners Diagonal, LU and "
                                      f"DenseInversePreconditioner, not {type(P).__name__}: a transposed V-cycle is a follow-up")
        if self._A_plain is not None:
            A_csr = self._A_plain.to_scipy_csr()            # closures="tangent" with the eddy closure: the own A(nu(b_base))
        elif getattr(ms.A, "paired", False):
            # node records are an HBM layout that does not download as CSR: the same entries assembled once more into a plain
            # pattern, by the routine and the engine that assembled them (constant nu, Laplacian form: what InversionToolkit asks
            # of a matrix before it calls block_nodes), from the engine's tables as they stand
            from .inversion import assemble_A_inversion, device_fe
            frc = self.model.forcings
            if not getattr(self.model.inversion, "assembled_here", False) or callable(frc.nu) or frc.eddy_param.is_on:
                raise NotImplementedError("LinearizedModel: the adjoint cannot transpose an inversion matrix stored by node records "
                                          "unless InversionToolkit assembled it itself with a constant nu: pass a plain A")
            fe = device_fe(self.arch, self.model.fe_data)
            A_csr = assemble_A_inversion(fe, self.model.params, fe.new_matrix("A"), False).to_scipy_csr()
        else:
            A_csr = ms.A.to_scipy_csr()
        A_T = DeviceCSR.from_scipy(self.ctx, A_csr.T)           # (from_scipy reads CSC: the transpose of a CSR matrix as it stands)
        B_T = DeviceCSR.from_scipy(self.ctx, self.B.to_scipy_csr().T)
        mem = getattr(ms.workspace, "memory", 20)
        if isinstance(P, LU):
            P_T = LU(A_T)
        elif isinstance(P, DenseInversePreconditioner):
            P_T = DenseInversePreconditioner(self.arch, A_T, storage=P.storage)
        else:
            P_T = P
        ws = (FgmresWorkspace if isinstance(P, DenseInversePreconditioner) else GmresWorkspace)(self.ctx, self.n_inv, memory=mem)
        kw = dict(self.inv_solver.kwargs)
        solver = IterativeSolverToolkit(A_T, P_T, DeviceVector(self.ctx, self.n_inv), ws, kw, "Linearised adjoint inversion")
        self.adj_solver, self.B_T = solver, B_T
        self._adj = dict(gx=DeviceVector(self.ctx, self.n_inv), gb=DeviceVector(self.ctx, self.nb), ge=DeviceVector(self.ctx, self.nb))
        return self._adj

    def invert_adjoint(self, g_x: DeviceVector, out: DeviceVector = None):
        """out = B' A^-T g_x: A' y = g_x from a zero guess, then B' y.  Returns out (default: an own vector)."""
        adj = self._adjoint()
        s = self.adj_solver
        out = adj["gb"] if out is None else out
        s.y.copy_from(g_x)
        s.x.fill(0.0)
        iterative_solve(s)
        st = s.workspace.stats or {}
        if not st.get("solved", 1):
            raise RuntimeError(f"LinearizedModel.invert_adjoint: the transposed inversion did not reach rtol = {self.rtol:g} "
                               f"(atol = 0): {st}")
        self.n_inversion_iterations += int(st.get("niter", 0))
        self.n_inversions += 1
        self.n_adjoint_inversions += 1
        self.B_T.mul(s.x, out, alpha=1.0, beta=0.0)
        if self._eddy is not None:  # + g(y): the adjoint of db -> r_x(db)
            self.fe.tangent_eddy_adjoint(*self._eddy_args(), self.b_base, self.x_base, s.x, adj["ge"], **self._eddy_kw())
            out.axpby(1.0, adj["ge"], 1.0)
        return out

    def apply_adjoint(self, lam: DeviceVector, out: DeviceVector = None):
        """out = J' lam = -g_b - B' A^-T g_x - c (Kh + Kv) lam with (g_b, g_x) the adjoint of the tangent load
        (npg_fe_tangent_adjoint): <lam, apply(db)> = <apply_adjoint(lam), db>.  Kh and Kv are used as stored (symmetric to rounding)."""
        out = DeviceVector(self.ctx, self.nb) if out is None else out
        if out is lam:
            raise ValueError("LinearizedModel.apply_adjoint: out must not be lam")
        adj = self._adjoint()
        self.fe.tangent_adjoint(self.N2, self.b_base, self.x_base, lam, out, adj["gx"])
        self.Kh.mul(lam, out, alpha=-self.c, beta=-1.0)
        self._vertical_diffusion(lam, out)            # D_v is symmetric: its own adjoint
        out.axpby(-1.0, self.invert_adjoint(adj["gx"]), 1.0)
        self.n_adjoint_applies += 1
        return out

    # ---- the backward-Euler tangent step ----------------------------------------------------------------------------------------------
    def _preconditioner(self, dt):
        """(M + dt c (Kh + Kv))^-1: own matrix, own Jacobi vector or LU, own CG workspace; rebuilt when dt changes"""
        if self._lhs_dt != dt:
            if self._lhs is None:
                self._lhs = self.fe.new_matrix("b")
                self._lhs_y = DeviceVector(self.ctx, self.nb)
                self._lhs_ws = CgWorkspace(self.ctx, self.nb)
            P = None if isinstance(self.arch, CPU) else Diagonal(DeviceVector(self.ctx, self.nb))
            collect_evolution_LHS_into(self._lhs, P, self.model.params, _bdf1(dt), self.M, self.Kh, self.Kv)
            self._lhs_P = LU(self._lhs) if P is None else P
            self._lhs_dt = dt
        return self._lhs, self._lhs_P

    def _precond_apply(self, dt, r, z):
        A, P = self._preconditioner(dt)
        if isinstance(P, LU):
            z.upload(P.solve(r.to_host()))
            return z
        ws = self._lhs_ws
        ws.x.fill(0.0)
        st = ws.solve(A, r, ws.x, P, atol=0.0, rtol=min(self.rtol, 1e-10), itmax=0)
        if not st.get("solved", 1):
            raise RuntimeError(f"LinearizedModel: the preconditioner's CG did not converge: {st}")
        z.copy_from(ws.x)
        return z

    def _step_operator(self, dt, w, out, adjoint=False):
        """out = (M - dt J) w, or (M - dt J') w"""
        (self.apply_adjoint if adjoint else self.apply)(w, out)
        self.M.mul(w, out, alpha=1.0, beta=-dt)
        return out

    def implicit_step(self, v: DeviceVector, dt, out: DeviceVector = None, rtol=None, memory=30, itmax=300, adjoint=False):
        """out = (M - dt J)^-1 M v: a backward-Euler step of length dt of the tangent model M d_t db = J db.

        Restarted GMRES(memory) over DeviceVector operations with modified Gram-Schmidt, right-preconditioned by
        (M + dt c (Kh + Kv))^-1 (GPU(): Jacobi-CG; CPU(): LU) from a zero guess; the directions are kept preconditioned, so an inexact
        CG is harmless.  Stops when the TRUE residual ||(M - dt J) out - M v|| <= rtol ||M v|| (default rtol: 100 x the model's).
        `last_step` reports dict(niter, npass, rnorm, rnorm0); the inner iterations are also counted in `n_inner`.
        adjoint=True solves (M - dt J') out = M v instead - a step of the adjoint model - with the same GMRES, the same true-residual
        check and the same preconditioner: (M + dt c (Kh + Kv)) is symmetric."""
        dt = float(dt)
        if not (np.isfinite(dt) and dt > 0.0):
            raise ValueError(f"LinearizedModel.implicit_step: dt must be positive, got {dt}")
        rtol = 100.0 * self.rtol if rtol is None else float(rtol)
        out = DeviceVector(self.ctx, self.nb) if out is None else out
        if out is v:
            raise ValueError("LinearizedModel.implicit_step: out must not be v")
        if adjoint:
            self._adjoint()             # an unsupported preconditioner refuses here, before any work vector is touched
        if self._gm is None or len(self._gm["V"]) < memory + 1:
            self._gm = dict(V=[DeviceVector(self.ctx, self.nb) for _ in range(memory + 1)],
                            Z=[DeviceVector(self.ctx, self.nb) for _ in range(memory)])
        V, Z = self._gm["V"], self._gm["Z"]
        rhs, r, w = self._w[0], self._w[1], self._w[2]
        self.M.mul(v, rhs)
        bnorm = rhs.norm()
        out.fill(0.0)
        stats = dict(niter=0, npass=0, rnorm0=bnorm, rnorm=bnorm, solved=True)
        self.last_step = stats
        if bnorm == 0.0:
            return out
        target = rtol * bnorm
        r.copy_from(rhs)
        rnorm = bnorm
        while rnorm > target:
            if stats["niter"] >= itmax:
                stats["solved"] = False
                raise RuntimeError(f"LinearizedModel.implicit_step: no convergence to rtol = {rtol:g} in {itmax} iterations: {stats}")
            stats["npass"] += 1
            V[0].axpby(1.0 / rnorm, r, 0.0)
            H = np.zeros((memory + 1, memory))
            g = np.zeros(memory + 1)
            g[0] = rnorm
            cs, sn = np.zeros(memory), np.zeros(memory)
            k = 0
            est = rnorm
            # the estimate steers the cycle; a cycle ends a little below the target so that the true residual passes the first time
            while k < memory and est > 0.5 * target and stats["niter"] < itmax:
                self._precond_apply(dt, V[k], Z[k])
                self._step_operator(dt, Z[k], w, adjoint)
                for i in range(k + 1):
                    H[i, k] = V[i].dot(w)
                    w.axpby(-H[i, k], V[i], 1.0)
                H[k + 1, k] = w.norm()
                if H[k + 1, k] > 0.0:
                    V[k + 1].axpby(1.0 / H[k + 1, k], w, 0.0)
                for i in range(k):
                    t = cs[i] * H[i, k] + sn[i] * H[i + 1, k]
                    H[i + 1, k] = -sn[i] * H[i, k] + cs[i] * H[i + 1, k]
                    H[i, k] = t
                rho = np.hypot(H[k, k], H[k + 1, k])
                cs[k], sn[k] = H[k, k] / rho, H[k + 1, k] / rho
                H[k, k], H[k + 1, k] = rho, 0.0
                g[k + 1] = -sn[k] * g[k]
                g[k] = cs[k] * g[k]
                est = abs(g[k + 1])
                k += 1
                stats["niter"] += 1
                self.n_inner += 1
            y = np.linalg.solve(np.triu(H[:k, :k]), g[:k]) if k else np.zeros(0)
            for i in range(k):
                out.axpby(y[i], Z[i], 1.0)
            self._step_operator(dt, out, r, adjoint)        # the true residual
            r.axpby(1.0, rhs, -1.0)
            rnorm = r.norm()
            stats["rnorm"] = rnorm
        return out

    # ---- eigenmodes -------------------------------------------------------------------------------------------------------------------
    def eigenmodes(self, n, dt, ncv=None, tol=1e-8, maxrestart=60, v0=None, seed=0, inner_rtol=None, side="right"):
        """The `n` eigenmodes J v = sigma M v nearest the shift 1 / dt, sorted by descending Re sigma, as EigenModes.

        Thick-restart Arnoldi (Krylov-Schur) on P = (M - dt J)^-1 M, the backward-Euler propagator of the tangent model over dt
        (implicit_step).  P has the eigenvectors of the pencil (J, M) EXACTLY, with mu = 1 / (1 - dt sigma): the largest |mu| are the sigma
        nearest 1 / dt, and sigma = (1 - 1 / mu) / dt.  `dt` therefore CHOOSES THE SHIFT - a positive real one: with dt of the order of
        the slowest time scale the method finds the least-damped and the growing modes.  Modes with |Im sigma| >> 1 / dt are out of its
        reach (their |mu| is small whatever their growth rate): lower dt to look for them.

        Real arithmetic: the basis lives on the device (ncv + 1 vectors and as many again for the restart), the small matrices go
        through scipy.linalg.schur (real form) on the host, and a conjugate pair is never split at a restart.  `tol` bounds the residual
        ||J v - sigma M v|| / (|sigma| ||M v||) of every returned mode, recomputed with `apply`; the Arnoldi estimates only decide when
        to look.  ncv: the size of the Krylov space (default max(20, 2 n + 10), at most nb - 1); v0: a start vector (host, native
        order) instead of the seeded random one; inner_rtol: the tolerance of the shift-and-invert solves (default: from tol / 10 down
        to the inversions' rtol, tightened by |mu - 1| of the wanted modes - a solve's error e enters a residual as e / |mu - 1|).
        side="left": the modes J' w = sigma M w (w' J = sigma w' M) - the same driver on the adjoint step, residuals recomputed with
        `apply_adjoint`."""
        import scipy.linalg as sla
        if side not in ("left", "right"):
            raise ValueError(f"LinearizedModel.eigenmodes: side must be 'left' or 'right', got {side!r}")
        left = side == "left"
        n, dt = int(n), float(dt)
        nb = self.nb
        if n < 1 or n >= nb:
            raise ValueError(f"LinearizedModel.eigenmodes: n must lie in [1, {nb - 1}], got {n}")
        if not (np.isfinite(dt) and dt > 0.0):
            raise ValueError(f"LinearizedModel.eigenmodes: dt must be positive, got {dt}")
        m = min(nb - 1, max(20, 2 * n + 10)) if ncv is None else int(ncv)
        if not n + 2 <= m <= nb - 1:
            raise ValueError(f"LinearizedModel.eigenmodes: ncv must lie in [n + 2, nb - 1] = [{n + 2}, {nb - 1}], got {m}")
        inner = max(0.1 * tol, self.rtol) if inner_rtol is None else float(inner_rtol)
        if left:
            self._adjoint()
        d = self.model.fe_data.dofs
        count0 = (self.n_applies + self.n_adjoint_applies, self.n_inversions, self.n_inner)
        V = [DeviceVector(self.ctx, nb) for _ in range(m + 1)]
        W = [DeviceVector(self.ctx, nb) for _ in range(m + 1)]
        if v0 is None:
            V[0].upload(np.random.default_rng(seed).standard_normal(nb), d.p_b)
        else:
            V[0].upload(np.asarray(v0, dtype=float), d.p_b)
        nrm = V[0].norm()
        if not nrm > 0.0:
            raise ValueError("LinearizedModel.eigenmodes: the start vector is zero")
        V[0].axpby(1.0 / nrm, V[0], 0.0)
        H = np.zeros((m + 1, m))
        w = self._w[3]
        k = 0                   # columns of H that hold a Krylov-Schur decomposition
        tol_a = tol             # what the Arnoldi estimates must reach before the true residuals are looked at
        restarts = 0
        result = None
        while True:
            j = k
            while j < m:        # expand: P V[j], orthogonalised twice (modified Gram-Schmidt)
                self.implicit_step(V[j], dt, w, rtol=inner, adjoint=left)
                for _ in range(2):
                    for i in range(j + 1):
                        h = V[i].dot(w)
                        H[i, j] += h
                        w.axpby(-h, V[i], 1.0)
                beta = w.norm()
                H[j + 1, j] = beta
                j += 1
                if beta <= 1e-14 * max(np.abs(H[:j, j - 1]).max(), 1e-300):
                    H[j, j - 1] = 0.0       # an invariant subspace: nothing to add
                    break
                V[j].axpby(1.0 / beta, w, 0.0)
            mm = j
            Hm, brow = H[:mm, :mm].copy(), H[mm, :mm].copy()
            mu = sla.eigvals(Hm)
            order = np.argsort(-np.abs(mu), kind="stable")
            mod = np.abs(mu[order])

            def cut(p):
                """move p down to the nearest gap in |mu| so that no pair (and no tie) is split"""
                while 0 < p < mm and mod[p - 1] - mod[p] <= 1e-12 * mod[0]:
                    p -= 1
                return p
            p = cut(min(n + max((mm - n) // 2, 1), mm - 1)) if mm == m else mm
            if p < n:           # the gap below n lies inside a cluster: keep the whole cluster
                p = n
                while p < mm - 1 and mod[p - 1] - mod[p] <= 1e-12 * mod[0]:
                    p += 1
            thr = 0.5 * (mod[p - 1] + mod[p]) if p < mm else -1.0
            T, Zs, sdim = sla.schur(Hm, output="real", sort=lambda re, im: np.hypot(re, im) > thr)
            p = int(sdim)
            Tp, bp = T[:p, :p], brow @ Zs[:, :p]
            lam, S = sla.eig(Tp)
            S /= np.linalg.norm(S, axis=0)
            est = np.abs(bp @ S) / np.maximum(np.abs(lam), 1e-300)
            pick = np.argsort(-np.abs(lam), kind="stable")[:n]
            done = mm < m or bool((est[pick] <= tol_a).all()) or restarts >= maxrestart
            if inner_rtol is None:
                # an error e of a solve enters a mode's residual as e / |mu - 1|: modes with |sigma| << 1 / dt need tighter solves
                inner = max(min(inner, 0.1 * tol * float(np.abs(lam[pick] - 1.0).min())), self.rtol)
            # the new basis: V[:p] <- V[:mm] Zs[:, :p], then the residual direction
            for i in range(p):
                _lincomb_many(W[i], Zs[:, i], V[:mm])
            W[p].copy_from(V[mm])
            V, W = W, V
            H[:] = 0.0
            H[:p, :p] = Tp
            H[p, :p] = bp
            k = p
            if done:
                result = self._finish(lam[pick], S[:, pick], V, p, dt, tol, count0, restarts, side)
                worst = float(result.residuals.max())
                if result.converged.all() or mm < m or restarts >= maxrestart or tol_a <= 1e-15:
                    return result
                tol_a = max(min(tol_a * 0.1, tol_a * 0.1 * tol / worst), 1e-15)
                if inner_rtol is None:
                    inner = max(0.1 * inner, self.rtol)
            restarts += 1

    def _finish(self, mu, S, V, p, dt, tol, count0, restarts, side="right"):
        """the Ritz vectors V[:p] S, normalised, with their true residuals"""
        op = self.apply_adjoint if side == "left" else self.apply
        d = self.model.fe_data.dofs
        sigma = (1.0 - 1.0 / mu) / dt
        order = np.argsort(-sigma.real, kind="stable")
        sigma, S = sigma[order], S[:, order]
        n = len(sigma)
        vecs = np.zeros((n, self.nb), dtype=complex)
        res = np.zeros(n)
        vr, vi, a, b = self._w[0], self._w[1], self._w[2], DeviceVector(self.ctx, self.nb)
        for i in range(n):
            cplx = abs(sigma[i].imag) > 0.0 or np.abs(S[:, i].imag).max() > 0.0
            _lincomb_many(vr, S[:, i].real, V[:p])
            Jv = op(vr, a).to_host(d.inv_p_b).astype(complex)
            Mv = self.M.mul(vr, b).to_host(d.inv_p_b).astype(complex)
            v = vr.to_host(d.inv_p_b).astype(complex)
            if cplx:
                _lincomb_many(vi, S[:, i].imag, V[:p])
                Jv += 1j * op(vi, a).to_host(d.inv_p_b)
                Mv += 1j * self.M.mul(vi, b).to_host(d.inv_p_b)
                v += 1j * vi.to_host(d.inv_p_b)
            res[i] = np.linalg.norm(Jv - sigma[i] * Mv) / (abs(sigma[i]) * np.linalg.norm(Mv))
            v /= np.sqrt(np.vdot(v, Mv).real)                        # unit M-norm (M is symmetric positive definite)
            big = v[np.argmax(np.abs(v))]
            vecs[i] = v * (np.conj(big) / abs(big))                  # the largest entry real (and positive)
            if not cplx:
                vecs[i] = vecs[i].real
        return EigenModes(sigma, vecs, res, res <= tol, self.n_applies + self.n_adjoint_applies - count0[0], self.n_inversions - count0[1],
                          dt, self.n_inner - count0[2], restarts, side)

    # ---- both sets of modes -----------------------------------------------------------------------------------------------------------
    def mass_matrix_native(self):
        """M as a scipy CSR matrix over the free DoFs in native order (the order of EigenModes.vectors)"""
        p = self.model.fe_data.dofs.inv_p_b
        return self.M.to_scipy_csr()[p][:, p].tocsr()

    def mode_pairs(self, n, dt, **kw):
        """The `n` modes nearest 1 / dt from both sides, matched and scaled so that w_i' M v_i = 1, as ModePairs.  **kw: eigenmodes'."""
        if "side" in kw:
            raise ValueError("LinearizedModel.mode_pairs: it computes both sides; do not pass side")
        self._adjoint()
        right = self.eigenmodes(n, dt, side="right", **kw)
        left = self.eigenmodes(n, dt, side="left", **kw)
        return ModePairs.from_modes(right, left, self.mass_matrix_native())


class ModePairs:
    """What LinearizedModel.mode_pairs returns: right modes v_i (J v = sigma M v) and left modes w_i (w' J = sigma w' M) of the same
    eigenvalues, biorthogonal in the BILINEAR form - w_i' M v_j = 0 for sigma_i != sigma_j, no conjugate - and scaled to w_i' M v_i = 1.

    sigma        complex (n,), from the right modes (sorted by descending real part)
    sigma_left   the left modes' own eigenvalues, in the matched order
    right, left  complex (n, nb), native free-DoF order; the right vectors are EigenModes' (unit M-norm), the left carry the scale
    left_M       (n, nb): row i is w_i' M, what `amplitudes` multiplies with
    condition    kappa_i = ||w_i||_M ||v_i||_M / |w_i' M v_i| with ||x||_M^2 = x^H M x: 1 for a normal pencil
    residuals_right, residuals_left, dt   from the two EigenModes"""

    _fields = ("sigma", "sigma_left", "right", "left", "left_M", "condition", "residuals_right", "residuals_left")

    def __init__(self, sigma, sigma_left, right, left, left_M, condition, residuals_right, residuals_left, dt):
        self.sigma, self.sigma_left = np.asarray(sigma, dtype=complex), np.asarray(sigma_left, dtype=complex)
        self.right, self.left = np.asarray(right, dtype=complex), np.asarray(left, dtype=complex)
        self.left_M = np.asarray(left_M, dtype=complex)
        self.condition = np.asarray(condition, dtype=float)
        self.residuals_right, self.residuals_left = np.asarray(residuals_right, dtype=float), np.asarray(residuals_left, dtype=float)
        self.dt = float(dt)

    @classmethod
    def from_modes(cls, right, left, M):
        """match the left modes to the right ones by nearest sigma (a conjugate pair may come in either order) and scale them"""
        if right.side != "right" or left.side != "left" or len(right) != len(left):
            raise ValueError("ModePairs.from_modes: needs as many left modes as right modes")
        n, used, order = len(right), set(), []
        for i in range(n):
            j = min((j for j in range(n) if j not in used), key=lambda j: abs(right.sigma[i] - left.sigma[j]))
            used.add(j)
            order.append(j)
        V, W = right.vectors, left.vectors[order].copy()
        MV = (M @ V.T).T                                               # row i: M v_i
        cond = np.zeros(n)
        for i in range(n):
            wMv = W[i] @ MV[i]                                         # bilinear: no conjugate
            nw = np.sqrt(np.vdot(W[i], M @ W[i]).real)
            nv = np.sqrt(np.vdot(V[i], MV[i]).real)
            if wMv == 0.0:
                raise RuntimeError(f"ModePairs.from_modes: left mode {order[i]} is M-orthogonal to right mode {i}: not the same eigenvalue")
            cond[i] = nw * nv / abs(wMv)
            W[i] = W[i] / wMv
        left_M = (M.T @ W.T).T
        return cls(right.sigma, left.sigma[order], V, W, left_M, cond, right.residuals, left.residuals[order], right.dt)

    def __len__(self):
        return len(self.sigma)

    def amplitudes(self, db):
        """a_i = w_i' M db: the coordinates of db (native order, real or complex) in the right modes"""
        return self.left_M @ np.asarray(db)

    def reconstruct(self, a):
        """sum_i a_i v_i"""
        return np.asarray(a) @ self.right

    def save(self, path):
        np.savez(path, dt=self.dt, **{k: getattr(self, k) for k in self._fields})
        return path

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(*[z[k] for k in cls._fields], float(z["dt"]))

    def __repr__(self):
        return f"ModePairs: {len(self)} modes nearest 1/dt = {1.0 / self.dt:.3e}, sigma = {self.sigma}, condition = {self.condition}"


def _lincomb_many(out, coef, xs):
    """out = sum_k coef[k] xs[k], eight terms per launch (out is none of the xs)"""
    coef = np.asarray(coef, dtype=float)
    first = True
    for s in range(0, len(xs), 7):
        cs, vs = list(coef[s:s + 7]), list(xs[s:s + 7])
        if first:
            out.lincomb(cs, vs)
            first = False
        else:
            out.lincomb([1.0] + cs, [out] + vs)
    return out
