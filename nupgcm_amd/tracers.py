"""Passive tracers carried by the flow (npg_tracers_rhs): ideal age, dyes, a second component with its own background
gradient and surface flux.  The reference evolves b' alone.

A tracer obeys the model's own advection-diffusion equation, stepped every timestep with the same BDF scheme, the same matrix
A = M + theta (Kh + Kv), the same preconditioner and the same velocity extrapolation as b':

    A c^{n+1} = int ( c1 c + c2 c_prev - cdt ( u~ . grad c~ + u~_z Gamma - S ) ) phi  -  Dirichlet lift  +  theta Gamma rhs_diff1  +  dt flux

The full tracer is Gamma z + c.  The K right-hand sides come from ONE fused element launch that evaluates the velocity at the
quadrature points once per cell (csrc/tracers.hip); the K solves are K warm-started CG solves on views of the stacked vectors, or
(batched=True) one batched CG per group of at most 32 tracers that streams the matrix once per iteration for up to
eight columns, with the same bits.
Tracers use the buoyancy's diffusivities - the engine's current kappa_h / kappa_v tables, so they follow the convection closure -
and the buoyancy's Dirichlet tags with values of their own.  They are passive: u, p and b' do not change by a bit.

isoneutral=Isoneutral(kappa, slope_max, bz_min) gives the tracers an operator of their own, A_c = M + theta (K_iso + Kv):
the small-slope rotated tensor of the running buoyancy B = N2 z + b', rebuilt on the device every step, instead of kappa_h along the
mesh's x-y planes.  A dye then spreads along the buoyancy surfaces and crosses them with kappa_v alone."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Any

import numpy as np

from . import _lib as L
from .architectures import DeviceVector
from .assembly import eval_at_quad_points
from .evolution import evolution_parameter
from .iterative_solvers import BatchedCgWorkspace, CgWorkspace, Diagonal, IterativeSolverToolkit, iterative_solve
from .timesteppers import BDF1


@dataclass
class TracerSpec:
    """name; initial (a function of x, an array in native free-DoF order as set_b takes, or None = 0); dirichlet (a number, a function
    of x, or None = 0, on the buoyancy's Dirichlet tags); gamma (background gradient: the full tracer is gamma z + c); source (uniform);
    flux (a number, a function of x, or None: surface flux over the mesh's surface tags, scaled as build_rhs_flux scales b's)"""
    name: str
    initial: Any = None
    dirichlet: Any = None
    gamma: float = 0.0
    source: float = 0.0
    flux: Any = None


@dataclass
class Isoneutral:
    """Isoneutral mixing of the tracers: kappa (a number or a function of x, evaluated at the points of the engine's volume rule as
    kappa_h is) along the surfaces of B = N2 z + b', the engine's current kappa_v across them.

    The slope S = -grad_h B / max(d_z B, bz_min) is taken in MESH coordinates, in which the model's equation carries kappa_h on grad_h
    and kappa_v on d_z under one prefactor; a physical slope is (H / L) times S.  There are no defaults for the two thresholds:
      slope_max  the largest mesh-coordinate slope along which kappa acts; steeper surfaces are mixed along a surface of that slope.  The
                 entry kappa |S|^2 of the tensor competes with kappa_v: choose slope_max so that kappa slope_max^2 stays within what
                 the vertical resolution and the solver's conditioning bear - a physical slope of 1e-2 on a basin of aspect ratio H / L
                 is slope_max = 1e-2 L / H.
      bz_min     the smallest d_z B the slope divides by, > 0: a small fraction of N2 (1e-2 N2 ... 1e-1 N2) where the stratification
                 is the background's, larger where convection leaves d_z B near 0 and the slope would otherwise be noise.
    slope_max = 0 gives level mixing with kappa in place of kappa_h."""
    kappa: Any
    slope_max: float
    bz_min: float


def _spec(t):
    if isinstance(t, TracerSpec):
        return t
    if isinstance(t, dict):
        return TracerSpec(**t)
    raise TypeError(f"PassiveTracers: a tracer is a TracerSpec or a dict of its fields, got {type(t).__name__}")


def _solve_stats(stats):
    return dict(stats) if stats is not None else None


class PassiveTracers:
    """PassiveTracers(model, tracers): K tracers on the model's mesh, set as `model.tracers`; run() then steps them directly after
    evolve().  `c`, `c_prev`, `c_curr` are stacked device vectors (tracer k at k * n_b, the buoyancy's numbering); `values(k | name)`
    returns tracer k in native free-DoF order on the host; `stats[i]` holds the K CG statistics of step i.
    batched=True solves the K systems of a step with BatchedCgWorkspace (groups of at most 32 tracers); every tracer keeps the bits of
    the per-tracer solve.  On CPU() iterative_solve takes the reference's direct-solve branches for these sizes, which have no batched
    form: there batched=True runs the per-tracer path.
    isoneutral=Isoneutral(kappa, slope_max, bz_min): the tracers mix along the running buoyancy's surfaces with a matrix A_c and a
    Jacobi vector P_c of their own, rebuilt every step (`A`, `P`, `Kiso`); `clip_counts` reports the shares of the quadrature points
    floored by bz_min and clipped by slope_max in the last step.  Such tracers always take Jacobi-CG (on CPU() too: the matrix changes
    every step, there is nothing to factorise once), and a model with a restoring surface condition or a sponge is accepted: A_c holds
    neither of their matrices."""

    def __init__(self, model, tracers, batched=False, isoneutral=None):
        if getattr(model, "comm", None) is not None or getattr(model, "layout", None) is not None \
                or getattr(model.arch.ctx, "nranks", 1) > 1:
            raise NotImplementedError("PassiveTracers: distributed and mesh-partitioned models are not supported; tracers run on a "
                                      "single-device model")
        if model.evolution is None:
            raise ValueError("PassiveTracers: the model has no EvolutionToolkit")
        if isoneutral is not None and not isinstance(isoneutral, Isoneutral):
            raise TypeError(f"PassiveTracers: isoneutral must be an Isoneutral(kappa, slope_max, bz_min), got {type(isoneutral).__name__}")
        self.isoneutral = isoneutral
        if isoneutral is None and getattr(getattr(model, "surface_forcing", None), "restoring", False):
            raise NotImplementedError("PassiveTracers on a model with a restoring surface condition (SurfaceForcing(restoring=...)) is out "
                                      "of scope: the tracers share the evolution's matrix and would be restored towards 0")
        if isoneutral is None and getattr(getattr(model, "interior_forcing", None), "restoring", False):
            raise NotImplementedError("PassiveTracers on a model with a sponge (InteriorForcing(restoring=...)) is out of scope: the "
                                      "tracers share the evolution's matrix and would be restored towards 0")
        self.specs = [_spec(t) for t in tracers]
        if not self.specs:
            raise ValueError("PassiveTracers: at least one tracer is needed")
        names = [s.name for s in self.specs]
        if len(set(names)) != len(names):
            raise ValueError(f"PassiveTracers: tracer names must be distinct, got {names}")
        self.names = names
        self.model = model
        ev, fed = model.evolution, model.fe_data
        self.fe = ev.fe
        ctx = self.ctx = model.arch.ctx
        K, nb = len(self.specs), fed.dofs.nb
        self.ntracer, self.nb = K, nb
        h = C.c_void_p()
        L.check(L.lib().npg_tracers_create(self.fe.h, K, C.byref(h)))
        self.h = h
        s, d, t, m = fed.spaces, fed.dofs, fed.tables, fed.mesh
        diri_nodes = np.nonzero(s.b_dof < 0)[0]                      # the order of DeviceTables.b_diri
        xd = m.node_coords[:s.nb_nodes][diri_nodes]
        c0 = np.zeros(K * nb)
        flux = np.zeros(K * nb)
        any_flux = False
        self.gamma, self.source = np.zeros(K), np.zeros(K)
        for k, sp in enumerate(self.specs):
            dv = None
            if sp.dirichlet is not None:
                dv = np.zeros(len(t.b_diri))                         # (embedded 2-D meshes: one spare zero behind the nodes' values)
                v = sp.dirichlet(xd) if callable(sp.dirichlet) else np.full(len(diri_nodes), float(sp.dirichlet))
                dv[:len(diri_nodes)] = np.asarray(v, dtype=float)
                dv = L.as_f64(dv)
            self.gamma[k], self.source[k] = float(sp.gamma), float(sp.source)
            L.check(L.lib().npg_tracers_set(self.h, k, None if dv is None else L.ptr(dv), self.gamma[k], self.source[k]))
            if sp.initial is not None:
                vals = s.interpolate_b(sp.initial) if callable(sp.initial) else np.asarray(sp.initial, dtype=float)
                if vals.shape != (nb,):
                    raise ValueError(f"PassiveTracers: tracer '{sp.name}': expected {nb} free values, got {vals.shape}")
                c0[k * nb:(k + 1) * nb] = vals[d.p_b]
            if sp.flux is not None:
                fn = sp.flux if callable(sp.flux) else (lambda x, c=float(sp.flux): np.full(x.shape[:-1], c))
                load = m.surface_load(lambda x: model.params.alpha * fn(x))[:s.nb_nodes]
                pos = t.b_pos
                f = np.zeros(nb)
                f[pos[pos >= 0]] = load[pos >= 0]
                flux[k * nb:(k + 1) * nb] = f
                any_flux = True
        self.c = DeviceVector.from_host(ctx, c0)
        self.c_prev, self.c_curr = self.c.copy(), self.c.copy()
        self.y = DeviceVector(ctx, K * nb)
        self.flux = DeviceVector.from_host(ctx, flux) if any_flux else None
        # (isoneutral: the background gradient diffuses through the rotated tensor inside the fused launch; rhs_diff1 is not used)
        self.rhs_diff1 = self.fe.rhs_diff(1.0, DeviceVector(ctx, nb)) if np.any(self.gamma != 0.0) and isoneutral is None else None
        self.A, self.P, self.Kiso = ev.solver.A, ev.solver.P, None
        if isoneutral is not None:
            kap = L.as_f64(eval_at_quad_points(m, isoneutral.kappa).T)               # [nq][ncell]
            L.check(L.lib().npg_tracers_set_isoneutral(self.h, L.ptr(kap), float(isoneutral.slope_max), float(isoneutral.bz_min)))
            self.Kiso, self.A = self.fe.new_matrix("b"), self.fe.new_matrix("b")
            self.P = Diagonal(DeviceVector(ctx, nb))
        # K solves with the evolution toolkit's own A and P, each with its own workspace (warm start: the workspace's x aliases the
        # tracer's slice of c, as IterativeSolverToolkit.x aliases workspace.x)
        self.solvers = []
        for k in range(K):
            ws = CgWorkspace(ctx, nb)
            ws.x = self.c.view(k * nb, nb)
            self.solvers.append(IterativeSolverToolkit(self.A, self.P, self.y.view(k * nb, nb), ws, ev.solver.kwargs,
                                                       f"Tracer {names[k]}"))
        # batched: one workspace per group of at most 32 tracers, its x the group's window of c (the warm start)
        self.batched = bool(batched) and ctx.device >= 0
        self.groups = []
        if self.batched:
            for k0 in range(0, K, L.NPG_CG_MULTI_MAX):
                kc = min(L.NPG_CG_MULTI_MAX, K - k0)
                ws = BatchedCgWorkspace(ctx, nb, kc)
                ws.x = self.c.view(k0 * nb, kc * nb)
                self.groups.append((k0, kc, ws, self.y.view(k0 * nb, kc * nb)))
        self.stats = []

    def __del__(self):
        try:
            if self.h:
                L.lib().npg_tracers_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def index(self, k):
        return self.names.index(k) if isinstance(k, str) else int(k)

    def view(self, k, which="c"):
        """tracer k's window of a stacked vector ("c", "c_prev", "c_curr", "y")"""
        k = self.index(k)
        return getattr(self, which).view(k * self.nb, self.nb)

    def values(self, k):
        """tracer k (index or name) on the host, free values in native order - as State.b"""
        return self.view(k).to_host(self.model.fe_data.dofs.inv_p_b)

    def rhs(self, scheme, dt, theta, x_inv, x_inv_prev, y=None):
        """one npg_tracers_rhs call on the current c / c_prev into `y` (default: the solvers' right-hand sides)"""
        y = self.y if y is None else y
        L.check(L.lib().npg_tracers_rhs(self.h, int(scheme), float(dt), float(theta), self.c.h, self.c_prev.h, x_inv.h, x_inv_prev.h,
                                        None if self.rhs_diff1 is None else self.rhs_diff1.h,
                                        None if self.flux is None else self.flux.h, y.h))
        return y

    def update_isoneutral(self, b=None):
        """the tensor tables from b' (default: the model's current b_vec) and K_iso from them: two launches"""
        b = self.model.b_vec if b is None else b
        L.check(L.lib().npg_tracers_isoneutral_update(self.h, float(self.model.params.N2), b.h))
        L.check(L.lib().npg_tracers_isoneutral_matrix(self.h, self.Kiso.h))
        return self.Kiso

    def isoneutral_info(self):
        """dict(floored, clipped, points, state) of the last update (state: L.NPG_REDI_OFF / _SET / _UPDATED)"""
        nf, ncl, npt, st = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
        L.check(L.lib().npg_tracers_isoneutral_info(self.h, C.byref(nf), C.byref(ncl), C.byref(npt), C.byref(st)))
        return dict(floored=nf.value, clipped=ncl.value, points=npt.value, state=st.value)

    def isoneutral_tables(self):
        """(kxz, kyz, kzz) of the last update on the host, (ncell, nq) each"""
        m = self.model.fe_data.mesh
        out = [np.empty((len(m.q_w), m.ncell)) for _ in range(3)]
        L.check(L.lib().npg_tracers_isoneutral_tables(self.h, *(L.ptr(a) for a in out)))
        return tuple(np.ascontiguousarray(a.T) for a in out)

    @property
    def clip_counts(self):
        """(floored share, clipped share) of the quadrature points in the last step's tensor; None without isoneutral mixing"""
        if self.isoneutral is None:
            return None
        i = self.isoneutral_info()
        return (i["floored"] / i["points"], i["clipped"] / i["points"]) if i["points"] else (0.0, 0.0)

    def _step_isoneutral(self, model, x_inv_prev):
        """tensor from the b' just solved -> K_iso -> A_c = M + theta (K_iso + Kv), its Jacobi vector -> the fused right-hand side ->
        K Jacobi-CG solves with (A_c, P_c)"""
        ev, ts, prm = model.evolution, model.timestepper, model.params
        theta = evolution_parameter(prm, ts)               # (the current dt: an adaptive step is followed)
        self.update_isoneutral(model.b_vec)
        self.A.combine(1.0, ev.M, theta, self.Kiso, ev.Kv)
        self.A.inv_diag(self.P.diag)
        scheme = L.NPG_BDF1 if isinstance(ts, BDF1) else L.NPG_BDF2
        self.rhs(scheme, ts.dt, theta, model.inversion.solver.x, x_inv_prev)
        step_stats = []
        if self.batched:
            for _k0, _kc, ws, yg in self.groups:
                step_stats.extend(_solve_stats(st) for st in ws.solve(self.A, yg, ws.x, self.P, **ev.solver.kwargs))
        else:
            for s in self.solvers:
                s.workspace.solve(self.A, s.y, s.x, self.P, **s.kwargs)
                step_stats.append(_solve_stats(s.workspace.stats))
        self.stats.append(step_stats)
        return self

    def step(self, model, x_inv_prev):
        """what evolve() does for b', for every tracer: [convection closure on: rhs_diff1 from the refreshed kappa_v] -> one fused
        right-hand-side call -> K CG solves with the evolution toolkit's A and P (already rebuilt by evolve() for this step) - or,
        batched, one solve per group of at most 32 tracers."""
        ev, ts, prm = model.evolution, model.timestepper, model.params
        self.c_curr.copy_from(self.c)                    # what run() does for b_curr before evolve()
        if self.isoneutral is not None:
            return self._step_isoneutral(model, x_inv_prev)
        if self.rhs_diff1 is not None and model.forcings.conv_param.is_on:
            self.fe.rhs_diff(1.0, self.rhs_diff1)
        theta = evolution_parameter(prm, ts)
        scheme = L.NPG_BDF1 if isinstance(ts, BDF1) else L.NPG_BDF2
        self.rhs(scheme, ts.dt, theta, model.inversion.solver.x, x_inv_prev)
        step_stats = []
        if self.batched:
            for _k0, _kc, ws, yg in self.groups:
                step_stats.extend(_solve_stats(st) for st in ws.solve(ev.solver.A, yg, ws.x, ev.solver.P, **ev.solver.kwargs))
            self.stats.append(step_stats)
            return self
        for s in self.solvers:
            s.A, s.P = ev.solver.A, ev.solver.P          # (CPU(): collect_evolution_LHS replaces the factorisation object)
            iterative_solve(s)
            step_stats.append(_solve_stats(s.workspace.stats))
        self.stats.append(step_stats)
        return self

    def rotate(self):
        """the history rotation of run(): c_prev <-> c_curr"""
        self.c_prev, self.c_curr = self.c_curr, self.c_prev

    def maxabs(self):
        return self.c.maxabs()
