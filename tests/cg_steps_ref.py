"""An extended-precision CG and the checks shared by tests/test_cg_steps.py (host library) and tests/test_gpu_cg_steps.py (device):
npg_cg_solve (csrc/cg.hip: k_cg_init / k_cg_spmv / k_cg_update<1> / k_cg_direction) step by step against something that is not the
project's own code.

Reference: `cg_run` in numpy.longdouble (64-bit mantissa), the sparse product written out as np.add.reduceat over the CSR arrays,
with the device's recurrence
    r = b - A x0, z = P r, p = z, gamma = r'z ; alpha = gamma / p'Ap ; x += alpha p ; r -= alpha Ap ; z = P r ;
    beta = gamma' / gamma ; p = z + beta p
It returns xs[k] (the iterate a solve with itmax = k returns), hist[k] = sqrt(r'z) and the status of the stopping rule:
1 solved, 2 itmax, 3 breakdown (r'z of the start not finite, p'Ap <= 0 or NaN: no step is taken), 4 zero residual at the start.

Noise: the same recurrence in fp64 with three summation orders of every inner product and row sum (numpy's pairwise sum, the same
reversed, strictly serial cumsum).  Their largest deviation from the longdouble run at step k is that step's noise,
    noise_x[k] = max |x - x_ld| / max |x_ld|          noise_h[k] = |h - h_ld| / h_ld[0]
and the bar for the library under test at step k is 16 * noise[k], floored at 1e-15, measured against the longdouble run.  The
device's tree (lanes, waves, workgroups, 32 slices) is one more order of the same fp64 sums; 16 is the margin for an unlucky one.
A kernel that drops a row, a lane, a tile or a partial row moves gamma by about 1/n of itself (3e-6 at n = 300 001); the bars are
1e-15 .. 4e-13.

Only steps k with hist_ld[j] >= 1e-6 hist_ld[0] for all j <= k are checked: once the residual is gone the recurrence divides 0 by 0
(the arrowhead under Jacobi after about 3 steps, n = 1 after one)."""
import numpy as np
import pytest
import scipy.sparse as sp

import nupgcm_amd as npg
from nupgcm_amd import _lib as L
from tests import cg_multi_ref as cm

if not np.finfo(np.longdouble).eps < 1e-18:
    pytest.skip("numpy.longdouble has no 64-bit mantissa here", allow_module_level=True)

LD = np.longdouble
KS = (1, 2, 3, 4, 5, 8, 9)          # the host looks at the state every 4 iterations: 3, 4, 5, 8, 9 straddle that
MARGIN, FLOOR = 16.0, 1e-15
ORDERS = ("pairwise", "reversed", "serial")


def _sum(v, order):
    if order == "serial":
        return np.cumsum(v)[-1]
    return np.sum(v[::-1]) if order == "reversed" else np.sum(v)


def matvec(A, x, order="pairwise"):
    """A x in x's type; the row sums by np.add.reduceat (scipy does not multiply in longdouble), which adds a row's products one
    after the other: first to last, or last to first when order is "reversed" """
    n = A.shape[0]
    prod = A.data.astype(x.dtype) * x[A.indices]
    out = np.zeros(n, dtype=x.dtype)
    full = np.flatnonzero(np.diff(A.indptr) > 0)
    if full.size == 0:
        return out
    if order == "reversed":
        out[full[::-1]] = np.add.reduceat(prod[::-1], (A.nnz - A.indptr[full + 1])[::-1])
    else:
        out[full] = np.add.reduceat(prod, A.indptr[full])
    return out


def cg_run(A, Pd, b, x0, itmax, atol=0.0, rtol=0.0, dtype=LD, order="pairwise"):
    """-> xs (list: xs[k] is the iterate after k iterations), hist (array), status, niter.  Pd: the diagonal of P, or a callable
    z = Pd(r, order) that works in r's type"""
    A = sp.csr_matrix(A)
    A.sort_indices()
    T = dtype
    b, x = np.asarray(b, T), np.array(x0, T)
    if callable(Pd):
        def P(r):
            return Pd(r, order)
    else:
        Pd = np.asarray(Pd, T)

        def P(r):
            return Pd * r
    with np.errstate(all="ignore"):
        r = b - matvec(A, x, order)
        z = P(r)
        p = z.copy()
        gamma = _sum(r * z, order)
        h0 = np.sqrt(gamma)
        eps = T(atol) + T(rtol) * h0
        xs, hist, it = [x.copy()], [h0], 0
        status = 3 if not np.isfinite(gamma) else 4 if gamma == 0 else 1 if h0 <= eps else 0
        while status == 0:
            Ap = matvec(A, p, order)
            pAp = _sum(p * Ap, order)
            if not pAp > 0:
                status = 3
                break
            alpha = gamma / pAp
            x = x + alpha * p
            r = r - alpha * Ap
            z = P(r)
            g = _sum(r * z, order)
            h = np.sqrt(g)
            it += 1
            xs.append(x.copy())
            hist.append(h)
            status = 1 if (h <= eps or h + 1 <= 1) else 2 if it >= itmax else 3 if g != g else 0
            p = z + (g / gamma) * p
            gamma = g
    return xs, np.array(hist, T), status, it


class Steps:
    """longdouble run and per-step noise of one system, made once and read-only afterwards"""

    def __init__(self, A, Pd, b, x0, itmax, same_ending=False, **kw):
        self.xs, self.hist, self.status, self.niter = cg_run(A, Pd, b, x0, itmax, **kw)
        K = self.niter
        ok = self.hist >= LD(1e-6) * self.hist[0]
        self.kmax = K if ok.all() else int(np.argmin(ok)) - 1          # the last step before the residual is gone
        self.noise_x, self.noise_h = np.zeros(K + 1), np.zeros(K + 1)
        for order in ORDERS:
            xs, hist, status, niter = cg_run(A, Pd, b, x0, itmax, dtype=np.float64, order=order, **kw)
            if same_ending:
                assert (status, niter) == (self.status, self.niter), (order, status, niter, self.status, self.niter)
            assert niter >= self.kmax
            for k in range(self.kmax + 1):
                self.noise_x[k] = max(self.noise_x[k], self.dev_x(k, xs[k]))
                self.noise_h[k] = max(self.noise_h[k], self.dev_h(k, hist[k]))
        for a in (self.hist, self.noise_x, self.noise_h, *self.xs):
            a.setflags(write=False)

    def dev_x(self, k, x):
        scale = np.abs(self.xs[k]).max()
        return float(np.abs(np.asarray(x, LD) - self.xs[k]).max() / (scale if scale > 0 else LD(1)))

    def dev_h(self, k, h):
        return float(abs(LD(h) - self.hist[k]) / self.hist[0])

    def bar_x(self, k):
        return max(MARGIN * self.noise_x[k], FLOOR)

    def bar_h(self, k):
        return max(MARGIN * self.noise_h[k], FLOOR)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
# (id, builder, lanes asserted or None); the preconditioner rotates over none / scalar / diagonal with the position in this list
CASES = [("tri1", lambda: cm.tridiagonal(1), None),
         ("tri255", lambda: cm.tridiagonal(255), None), ("tri256", lambda: cm.tridiagonal(256), None),
         ("tri257", lambda: cm.tridiagonal(257), None),
         ("tri1023", lambda: cm.tridiagonal(1023), None), ("tri1024", lambda: cm.tridiagonal(1024), None),
         ("tri1025", lambda: cm.tridiagonal(1025), None),
         ("tri8192", lambda: cm.tridiagonal(8192), None), ("tri8193", lambda: cm.tridiagonal(8193), None),
         ("tri65536", lambda: cm.tridiagonal(65536), None), ("tri65537", lambda: cm.tridiagonal(65537), None),
         ("tri300001", lambda: cm.tridiagonal(300001), None),
         ("laplace7_lanes4", lambda: cm.laplace7(20), 4),
         ("banded2000_lanes8", lambda: cm.banded(2000, 12), 8),
         ("banded300_lanes16", lambda: cm.banded(300, 50), 16),
         ("dense300_lanes32", lambda: cm.banded(300, 299), 32),
         ("arrowhead", lambda: cm.arrowhead(6000), None)]
PRECONDS = ("none", "scalar", "diagonal")
HOST_MAX_N = 8193


def case_ids(max_n=None):
    sizes = dict(tri65536=65536, tri65537=65537, tri300001=300001)
    return [c[0] for c in CASES if max_n is None or sizes.get(c[0], 0) <= max_n]


_systems = {}


def system(cid):
    """matrix, preconditioner kind and diagonal, b, x0 and the reference of a case: made once, shared by every test that asks"""
    if cid not in _systems:
        i = [c[0] for c in CASES].index(cid)
        A = sp.csr_matrix(CASES[i][1]())
        A.sort_indices()
        n = A.shape[0]
        kind = PRECONDS[i % 3]
        rng = np.random.default_rng(cm.SEED + i)
        b, x0 = rng.standard_normal(n), rng.standard_normal(n)
        Pd = dict(none=np.ones(n), scalar=np.full(n, 1.0 / float(A.diagonal().mean())), diagonal=1.0 / A.diagonal())[kind]
        ref = Steps(A, Pd, b, x0, max(KS))
        _systems[cid] = (A, kind, Pd, b, x0, ref, CASES[i][2])
    return _systems[cid]


def device_precond(ctx, kind, Pd):
    if kind == "none":
        return None
    if kind == "scalar":
        return npg.Diagonal(scalar=float(Pd[0]), n=len(Pd))
    return npg.Diagonal(npg.DeviceVector.from_host(ctx, Pd))


def full_history(ws, room):
    """the workspace's history through a buffer with `room` entries (CgWorkspace.history asks for niter + 1 only)"""
    buf = np.full(room, -1.0)
    k = L.lib().npg_cg_history(ws.h, L.ptr(buf), buf.size)
    return buf[:max(k, 0)].copy()


def solve(ctx, A_dev, P, b, x0, ws=None, **kw):
    ws = ws or npg.CgWorkspace(ctx, len(b))
    x = npg.DeviceVector.from_host(ctx, x0)
    st = dict(ws.solve(A_dev, npg.DeviceVector.from_host(ctx, b), x, P, **kw))
    return x.to_host(), st, full_history(ws, st["niter"] + 8), ws


def check_steps(ctx, cid):
    """one case: itmax = k for every k of KS the reference still resolves; returns the measured maxima"""
    A, kind, Pd, b, x0, ref, lanes = system(cid)
    n = A.shape[0]
    if lanes is not None:
        assert cm.expected_lanes(A) == lanes
    ks = [k for k in KS if k <= ref.kmax]
    if n == 1:
        ks = [1]            # one step solves it; what follows divides 0 by 0
    else:
        assert len(ks) >= 2 and ref.kmax >= 2, (cid, ref.kmax, ref.hist)
    A_dev = npg.DeviceCSR.from_scipy(ctx, A)
    P = device_precond(ctx, kind, Pd)
    worst = dict(x=0.0, h=0.0, nx=0.0, nh=0.0, rx=0.0, rh=0.0)
    last = None
    for k in ks:
        x, st, hist, ws = solve(ctx, A_dev, P, b, x0, atol=0.0, rtol=0.0, itmax=k)
        last = (x, st, hist, ws)
        assert st["niter"] == k, (cid, k, st)
        assert len(hist) == k + 1, (cid, k, len(hist))
        if n == 1:
            # x_1 = b / a whatever the start; the residual after it is 0 or an ulp of rounding: status 1 exactly when it is 0
            assert st["status"] == (1 if hist[1] == 0.0 else 2) and st["solved"] == (hist[1] == 0.0), st
            assert abs(x[0] - b[0] / A[0, 0]) <= 2 * np.spacing(abs(b[0] / A[0, 0])), (x[0], b[0] / A[0, 0])
            checked = [0]
        else:
            assert st["status"] == 2 and st["solved"] == 0, (cid, k, st)      # the reference with itmax = k: status 2 at step k
            checked = range(k + 1)
        for j in checked:
            dh = ref.dev_h(j, hist[j])
            worst["h"], worst["nh"] = max(worst["h"], dh), max(worst["nh"], ref.noise_h[j])
            worst["rh"] = max(worst["rh"], dh / max(ref.noise_h[j], FLOOR / MARGIN))
            assert dh <= ref.bar_h(j), f"{cid} itmax={k}: history[{j}] off by {dh:.3e}, noise {ref.noise_h[j]:.3e}, bar {ref.bar_h(j):.3e}"
        if n > 1:
            dx = ref.dev_x(k, x)
            worst["x"], worst["nx"] = max(worst["x"], dx), max(worst["nx"], ref.noise_x[k])
            worst["rx"] = max(worst["rx"], dx / max(ref.noise_x[k], FLOOR / MARGIN))
            assert dx <= ref.bar_x(k), f"{cid} itmax={k}: x off by {dx:.3e}, noise {ref.noise_x[k]:.3e}, bar {ref.bar_x(k):.3e}"
        assert st["rnorm0"] == hist[0] and st["rnorm"] == hist[k]
    # history()[0] against sqrt(r'Pr) formed in longdouble from x0
    r0 = np.asarray(b, LD) - matvec(A, np.asarray(x0, LD))
    h0 = np.sqrt(np.sum(r0 * np.asarray(Pd, LD) * r0))
    assert abs(LD(last[2][0]) - h0) <= ref.bar_h(0) * h0
    # the largest k again: in a fresh workspace, and in the same workspace a second time
    k = ks[-1]
    for ws in (None, last[3], last[3]):
        x, st, hist, _ = solve(ctx, A_dev, P, b, x0, ws=ws, atol=0.0, rtol=0.0, itmax=k)
        assert cm.same_bits(x, last[0]) and cm.same_bits(hist, last[2]), (cid, "rerun", ws is None)
        assert all(cm.same_bits(st[key], last[1][key]) for key in cm.KEYS)
    print(f"cg_steps {cid} n={n} {kind} k<={k}: x dev {worst['x']:.2e} noise {worst['nx']:.2e} ratio {worst['rx']:.2f} | "
          f"history dev {worst['h']:.2e} noise {worst['nh']:.2e} ratio {worst['rh']:.2f}")
    return worst


def triangular_precond(LU):
    """z = U^-1 L^-1 r for cg_run, from factors stored in one CSR pattern (strictly lower: L, unit diagonal implied; rest: U):
    row by row in r's type, each row's sum in the order asked for"""
    LU = sp.csr_matrix(LU)
    LU.sort_indices()
    n, rp, ci = LU.shape[0], LU.indptr, LU.indices
    dg = np.array([rp[i] + int(np.searchsorted(ci[rp[i]:rp[i + 1]], i)) for i in range(n)])
    assert (ci[dg] == np.arange(n)).all()

    def apply(r, order):
        v = LU.data.astype(r.dtype)
        t, z = r.copy(), np.zeros_like(r)
        for i in range(n):
            if dg[i] > rp[i]:
                t[i] = r[i] - _sum(v[rp[i]:dg[i]] * t[ci[rp[i]:dg[i]]], order)
        for i in range(n - 1, -1, -1):
            s = _sum(v[dg[i] + 1:rp[i + 1]] * z[ci[dg[i] + 1:rp[i + 1]]], order) if rp[i + 1] > dg[i] + 1 else 0
            z[i] = (t[i] - s) / v[dg[i]]
        return z
    return apply


# ---- endings and reuse -------------------------------------------------------------------------------------------------------------------
def indefinite(n=257, at=128):
    """tridiagonal(n) with A[at, at] = -2.5"""
    A = sp.lil_matrix(cm.tridiagonal(n))
    A[at, at] = -2.5
    return A.tocsr()


def check_reuse(ctx):
    """one CgWorkspace: an ordinary solve, a NaN in y, an Inf in x0, the ordinary solve again with the bits of the first"""
    n = 257
    case = cm.Case(ctx, cm.tridiagonal(n), "reuse", ncol=1)
    ws = npg.CgWorkspace(ctx, n)
    y, x0 = case.Y[0], case.X0[0]
    x1, st1, h1, _ = solve(ctx, case.A, case.P, y, x0, ws=ws, atol=1e-6, rtol=1e-6, itmax=200)
    assert st1["status"] == 1 and st1["niter"] > 8
    yn = y.copy()
    yn[n // 2] = np.nan
    _, st, h, _ = solve(ctx, case.A, case.P, yn, x0, ws=ws, atol=1e-6, rtol=1e-6, itmax=200)
    assert st["status"] == 3 and st["solved"] == 0 and st["niter"] <= 1 and len(h) == st["niter"] + 1, st
    xi = x0.copy()
    xi[n // 3] = np.inf
    _, st, h, _ = solve(ctx, case.A, case.P, y, xi, ws=ws, atol=1e-6, rtol=1e-6, itmax=200)
    assert st["status"] == 3 and st["solved"] == 0 and st["niter"] <= 1 and len(h) == st["niter"] + 1, st
    x2, st2, h2, _ = solve(ctx, case.A, case.P, y, x0, ws=ws, atol=1e-6, rtol=1e-6, itmax=200)
    print(f"cg reuse: first solve status {st1['status']} niter {st1['niter']}; after NaN and Inf: status {st2['status']} niter {st2['niter']}")
    assert st2["status"] == 1, st2
    assert cm.same_bits(x2, x1) and cm.same_bits(h2, h1)
    assert all(cm.same_bits(st2[key], st1[key]) for key in cm.KEYS)


def check_curvature(ctx):
    """p'Ap <= 0 ends the solve at once: status 3, the iterate / count / history of the last completed iteration.  The system and
    the reference are fixed by the seed, so the host and the device library are held to the same status and niter"""
    A = indefinite()
    n = A.shape[0]
    rng = np.random.default_rng(cm.SEED + 77)
    b, x0 = rng.standard_normal(n), rng.standard_normal(n)
    ref = Steps(A, np.ones(n), b, x0, 40, same_ending=True, atol=1e-6, rtol=1e-6)
    assert ref.status == 3 and 0 < ref.niter < 40, (ref.status, ref.niter)
    x, st, hist, _ = solve(ctx, npg.DeviceCSR.from_scipy(ctx, A), None, b, x0, atol=1e-6, rtol=1e-6, itmax=40)
    print(f"cg curvature: reference stops after {ref.niter} iterations; library: status {st['status']} niter {st['niter']} "
          f"history {len(hist)}")
    assert st["status"] == 3 and st["solved"] == 0, st
    assert st["niter"] == ref.niter
    assert len(hist) == st["niter"] + 1
    k = ref.niter
    dx = ref.dev_x(k, x)
    print(f"cg curvature: x dev {dx:.2e} noise {ref.noise_x[k]:.2e}")
    assert dx <= ref.bar_x(k), (dx, ref.noise_x[k])
    for j in range(k + 1):
        assert ref.dev_h(j, hist[j]) <= ref.bar_h(j), (j, ref.dev_h(j, hist[j]), ref.noise_h[j])
    # the all-zero matrix (stored zeros) with a non-zero y: p'Ap == 0 at the first step
    Z = sp.csr_matrix(cm.tridiagonal(n))
    Z.data[:] = 0.0
    xz, sz, hz, _ = solve(ctx, npg.DeviceCSR.from_scipy(ctx, Z), None, b, x0, atol=1e-6, rtol=1e-6, itmax=40)
    print(f"cg curvature: zero matrix: status {sz['status']} niter {sz['niter']}")
    assert sz["status"] == 3 and sz["solved"] == 0 and sz["niter"] == 0 and len(hz) == 1, sz
    nb = float(np.sqrt(np.sum(np.asarray(b, LD) ** 2)))
    assert cm.same_bits(xz, x0) and abs(hz[0] - nb) <= n * np.finfo(float).eps * nb       # r = b - 0 x0 = b; a sum of n squares
