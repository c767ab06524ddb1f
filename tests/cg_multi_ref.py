"""Synthetic SPD matrices and the checks shared by tests/test_cg_multi.py (host library) and tests/test_gpu_cg_multi.py (device): the
batched CG (npg_cg_multi_*, BatchedCgWorkspace) against the existing single-column solver (npg_cg_solve, CgWorkspace) on
the same context.  The tolerance is ZERO: per column the batched solve has the single solve's bits of x, and the same niter, status,
solved, rnorm0, rnorm and history.  Floats are compared as 64-bit patterns, so a NaN equals the same NaN.

Every matrix is the smallest at which one path of the product kernel can go wrong (sizes are in the builders' docstrings); lanes per
row follow npg_csr_create's rule on the mean row length: <= 12 -> 4, <= 64 -> 8, <= 256 -> 16, else 32 (`expected_lanes`)."""
import ctypes as C

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import nupgcm_amd as npg
from nupgcm_amd import _lib as L
from nupgcm_amd.architectures import Context

SEED = 20261018
KEYS = ("solved", "niter", "npass", "status", "nreorth", "nflagged", "rnorm0", "rnorm")
NEW = {"npg_cg_multi_create", "npg_cg_multi_destroy", "npg_cg_multi_solve", "npg_cg_multi_history"}
KW = dict(atol=1e-6, rtol=1e-6, itmax=0)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).reshape(-1).view(np.uint64)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and bool(np.array_equal(a, b))


# ---- matrices ----------------------------------------------------------------------------------------------------------------------------
def tridiagonal(n):
    """(-1, 2.5, -1): condition number below 9, a few dozen iterations.  n = 257: two tiles (256 rows + 1 row); n = 70 001: 274 tiles,
    more than the 256-workgroup cap (grid-stride loop over tiles, descriptor prefetch), and G2 = 69 < 256; 4 lanes per row"""
    if n == 1:
        return sp.csr_matrix(np.array([[2.5]]))
    return sp.diags([-1.0, 2.5, -1.0], [-1, 0, 1], shape=(n, n), format="csr")


def arrowhead(n=6000):
    """A[0, 0] = n, A[i, i] = 2, A[0, i] = A[i, 0] = 0.5: Schur complement n - 0.125 (n - 1) > 0.  Row 0 holds n entries, more than
    a tile's 5824 product slots: the whole-workgroup row path"""
    A = sp.lil_matrix((n, n))
    A.setdiag(2.0)
    A[0, :] = 0.5
    A[:, 0] = 0.5
    A[0, 0] = float(n)
    return A.tocsr()


def laplace7(m=20):
    """7-point Laplacian + identity on m^3 points: at most 7 entries per row -> 4 lanes; 8000 rows = 32 tiles"""
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(m, m))
    I = sp.identity(m)
    return (sp.kron(sp.kron(T, I), I) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(I, I), T) + sp.identity(m ** 3)).tocsr()


def banded(n, half):
    """A[i, j] = -1 / (1 + |i - j|) for 0 < |i - j| <= half, strictly dominant diagonal.  (n, half) = (300, 50): 93 entries per row
    on average -> 16 lanes; (300, 299): dense, 300 per row -> 32 lanes, 19 rows per tile"""
    i, j = np.indices((n, n))
    d = np.abs(i - j)
    A = np.where((d > 0) & (d <= half), -1.0 / (1.0 + d), 0.0)
    A[np.arange(n), np.arange(n)] = np.abs(A).sum(axis=1) + 1.0
    return sp.csr_matrix(A)


def expected_lanes(A):
    mean = A.nnz / A.shape[0]
    return 4 if mean <= 12 else 8 if mean <= 64 else 16 if mean <= 256 else 32


# ---- solves ------------------------------------------------------------------------------------------------------------------------------
class Case:
    """one matrix on one context with a preconditioner, ncol fixed right-hand sides and random warm starts; the single-column solves
    of those columns are made once and shared"""

    def __init__(self, ctx, A, label, ncol=8, precond="jacobi", A_dev=None, P=None, seed=SEED):
        self.ctx, self.label = ctx, label
        self.As = sp.csr_matrix(A)
        self.n = self.As.shape[0]
        rng = np.random.default_rng(seed)
        self.Y = rng.standard_normal((ncol, self.n))
        self.X0 = rng.standard_normal((ncol, self.n))
        self.A = A_dev if A_dev is not None else npg.DeviceCSR.from_scipy(ctx, self.As)
        if P is not None:
            self.P = P
        elif precond == "jacobi":
            self.P = npg.Diagonal(npg.DeviceVector.from_host(ctx, 1.0 / self.As.diagonal()))
        elif precond == "scalar":
            self.P = npg.Diagonal(scalar=1.0 / float(self.As.diagonal().mean()), n=self.n)
        else:
            self.P = None
        self._single = {}

    def with_precond(self, precond):
        return Case(self.ctx, self.As, f"{self.label} {precond}", ncol=len(self.Y), precond=precond, A_dev=self.A)

    def solve_single(self, y, x0, **kw):
        ws = npg.CgWorkspace(self.ctx, self.n)
        x = npg.DeviceVector.from_host(self.ctx, x0)
        st = ws.solve(self.A, npg.DeviceVector.from_host(self.ctx, y), x, self.P, **{**KW, **kw})
        return x.to_host(), st, ws.history().copy()

    def single(self, k, **kw):
        key = (k, tuple(sorted(kw.items())))
        if key not in self._single:
            self._single[key] = self.solve_single(self.Y[k], self.X0[k], **kw)
        return self._single[key]

    def solve_batched(self, Y, X0, ws=None, **kw):
        Y, X0 = np.atleast_2d(Y), np.atleast_2d(X0)
        K = len(Y)
        ws = ws or npg.BatchedCgWorkspace(self.ctx, self.n, K)
        x = npg.DeviceVector.from_host(self.ctx, X0.reshape(-1))
        st = ws.solve(self.A, npg.DeviceVector.from_host(self.ctx, Y.reshape(-1)), x, self.P, **{**KW, **kw})
        assert len(st) == K and ws.stats is st
        return x.to_host().reshape(K, self.n), st, [ws.history(k).copy() for k in range(K)]


def compare(label, k, got, ref):
    """column k of a batched solve against its single solve: bits of x, statistics, history"""
    (x, st, hist), (xr, sr, hr) = got, ref
    assert same_bits(x, xr), f"{label} column {k}: x differs in {int(np.count_nonzero(bits(x) != bits(xr)))} of {len(xr)} entries"
    for key in KEYS:
        assert same_bits(st[key], sr[key]), f"{label} column {k}: {key} {st[key]!r} != {sr[key]!r}"
    assert same_bits(hist, hr), f"{label} column {k}: history"
    assert len(hist) == sr["niter"] + 1


def check_columns(case, cols, ws=None, **kw):
    """the columns `cols` of the case in ONE batched call against their single solves; returns the batched statistics"""
    cols = list(cols)
    X, st, hist = case.solve_batched(case.Y[cols], case.X0[cols], ws=ws, **kw)
    for j, k in enumerate(cols):
        compare(f"{case.label} K={len(cols)}", k, (X[j], st[j], hist[j]), case.single(k, **kw))
    print(f"cg_multi {case.label}: K = {len(cols)}, niter {[s['niter'] for s in st]}, status {[s['status'] for s in st]}")
    return st


def check_special(case, Y, X0, special, want_status, **kw):
    """columns given explicitly (one of them, `special`, ends differently) in one batched call, each against its own single solve"""
    X, st, hist = case.solve_batched(Y, X0, **kw)
    ref = [case.solve_single(Y[k], X0[k], **kw) for k in range(len(Y))]
    for k in range(len(Y)):
        compare(f"{case.label} special", k, (X[k], st[k], hist[k]), ref[k])
    print(f"cg_multi {case.label}: special column {special}: status {st[special]['status']} after {st[special]['niter']} iterations; "
          f"all: niter {[s['niter'] for s in st]}, status {[s['status'] for s in st]}")
    assert st[special]["status"] == want_status
    return st, X


# ---- columns that end differently --------------------------------------------------------------------------------------------------------
def check_endings(case):
    """each special column sits at position 1 of three, beside two ordinary columns"""
    n = case.n
    Y, X0 = case.Y[:3].copy(), case.X0[:3].copy()
    # zero right-hand side with a zero start: status 4
    Y4, X4 = Y.copy(), X0.copy()
    Y4[1], X4[1] = 0.0, 0.0
    st, X = check_special(case, Y4, X4, 1, 4)
    assert st[1]["niter"] == 0 and not X[1].any() and st[0]["status"] == st[2]["status"] == 1
    # a start that already satisfies the stopping rule: status 1 after 0 iterations (the residual of a direct solve is far below atol)
    X1 = X0.copy()
    X1[1] = spla.spsolve(sp.csc_matrix(case.As), Y[1]) if n > 1 else Y[1] / case.As[0, 0]
    st, X = check_special(case, Y, X1, 1, 1)
    assert st[1]["niter"] == 0 and same_bits(X[1], X1[1])
    # itmax = 3 on columns that need more: status 2 (every column of the call has the same itmax, as in the single solver)
    st, _ = check_special(case, Y, X0, 1, 2, itmax=3)
    assert [s["niter"] for s in st] == [3, 3, 3]
    # a NaN in one column's right-hand side: status 3, the others untouched by it
    Yn = Y.copy()
    Yn[1, n // 2] = np.nan
    st, X = check_special(case, Yn, X0, 1, 3)
    assert st[0]["status"] == st[2]["status"] == 1 and np.isfinite(X[0]).all() and np.isfinite(X[2]).all()
    # a column that finishes many iterations before the slowest one: its x is the single solve's, so it was frozen
    Xf = X0.copy()
    Xf[1] = (spla.spsolve(sp.csc_matrix(case.As), Y[1]) if n > 1 else Y[1] / case.As[0, 0]) * (1.0 + 1e-5)
    st, _ = check_special(case, Y, Xf, 1, 1)
    slow = max(st[0]["niter"], st[2]["niter"])
    assert 0 < st[1]["niter"] <= slow - 8, (st[1]["niter"], slow)       # at least two host checks (every 4 iterations) earlier
    check_reuse_after_nonfinite(case.ctx)
    check_curvature_column(case.ctx)


def check_reuse_after_nonfinite(ctx):
    """one BatchedCgWorkspace, K = 3 in every call: an ordinary solve, a NaN in column 1's y, an Inf in column 1's x0, the ordinary
    solve again - with the bits of the first one, and every column of every call with the bits of its single solve"""
    case = Case(ctx, tridiagonal(257), "tridiagonal n=257 reuse", ncol=3)
    n, kw = case.n, dict(itmax=200)
    ws = npg.BatchedCgWorkspace(ctx, n, 3)
    Y, X0 = case.Y, case.X0
    first = case.solve_batched(Y, X0, ws=ws, **kw)
    assert [s["status"] for s in first[1]] == [1, 1, 1]
    Yn, Xi = Y.copy(), X0.copy()
    Yn[1, n // 2] = np.nan
    Xi[1, n // 3] = np.inf
    for Yp, Xp in ((Yn, X0), (Y, Xi)):
        X, st, hist = case.solve_batched(Yp, Xp, ws=ws, **kw)
        assert st[1]["status"] == 3 and st[1]["solved"] == 0 and st[1]["niter"] <= 1 and len(hist[1]) == st[1]["niter"] + 1, st[1]
        for k in range(3):
            compare(f"{case.label} poisoned", k, (X[k], st[k], hist[k]), case.solve_single(Yp[k], Xp[k], **kw))
        assert st[0]["status"] == st[2]["status"] == 1
    again = case.solve_batched(Y, X0, ws=ws, **kw)
    print(f"cg_multi {case.label}: status {[s['status'] for s in first[1]]} before, {[s['status'] for s in again[1]]} after a NaN and an Inf")
    for k in range(3):
        compare(f"{case.label} again", k, (again[0][k], again[1][k], again[2][k]), (first[0][k], first[1][k], first[2][k]))
        compare(f"{case.label} again", k, (again[0][k], again[1][k], again[2][k]), case.single(k, **kw))


def check_curvature_column(ctx):
    """tridiagonal(257) with A[128, 128] = -2.5, no preconditioner, itmax = 40.  Column 1 starts at 0 with y = e_128: p'Ap = -2.5 at
    the first step, status 3 after 0 iterations with x untouched.  Columns 0 and 2 start at 0 with right-hand sides supported on rows
    0 .. 59 and 200 .. 256: a tridiagonal Krylov space widens by one row per iteration, so within 40 iterations they never meet row
    128 and are ordinary positive-definite solves.  Every column has the bits of its single solve."""
    n, at = 257, 128
    A = sp.lil_matrix(tridiagonal(n))
    A[at, at] = -2.5
    case = Case(ctx, A.tocsr(), "indefinite tridiagonal n=257", ncol=3, precond="none")
    Y, X0 = np.zeros((3, n)), np.zeros((3, n))
    Y[0, :60], Y[2, 200:] = case.Y[0, :60], case.Y[2, 200:]
    Y[1, at] = 1.0
    st, X = check_special(case, Y, X0, 1, 3, itmax=40)
    assert st[1]["niter"] == 0 and st[1]["solved"] == 0 and not X[1].any()
    assert st[0]["status"] == st[2]["status"] == 1 and 8 < st[0]["niter"] < 40 and 8 < st[2]["niter"] < 40, st
    for k in (0, 2):                                        # and they solved their systems
        assert np.abs(case.As @ X[k] - Y[k]).max() <= 1e-5 * np.abs(Y[k]).max()
    # a random column meets the negative entry after a few steps: status 3 there, with the single solve's bits beside two ordinary ones
    Yr, Xr = Y.copy(), X0.copy()
    Yr[1], Xr[1] = case.Y[1], case.X0[1]
    st, _ = check_special(case, Yr, Xr, 1, 3, itmax=40)
    assert 0 < st[1]["niter"] < 40 and st[0]["status"] == st[2]["status"] == 1
    # the all-zero matrix (stored zeros): p'Ap == 0 at the first step of every column
    Z = sp.csr_matrix(tridiagonal(n))
    Z.data[:] = 0.0
    zero = Case(ctx, Z, "zero matrix n=257", ncol=3, precond="none")
    X, st, hist = zero.solve_batched(zero.Y, zero.X0, itmax=40)
    for k in range(3):
        compare(zero.label, k, (X[k], st[k], hist[k]), zero.single(k, itmax=40))
        assert st[k]["status"] == 3 and st[k]["niter"] == 0 and st[k]["solved"] == 0 and same_bits(X[k], zero.X0[k])


def check_independence(case):
    """column k's bits: in a K = 5 call, in the call with the columns reversed, alone; two identical calls"""
    cols = [0, 1, 2, 3, 4]
    ws = npg.BatchedCgWorkspace(case.ctx, case.n, 5)
    check_columns(case, cols)
    check_columns(case, cols[::-1])
    for k in cols:
        check_columns(case, [k])
    a = case.solve_batched(case.Y[cols], case.X0[cols], ws=ws)
    b = case.solve_batched(case.Y[cols], case.X0[cols], ws=ws)          # the same workspace again
    for k in cols:
        compare(f"{case.label} repeated", k, (b[0][k], b[1][k], b[2][k]), (a[0][k], a[1][k], a[2][k]))


def grouped_solve(case, Y, X0, cap=L.NPG_CG_MULTI_MAX):
    """PassiveTracers' grouping: one stacked c, one BatchedCgWorkspace per group of at most `cap` columns whose x is the group's window"""
    K, n = Y.shape
    c = npg.DeviceVector.from_host(case.ctx, X0.reshape(-1))
    y = npg.DeviceVector.from_host(case.ctx, Y.reshape(-1))
    stats, hists, groups = [], [], []
    for k0 in range(0, K, cap):
        kc = min(cap, K - k0)
        ws = npg.BatchedCgWorkspace(case.ctx, n, kc)
        ws.x = c.view(k0 * n, kc * n)
        groups.append(kc)
        stats.extend(ws.solve(case.A, y.view(k0 * n, kc * n), ws.x, case.P, **KW))
        hists.extend(ws.history(k).copy() for k in range(kc))
        assert same_bits(ws.view(kc - 1).to_host(), c.view((k0 + kc - 1) * n, n).to_host())
    return c.to_host().reshape(K, n), stats, hists, groups


def check_cap_and_grouping(ctx):
    """K = 32 (the cap) in one call and K = 33 in two groups, on the n = 257 tridiagonal"""
    case = Case(ctx, tridiagonal(257), "tridiagonal n=257", ncol=33)
    check_columns(case, range(32))
    X, st, hist, groups = grouped_solve(case, case.Y, case.X0)
    assert groups == [32, 1]
    for k in range(33):
        compare("tridiagonal n=257 grouped K=33", k, (X[k], st[k], hist[k]), case.single(k))
    with np.testing.assert_raises(L.DeviceError):
        npg.BatchedCgWorkspace(ctx, 257, 33)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def _refused(fn, needle):
    try:
        fn()
    except L.DeviceError as e:
        assert e.code == -1 and needle in str(e), str(e)
        return
    raise AssertionError(f"not refused: expected NPG_EINVAL with '{needle}'")


def check_refusals(ctx, device, blocked=None):
    """every refusal of npg_cg_multi_create / _solve: NPG_EINVAL with its message, x untouched"""
    n, K = 257, 3
    case = Case(ctx, tridiagonal(n), "refusals", ncol=K)
    lib = L.lib()
    for bad in (0, -1, 33):
        _refused(lambda: npg.BatchedCgWorkspace(ctx, n, bad), "ncol_max")
    _refused(lambda: L.check(lib.npg_cg_multi_create(ctx.h, n, 2, None)), "bad argument")
    ws = npg.BatchedCgWorkspace(ctx, n, K)
    y = npg.DeviceVector.from_host(ctx, case.Y.reshape(-1))
    x = npg.DeviceVector.from_host(ctx, case.X0.reshape(-1))
    before = x.to_host()
    kind, s, dh = case.P.kind()

    def call(A=case.A, kind=kind, dh=dh, ncol=K, y=y, x=x, w=ws):
        st = (L.SolveStats * 40)()
        L.check(lib.npg_cg_multi_solve(w.h if w is not None else None, A.h if A is not None else None, kind, s, dh, ncol,
                                       y.h if y is not None else None, x.h if x is not None else None, 1e-6, 1e-6, 0, st))

    for kw in (dict(A=None), dict(y=None), dict(x=None), dict(w=None)):
        _refused(lambda: call(**kw), "NULL argument")
    for bad in (0, -2, K + 1):
        _refused(lambda: call(ncol=bad), "the workspace holds 1 .. 3 columns")
    short = npg.DeviceVector(ctx, 2 * n)
    _refused(lambda: call(y=short), "columns want vectors of")
    _refused(lambda: call(x=short), "columns want vectors of")
    _refused(lambda: call(ncol=2), "columns want vectors of")                      # two columns, vectors of three
    other = npg.DeviceCSR.from_scipy(ctx, tridiagonal(n + 1))
    _refused(lambda: call(A=other), "but A is 258x258")
    _refused(lambda: call(kind=L.NPG_PRECOND_DIAG, dh=None), "bad preconditioner")
    _refused(lambda: call(kind=L.NPG_PRECOND_DIAG, dh=short.h), "bad preconditioner")
    _refused(lambda: call(kind=7), "bad preconditioner")
    ctx2 = Context(ctx.device)                                  # a second context of the same library (contexts live as long as the process)
    y2 = npg.DeviceVector.from_host(ctx2, case.Y.reshape(-1))
    x2 = npg.DeviceVector.from_host(ctx2, case.X0.reshape(-1))
    A2 = npg.DeviceCSR.from_scipy(ctx2, case.As)
    for kw in (dict(y=y2), dict(x=x2), dict(A=A2)):
        _refused(lambda: call(**kw), "must belong to one context")
    assert same_bits(x2.to_host(), case.X0)
    if device:
        # record form and internal renumbering: a 6 x 6 matrix of two (x, y, z) nodes with the {K, C} = {2, 0.5} node-block structure
        w6 = npg.BatchedCgWorkspace(ctx, 6, 1)
        v6 = npg.DeviceVector.from_host(ctx, np.ones(6))
        x6 = npg.DeviceVector.from_host(ctx, np.arange(6.0))
        node = np.array([[2.0, 0.5, 0.0], [-0.5, 2.0, 0.0], [0.0, 0.0, 2.0]])
        A6 = sp.block_diag([node, node], format="csr")
        packed = npg.DeviceCSR.from_scipy(ctx, A6)
        assert packed.pack_nodes(2, 0)
        renum = npg.DeviceCSR.from_scipy(ctx, A6)
        assert renum.block_nodes_dofs([0, 0, 0, 1, 1, 1], [0, 1, 2, 0, 1, 2])
        for A, needle in ((packed, "full node records"), (renum, "internal renumbering")):
            _refused(lambda: call(A=A, kind=L.NPG_PRECOND_NONE, dh=None, ncol=1, y=v6, x=x6, w=w6), needle)
        if blocked is not None:            # a matrix stored by node blocks (the model's inversion matrix): plain CSR only
            nA = blocked.shape[0]
            wA, vA = npg.BatchedCgWorkspace(ctx, nA, 1), npg.DeviceVector(ctx, nA)
            _refused(lambda: call(A=blocked, kind=L.NPG_PRECOND_NONE, dh=None, ncol=1, y=vA, x=vA, w=wA), "plain CSR only")
        assert same_bits(x6.to_host(), np.arange(6.0))
    assert same_bits(x.to_host(), before)
    assert ws.history(0).size == 0                                              # nothing was solved
    call()                                                                      # and the same arguments, unbroken, are served
    assert not same_bits(x.to_host(), before)


def check_exports():
    assert NEW <= set(L.declared_symbols())
    for path in (L.HOST_LIB_PATH, L.LIB_PATH):
        lib = C.CDLL(path)
        assert not [s for s in NEW if not hasattr(lib, s)], path
    assert npg.BatchedCgWorkspace is npg.iterative_solvers.BatchedCgWorkspace and L.NPG_CG_MULTI_MAX == 32


# ---- tracers -----------------------------------------------------------------------------------------------------------------------------
SPECS4 = [dict(name="age", dirichlet=lambda x: 0.3 + 0.5 * x[..., 0], gamma=0.0, source=1.0, flux=None),
          dict(name="dye", dirichlet=-0.7, gamma=1.7, source=-0.4, flux=lambda x: 2e-2 * np.cos(2.0 * x[..., 1])),
          dict(name="salt", dirichlet=lambda x: np.cos(3.0 * x[..., 0]) + x[..., 1] + x[..., 2], gamma=-0.6, source=0.25, flux=0.05),
          dict(name="heat", dirichlet=0.2, gamma=0.9, source=0.1, flux=lambda x: -1e-2 * np.sin(x[..., 0]))]


def check_tracers(arch, build_model, expect_batched):
    """bowl_mixing, 3 steps of run() with 4 tracers: batched=True against batched=False to the bit, and u, p, b' against a run
    without tracers"""
    runs = {}
    for mode in (None, False, True):
        m = build_model("bowl_mixing", nsteps=3, arch=arch)
        if mode is not None:
            m.tracers = npg.PassiveTracers(m, SPECS4, batched=mode)
            assert m.tracers.batched == (mode and expect_batched) and len(m.tracers.groups) == (1 if mode and expect_batched else 0)
        npg.run(m)
        runs[mode] = m
    a, b = runs[False].tracers, runs[True].tracers
    for name in ("c", "c_prev", "c_curr"):
        assert same_bits(getattr(a, name).to_host(), getattr(b, name).to_host()), name
    assert len(a.stats) == len(b.stats) == 3
    for i in range(3):
        assert len(a.stats[i]) == len(b.stats[i]) == 4
        for k in range(4):
            for key in a.stats[i][k]:
                if key != "seconds":
                    assert same_bits(a.stats[i][k][key], b.stats[i][k][key]), (i, k, key)
    print(f"cg_multi tracers: niter per step and tracer {[[s['niter'] for s in st] for st in b.stats]}")
    assert min(np.abs(b.values(k)).max() for k in range(4)) > 0.0
    for name in ("u", "p", "b"):
        for mode in (False, True):
            assert same_bits(getattr(runs[None].state, name), getattr(runs[mode].state, name)), (name, mode)
