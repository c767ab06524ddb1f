"""Restarted, left-preconditioned GMRES(memory) restated in fp64 numpy, step by step, with the rounding points of the device's
kernels (nupgcm_amd/csrc/gmres.hip) as switches - the yardstick of tests/test_gpu_gmres_steps.py.

What the device computes in one restart cycle, and where this restatement rounds:

  R1   r = P (b - A x), beta = ||r||                                 fp64 (the next SpMV input is r itself, scaled after the product)
  K1   v_j = wt / beta_j is STORED (fp32 with `basis32`); the SpMV reads wt, not the stored column, in fp64 or - `gather32`, the
       XG instances - from the fp32 copy of wt; w = P (A wt) / beta_j
  K2   h = V'w and wt = w - V h with V the STORED columns (fp32 with `basis32`), all sums fp64
  K1   the next column's norm: ||w||^2 - ||h||^2 (Pythagoras) while that is far from cancellation, the explicitly summed ||wt||^2
       otherwise (finalize_column: threshold max(eta^2, 1e-4) on one GPU); Givens rotations, residual estimate |zeta|
  XU   back substitution R y = z over the columns of the cycle, x += V y with V the STORED columns

Orthogonalisation: `passes=2` is classical Gram-Schmidt with two full passes (CGS2) and the explicit norm - the best fp64 answer,
independent of which columns the device's selective second-pass test picks; it is what the fp64 instances are compared with.
`passes=1` is the fast kernels' arithmetic (one classical pass, norm as above): with an fp32-stored basis V'V = I only to ~1e-7, so
a second pass would move every column by that much - the mirror of the fast fp32 instances has to leave it out as they do.  The
full kernels asked for eta > 1 take the second pass on every column, against the same stored columns: `passes=2` with `basis32`.

History layout = GmresWorkspace.history(): entry 0 is the first true residual, entry i the estimate after iteration i (a restart
adds no entry: the estimate of the first iteration of a cycle already rests on the cycle's true residual, so a wrong R1 shows in
the entry after every restart)."""
import numpy as np

BTOL = np.finfo(float).eps ** 0.75


def sym_givens(a, b):
    """Krylov.jl's sym_givens, as gmres.hip's sym_givens: (c, s, rho) with [c s; s -c] [a; b] = [rho; 0]"""
    if b == 0.0:
        return (1.0 if a == 0.0 else float(np.copysign(1.0, a))), 0.0, abs(a)
    if a == 0.0:
        return 0.0, float(np.copysign(1.0, b)), abs(b)
    if abs(b) > abs(a):
        t = a / b
        s = float(np.copysign(1.0, b)) / np.sqrt(1.0 + t * t)
        return s * t, s, b / s
    t = b / a
    c = float(np.copysign(1.0, a)) / np.sqrt(1.0 + t * t)
    return c, c * t, a / c


def _r32(v):
    return np.asarray(v, dtype=np.float32).astype(np.float64)


def gmres_steps(A, b, x0, memory, itmax, P=None, basis32=False, gather32=False, passes=2, pyth_eta=None, atol=0.0, rtol=0.0,
                xs_at=()):
    """A: scipy sparse (or dense) n x n, b, x0: fp64 vectors, P: None, a scalar or a vector (w = P A v).
    basis32: the stored basis columns (Gram-Schmidt sums, x += V y) are rounded to fp32; gather32: the SpMV input is rounded to fp32.
    passes: 2 = CGS2 with explicit norms; 1 = one classical pass, the norm by Pythagoras while ||w||^2 - ||h||^2 >= thr ||w||^2
    (thr = max(pyth_eta^2, 1e-4); pyth_eta=None: always the explicit norm).
    Returns dict(hist, x, H (one (m+1) x m Hessenberg matrix per cycle, as orthogonalised, before the rotations), V (the stored
    basis columns of every cycle, one per row), betas (the true
    residual norm every cycle started from), niter, status (1 solved, 2 itmax, 3 breakdown, 4 zero residual), xs: {k: the iterate
    a solve with itmax = k returns} for every k in xs_at)."""
    b = np.asarray(b, dtype=np.float64)
    n = b.size
    x = np.array(x0, dtype=np.float64)
    p = None if P is None else (np.float64(P) if np.isscalar(P) else np.asarray(P, dtype=np.float64))
    prec = (lambda v: v) if p is None else (lambda v: p * v)
    stored = _r32 if basis32 else (lambda v: v)
    spmv_in = _r32 if gather32 else (lambda v: v)
    thr = None if pyth_eta is None else max(pyth_eta * pyth_eta, 1e-4)
    hist, Hs, Vs, betas, xs = [], [], [], [], {}
    it, status, eps_ = 0, 0, None
    while status == 0:
        wt = prec(b - A @ x)                                  # R1
        beta = float(np.sqrt(wt @ wt))
        betas.append(beta)
        if eps_ is None:
            hist.append(beta)
            eps_ = atol + rtol * beta
            if beta == 0.0:
                status = 4
                break
        V = np.zeros((memory, n))
        H = np.zeros((memory + 1, memory))
        cs, sn, z = np.zeros(memory), np.zeros(memory), np.zeros(memory)
        R = np.zeros((memory, memory))
        zeta, hbis, kk = beta, beta, 0
        for j in range(memory):
            inv = 1.0 / hbis
            V[j] = stored(wt * inv)                           # K1: the stored column
            w = prec(A @ spmv_in(wt)) * inv                   # ... and the product of the UNROUNDED (or gather-copy) wt
            h = V[:j + 1] @ w                                 # K2: sums against the stored columns
            wt = w - V[:j + 1].T @ h
            if passes == 2:
                h2 = V[:j + 1] @ wt
                wt = wt - V[:j + 1].T @ h2
                h = h + h2
                n2 = wt @ wt
            else:
                wn2 = w @ w
                n2f = wn2 - h @ h
                n2 = max(n2f, 0.0) if (thr is not None and n2f >= thr * wn2) else wt @ wt
            hbis = float(np.sqrt(n2))
            H[:j + 1, j], H[j + 1, j] = h, hbis
            col = h.copy()                                    # previous rotations, then the new one
            for i in range(j):
                col[i], col[i + 1] = cs[i] * col[i] + sn[i] * col[i + 1], sn[i] * col[i] - cs[i] * col[i + 1]
            cs[j], sn[j], rho = sym_givens(col[j], hbis)
            col[j] = rho
            R[:j + 1, j] = col
            z[j] = cs[j] * zeta
            zeta = sn[j] * zeta
            rnorm = abs(zeta)
            it += 1
            kk = j + 1
            hist.append(rnorm)
            if it in xs_at:
                xs[it] = x + V[:kk].T @ _back_substitute(R, z, kk)
            if rnorm <= eps_ or rnorm + 1.0 <= 1.0:
                status = 1
            elif it >= itmax:
                status = 2
            elif hbis <= BTOL:
                status = 3
            if status:
                break
        Hs.append(H[:kk + 1, :kk].copy())
        Vs.append(V[:kk].copy())
        x = x + V[:kk].T @ _back_substitute(R, z, kk)         # XU
    return dict(hist=np.asarray(hist), x=x, H=Hs, V=Vs, betas=np.asarray(betas), niter=it, status=status, xs=xs)


def _back_substitute(R, z, kk):
    """k_gmres_update: column-oriented back substitution, a diagonal entry below BTOL gives a zero coefficient"""
    y = z[:kk].copy()
    for c in range(kk - 1, -1, -1):
        y[c] = 0.0 if abs(R[c, c]) <= BTOL else y[c] / R[c, c]
        y[:c] -= R[:c, c] * y[c]
    return y


def true_residual(A, b, x, P=None):
    """||P (b - A x)|| in fp64 on the host (what R1 forms on the device)"""
    r = np.asarray(b, dtype=np.float64) - A @ np.asarray(x, dtype=np.float64)
    if P is not None:
        r = (np.float64(P) if np.isscalar(P) else np.asarray(P)) * r
    return float(np.linalg.norm(r))
