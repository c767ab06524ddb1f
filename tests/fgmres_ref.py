"""Inputs and reference runs for tests/test_gpu_fgmres_steps.py: unpreconditioned flexible GMRES (npg_fgmres_solve) against
oracle.mg_oracle.fgmres, iteration by iteration.

The tolerance of a case comes from the reference alone: the restatement is run on the system as given and on the same system
with its rows and columns symmetrically permuted - the same mathematics, other summation orders.  The largest relative difference
of the two residual histories, and of the two solutions mapped back, is the rounding floor of the case."""
import functools

import numpy as np
import scipy.sparse as sp

from oracle import mg_oracle as mo

SCALE, RTOL = 3.0, 1e-10


def system(n):
    """diagonal linspace(1, 200, n), shuffled, plus a sparse non-symmetric perturbation (about 4 entries per row, magnitude 0.3);
    right-hand side and a non-zero warm start; seed = n"""
    rng = np.random.default_rng(n)
    d = np.linspace(1.0, 200.0, n)
    rng.shuffle(d)
    k = min(4, n - 1)
    rows = np.repeat(np.arange(n), k)
    cols = rng.integers(0, n, size=n * k)
    vals = 0.3 * rng.standard_normal(n * k)
    keep = rows != cols
    A = sp.csr_matrix(sp.csr_matrix((vals[keep], (rows[keep], cols[keep])), shape=(n, n)) + sp.diags(d))
    A.sort_indices()
    b = rng.standard_normal(n)
    x0 = 0.1 * rng.standard_normal(n)
    return A, b, x0


class Ref:
    pass


@functools.lru_cache(maxsize=None)
def reference(n, memory, itmax=0):
    """the restatement's run and the rounding floors of the case (read-only)"""
    A, b, x0 = system(n)
    kw = dict(m=memory, scale=SCALE, atol=0.0, rtol=RTOL, itmax=itmax)
    x, st = mo.fgmres(A, b, None, x0=x0, **kw)
    p = np.random.default_rng(n + 7919 * memory).permutation(n)
    Ap = sp.csr_matrix(A[p][:, p])
    Ap.sort_indices()
    xp, sp_ = mo.fgmres(Ap, b[p], None, x0=x0[p], **kw)
    xb = np.empty(n)
    xb[p] = xp
    h, hp = np.array(st["residuals"]), np.array(sp_["residuals"])
    r = Ref()
    r.A, r.b, r.x0, r.x, r.stats, r.hist = A, b, x0, x, st, h
    r.same_niter = st["niter"] == sp_["niter"]
    m = min(len(h), len(hp))
    big = h[:m] > 1e-13 * h[0]
    r.floor_hist = float(np.max(np.abs(h[:m] - hp[:m])[big] / h[:m][big]))
    r.floor_x = float(np.linalg.norm(xb - x) / np.linalg.norm(x))
    r.tol_hist = max(1e-6, 100.0 * r.floor_hist)
    r.tol_x = max(1e-9, 100.0 * r.floor_x)
    for a in (r.b, r.x0, r.x, r.hist):
        a.setflags(write=False)
    return r
