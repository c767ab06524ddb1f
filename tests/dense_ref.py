"""Inputs, extended-precision reference and componentwise error bounds for the explicit dense inverse of nupgcm_amd/csrc/dense_inv.hip
(k_dense_gemv_part<double> / k_dense_gemv_part4 / k_dense_gemv_part8h + k_dense_gemv_sum) - the yardstick of
tests/test_gpu_dense_inverse.py, guarded without a GPU by tests/test_dense_ref.py.

The kernels' structure sets the sizes (SIZES): 512-column chunks, four columns per trip of a software-pipelined loop with a tail
taken column by column, 4 (fp32) or 8 (fp16) adjacent rows per thread read from a padded leading dimension, 256 threads per
workgroup.

Bounds.  z = M r with M the stored inverse, |z - z_ref|_i bounded row by row through S = |A^-1| |r|, eps = 4 n 2^-53 for the fp64
products and sums of a row (and the error of the fp64 inverse that is rounded):

  fp32 storage          (2^-24 + eps) S_i                         every entry rounded once to 24 bits, products and sums fp64
  scaled fp16 storage   (2^-11 + 2^-24 + 513 2^-24 + eps) S_i     entry / cs_j rounded to 11 bits; x_j cs_j rounded to fp32; fp32
                        + 2^-25 sum_j |r_j| cs_j                  sums over at most 512 columns and the conversion; entries below
                                                                  2^-14 cs_j are fp16 subnormals: absolute spacing 2^-24 cs_j

Nothing in them is fitted to a result."""
import functools

import numpy as np
import scipy.sparse as sp

SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 511, 512, 513, 515, 1025, 1031, 2053)
CHUNK = 512            # kGemvChunkCols


def system(n):
    """non-symmetric, strictly diagonally dominant sparse matrix (CSR, sorted): about 6 random off-diagonals per row, diagonal
    +-(rowsum + 1) U(1.5, 2.5); seed = n"""
    rng = np.random.default_rng(n)
    k = min(6, n - 1)
    rows = np.repeat(np.arange(n), k)
    cols = rng.integers(0, n, size=n * k)
    vals = rng.standard_normal(n * k)
    keep = rows != cols
    off = sp.csr_matrix((vals[keep], (rows[keep], cols[keep])), shape=(n, n))
    rowsum = np.asarray(abs(off).sum(axis=1)).ravel()
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    diag = sign * (rowsum + 1.0) * rng.uniform(1.5, 2.5, n)
    A = sp.csr_matrix(off + sp.diags(diag))
    A.sort_indices()
    return A


def unit_columns(n):
    return sorted({j for j in (0, 3, 511, 512, n - (n % 4) - 1, n - 1) if 0 <= j < n})


def right_hand_sides(n):
    """columns: standard_normal(n) (no magnitude spread: a dropped column cannot hide), then the unit vectors e_j"""
    rng = np.random.default_rng(n + 1000003)
    js = unit_columns(n)
    R = np.zeros((n, 1 + len(js)))
    R[:, 0] = rng.standard_normal(n)
    for c, j in enumerate(js):
        R[j, 1 + c] = 1.0
    return R


def solve_extended(Ad, R):
    """A^-1 R to extended precision: np.linalg.solve, then iterative refinement with the residual formed in np.longdouble, until
    the correction is below 1e-18 relative"""
    assert np.finfo(np.longdouble).eps < 2e-19, "np.longdouble must be an extended type"
    Al = Ad.astype(np.longdouble)
    Rl = R.astype(np.longdouble)
    Z = np.linalg.solve(Ad, R).astype(np.longdouble)
    for _ in range(8):
        res = Rl - Al @ Z
        dZ = np.linalg.solve(Ad, res.astype(np.float64))
        Z = Z + dZ
        if np.all(np.abs(dZ).max(axis=0) <= 1e-18 * np.abs(Z).max(axis=0)):
            return Z
    raise AssertionError("iterative refinement did not reach 1e-18")


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(n):
    """everything a test needs at size n, computed once and read-only"""
    c = Case()
    c.n = n
    c.A = system(n)
    Ad = c.A.toarray()
    c.R = right_hand_sides(n)
    c.Zref = solve_extended(Ad, c.R)
    c.inv = np.linalg.inv(Ad)
    c.cond = np.linalg.cond(Ad)
    c.S = np.abs(c.inv) @ np.abs(c.R)
    c.cs = np.abs(c.inv).max(axis=0)
    c.sub = np.abs(c.R).T @ c.cs                                        # sum_j |r_j| cs_j, per right-hand side
    eps = 4.0 * n * 2.0 ** -53
    c.bound32 = (2.0 ** -24 + eps) * c.S
    c.bound16 = (2.0 ** -11 + 2.0 ** -24 + 513 * 2.0 ** -24 + eps) * c.S + 2.0 ** -25 * c.sub[None, :]
    # fp64 storage: what an explicit inverse of LAPACK's (getrf + getri) gives on the host; the device forms the same matrix
    # from rocSOLVER's getrf + getrs against the identity - one rounded inverse of the same conditioning, then one product
    c.e_np_columns = (np.linalg.norm((c.inv @ c.R).astype(np.longdouble) - c.Zref, axis=0)
                      / np.linalg.norm(c.Zref, axis=0)).astype(np.float64)
    c.e_np = float(c.e_np_columns.max())
    for a in (c.R, c.Zref, c.inv, c.S, c.cs, c.sub, c.bound32, c.bound16):
        a.setflags(write=False)
    return c


def worst_ratio(Z, Zref, bound):
    """max_i |z - z_ref|_i / bound_i (bound_i = 0 admits no error)"""
    err = np.abs(np.asarray(Z).astype(np.longdouble) - Zref).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(q.max())


def emulate_fp32(inv, R):
    return inv.astype(np.float32).astype(np.float64) @ R


def emulate_fp16(inv, R):
    """the fp16 path's arithmetic: columns scaled by their largest magnitude, entries fp64 -> fp32 -> fp16, x cs rounded to fp32,
    fp32 fused multiply-adds over each 512-column chunk in column order, chunks summed in fp64"""
    n = inv.shape[0]
    cs = np.abs(inv).max(axis=0)
    cs[cs == 0] = 1.0
    Mh = (inv / cs).astype(np.float32).astype(np.float16).astype(np.float64)
    X = (R * cs[:, None]).astype(np.float32).astype(np.float64)
    Z = np.zeros(R.shape)
    for j0 in range(0, n, CHUNK):
        a = np.zeros(R.shape, dtype=np.float32)
        for j in range(j0, min(n, j0 + CHUNK)):
            a = (a.astype(np.float64) + Mh[:, j:j + 1] * X[j:j + 1, :]).astype(np.float32)
        Z += a.astype(np.float64)
    return Z


def probe_vectors(n):
    """the two probe vectors of the library's own fp16 acceptance check (dense_build), as columns"""
    i = np.arange(n, dtype=np.int64)
    return np.stack([np.sin(0.37 * i) + 0.5, np.where((i * 2654435761) & 64, 1.0, -1.0) * (1.0 + (i % 7))], axis=1)


def acceptance_statistics(Y64, Y16):
    """that check's statistics: relative row errors of the fp16 results against the fp64 ones over the rows above 1e-8 of the
    largest; the library keeps fp16 while median <= 5e-3 and 99th percentile <= 0.2.  Returns [(median, p99)] per probe."""
    out = []
    for a, b in zip(Y64.T, Y16.T):
        ok = np.abs(a) > 1e-8 * np.abs(a).max()
        r = np.sort(np.abs(b[ok] - a[ok]) / np.abs(a[ok]))
        if len(r):
            out.append((float(r[len(r) // 2]), float(r[int(0.99 * (len(r) - 1))])))
    return out
