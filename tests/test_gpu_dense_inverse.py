"""The explicit dense inverse of csrc/dense_inv.hip at the edge sizes of its kernels, against an extended-precision reference with
derived componentwise bounds (tests/dense_ref.py): k_dense_gemv_part<double>, k_dense_gemv_part4 (fp32 storage),
k_dense_gemv_part8h (column-scaled fp16 storage), k_dense_gemv_sum, k_to_float_ld, k_to_half_ld, k_col_absmax.

Two routes reach them: NPG_PC_DENSE (fp64 / fp32 storage) and a one-level multigrid whose cycle IS dense_apply(b, x, 1, 0)
(fp64 / fp32 / fp16 storage; applied twice, so the second application replays the captured graph).  Which storage ran is read
from cycle_bytes(): a fall-back from fp16 to fp32 changes it.

Sizes (dense_ref.SIZES): n < 4, n < 8 - one thread, mostly padding rows; 513 / 515 / 1031 - a last chunk of 1 / 3 / 7 columns
(no whole trip; tail only; one trip, three tail columns, nothing prefetched); 1025 / 2053 - a second workgroup of the fp32 /
fp16 kernel, 2053 with five chunks; 255 - 257 - the workgroup edge of the fp64 kernel.

fp64 storage has no derivable bound (rocSOLVER's constants): the yardstick is what an explicit inverse gives in numpy on the
same system (LAPACK's getrf + getri; the device's comes from rocSOLVER's getrf + getrs against the identity - either way a
rounded inverse of a matrix of condition number below 25, then one product), e_np = max over the right-hand sides of
||inv(A) r - z_ref|| / ||z_ref||, measured on the host:

      n     e_np          n     e_np          n     e_np
      1   9.0e-17         8   1.7e-16       512   6.0e-16
      2   2.2e-16         9   2.1e-16       513   5.5e-16
      3   8.9e-17       255   6.2e-16       515   5.7e-16
      4   8.2e-17       256   8.0e-16      1025   6.1e-16
      5   1.3e-16       257   4.9e-16      1031   6.7e-16
      7   1.2e-16       511   5.5e-16      2053   6.7e-16

and the device must stay within 16 max(e_np, n 2^-53) for every right-hand side (16: other pivot ties and blocking, and getrs
in place of getri; the device measured at most 0.062 of that bar, at n = 2, and 0.002 at n >= 255).  This is the comparison that rocsolver_dgetri failed at
n = 255 and n = 511, by 1e12 (profiles/dense_inverse_getri.txt)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

import nupgcm_amd as npg  # noqa: E402
from nupgcm_amd import _lib as L  # noqa: E402
from nupgcm_amd import multigrid as mgm  # noqa: E402
from tests import dense_ref as dr  # noqa: E402


@pytest.fixture(scope="module")
def arch():
    a = npg.GPU()
    a.ctx
    return a


def _expected_bytes(n, storage):
    elem, ld = {"fp16": (2, (n + 7) // 8 * 8), "fp32": (4, (n + 3) // 4 * 4), "fp64": (8, n)}[storage]
    return elem * n * ld + 16 * (-(-n // dr.CHUNK)) * n + 24 * n


def _apply_columns(P, ctx, R, twice):
    """P applied to every column of R through ONE pair of device vectors; `twice`: each application repeated into a poisoned
    output - the replay of the captured graph - and required to give the same bits"""
    n = R.shape[0]
    r, z = npg.DeviceVector(ctx, n), npg.DeviceVector(ctx, n)
    Z = np.empty(R.shape)
    for c in range(R.shape[1]):
        r.upload(np.ascontiguousarray(R[:, c]))
        z.fill(np.nan)
        Z[:, c] = P.apply(r, z).to_host()
        if twice:
            z.fill(np.nan)
            assert np.array_equal(P.apply(r, z).to_host(), Z[:, c]), f"column {c}: the replayed application differs"
    return Z


def _check(c, storage, Z, what):
    if storage == "fp64":
        err = np.linalg.norm(Z.astype(np.longdouble) - c.Zref, axis=0) / np.linalg.norm(c.Zref, axis=0)
        bar = 16.0 * np.maximum(c.e_np_columns, c.n * 2.0 ** -53)
        print(f"{what} n = {c.n} fp64: error / bar {float(np.max(err / bar)):.3f}")
        assert np.all(err <= bar), (what, c.n, err, bar)
    else:
        q = dr.worst_ratio(Z, c.Zref, c.bound32 if storage == "fp32" else c.bound16)
        print(f"{what} n = {c.n} {storage}: error / bound {q:.3f}")
        assert q <= 1.0, (what, c.n, storage, q)


@pytest.mark.parametrize("n", dr.SIZES)
def test_dense_inverse_preconditioner_at_edge_sizes(arch, n):
    """NPG_PC_DENSE, fp64 and fp32 storage"""
    c, ctx = dr.case(n), arch.ctx
    A = npg.DeviceCSR.from_scipy(ctx, c.A)
    Z = {}
    for storage in ("fp64", "fp32"):
        P = mgm.DenseInversePreconditioner(arch, A, storage=storage)
        assert P.cycle_bytes() == 0
        Z[storage] = _apply_columns(P, ctx, c.R, twice=False)
        _check(c, storage, Z[storage], "dense")
        assert P.cycle_bytes() == _expected_bytes(n, storage)
    if n >= 255:
        assert not np.array_equal(Z["fp32"][:, 0], Z["fp64"][:, 0])


@pytest.mark.parametrize("n", [n for n in dr.SIZES if n >= 2])
def test_one_level_multigrid_is_the_dense_inverse(arch, n):
    """a one-level cycle with a dense inverse is dense_apply(b, x, 1, 0): fp64, fp32 and column-scaled fp16 storage, the second
    application replayed from the captured graph"""
    c, ctx = dr.case(n), arch.ctx
    lib = L.lib()
    A = npg.DeviceCSR.from_scipy(ctx, c.A)
    ops = [npg.DeviceCSR.from_scipy(ctx, sp.csr_matrix(M)) for M in
           (np.ones((n - 1, 1)), np.ones((1, n - 1)), sp.identity(n - 1, format="csr"), np.ones((1, 1)))]
    Z = {}
    for storage, mode in (("fp64", 1), ("fp32", 2), ("fp16", 3)):
        P = mgm.GeneralPreconditioner(ctx, L.NPG_PC_MG, 1)
        P._keep += [A] + ops
        L.check(lib.npg_precond_mg_set_level(P.h, 0, A.h, n - 1, *[o.h for o in ops], None, None))
        L.check(lib.npg_precond_mg_set_coarse_dense(P.h, mode))
        Z[storage] = _apply_columns(P, ctx, c.R, twice=True)
        _check(c, storage, Z[storage], "one-level")
        # the storage that ran: the fp16 case cannot pass on the fp32 fall-back
        assert P.cycle_bytes() == _expected_bytes(n, storage), (storage, P.cycle_bytes())
    if n >= 255:
        assert not np.array_equal(Z["fp32"][:, 0], Z["fp64"][:, 0])
        assert not np.array_equal(Z["fp16"][:, 0], Z["fp32"][:, 0])
