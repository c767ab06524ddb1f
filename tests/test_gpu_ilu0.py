"""ILU(0) on the GPU (csrc/ilu.hip) through the C ABI - the inner preconditioner of the reference's GPU P-block
(src/preconditioners.jl:101-107: kp_ilu0 + CG with ldiv = true, itmax = 100) - against the CPU restatement
(oracle/ilu0_oracle.py, pinned by the factorisation's defining properties: tests/test_oracle_ilu0.py)."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

pytestmark = pytest.mark.gpu

import nupgcm_amd as npg  # noqa: E402
from nupgcm_amd import multigrid as mgm  # noqa: E402
from nupgcm_amd import workloads  # noqa: E402
from oracle import ilu0_oracle as io  # noqa: E402
from oracle import recipe as rc  # noqa: E402
from tests import cg_multi_ref as cm  # noqa: E402
from tests.helpers import rel  # noqa: E402


@pytest.fixture(scope="module")
def arch():
    a = npg.GPU()
    a.ctx
    return a


def _random_spd(n, density, seed):
    rng = np.random.default_rng(seed)
    M = sp.random(n, n, density=density, random_state=seed, format="csr")
    M = M + M.T
    return sp.csr_matrix(M + sp.diags(np.asarray(abs(M).sum(axis=1)).ravel() + 0.5 + rng.random(n)))


def test_factors_and_solves_match_the_restatement(arch):
    """random SPD pattern (n = 1500): the factors entry by entry, z = U^-1 L^-1 r, the level counts of the analysis, and the
    CG iteration - counts, residual history end and solution - against the CPU restatement"""
    ctx = arch.ctx
    A = _random_spd(1500, 0.004, 7)
    Ad = npg.DeviceCSR.from_scipy(ctx, A)
    M = npg.DeviceILU0(Ad)
    LU = io.ilu0(A)
    F = M.factors()
    assert (F.indices == LU.indices).all() and np.abs(F.data - LU.data).max() < 1e-12 * np.abs(LU.data).max()
    assert M.levels == io.levels(A) and M.levels[0] > 3
    r = np.sin(np.arange(1500) * 0.7) + 0.2
    z = M.ldiv(npg.DeviceVector.from_host(ctx, r)).to_host()
    assert rel(z, io.solve(LU, r)) < 1e-12
    z2 = M.ldiv(npg.DeviceVector.from_host(ctx, 2 * r)).to_host()          # a second (r, z) pair: another captured sequence
    assert rel(z2, 2 * z) < 1e-13
    b = np.cos(np.arange(1500) * 0.3)
    x0 = 0.05 * np.sin(np.arange(1500.0))
    x = npg.DeviceVector.from_host(ctx, x0)
    st = M.cg(Ad, npg.DeviceVector.from_host(ctx, b), x, atol=1e-9, rtol=1e-9)
    xo, it, solved, hist = io.pcg(A, b, LU, x0=x0, atol=1e-9, rtol=1e-9)
    assert st["solved"] == 1 and solved and st["niter"] == it
    assert abs(st["rnorm0"] - hist[0]) < 1e-10 * hist[0] and abs(st["rnorm"] - hist[-1]) < 1e-6 * hist[0]
    assert rel(x.to_host(), xo) < 1e-9 and rel(A @ x.to_host(), b) < 1e-7
    st5 = M.cg(Ad, npg.DeviceVector.from_host(ctx, b), npg.DeviceVector(ctx, 1500), atol=0.0, rtol=1e-30, itmax=5)
    assert st5["solved"] == 0 and st5["niter"] == 5 and st5["status"] == 2      # itmax honoured and reported
    # new values on the same pattern
    A2 = sp.csr_matrix(A + sp.diags(np.full(1500, 0.3)))
    Ad2 = npg.DeviceCSR.from_scipy(ctx, A2)
    M.refactor(Ad2)
    assert np.abs(M.factors().data - io.ilu0(A2).data).max() < 1e-12 * np.abs(LU.data).max()


def test_exact_on_a_full_band(arch):
    """a full band is closed under elimination: the factors are the exact LU, z = A^-1 r, CG converges in one iteration"""
    ctx = arch.ctx
    n, bw = 4000, 4
    rng = np.random.default_rng(11)
    diags = [rng.uniform(-1, 1, n - d) for d in range(1, bw + 1)]
    A = sum(sp.diags(v, d) + sp.diags(v, -d) for d, v in zip(range(1, bw + 1), diags))
    A = sp.csr_matrix(A + sp.diags(np.asarray(abs(A).sum(axis=1)).ravel() + 1.0))
    Ad = npg.DeviceCSR.from_scipy(ctx, A)
    M = npg.DeviceILU0(Ad)
    assert M.levels == (n, n)                                   # a band chains every row to the one before it
    r = rng.standard_normal(n)
    z = M.ldiv(npg.DeviceVector.from_host(ctx, r)).to_host()
    assert rel(z, spla.spsolve(sp.csc_matrix(A), r)) < 1e-11
    x = npg.DeviceVector(ctx, n)
    st = M.cg(Ad, npg.DeviceVector.from_host(ctx, r), x, atol=0.0, rtol=1e-10)
    assert st["solved"] == 1 and st["niter"] <= 1 and rel(A @ x.to_host(), r) < 1e-9


# ---- the edges of the three kernels ------------------------------------------------------------------------------------------------------
# Measured maxima on one MI355X (relative to the largest factor / to the norm of the reference vector; bar 1e-12 everywhere):
#   factors: banded(300, 70), arrow n = 1024, nonsymmetric n = 1500, blocks n = 140 000: 0 (the restatement's bits: the kernel subtracts
#            in the restatement's order and the build does not contract a*b+c)
#   ldiv:    banded(300, 70) 6.2e-16, arrow n = 1024 4.6e-17, nonsymmetric n = 1500 1.4e-16, blocks n = 140 000 0
#   cg:      blocks n = 600 002: 1 iteration, x 1.2e-16 of the closed form
#   pcg step by step (itmax = 1 .. 5): x deviates by 2.2e-16 .. 2.7e-16 at a noise of 2.6e-16 .. 4.4e-16 (largest ratio 1.02, bar 16),
#            rnorm0 by 1.0e-16 at 1.9e-16, rnorm by at most 0.53 of its noise
def _factors_close(M, LU, label):
    F = M.factors()
    LU = sp.csr_matrix(LU)
    LU.sort_indices()
    assert (F.indptr == LU.indptr).all() and (F.indices == LU.indices).all()
    d = np.abs(F.data - LU.data).max() / np.abs(LU.data).max()
    print(f"ilu0 {label}: factors {d:.2e}")
    assert d < 1e-12
    return d


def _ldiv_close(M, r, z_ref, label):
    z = M.ldiv(npg.DeviceVector.from_host(M.ctx, r)).to_host()
    d = rel(z, z_ref)
    print(f"ilu0 {label}: ldiv {d:.2e}")
    assert d < 1e-12
    return z


def test_a_single_row(arch):
    """n = 1: the factor is the entry, z = r / a, CG ends after one step"""
    ctx = arch.ctx
    A = sp.csr_matrix(np.array([[2.5]]))
    Ad = npg.DeviceCSR.from_scipy(ctx, A)
    M = npg.DeviceILU0(Ad)
    assert M.levels == (1, 1) and M.factors().data.tolist() == [2.5]
    z = M.ldiv(npg.DeviceVector.from_host(ctx, np.array([0.7]))).to_host()
    assert abs(z[0] - 0.7 / 2.5) <= np.spacing(0.7 / 2.5)
    x = npg.DeviceVector(ctx, 1)
    st = M.cg(Ad, npg.DeviceVector.from_host(ctx, np.array([-1.3])), x, atol=0.0, rtol=1e-12, itmax=5)
    assert st["solved"] == 1 and st["niter"] == 1 and st["status"] == 1
    assert abs(x.to_host()[0] + 1.3 / 2.5) <= 2 * np.spacing(1.3 / 2.5)


def test_rows_longer_than_a_wavefront_on_a_full_band(arch):
    """banded(300, 70): 141 entries per row (the 64-lane staging loop makes three trips), 70 upper entries per eliminated row (the
    jj loop a second trip), 70 entries on each side in the triangular solves (the 16-lane loop five trips).  A full band: the
    factors are the exact LU, z = A^-1 r"""
    A = cm.banded(300, 70)
    M = npg.DeviceILU0(npg.DeviceCSR.from_scipy(arch.ctx, A))
    assert M.levels == (300, 300)
    _factors_close(M, io.ilu0(A), "banded(300, 70)")
    r = np.random.default_rng(3).standard_normal(300)
    _ldiv_close(M, r, np.linalg.solve(A.toarray(), r), "banded(300, 70)")


def _arrow(n, seed=5):
    """last row and last column dense with nonsymmetric values, strictly dominant diagonal: elimination makes no fill"""
    rng = np.random.default_rng(seed)
    A = sp.lil_matrix((n, n))
    A[n - 1, :] = rng.uniform(-1.0, 1.0, n)
    A[:, n - 1] = rng.uniform(-1.0, 1.0, n).reshape(n, 1)
    A.setdiag(2.5 + rng.random(n))
    A[n - 1, n - 1] = n + 1.0
    return A.tocsr()


def test_a_row_at_the_limit_of_1024_entries(arch):
    """n = 1024: the last row holds exactly kIluMaxRow entries - 1023 eliminations, a binary search over 1024 columns; no fill,
    so the factors are the exact LU.  n = 1025: refused"""
    ctx = arch.ctx
    A = _arrow(1024)
    assert np.diff(A.indptr).max() == 1024
    M = npg.DeviceILU0(npg.DeviceCSR.from_scipy(ctx, A))
    assert M.levels == (2, 2)
    _factors_close(M, io.ilu0(A), "arrow n=1024")
    r = np.random.default_rng(4).standard_normal(1024)
    _ldiv_close(M, r, np.linalg.solve(A.toarray(), r), "arrow n=1024")
    with pytest.raises(npg._lib.DeviceError, match="limit"):
        npg.DeviceILU0(npg.DeviceCSR.from_scipy(ctx, _arrow(1025)))


def test_a_nonsymmetric_pattern(arch):
    """n = 1500, nonsymmetric pattern and values, strictly dominant diagonal: the binary search misses (u_kj without a place in row
    i), U's pattern is not the transpose of L's, and the two level counts differ"""
    n = 1500
    rng = np.random.default_rng(9)
    B = sp.random(n, n, density=0.004, random_state=9, format="csr")
    B.data[:] = rng.uniform(-1.0, 1.0, B.nnz)
    B = sp.lil_matrix(B)
    B.setdiag(0.0)
    B.setdiag(rng.uniform(-1.0, 1.0, 200), -1)           # a chain below the diagonal of the first 201 rows: L's graph is deeper than U's
    B = B.tocsr()
    B.eliminate_zeros()
    A = sp.csr_matrix(B + sp.diags(np.asarray(abs(B).sum(axis=1)).ravel() + 0.5 + rng.random(n)))
    A.sort_indices()
    assert ((A != 0) != (A.T != 0)).nnz > 0
    M = npg.DeviceILU0(npg.DeviceCSR.from_scipy(arch.ctx, A))
    lev = io.levels(A)
    assert M.levels == lev and lev[0] != lev[1], lev
    LU = io.ilu0(A)
    _factors_close(M, LU, "nonsymmetric n=1500")
    r = np.cos(np.arange(n) * 0.37) + 0.1
    _ldiv_close(M, r, io.solve(LU, r), "nonsymmetric n=1500")


def _blocks(m, seed=13):
    """block diagonal of m symmetric positive-definite 2 x 2 blocks [[a, b], [b, c]] and the closed form of its LU:
    l = b / a, U = [[a, b], [0, c - l b]]"""
    rng = np.random.default_rng(seed)
    a, c, b = 2.0 + rng.random(m), 2.0 + rng.random(m), rng.uniform(-1.0, 1.0, m)
    idx = 2 * np.arange(m)
    A = sp.csr_matrix((np.stack([a, b, b, c], axis=1).ravel(), np.stack([idx, idx + 1, idx, idx + 1], axis=1).ravel(),
                       2 * np.arange(2 * m + 1)), shape=(2 * m, 2 * m))
    l = b / a
    u = c - l * b
    LU = sp.csr_matrix((np.stack([a, b, l, u], axis=1).ravel(), A.indices, A.indptr), shape=A.shape)

    def solve(r):                               # the 2 x 2 LU solve, written out
        t1 = r[1::2] - l * r[0::2]
        z = np.empty_like(r)
        z[1::2] = t1 / u
        z[0::2] = (r[0::2] - b * z[1::2]) / a
        return z
    return A, LU, solve


def test_a_level_wider_than_the_workgroup_cap(arch):
    """70 000 blocks (n = 140 000): both levels hold 70 000 rows, more than the factor kernel's 65 535 workgroups - its grid-stride
    loop takes a second trip"""
    A, LU, solve = _blocks(70000)
    M = npg.DeviceILU0(npg.DeviceCSR.from_scipy(arch.ctx, A))
    assert M.levels == (2, 2)
    _factors_close(M, LU, "blocks n=140000")
    r = np.random.default_rng(14).standard_normal(A.shape[0])
    _ldiv_close(M, r, solve(r), "blocks n=140000")


def test_cg_beyond_one_trip_of_its_vector_kernels(arch):
    """300 001 blocks (n = 600 002) through M.cg: n > 65 536 is a second trip in k_dot_part, n > 2048 x 256 a second trip in
    k_pcg_update and k_pcg_direction.  The factors are exact, so CG ends in at most 2 iterations"""
    ctx = arch.ctx
    A, LU, solve = _blocks(300001)
    Ad = npg.DeviceCSR.from_scipy(ctx, A)
    M = npg.DeviceILU0(Ad)
    b = np.random.default_rng(15).standard_normal(A.shape[0])
    x = npg.DeviceVector.from_host(ctx, 0.1 * np.cos(np.arange(A.shape[0]) * 0.01))
    st = M.cg(Ad, npg.DeviceVector.from_host(ctx, b), x, atol=0.0, rtol=1e-12, itmax=5)
    d = rel(x.to_host(), solve(b))
    print(f"ilu0 blocks n=600002: cg niter {st['niter']} status {st['status']} x {d:.2e}")
    assert st["solved"] == 1 and 1 <= st["niter"] <= 2
    assert d < 1e-12


def test_cg_step_by_step_against_the_longdouble_cg(arch):
    """ilu_pcg_raw on the n = 1500 random SPD matrix with itmax = 1 .. 5 at atol = 0, rtol = 1e-30: status 2, niter == k, and x_k,
    rnorm0 and rnorm within the bars of tests/cg_steps_ref.py (16 x the fp64 summation noise, floored at 1e-15) of the longdouble CG
    with M = the restatement's factors, solved row by row in longdouble"""
    from tests import cg_steps_ref as cs
    ctx = arch.ctx
    n = 1500
    A = _random_spd(n, 0.004, 7)
    Ad = npg.DeviceCSR.from_scipy(ctx, A)
    M = npg.DeviceILU0(Ad)
    b = np.cos(np.arange(n) * 0.3)
    x0 = 0.05 * np.sin(np.arange(float(n)))
    ref = cs.Steps(A, cs.triangular_precond(io.ilu0(A)), b, x0, 5, atol=0.0, rtol=1e-30)
    assert ref.kmax == 5 and ref.status == 2
    worst = [0.0, 0.0]
    for k in range(1, 6):
        x = npg.DeviceVector.from_host(ctx, x0)
        st = M.cg(Ad, npg.DeviceVector.from_host(ctx, b), x, atol=0.0, rtol=1e-30, itmax=k)
        assert st["status"] == 2 and st["niter"] == k and st["solved"] == 0, st
        dx, d0, dk = ref.dev_x(k, x.to_host()), ref.dev_h(0, st["rnorm0"]), ref.dev_h(k, st["rnorm"])
        worst = [max(worst[0], dx / max(ref.noise_x[k], cs.FLOOR / cs.MARGIN)),
                 max(worst[1], d0 / max(ref.noise_h[0], cs.FLOOR / cs.MARGIN), dk / max(ref.noise_h[k], cs.FLOOR / cs.MARGIN))]
        print(f"ilu0 pcg itmax={k}: x dev {dx:.2e} noise {ref.noise_x[k]:.2e} | rnorm0 dev {d0:.2e} noise {ref.noise_h[0]:.2e} | "
              f"rnorm dev {dk:.2e} noise {ref.noise_h[k]:.2e}")
        assert dx <= ref.bar_x(k) and d0 <= ref.bar_h(0) and dk <= ref.bar_h(k)
    print(f"ilu0 pcg: largest deviation / noise: x {worst[0]:.2f}, rnorm {worst[1]:.2f}")


def test_argument_errors(arch):
    ctx = arch.ctx
    with pytest.raises(npg._lib.DeviceError, match="square"):
        npg.DeviceILU0(npg.DeviceCSR.from_scipy(ctx, sp.csr_matrix(np.ones((3, 4)))))
    with pytest.raises(npg._lib.DeviceError, match="no diagonal"):
        npg.DeviceILU0(npg.DeviceCSR.from_scipy(ctx, sp.csr_matrix(np.array([[1.0, 2.0, 0.0], [3.0, 0.0, 1.0], [0.0, 1.0, 2.0]]))))
    A = _random_spd(200, 0.03, 2)
    M = npg.DeviceILU0(npg.DeviceCSR.from_scipy(ctx, A))
    with pytest.raises(npg._lib.DeviceError, match="pattern"):
        M.refactor(npg.DeviceCSR.from_scipy(ctx, _random_spd(200, 0.05, 3)))
    with pytest.raises(npg._lib.DeviceError, match="alias"):
        v = npg.DeviceVector(ctx, 200)
        npg._lib.check(npg._lib.lib().npg_ilu0_apply(M.h, v.h, v.h))
    # a zero pivot is REPORTED (csrilu02 does; round 4 returned OK and the NaN factors surfaced later as a CG breakdown - ADVICE):
    # u_11 = 0 after eliminating row 1 with row 0 of [[1, 1], [1, 1]]; and an explicitly stored zero on the diagonal
    for Z in (np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 1.0], [0.0, 1.0, 2.0]]), None):
        if Z is None:
            Zs = sp.csr_matrix((np.array([0.0, 1.0, 1.0, 3.0]), np.array([0, 1, 0, 1]), np.array([0, 2, 4])), shape=(2, 2))
        else:
            Zs = sp.csr_matrix(Z)
        with pytest.raises(npg._lib.DeviceError, match="pivot"):
            npg.DeviceILU0(npg.DeviceCSR.from_scipy(ctx, Zs))
    Abad = sp.csr_matrix(A.copy())
    Abad.sort_indices()
    k = Abad.indptr[0] + int(np.searchsorted(Abad.indices[Abad.indptr[0]:Abad.indptr[1]], 0))
    assert Abad.indices[k] == 0
    Abad.data[k] = 0.0                                        # same pattern, first pivot zero
    with pytest.raises(npg._lib.DeviceError, match="pivot"):
        M.refactor(npg.DeviceCSR.from_scipy(ctx, Abad))


def test_velocity_block_of_the_reference_with_ilu0(arch):
    """BlockDiagonalPreconditioner(u_precond="ilu0") on bowl3D h = 0.1 - P_block_setup(::GPU) of src/preconditioners.jl:101-107:
    the friction block's factors equal the restatement's, the inner CG needs several times fewer iterations than with the Jacobi
    vector, the block solves what scipy solves, and the preconditioned inversion lands on the direct solve"""
    prm, frc = workloads.example_parameters()
    prm.eps = 0.5
    fed = workloads.example_fe_data(workloads.bowl_mesh_model("bowl3D_h0.1"))
    S = rc.setup("example", eps=0.5)
    d, ctx = fed.dofs, arch.ctx
    n = d.nu + d.np
    Pi = npg.BlockDiagonalPreconditioner(arch, prm, fed, u_itmax=0, p_itmax=0, atol=1e-12, rtol=1e-10, u_precond="ilu0")
    Pj = npg.BlockDiagonalPreconditioner(arch, prm, fed, u_itmax=0, p_itmax=0, atol=1e-12, rtol=1e-10)
    F = Pi.ilu.A.to_scipy_csr()
    F.sort_indices()
    assert Pi.ilu.levels[0] > 10 and np.abs(Pi.ilu.factors().data - io.ilu0(F).data).max() < 1e-11 * np.abs(F.data).max()
    r = np.cos(np.arange(n) * 0.11)
    zi = Pi.apply(npg.DeviceVector.from_host(ctx, r), npg.DeviceVector(ctx, n)).to_host()
    zj = Pj.apply(npg.DeviceVector.from_host(ctx, r), npg.DeviceVector(ctx, n)).to_host()
    assert rel(F @ zi[:d.nu], r[:d.nu]) < 1e-8 and rel(zi, zj) < 1e-7
    (_, inner_i), (_, inner_j) = Pi.counters(), Pj.counters()
    assert 2 * inner_i < inner_j, (inner_i, inner_j)            # (both counts include the pressure block's Jacobi-CG iterations)
    with pytest.raises(ValueError):
        npg.BlockDiagonalPreconditioner(arch, prm, fed, u_precond="ssor")
    # (every inner iteration is two triangular solves of hundreds of level launches: a loose outer tolerance keeps the test short)
    inv = npg.InversionToolkit(arch, fed, prm, frc, preconditioner="block_diagonal", atol=1e-5, rtol=1e-5,
                               precond_kw=dict(u_itmax=100, p_itmax=0, u_precond="ilu0"))
    bfree = S.orc.interpolate_b(lambda x: 0.1 * np.exp(-(x[..., 2] + 0.5 * (1 - x[..., 0] ** 2 - x[..., 1] ** 2)) / 0.05))
    npg.inversion.invert(inv, npg.DeviceVector.from_host(ctx, bfree, d.p_b))
    st = inv.solver.workspace.stats
    x = inv.solver.x.to_host(d.inv_p_inversion)
    xd = spla.splu(sp.csc_matrix(S.A)).solve(S.B @ bfree + S.b0)
    assert st["solved"] == 1 and rel(x[:d.nu], xd[:d.nu]) < 1e-2            # (1e-5 in the scaled residual: a few 1e-3 in u)
