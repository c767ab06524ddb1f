"""The row kernels of the flexible GMRES in csrc/fgmres.hip - k_mdot<NG>, k_mupdate<NG>, k_sum_partials, k_combine_z - in every
instance and at their edges, iteration by iteration against oracle.mg_oracle.fgmres (no preconditioner).

  memory 1, 8, 9, 16, 17, 23     the edges of by_groups (NG = 1: k <= 8, NG = 2: k <= 16, NG = 3 beyond) and the creation limit
  n      1, 31, 33, 257, 3000    ld = round32(n) with n no multiple of 32; one row; one workgroup and a part of the next; twelve
  n      300 001 (memory 17)     beyond 1024 workgroups x 256 rows: the grid-stride loops take a second trip

Every system (tests/fgmres_ref.py) needs more than 2 memory + 1 iterations where n allows it, so k reaches `memory` and restarts
happen; n = 1 ends in its first iteration, the happy breakdown.  Not every case ends by convergence: restarted GMRES at these
memories does not reach rtol = 1e-10 on the small systems within the default iteration limit 2 n, which the library and the
restatement share - n = 31 (memories 1 - 17: 62 iterations), n = 33 (every memory: 66) and n = 257 with memory 1 (514) end
there with solved = 0.  Those cases compare the default-itmax path, iteration for iteration, and not a converged solve; the
others (n = 31 with memory 23, n = 257 with memory 8 - 23, n = 3000) converge in 54 - 1487 iterations.

Tolerances come from the reference: 100 x the rounding floor of the case - the restatement against itself on the symmetrically
permuted system - and not below the 1e-6 (history) / 1e-9 (x) of test_fgmres_without_preconditioner_matches_restatement.
Measured floors, history / x (n = 1: exactly 0 for every memory):

  memory        n = 31               n = 33               n = 257              n = 3000
     1     2.5e-15 / 2.1e-15    1.6e-15 / 8.5e-16    1.3e-12 / 4.7e-15    7.7e-08 / 1.6e-15
     8     5.4e-14 / 9.1e-16    3.6e-14 / 3.7e-16    2.4e-08 / 2.0e-16    4.4e-09 / 1.3e-16
     9     2.3e-13 / 3.3e-15    2.0e-14 / 1.3e-16    5.0e-09 / 1.2e-16    6.5e-10 / 1.2e-16
    16     1.2e-10 / 2.1e-17    1.0e-11 / 1.1e-17    3.7e-09 / 1.1e-16    2.3e-09 / 1.0e-16
    17     8.3e-11 / 2.3e-16    3.4e-12 / 1.8e-17    1.2e-09 / 8.2e-17    1.2e-09 / 1.3e-16
    23     7.2e-09 / 1.1e-16    1.2e-09 / 1.2e-16    3.6e-09 / 8.8e-17    3.8e-10 / 1.1e-16

  n = 300 001, memory 17, itmax 40: 6.3e-15 / 2.0e-16 (1.3e-14 / 5.7e-16 on another host: the long dot products follow its
  BLAS threads);  n = 3000, memory 9, itmax 13: 6.0e-16 / 4.6e-16

(the history floors are those of the last entries, estimates 1e-10 below the first), so the history is held to 7.7e-6 at
(n, memory) = (3000, 1), to 2.4e-6 at (257, 8), to 1e-6 elsewhere, and x to 1e-9 everywhere."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

import nupgcm_amd as npg  # noqa: E402
from tests import fgmres_ref as fr  # noqa: E402
from tests.helpers import rel  # noqa: E402


@pytest.fixture(scope="module")
def arch():
    a = npg.GPU()
    a.ctx
    return a


def _solve_and_compare(arch, n, memory, itmax=0):
    ref = fr.reference(n, memory, itmax)
    assert ref.same_niter                                   # the case is not decided by rounding at its last iteration
    ctx = arch.ctx
    A, b = ref.A, ref.b
    Ad = npg.DeviceCSR.from_scipy(ctx, A)
    ws = npg.FgmresWorkspace(ctx, n, memory=memory)
    x = npg.DeviceVector.from_host(ctx, ref.x0)
    st = ws.solve(Ad, npg.DeviceVector.from_host(ctx, b), x, None, atol=0.0, rtol=fr.RTOL, scale=fr.SCALE, itmax=itmax)
    h, xs = ws.history(), x.to_host()
    m = min(len(h), len(ref.hist))
    print(f"n = {n}, memory = {memory}: niter {st['niter']} (restatement {ref.stats['niter']}), npass {st['npass']}, "
          f"history off by {np.max(np.abs(h[:m] - ref.hist[:m]) / np.maximum(ref.hist[:m], 1e-13 * h[0])):.1e} "
          f"(floor {ref.floor_hist:.1e}), x by {rel(xs, ref.x):.1e} (floor {ref.floor_x:.1e})")
    assert st["niter"] == ref.stats["niter"] and st["solved"] == int(ref.stats["solved"])
    assert st["npass"] == -(-st["niter"] // memory)
    assert len(h) == st["niter"] + 1
    assert np.allclose(h, ref.hist, rtol=ref.tol_hist, atol=1e-13 * h[0])
    assert rel(xs, ref.x) < ref.tol_x
    assert abs(st["rnorm"] - fr.SCALE * np.linalg.norm(b - A @ xs)) < 1e-6 * st["rnorm0"] * 1e-4 + 1e-12
    return st, ref, xs


@pytest.mark.parametrize("memory", [1, 8, 9, 16, 17, 23])
@pytest.mark.parametrize("n", [1, 31, 33, 257, 3000])
def test_fgmres_steps_match_restatement(arch, n, memory):
    st, ref, _ = _solve_and_compare(arch, n, memory)
    if n <= memory:
        assert st["solved"] == 1 and st["niter"] <= n                    # the happy breakdown
    else:
        assert st["niter"] > min(2 * memory + 1, 2 * n - 1) and st["npass"] >= 2


def test_fgmres_steps_beyond_the_grid_cap(arch):
    """n = 300 001 > 1024 x 256: the second trip of the grid-stride loops of k_mdot<3>, k_mupdate<3> and k_combine_z"""
    st, _, _ = _solve_and_compare(arch, 300001, 17, itmax=40)
    assert st["niter"] == 40 and st["npass"] == 3 and st["status"] == 2


def test_fgmres_itmax_inside_a_restart_cycle(arch):
    st, _, _ = _solve_and_compare(arch, 3000, 9, itmax=13)               # x: the restatement's after 13 iterations
    assert st["niter"] == 13 and st["npass"] == 2 and st["status"] == 2 and st["solved"] == 0


def test_fgmres_start_at_the_exact_solution(arch):
    """integer data: y - A x0 is exactly zero -> status 4, no iteration, x untouched"""
    ctx = arch.ctx
    n = 257
    rng = np.random.default_rng(11)
    A = sp.csr_matrix(sp.random(n, n, density=0.02, random_state=12, data_rvs=lambda k: rng.integers(-3, 4, k).astype(float))
                      + sp.diags(rng.integers(5, 9, n).astype(float)))
    x0 = rng.integers(-8, 9, n).astype(float)
    y = A @ x0
    assert np.all(y == np.round(y))
    ws = npg.FgmresWorkspace(ctx, n, memory=9)
    x = npg.DeviceVector.from_host(ctx, x0)
    st = ws.solve(npg.DeviceCSR.from_scipy(ctx, A), npg.DeviceVector.from_host(ctx, y), x, None, atol=0.0, rtol=fr.RTOL, scale=fr.SCALE)
    assert st["status"] == 4 and st["niter"] == 0 and st["npass"] == 0 and st["rnorm"] == 0.0
    assert np.array_equal(x.to_host(), x0) and len(ws.history()) == 1


def test_fgmres_memory_limit(arch):
    npg.FgmresWorkspace(arch.ctx, 33, memory=23)
    with pytest.raises(npg._lib.DeviceError, match="1..23"):
        npg.FgmresWorkspace(arch.ctx, 33, memory=24)
