"""The batched CG on the GPU (csrc/cg.hip: k_cgm_init / k_cgm_spmv for the products, then k_cg_update<C> / k_cg_direction, which the
single solve runs too with one column) against npg_cg_solve (k_cg_init / k_cg_spmv for the products) on the same
context, at tolerance zero: per column the bits of x, niter, status, solved, rnorm0, rnorm and the history (tests/cg_multi_ref.py).

Which product-kernel instance each matrix runs (lanes per row from npg_csr_create's rule, asserted below; column blocks from K):
  tridiagonal n = 1, 257, 70 001 and the 7-point Laplacian + I on 20^3 ... 4 lanes
  the model's matrix (P2, 27 entries per row) and the arrowhead ............ 8 lanes / 4 lanes + the whole-workgroup row path
  banded n = 300, half-width 50 ............................................. 16 lanes
  dense n = 300 ............................................................. 32 lanes
  K = 1, 2, 3 (in the 4-column instance), 5 and 8 (8-column), 32 (four launches of the 8-column instance) and 33 (two workspaces)."""
import pytest

import nupgcm_amd as npg
from tests import cg_multi_ref as cm
from tests import helpers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return npg.GPU().ctx


@pytest.fixture(scope="module")
def model_case(ctx):
    """the bowl_mixing evolution matrix on bowl3D h = 0.1, P2, with its own Jacobi preconditioner"""
    model = helpers.build_model("bowl_mixing", nsteps=3, arch=npg.GPU())
    s = model.evolution.solver
    assert isinstance(s.P, npg.Diagonal) and s.P.diag is not None
    case = cm.Case(ctx, s.A.to_scipy_csr(), "bowl_mixing evolution matrix", A_dev=s.A, P=s.P)
    assert cm.expected_lanes(case.As) == 8
    return case


@pytest.mark.parametrize("K", [1, 2, 3, 5, 8])
def test_the_models_matrix_with_its_jacobi_preconditioner(model_case, K):
    st = cm.check_columns(model_case, range(K))
    assert all(s["status"] == 1 and s["niter"] > 0 for s in st)


@pytest.mark.parametrize("precond", ["none", "scalar"])
def test_the_models_matrix_with_other_preconditioners(model_case, precond):
    cm.check_columns(model_case.with_precond(precond), range(3))


@pytest.mark.parametrize("n", [1, 257])
def test_smallest_sizes(ctx, n):
    cm.check_columns(cm.Case(ctx, cm.tridiagonal(n), f"tridiagonal n={n}"), range(3))


def test_more_tiles_than_workgroups(ctx):
    """n = 70 001: 274 tiles on at most 256 workgroups, G2 = 69"""
    case = cm.Case(ctx, cm.tridiagonal(70001), "tridiagonal n=70001", ncol=3)
    st = cm.check_columns(case, range(3))
    assert all(12 <= s["niter"] <= 200 for s in st)


@pytest.mark.parametrize("name,lanes", [("arrowhead", 4), ("laplace7", 4), ("banded16", 16), ("dense32", 32)])
def test_row_shapes_and_lanes_per_row(ctx, name, lanes):
    A = dict(arrowhead=lambda: cm.arrowhead(6000), laplace7=lambda: cm.laplace7(20), banded16=lambda: cm.banded(300, 50),
             dense32=lambda: cm.banded(300, 299))[name]()
    assert cm.expected_lanes(A) == lanes
    cm.check_columns(cm.Case(ctx, A, name), range(3))


def test_columns_that_end_differently(ctx):
    cm.check_endings(cm.Case(ctx, cm.laplace7(12), "laplace7 12^3"))


def test_independence_of_the_columns(ctx):
    cm.check_independence(cm.Case(ctx, cm.tridiagonal(257), "tridiagonal n=257"))


def test_the_cap_of_32_columns_and_grouping_of_33(ctx):
    cm.check_cap_and_grouping(ctx)


def test_refusals(ctx):
    inv = helpers.build_model("bowl_mixing", nsteps=3, arch=npg.GPU(), block_nodes=True).inversion.solver.A
    assert inv.paired                                                   # stored by node blocks
    cm.check_refusals(ctx, device=True, blocked=inv)


def test_passive_tracers_batched_against_unbatched():
    cm.check_tracers(npg.GPU(), helpers.build_model, expect_batched=True)
