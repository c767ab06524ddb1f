"""The batched CG (npg_cg_multi_*, BatchedCgWorkspace) on the host library, where it is a loop over the columns that runs
the existing host CG on each column's slice: per column the bits of x, the statistics and the history of CgWorkspace.solve, at
tolerance zero.  The matrices, the columns that end differently, independence and the refusals are those of
tests/test_gpu_cg_multi.py at the small sizes (tests/cg_multi_ref.py).  No GPU."""
import pytest

import nupgcm_amd as npg
from tests import cg_multi_ref as cm
from tests import helpers


@pytest.fixture(scope="module")
def ctx():
    return npg.CPU().ctx


@pytest.fixture(scope="module")
def model_case(ctx):
    """the bowl_mixing evolution matrix on bowl3D h = 0.1, P2, with the Jacobi preconditioner made from its diagonal (on CPU() the
    toolkit's own P is a factorisation)"""
    model = helpers.build_model("bowl_mixing", nsteps=3, arch=npg.CPU())
    A = model.evolution.solver.A
    return cm.Case(ctx, A.to_scipy_csr(), "bowl_mixing evolution matrix", A_dev=A)


def test_both_libraries_export_the_batched_cg_entry_points():
    cm.check_exports()


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


@pytest.mark.parametrize("name", ["arrowhead", "laplace7", "banded16", "dense32"])
def test_row_shapes(ctx, name):
    A = dict(arrowhead=lambda: cm.arrowhead(6000), laplace7=lambda: cm.laplace7(20), banded16=lambda: cm.banded(300, 50),
             dense32=lambda: cm.banded(300, 299))[name]()
    cm.check_columns(cm.Case(ctx, A, name), range(3))


def test_columns_that_end_differently(ctx):
    cm.check_endings(cm.Case(ctx, cm.laplace7(12), "laplace7 12^3"))


def test_independence_of_the_columns(ctx):
    cm.check_independence(cm.Case(ctx, cm.tridiagonal(257), "tridiagonal n=257"))


def test_the_cap_of_32_columns_and_grouping_of_33(ctx):
    cm.check_cap_and_grouping(ctx)


def test_refusals(ctx):
    cm.check_refusals(ctx, device=False)


def test_passive_tracers_batched_runs_the_per_tracer_path_on_the_host():
    """CPU(): iterative_solve takes the direct-solve branches, which have no batched form - batched=True falls back"""
    cm.check_tracers(npg.CPU(), helpers.build_model, expect_batched=False)
