"""npg_cg_solve of the HOST library step by step against the longdouble CG of tests/cg_steps_ref.py, at the sizes up to 8193, with
the bars computed exactly as for the device (tests/test_gpu_cg_steps.py); its endings and the reuse of a workspace that has seen a
NaN or an Inf.  No GPU."""
import pytest

import nupgcm_amd as npg
from tests import cg_steps_ref as cs


@pytest.fixture(scope="module")
def ctx():
    return npg.CPU().ctx


@pytest.mark.parametrize("cid", cs.case_ids(cs.HOST_MAX_N))
def test_every_step_against_the_longdouble_cg(ctx, cid):
    cs.check_steps(ctx, cid)


def test_a_workspace_that_has_seen_nan_and_inf_solves_again(ctx):
    cs.check_reuse(ctx)


def test_non_positive_curvature_ends_the_solve_at_once(ctx):
    cs.check_curvature(ctx)
