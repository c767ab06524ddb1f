"""npg_cg_solve on the GPU (csrc/cg.hip: k_cg_init / k_cg_spmv / k_cg_update<1> / k_cg_direction) step by step against the longdouble
CG of tests/cg_steps_ref.py; its endings and the reuse of a workspace that has seen a NaN or an Inf, on both libraries.

Every case solves with atol = rtol = 0 and itmax = k from a random non-zero x0, for k in (1, 2, 3, 4, 5, 8, 9) as far as the
reference still resolves the residual, and asserts niter == k, status 2, a history of k + 1 entries, history()[0..k] and x_k within
16 x that step's fp64 summation noise (floored at 1e-15) of the longdouble run, history()[0] against sqrt(r'Pr) formed in longdouble
from x0, and bit-identical reruns of the largest k in a fresh and in the same workspace.  The preconditioner rotates over none /
scalar / diagonal with the case.

What each size reaches (a tridiagonal matrix has 256 rows per tile):
  n = 1 ........................ single row, one workgroup, G1 = G2 = 1; x_1 = b / a to 2 ulp
  n = 255, 256, 257 ............ one short tile, one full tile, a full tile plus one row
  n = 1023, 1024, 1025 ......... G2 goes from 1 to 2 workgroups of 1024 rows
  n = 8192, 8193 ............... 32 / 33 partial rows: the 33rd is the second load of slice 0 in reduce_partials
  n = 65 536, 65 537 ........... 256 / 257 tiles: the workgroup cap, all 8 loads per slice, the grid-stride tile loop with prefetch
  n = 300 001 .................. n > 1024 x 256: second trip of the row loops of k_cg_update and k_cg_direction
  laplace7(20) ................. 4 lanes per row, 32 tiles
  banded(2000, 12) ............. 8 lanes per row
  banded(300, 50), (300, 299) .. 16 and 32 lanes; 19 rows per tile in the dense one
  arrowhead(6000) .............. the whole-workgroup long-row path inside k_cg_init / k_cg_spmv

Measured on one MI355X, the maxima over the checked steps (deviation from the longdouble run, the fp64 noise, the largest
deviation / noise of a single step):
  tri1 n=1 none k<=1: x dev 0.00e+00 noise 0.00e+00 ratio 0.00 | history dev 1.13e-17 noise 1.13e-17 ratio 0.18
  tri255 n=255 scalar k<=9: x dev 5.62e-16 noise 1.67e-15 ratio 0.59 | history dev 2.52e-17 noise 4.18e-16 ratio 0.16
  tri256 n=256 diagonal k<=9: x dev 4.76e-16 noise 7.37e-16 ratio 1.00 | history dev 1.51e-16 noise 1.51e-16 ratio 1.00
  tri257 n=257 none k<=9: x dev 6.65e-16 noise 1.33e-15 ratio 0.96 | history dev 2.50e-17 noise 3.21e-16 ratio 0.08
  tri1023 n=1023 scalar k<=9: x dev 7.06e-16 noise 3.36e-15 ratio 0.69 | history dev 7.31e-17 noise 9.09e-16 ratio 0.73
  tri1024 n=1024 diagonal k<=9: x dev 5.88e-16 noise 1.88e-15 ratio 1.11 | history dev 5.51e-17 noise 4.33e-16 ratio 0.27
  tri1025 n=1025 none k<=9: x dev 1.10e-15 noise 2.24e-15 ratio 1.00 | history dev 6.81e-17 noise 3.22e-16 ratio 0.98
  tri8192 n=8192 scalar k<=9: x dev 1.35e-15 noise 1.04e-14 ratio 0.97 | history dev 6.87e-17 noise 2.52e-15 ratio 0.03
  tri8193 n=8193 diagonal k<=9: x dev 5.96e-16 noise 2.12e-15 ratio 0.88 | history dev 7.65e-17 noise 4.47e-16 ratio 0.19
  tri65536 n=65536 none k<=9: x dev 7.23e-16 noise 7.99e-15 ratio 0.40 | history dev 1.06e-16 noise 4.49e-15 ratio 0.04
  tri65537 n=65537 scalar k<=9: x dev 8.79e-16 noise 5.83e-15 ratio 0.78 | history dev 6.53e-17 noise 8.60e-16 ratio 0.11
  tri300001 n=300001 diagonal k<=9: x dev 1.25e-15 noise 9.15e-15 ratio 1.03 | history dev 7.42e-17 noise 5.76e-15 ratio 0.39
  laplace7_lanes4 n=8000 none k<=9: x dev 2.19e-15 noise 3.26e-15 ratio 0.79 | history dev 5.40e-17 noise 8.30e-16 ratio 0.54
  banded2000_lanes8 n=2000 scalar k<=9: x dev 3.02e-15 noise 2.46e-15 ratio 1.23 | history dev 1.03e-16 noise 2.37e-16 ratio 0.44
  banded300_lanes16 n=300 diagonal k<=9: x dev 4.53e-15 noise 5.16e-15 ratio 1.08 | history dev 4.17e-17 noise 3.74e-16 ratio 0.49
  dense300_lanes32 n=300 none k<=9: x dev 3.20e-15 noise 5.10e-15 ratio 1.54 | history dev 5.82e-17 noise 5.82e-17 ratio 0.93
  arrowhead n=6000 scalar k<=2: x dev 4.98e-14 noise 2.68e-12 ratio 0.12 | history dev 3.70e-16 noise 3.40e-16 ratio 1.85
No case comes near the margin of 16: the largest single-step ratio is 1.85 (history of the arrowhead, whose row 0 sums 6000 products
in the whole-workgroup order).  The arrowhead's three fp64 orders differ among themselves by 2.7e-12 in x, 50 x the device's own
deviation from the longdouble run.

Against the parent commit's device library: after a solve with a NaN in y the ordinary solve on the same workspace ends with status 3
after 1 iteration (single solver; in the batched one only that column, [1, 3, 1]); an Inf in x0 is reported as solved (status 1,
rnorm0 = inf); the curvature system ends with status 2 after 40 iterations where the reference stops after 3."""
import pytest

import nupgcm_amd as npg
from tests import cg_steps_ref as cs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return npg.GPU().ctx


@pytest.mark.parametrize("cid", cs.case_ids())
def test_every_step_against_the_longdouble_cg(ctx, cid):
    cs.check_steps(ctx, cid)


def test_a_workspace_that_has_seen_nan_and_inf_solves_again(ctx):
    cs.check_reuse(ctx)


def test_non_positive_curvature_ends_the_solve_at_once(ctx):
    """status 3 and the reference's niter - the figures tests/test_cg_steps.py pins for the host library with the same system and
    the same reference, so the two libraries agree (one process holds one architecture: they cannot be asked side by side)"""
    cs.check_curvature(ctx)
