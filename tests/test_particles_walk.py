"""Diffusing particles and reflecting walls (npg_particles_walk) on the CPU() architecture - libnupgcm_host.so runs the
same generator, the same displacement and the same walk as the device kernel (csrc/particles_walk_core.h) - against a numpy Philox, closed
recurrences and a numpy restatement of the walk (tests/particles_walk_ref.py).  No GPU.

Measured on the host library:
  generator                        3 known answers, 3 x 1000 x 3 words: equal
  neighbour table                  bowl: 1732 boundary faces = the fixture's facets; channel basin: 14 seam faces, all paired with -1 / +1
  free diffusion, 30 steps         0.123 of k 8 eps max|x|; mean within 1.1, variance within 2.7 standard errors; 7 cells reached
  linear kappa_v                   0.123 of the bound; mean dz 1.01 standard errors off c_d b k h
  flat surface                     0.009 of k 8 eps (advection, 27 - 30 reflections each), 0.066 with diffusion (1470 reflections)
  one step on the real state x 20  max|x - restatement| 3.3e-16 against 1e-12 max|x| = 9.8e-13; 0 of 2000 ambiguous; 3992 reflections
  census, 120 steps                before 569 648 586 580 617, after 571 631 580 635 583; 13 214 reflections, none lost or stuck
  periodic seam                    1.4e-15 (wrapped), 1.3e-15 (unwrapped) against 7.1e-14
  stuck                            500 of 500 stuck in the step the brute force says, none ambiguous"""
import pytest

import nupgcm_amd as npg
from tests import integrals_ref as ir
from tests import particles_walk_ref as wr
from tests import sampling_ref as sr


@pytest.fixture(scope="module")
def arch():
    return npg.CPU()


@pytest.fixture(scope="module")
def bare(arch):
    return ir.bare_model(arch)


def test_both_libraries_export_the_walk_entry_points():
    wr.check_exports()


def test_generator_against_the_numpy_philox(arch):
    wr.check_generator(arch)


def test_neighbour_table():
    wr.check_neighbours()


def test_free_diffusion_exact_per_particle(bare):
    wr.check_free_diffusion(bare)


def test_linear_kappa_v_against_the_recurrence(bare):
    wr.check_linear_kappa(bare)


def test_flat_surface_reflects(bare):
    wr.check_flat_surface(bare)


def test_one_step_against_the_numpy_restatement_on_the_real_state(arch):
    wr.check_one_step(sr.bowl_model(arch, "bowl_surface_flux", nsteps=3))


def test_well_mixed_census(bare):
    wr.check_census(bare)


def test_periodic_seam_walked(arch):
    wr.check_periodic(arch)


def test_a_walk_that_cannot_be_finished_is_stuck(bare):
    wr.check_stuck(bare)


def test_determinism(bare):
    wr.check_determinism(bare)


def test_refusals_and_edge_cases(bare):
    wr.check_refusals(bare)


def test_without_the_keywords_the_tracker_is_unchanged(bare):
    wr.check_opt_in(bare)


def test_tracker_with_diffusion_as_on_plot(arch, tmp_path):
    wr.check_hook(arch, tmp_path)
