"""Particle tracking (nupgcm_amd.particles) on the CPU() architecture - libnupgcm_host.so runs the same RK4 step, the same
remembered-cell rule and the same periodic wrap as the device kernel (csrc/particles_core.h) - against closed forms of RK4 on affine
flows, a numpy RK4 of the blended rotation, the brute-force locator for leaving the mesh and npg.nan_eval for the real state
(tests/particles_ref.py).  No GPU.

Measured on the host library:
  rotation, 126 steps              max|x - P4^126 x0| 3.8e-15 against 126 . 64 . eps . max|x| = 1.1e-12; no particle lost
  general affine, 2 steps          1.1e-16 against 1.2e-14
  leaving                          8 of 2000 alive after 60 steps, all lost by step 61 where the brute force says, none ambiguous; while
                                   alive 0.03 of k 8 eps
  time blend                       1.1e-16 against 6.8e-14
  real state (one step)            0 against 1e-12 max|x| for both configurations; cells = the elected cells
  periodic seam                    1.1e-15 (wrapped), 1.3e-15 (unwrapped) against 7.1e-14"""
import pytest

import nupgcm_amd as npg
from tests import integrals_ref as ir
from tests import particles_ref as pr
from tests import sampling_ref as sr


@pytest.fixture(scope="module")
def arch():
    return npg.CPU()


@pytest.fixture(scope="module")
def bare(arch):
    return ir.bare_model(arch)


def test_both_libraries_export_the_particles_entry_points():
    pr.check_exports()


def test_rotation_against_the_closed_form_across_cells(bare):
    pr.check_rotation(bare)


def test_general_affine_flow_against_the_closed_form(bare):
    pr.check_general_affine(bare)


def test_leaving_the_mesh_where_the_brute_force_says(bare):
    pr.check_leaving(bare)


def test_time_blend_against_a_numpy_rk4(bare):
    pr.check_blend(bare)


@pytest.mark.parametrize("name,nsteps", [("bowl_surface_flux", 3), ("bowl_diri", 1)])
def test_real_state_against_nan_eval(arch, name, nsteps):
    pr.check_real_state(sr.bowl_model(arch, name, nsteps=nsteps), name)


def test_determinism(bare):
    pr.check_determinism(bare)


def test_periodic_seam(arch):
    pr.check_periodic(arch)


def test_tracker_as_on_plot(arch, tmp_path):
    pr.check_hook(arch, tmp_path)


def test_refusals_and_edge_cases(bare):
    pr.check_refusals(bare)
