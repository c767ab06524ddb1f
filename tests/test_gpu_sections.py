"""Transports through sections on the GPU (libnupgcm_hip.so: k_section_pieces / k_section_fold): the restatement, the
bounds and the cases of tests/test_sections.py through the device library, and in addition the device against the host library on the
same state - the same plan, and without the convection closure every bit of every bin and piece, on every mesh (with it, channels 10
and 11 to the restatement's bound: tanh is another function there).  The piece counts cover no lane at all (a plane that misses), one
lane (the single tetrahedron), the Kuhn cube (face-aligned pieces with barycentrics 0 and 1, oblique sections), several workgroups
with a ragged last one (bowl: 477 and 1 033 pieces) and exactly 0, 1, 63, 64, 65, 255, 256, 257 pieces through the mask; the fold a
bin of more than 256 pieces beside empty and single-piece bins."""
import pytest

import nupgcm_amd as npg
from tests import sections_ref as xr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def arch():
    return npg.GPU()


@pytest.fixture(scope="module")
def bowl(arch):
    return xr.bowl(arch)


def test_plan_against_the_independent_cutter(bowl):
    xr.check_plans_bowl(bowl)


def test_degenerate_planes_are_counted_once_and_match_the_host_library(arch, bowl):
    xr.check_degenerate(arch, bowl, against_host=True)


def test_single_tetrahedron(arch):
    xr.check_single_tet(arch, against_host=True)


def test_closed_forms_and_the_host_library_on_the_kuhn_cube(arch):
    xr.check_closed_forms(arch, against_host=True)


@pytest.mark.parametrize("b_order", [2, 1])
def test_bowl_against_the_restatement_and_the_host_library(arch, b_order):
    xr.check_bowl(arch, b_order, against_host=True)


def test_dirichlet_values_and_the_pinned_pressure_vertex(arch):
    xr.check_dirichlet_and_pin(arch, against_host=True)


@pytest.mark.parametrize("b_order", [2, 1])
def test_channel_basin_across_the_seam(arch, b_order):
    xr.check_channel(arch, b_order, against_host=True)


def test_edge_sizes_through_the_mask(bowl):
    xr.check_masks(bowl, against_host=True)


def test_determinism_and_handle_behaviour(bowl):
    xr.check_determinism_and_handle(bowl)


def test_physics_on_a_stepped_model(arch):
    xr.check_physics(arch)


def test_refusals(arch, bowl):
    xr.check_python_refusals(bowl)
    xr.check_abi_refusals(bowl)
    xr.check_host_abi_refusals(bowl)
    xr.check_2d_refused(arch)
