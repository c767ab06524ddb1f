"""Transports through sections (nupgcm_amd.sections) on the CPU() architecture - libnupgcm_host.so builds the same plan
and runs the same per-piece arithmetic and fold as the device kernels (csrc/sections_core.h) - against the independent cutter and the
numpy restatement of tests/sections_ref.py, closed forms, degenerate planes, edge sizes through the mask, determinism, a stepped model
and the refusals.  No GPU."""
import pytest

import nupgcm_amd as npg
from tests import sections_ref as xr


@pytest.fixture(scope="module")
def arch():
    return npg.CPU()


@pytest.fixture(scope="module")
def bowl(arch):
    return xr.bowl(arch)


def test_exports():
    xr.check_exports()


def test_plan_against_the_independent_cutter(bowl):
    xr.check_plans_bowl(bowl)


def test_degenerate_planes_are_counted_once(arch, bowl):
    xr.check_degenerate(arch, bowl)


def test_single_tetrahedron(arch):
    xr.check_single_tet(arch)


def test_closed_forms(arch):
    xr.check_closed_forms(arch)


@pytest.mark.parametrize("b_order", [2, 1])
def test_bowl_against_the_restatement(arch, b_order):
    xr.check_bowl(arch, b_order)


def test_dirichlet_values_and_the_pinned_pressure_vertex(arch):
    xr.check_dirichlet_and_pin(arch)


@pytest.mark.parametrize("b_order", [2, 1])
def test_channel_basin_across_the_seam(arch, b_order):
    xr.check_channel(arch, b_order)


def test_edge_sizes_through_the_mask(bowl):
    xr.check_masks(bowl)


def test_determinism_and_handle_behaviour(bowl):
    xr.check_determinism_and_handle(bowl)


def test_physics_on_a_stepped_model(arch):
    xr.check_physics(arch)


def test_refusals(arch, bowl):
    xr.check_python_refusals(bowl)
    xr.check_abi_refusals(bowl)
    xr.check_2d_refused(arch)
