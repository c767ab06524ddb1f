"""Nodal gradient recovery (nupgcm_amd.nodal) on the CPU() architecture - libnupgcm_host.so runs the same per-cell and
per-node arithmetic as the device kernels (csrc/nodal_core.h) - against the numpy restatement of tests/nodal_ref.py, closed forms,
save_vtk's closure fields and file, determinism, field selection and the refusals.  No GPU."""
import pytest

import nupgcm_amd as npg
from tests import nodal_ref as nr
from tests import sampling_ref as sr


@pytest.fixture(scope="module")
def arch():
    return npg.CPU()


@pytest.fixture(scope="module")
def bowl(arch):
    return nr.bowl(arch)


def test_exports():
    nr.check_exports()


def test_single_tetrahedron(arch):
    nr.check_single_tet(arch)


def test_bowl_against_the_restatement(bowl):
    nr.check_bowl_shapes(bowl)


def test_p1_buoyancy_against_the_restatement(arch):
    nr.check_restatement(nr.bowl(arch, b_order=1), "bowl P1")


def test_edge_sizes_through_the_mask(bowl):
    nr.check_masks(bowl)


def test_dirichlet_values_and_the_pinned_pressure_vertex(arch):
    nr.check_dirichlet_and_pin(arch)


@pytest.mark.parametrize("b_order", [2, 1])
def test_channel_basin_across_the_seam(arch, b_order):
    nr.check_channel(arch, b_order)


def test_closed_forms(arch):
    nr.check_closed_forms(arch)


def test_closures_agree_with_save_vtk(arch):
    nr.check_closures_against_io(arch)


def test_save_vtk_with_and_without_nodal(arch, tmp_path):
    model = sr.bowl_model(arch, "bowl_surface_flux", nsteps=1)
    nr.check_vtk(model, tmp_path)


def test_determinism_and_field_selection(bowl):
    nr.check_determinism_and_selection(bowl)


def test_refusals(arch, bowl):
    nr.check_python_refusals(bowl)
    nr.check_abi_refusals(bowl)
    nr.check_2d_refused(arch)
