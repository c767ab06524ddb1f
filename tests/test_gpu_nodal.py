"""Nodal gradient recovery on the GPU (libnupgcm_hip.so: k_nodal_cells / k_nodal_nodes): the restatement, the bounds and
the cases of tests/test_nodal.py through the device library, and in addition the device against the host library on the same state -
every bit, on every mesh.  The node counts cover one lane (the single tetrahedron: 10 nodes), several workgroups with a ragged last
one (bowl: 7 434 nodes, 4 259 cells) and exactly 0, 1, 63, 64, 65, 255, 256, 257 nodes through the mask."""
import pytest

import nupgcm_amd as npg
from tests import nodal_ref as nr
from tests import sampling_ref as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def arch():
    return npg.GPU()


@pytest.fixture(scope="module")
def bowl(arch):
    return nr.bowl(arch)


def test_single_tetrahedron(arch):
    nr.check_single_tet(arch, against_host=True)


def test_bowl_against_the_restatement_and_the_host_library(bowl):
    nr.check_bowl_shapes(bowl, against_host=True)


def test_p1_buoyancy(arch):
    nr.check_restatement(nr.bowl(arch, b_order=1), "bowl P1", against_host=True)


def test_edge_sizes_through_the_mask(bowl):
    nr.check_masks(bowl, against_host=True)


def test_dirichlet_values_and_the_pinned_pressure_vertex(arch):
    nr.check_dirichlet_and_pin(arch, against_host=True)


@pytest.mark.parametrize("b_order", [2, 1])
def test_channel_basin_across_the_seam(arch, b_order):
    nr.check_channel(arch, b_order, against_host=True)


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
    nr.check_host_abi_refusals(bowl)
    nr.check_2d_refused(arch)
