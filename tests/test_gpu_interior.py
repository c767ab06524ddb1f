"""Interior buoyancy forcing on the GPU (libnupgcm_hip.so: k_interior_local / k_interior_gather / k_interior_matrix /
k_interior_budget): the restatement, the bounds and the cases of tests/test_interior.py through the device library, and in
addition the device against the host library on the same tables (the same bound as against the restatement - not a tolerance of its
own).  The cell counts cover seventeen workgroups with a ragged last one (bowl: 4 259 cells in rows of 256), exactly 0, 1, 63, 64, 65,
255, 256, 257 kept cells through `cells`, one cell (the single tetrahedron) and the periodic seam of the channel basin, P2 and P1."""
import numpy as np
import pytest

import nupgcm_amd as npg
from tests import boundary_ref as br
from tests import interior_ref as ir
from tests import sampling_ref as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def arch():
    return npg.GPU()


@pytest.fixture(scope="module")
def flux_model(arch):
    return sr.bowl_model(arch, "bowl_surface_flux")


@pytest.fixture(scope="module")
def mixing_model(arch):
    return ir.light_model(arch, ir.bowl_mesh(), config="bowl_mixing")


@pytest.fixture(scope="module")
def diri_model(arch):
    return ir.light_model(arch, ir.bowl_mesh(), config="bowl_diri")


@pytest.fixture(scope="module")
def p1_model(arch):
    return ir.light_model(arch, ir.bowl_mesh(), b_order=1)


def test_exports():
    ir.check_exports()


def test_loads_and_matrix_against_the_restatement(flux_model, mixing_model, diri_model, p1_model):
    nc = flux_model.fe_data.mesh.ncell
    assert nc == 4259 and nc % 256 != 0 and nc > 2 * 256                                   # several workgroups, a ragged last one
    ir.check_loads(flux_model, "bowl_surface_flux")
    assert (ir.ref_of(mixing_model).rows < 0).any()
    ir.check_loads(mixing_model, "bowl_mixing (Dirichlet surface and coastline)")
    assert np.abs(ir.ref_of(diri_model).bd).max() > 0.1                                    # non-zero Dirichlet values: the lift counts
    ir.check_loads(diri_model, "bowl_diri (non-zero Dirichlet values)")
    ir.check_loads(p1_model, "bowl_surface_flux P1")


def test_device_against_the_host_library(flux_model, diri_model, p1_model):
    ir.check_device_against_host(flux_model, "bowl_surface_flux")
    ir.check_device_against_host(diri_model, "bowl_diri")
    ir.check_device_against_host(p1_model, "bowl_surface_flux P1")


@pytest.mark.parametrize("n", ir.EDGE_COUNTS)
def test_loads_through_cells(mixing_model, n):
    cells = ir.first_cells(mixing_model.fe_data.mesh.ncell, n)
    ir.check_loads(mixing_model, f"first {n} cells", cells, matrix=n in (0, 65, 257))
    if n in (0, 65, 257):
        ir.check_device_against_host(mixing_model, f"first {n} cells", cells)


@pytest.mark.parametrize("b_order", [2, 1])
def test_loads_on_the_channel_basin(arch, b_order):
    model, _ = br.channel_random(arch, b_order)
    assert model.fe_data.mesh.periodic
    ir.check_loads(model, f"channel basin P{b_order}")
    ir.check_device_against_host(model, f"channel basin P{b_order}")


def test_single_tetrahedron(arch):
    ir.check_single_tet(arch)


def test_known_answers(arch, flux_model):
    ir.check_known_answers(arch, flux_model)


def test_time_rule(mixing_model):
    ir.check_time_rule(mixing_model)


@pytest.mark.parametrize("scheme", ["BDF2", "BDF1 adaptive"])
def test_operator(arch, scheme):
    ir.check_operator(arch, scheme)


def test_operator_with_a_surface_forcing(flux_model):
    ir.check_with_surface_forcing(flux_model)


def test_one_step_budget(arch):
    """a CG solve: the residual enters the budget, the solver tolerance drops out"""
    ir.check_one_step_budget(arch, lu=False)


def test_in_the_loop(arch):
    ir.check_in_the_loop(arch)


def test_a_detached_model_keeps_the_bits_of_one_without_a_forcing(arch):
    ir.check_parent_bits(arch)


def test_refusals(arch, flux_model):
    ir.check_refusals(arch, flux_model)
