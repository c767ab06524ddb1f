"""Interior buoyancy forcing - volume sources and sponge layers (nupgcm_amd.interior) - on the CPU() architecture:
libnupgcm_host.so runs the same per-cell arithmetic, the same gathers and the same plan as the device kernels
(csrc/interior_core.h) - against the numpy restatement of tests/interior_ref.py.  No GPU.

Every load row and every entry of R is compared with its own bound (terms + 8) eps sum |terms|; interior_ref prints the measured
errors before it asserts."""
import numpy as np
import pytest

import nupgcm_amd as npg
from tests import boundary_ref as br
from tests import interior_ref as ir
from tests import sampling_ref as sr


@pytest.fixture(scope="module")
def arch():
    return npg.CPU()


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
    assert nc == 4259 and nc % 256 != 0 and nc > 2 * 256                                   # several rows of 256, a ragged last one
    ir.check_loads(flux_model, "bowl_surface_flux")
    assert (ir.ref_of(mixing_model).rows < 0).any()
    ir.check_loads(mixing_model, "bowl_mixing (Dirichlet surface and coastline)")
    assert np.abs(ir.ref_of(diri_model).bd).max() > 0.1                                    # non-zero Dirichlet values: the lift counts
    ir.check_loads(diri_model, "bowl_diri (non-zero Dirichlet values)")
    ir.check_loads(p1_model, "bowl_surface_flux P1")


@pytest.mark.parametrize("n", ir.EDGE_COUNTS)
def test_loads_through_cells(mixing_model, n):
    cells = ir.first_cells(mixing_model.fe_data.mesh.ncell, n)
    ir.check_loads(mixing_model, f"first {n} cells", cells, matrix=n in (0, 65, 257))


@pytest.mark.parametrize("b_order", [2, 1])
def test_loads_on_the_channel_basin(arch, b_order):
    model, _ = br.channel_random(arch, b_order)
    assert model.fe_data.mesh.periodic
    ir.check_loads(model, f"channel basin P{b_order}")


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
    ir.check_one_step_budget(arch, lu=True)


def test_in_the_loop(arch):
    ir.check_in_the_loop(arch)


def test_a_detached_model_keeps_the_bits_of_one_without_a_forcing(arch):
    ir.check_parent_bits(arch)


def test_refusals(arch, flux_model):
    ir.check_refusals(arch, flux_model)
