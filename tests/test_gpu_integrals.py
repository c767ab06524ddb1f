"""Mesh integrals on the GPU (libnupgcm_hip.so: k_cell_integrals / k_integrals_fold): the restatement, the bounds and the
cases of tests/test_integrals.py through the device library, and in addition the device against the host library on the same state,
bit-identical repeat calls, masking, a cell count that is no multiple of the workgroup (4259 = 16 x 256 + 163, 672) and fewer cells
than one workgroup (the 2-D mesh's 173 cells; a mask that keeps about 100)."""
import numpy as np
import pytest

import nupgcm_amd as npg
from tests import integrals_ref as ir
from tests import sampling_ref as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def arch():
    return npg.GPU()


@pytest.fixture(scope="module")
def flux_model(arch):
    return sr.bowl_model(arch, "bowl_surface_flux", nsteps=3)


@pytest.mark.parametrize("name,b_order", [("bowl_surface_flux", 2), ("bowl_diri", 2), ("bowl_surface_flux", 1), ("bowl_diri", 1)])
def test_every_channel_against_the_restatement(arch, flux_model, name, b_order):
    model = flux_model if (name, b_order) == ("bowl_surface_flux", 2) else sr.bowl_model(arch, name, b_order=b_order, nsteps=3)
    assert model.fe_data.mesh.ncell % 256 != 0 and model.fe_data.mesh.ncell > 256           # several workgroups, a ragged last one
    ir.check_channels(model, f"{name} P{b_order}")
    ir.check_device_against_host(model, f"{name} P{b_order}")


def test_every_channel_on_the_embedded_2d_mesh(arch):
    model = ir.bowl2d_model(arch)
    assert model.fe_data.mesh.ncell < 256                                                    # fewer cells than one workgroup
    ir.check_channels(model, "bowl_mixing 2-D")
    ir.check_device_against_host(model, "bowl_mixing 2-D")


@pytest.mark.parametrize("b_order", [2, 1])
def test_every_channel_on_the_channel_basin(arch, b_order):
    model = sr.channel_model(arch, b_order)
    b = model.b_vec.to_host()
    ir.random_state(model)
    model.b_vec.upload(b)
    assert npg.MeshIntegrals(model).full_stress
    ir.check_channels(model, f"channel basin P{b_order}")
    ir.check_device_against_host(model, f"channel basin P{b_order}")


def test_polynomial_exactness(arch):
    ir.check_polynomial(arch)


def test_matrix_identities_flux_configuration(arch):
    ir.check_matrix_identities(sr.bowl_model(arch, "bowl_surface_flux"), "bowl_surface_flux", variance=True)


def test_matrix_identities_dirichlet_lift_and_full_stress(arch):
    ir.check_matrix_identities(sr.bowl_model(arch, "bowl_diri"), "bowl_diri")
    ir.check_matrix_identities(sr.channel_model(arch), "channel basin (full stress)")


def test_energy_balance_of_a_converged_inversion(arch):
    ir.check_energy_balance(arch)


def test_buoyancy_conservation_over_one_bdf1_step(arch):
    ir.check_buoyancy_conservation(arch)


def test_repeat_calls_and_masking(flux_model):
    ir.check_determinism_and_masking(flux_model, "bowl_surface_flux")


def test_fewer_cells_than_one_workgroup_by_masking(flux_model):
    nc = flux_model.fe_data.mesh.ncell
    mask = np.zeros(nc, dtype=bool)
    mask[np.random.default_rng(ir.SEED).choice(nc, 100, replace=False)] = True             # spread over all the workgroups
    ir.check_channels(flux_model, "100 cells of bowl_surface_flux", mask)
    ir.check_device_against_host(flux_model, "100 cells of bowl_surface_flux", mask)
    head = np.arange(nc) < 37                                                                # and inside the first workgroup alone
    ir.check_channels(flux_model, "the first 37 cells", head)


def test_refusals(flux_model):
    ir.check_refusals(flux_model)
