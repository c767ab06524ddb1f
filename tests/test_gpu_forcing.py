"""Time-dependent surface forcing on the GPU (libnupgcm_hip.so: k_forcing_local / k_forcing_gather / k_forcing_surface_matrix,
DESIGN.md 25): the restatement, the bounds and the cases of tests/test_forcing.py through the device library, and in addition the
device against the host library on the same tables (the same bound as against the restatement - not a tolerance of its own).  The
face counts cover three workgroups with a ragged last one (bowl: 753 surface faces in rows of 256), exactly 0, 1, 63, 64, 65, 255,
256, 257 faces through the mask, one face (the single tetrahedron) and the periodic seam of the channel basin, P2 and P1."""
import numpy as np
import pytest

import nupgcm_amd as npg
from tests import boundary_ref as br
from tests import forcing_ref as fr
from tests import sampling_ref as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def arch():
    return npg.GPU()


@pytest.fixture(scope="module")
def flux_model(arch):
    return sr.bowl_model(arch, "bowl_surface_flux")


@pytest.fixture(scope="module")
def wind_model(arch):
    return sr.bowl_model(arch, "bowl_wind")


@pytest.fixture(scope="module")
def p1_model(arch):
    return sr.bowl_model(arch, "bowl_surface_flux", b_order=1)


def test_exports():
    fr.check_exports()


def test_static_equivalence(flux_model, wind_model, p1_model):
    fr.check_static(flux_model, "bowl_surface_flux")
    fr.check_static(wind_model, "bowl_wind")
    fr.check_p1_static(p1_model)


def test_loads_against_the_restatement(flux_model, p1_model):
    nf = len(fr.Ref(flux_model).faces)
    assert nf == 753 and nf % 256 != 0 and nf > 2 * 256                                    # several workgroups, a ragged last one
    fr.check_loads(flux_model, "bowl_surface_flux")
    fr.check_device_against_host(flux_model, "bowl_surface_flux")
    fr.check_device_against_host(p1_model, "bowl_surface_flux P1")


@pytest.mark.parametrize("n", fr.EDGE_COUNTS)
def test_loads_through_the_mask(flux_model, n):
    mask = fr.masks(753)[n]
    fr.check_loads(flux_model, f"mask of {n} faces", mask)
    if n in (0, 65, 257):
        fr.check_matrix(flux_model, f"mask of {n} faces", mask)
        fr.check_device_against_host(flux_model, f"mask of {n} faces", mask)


@pytest.mark.parametrize("b_order", [2, 1])
def test_loads_on_the_channel_basin(arch, b_order):
    model, _ = br.channel_random(arch, b_order)
    assert model.fe_data.mesh.periodic
    fr.check_loads(model, f"channel basin P{b_order}")
    fr.check_matrix(model, f"channel basin P{b_order}")
    fr.check_device_against_host(model, f"channel basin P{b_order}")


def test_single_tetrahedron(arch):
    fr.check_single_tet(arch)


def test_time_rule(flux_model):
    fr.check_time_rule(flux_model)


def test_surface_matrix(arch, flux_model, p1_model):
    fr.check_matrix(flux_model, "bowl_surface_flux")
    fr.check_matrix(p1_model, "bowl_surface_flux P1")
    fr.check_axpy(arch, flux_model)


def test_one_step_budget(arch):
    """a CG solve: the residual enters the budget, the solver tolerance drops out"""
    fr.check_one_step_budget(arch, lu=False)


@pytest.mark.parametrize("scheme", ["BDF2", "BDF1 adaptive"])
def test_in_the_loop(arch, scheme):
    fr.check_in_the_loop(arch, scheme)


def test_refusals(arch, flux_model, wind_model):
    fr.check_refusals(arch, flux_model)
    fr.check_dirichlet_refusal(arch, wind_model)
