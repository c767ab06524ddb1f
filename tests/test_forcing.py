"""Time-dependent surface forcing and the restoring condition (nupgcm_amd.forcing) on the CPU() architecture -
libnupgcm_host.so runs the same per-face arithmetic, the same gathers and the same plan as the device kernels
(csrc/forcing_core.h) - against the numpy restatement of tests/forcing_ref.py.  No GPU.

Every vector and matrix entry is compared with the row's own bound (terms + 8) eps sum |terms|; forcing_ref prints the measured
errors before it asserts.  Measured on the host library (worst |err| / bound): loads 0.10, S entries 0.12, S 1 - load(gamma) 0.05,
A - (M + theta (Kh + Kv) + dt S) 0.15; static equivalence with the toolkits' vectors 0.03; one-step budget 7e-18 against 5e-13 with
max |r| = 5e-19 (LU) against 2e-17."""
import numpy as np
import pytest

import nupgcm_amd as npg
from tests import boundary_ref as br
from tests import forcing_ref as fr
from tests import sampling_ref as sr


@pytest.fixture(scope="module")
def arch():
    return npg.CPU()


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


def test_time_rule_function():
    fr.check_time_rule_function()


def test_static_equivalence(flux_model, wind_model, p1_model):
    fr.check_static(flux_model, "bowl_surface_flux")
    fr.check_static(wind_model, "bowl_wind")
    fr.check_p1_static(p1_model)


def test_loads_against_the_restatement(flux_model):
    assert len(fr.Ref(flux_model).faces) == 753                                           # three rows of 256, a ragged last one
    fr.check_loads(flux_model, "bowl_surface_flux")


@pytest.mark.parametrize("n", fr.EDGE_COUNTS)
def test_loads_through_the_mask(flux_model, n):
    mask = fr.masks(753)[n]
    assert mask.sum() == n
    fr.check_loads(flux_model, f"mask of {n} faces", mask)
    if n in (0, 65):
        fr.check_matrix(flux_model, f"mask of {n} faces", mask)


@pytest.mark.parametrize("b_order", [2, 1])
def test_loads_on_the_channel_basin(arch, b_order):
    model, _ = br.channel_random(arch, b_order)
    assert model.fe_data.mesh.periodic
    fr.check_loads(model, f"channel basin P{b_order}")
    fr.check_matrix(model, f"channel basin P{b_order}")


def test_single_tetrahedron(arch):
    fr.check_single_tet(arch)


def test_time_rule(flux_model):
    fr.check_time_rule(flux_model)


def test_surface_matrix(arch, flux_model, p1_model):
    fr.check_matrix(flux_model, "bowl_surface_flux")
    fr.check_matrix(p1_model, "bowl_surface_flux P1")
    fr.check_axpy(arch, flux_model)


def test_one_step_budget(arch):
    fr.check_one_step_budget(arch, lu=True)


@pytest.mark.parametrize("scheme", ["BDF2", "BDF1 adaptive"])
def test_in_the_loop(arch, scheme):
    fr.check_in_the_loop(arch, scheme)


def test_refusals(arch, flux_model, wind_model):
    fr.check_refusals(arch, flux_model)
    fr.check_dirichlet_refusal(arch, wind_model)
