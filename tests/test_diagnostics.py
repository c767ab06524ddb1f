"""The grid diagnostics on the CPU() architecture (libnupgcm_host.so runs the same sample_core.h arithmetic as the device kernel):
GridDiagnostics / npg_fe_grid_integrals against the brute-force evaluator reduced as the reference's post-processing reduces its
grid, against sample_to_grid + the host functions, closed forms, determinism and reuse, the periodic seam, argument errors and the
ABI.  The checks live in tests/diagnostics_ref.py.  No GPU."""
import ctypes

import pytest

import nupgcm_amd as npg
from nupgcm_amd import _lib as L
from tests import diagnostics_ref as dr
from tests import sampling_ref as sr


@pytest.fixture(scope="module")
def arch():
    return npg.CPU()


@pytest.fixture(scope="module")
def flux_model(arch):
    return sr.bowl_model(arch, "bowl_surface_flux", nsteps=3)


@pytest.fixture(scope="module")
def rest_model(arch):
    return sr.bowl_model(arch, "bowl_surface_flux")


def test_both_libraries_export_the_grid_integrals():
    assert "npg_fe_grid_integrals" in L.declared_symbols()
    for path in (L.HOST_LIB_PATH, L.LIB_PATH):
        assert hasattr(ctypes.CDLL(path), "npg_fe_grid_integrals"), path


def test_public_names():
    for name in ("GridDiagnostics", "GridIntegrals", "zonal_width", "zonal_mean", "overturning_streamfunction", "average_stratification"):
        assert hasattr(npg, name), name


def test_against_the_independent_evaluator(flux_model):
    dr.check_against_brute(flux_model, (24, 24, 24), exact_counts=True)


def test_against_the_independent_evaluator_non_cubic(flux_model):
    dr.check_against_brute(flux_model, (19, 24, 31), exact_counts=False, label="non-cubic ")


def test_against_sample_to_grid(flux_model):
    dr.check_against_sample_to_grid(flux_model, (24, 24, 24), label="bowl P2 ")


def test_at_rest(rest_model):
    dr.check_at_rest(rest_model)


@pytest.mark.parametrize("b_order", [2, 1])
def test_closed_forms(arch, b_order):
    dr.check_polynomial(arch, b_order)


def test_determinism_and_reuse(arch):
    dr.check_determinism_and_reuse(arch)


def test_periodic_channel_basin(arch):
    dr.check_periodic(arch)


def test_arguments(rest_model):
    dr.check_arguments(rest_model)
