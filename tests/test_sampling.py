"""Point sampling of the state on the CPU() architecture (libnupgcm_host.so: the same bins, acceptance rule, tie-break and shape
functions as the device kernels, csrc/sample_core.h) against the brute-force evaluator of tests/sampling_ref.py - location, boundary
points, values, polynomial exactness, NaN semantics, the periodic seam, the grid diagnostics and run()'s on_plot hook.  No GPU."""
import ctypes

import numpy as np
import pytest

import nupgcm_amd as npg
from nupgcm_amd import _lib as L
from tests import sampling_ref as sr

NEW = {"npg_locator_create", "npg_locator_destroy", "npg_locator_info", "npg_locator_find", "npg_located_create",
       "npg_located_destroy", "npg_located_upload", "npg_located_download", "npg_fe_sample"}


@pytest.fixture(scope="module")
def arch():
    return npg.CPU()


@pytest.fixture(scope="module")
def flux_model(arch):
    return sr.bowl_model(arch, "bowl_surface_flux", nsteps=3)


@pytest.fixture(scope="module")
def rest_model(arch):
    return sr.bowl_model(arch, "bowl_surface_flux")


def test_both_libraries_export_the_sampling_entry_points():
    assert NEW <= set(L.declared_symbols())
    for path in (L.HOST_LIB_PATH, L.LIB_PATH):
        lib = ctypes.CDLL(path)
        assert not [s for s in NEW if not hasattr(lib, s)], path
    assert not [s for s in L.declared_symbols() if not hasattr(ctypes.CDLL(L.LIB_PATH), s)]


def test_location_against_brute_force(flux_model):
    sr.check_location(flux_model)


def test_boundary_points_are_found(flux_model):
    sr.check_boundary_slice(flux_model)


@pytest.mark.parametrize("name,b_order", [("bowl_surface_flux", 2), ("bowl_diri", 2), ("bowl_surface_flux", 1), ("bowl_diri", 1)])
def test_values_against_the_host_evaluator(arch, flux_model, name, b_order):
    model = flux_model if (name, b_order) == ("bowl_surface_flux", 2) else sr.bowl_model(arch, name, b_order=b_order, nsteps=3)
    sr.compare_values(model, sr.box_points(model, 2500), label=f"{name} P{b_order}")


@pytest.mark.parametrize("b_order", [2, 1])
def test_polynomial_exactness(arch, b_order):
    sr.check_polynomial(arch, b_order)


def test_nan_semantics_and_determinism(flux_model):
    sr.check_nan_and_determinism(flux_model)


def test_periodic_mesh(arch):
    sr.check_periodic(arch)


def test_diagnostics(rest_model):
    sr.check_diagnostics(rest_model)


def test_run_hook(arch):
    sr.check_run_hook(arch)


def test_partitioned_models_are_refused(rest_model):
    rest_model.partition = object()
    try:
        with pytest.raises(NotImplementedError, match="partitioned"):
            npg.nan_eval(rest_model, "b", np.zeros((1, 3)))
        with pytest.raises(NotImplementedError):
            npg.PointLocator(rest_model)
    finally:
        del rest_model.partition
