"""Mesh integrals (nupgcm_amd.integrals) on the CPU() architecture - libnupgcm_host.so runs the same per-cell arithmetic
as the device kernel (csrc/integrals_core.h) - against the numpy restatement of tests/integrals_ref.py, closed forms, the assembled
matrices (x' A x, x' (B b + lift), b' M b, b' (Kh + Kv) b), the energy balance of a converged inversion and buoyancy conservation over
a BDF1 step.  No GPU.

Measured on the host library (bound = n_cells n_q eps S_abs unless said otherwise):
  every channel vs the restatement   at most 1e-3 of the bound (largest: ch7 of the channel basin 1.3e-12 against 1.8e-9)
  polynomial exactness               <= 1.0e-15 against 1.8e-12 .. 1.2e-11
  x'Ax 5.7e-14 (bound 1.1e-9); full stress 2.5e-16 (5.7e-12); x'(Bb + lift) 3.5e-18 (5.6e-12); b'Mb 0 (2.0e-12); b'(Kh+Kv)b 1.4e-14 (7.0e-11)
  energy balance                     |dissipation - production| 7.9e-23 against 2 |x'r| = 1.1e-22 (a direct solve: r is rounding)
  buoyancy conservation              1.1e-16 against sqrt(n_b) ||r_cg|| = 3.2e-16"""
import ctypes

import numpy as np
import pytest

import nupgcm_amd as npg
from nupgcm_amd import _lib as L
from tests import integrals_ref as ir
from tests import sampling_ref as sr

NEW = {"npg_integrals_create", "npg_integrals_destroy", "npg_integrals_compute"}


@pytest.fixture(scope="module")
def arch():
    return npg.CPU()


@pytest.fixture(scope="module")
def flux_model(arch):
    return sr.bowl_model(arch, "bowl_surface_flux", nsteps=3)


def test_both_libraries_export_the_integrals_entry_points():
    assert NEW <= set(L.declared_symbols())
    for path in (L.HOST_LIB_PATH, L.LIB_PATH):
        lib = ctypes.CDLL(path)
        assert not [s for s in NEW if not hasattr(lib, s)], path


@pytest.mark.parametrize("name,b_order", [("bowl_surface_flux", 2), ("bowl_diri", 2), ("bowl_surface_flux", 1), ("bowl_diri", 1)])
def test_every_channel_against_the_restatement(arch, flux_model, name, b_order):
    model = flux_model if (name, b_order) == ("bowl_surface_flux", 2) else sr.bowl_model(arch, name, b_order=b_order, nsteps=3)
    ir.check_channels(model, f"{name} P{b_order}")


def test_every_channel_on_the_embedded_2d_mesh(arch):
    ir.check_channels(ir.bowl2d_model(arch), "bowl_mixing 2-D")


@pytest.mark.parametrize("b_order", [2, 1])
def test_every_channel_on_the_channel_basin(arch, b_order):
    """periodic seam, function-valued nu, the full-stress channel; a random flow (the model is at rest)"""
    model = sr.channel_model(arch, b_order)
    b = model.b_vec.to_host()
    ir.random_state(model)
    model.b_vec.upload(b)
    assert npg.MeshIntegrals(model).full_stress
    ir.check_channels(model, f"channel basin P{b_order}")


def test_polynomial_exactness(arch):
    ir.check_polynomial(arch)


def test_matrix_identities_flux_configuration(arch, flux_model):
    ir.check_matrix_identities(sr.bowl_model(arch, "bowl_surface_flux"), "bowl_surface_flux", variance=True)


def test_matrix_identities_dirichlet_lift_and_full_stress(arch):
    ir.check_matrix_identities(sr.bowl_model(arch, "bowl_diri"), "bowl_diri")
    ir.check_matrix_identities(sr.channel_model(arch), "channel basin (full stress)")


def test_energy_balance_of_a_converged_inversion(arch):
    ir.check_energy_balance(arch)


def test_buoyancy_conservation_over_one_bdf1_step(arch):
    ir.check_buoyancy_conservation(arch)


def test_determinism_and_masking(flux_model):
    ir.check_determinism_and_masking(flux_model, "bowl_surface_flux")


def test_budget_recorder_as_on_plot(arch, tmp_path):
    ir.check_recorder(arch, tmp_path)


def test_refusals(flux_model):
    ir.check_refusals(flux_model)
