"""Column integrals (npg_columns_*) on the CPU() architecture - libnupgcm_host.so tiles the columns, integrates the segments
and folds them with the same code as the device kernels (csrc/columns_core.h) - against closed-form antiderivatives in extended
precision and a numpy restatement on the handle's segments (tests/columns_ref.py, where the bounds are derived).  No GPU.

Measured on the host library (err / bound, largest over the columns and channels):
  tiling                           8523 columns (422 dry), 64004 segments, at most 19 per column: npg_surfaces_*'s bits
  closed form, P2 and P1           17 integrals 0.11; end values 0.016
  real state (3 steps)             31 channels 0.005; 3356 of 8101 wet columns leave a cell through a vertex or an edge (slopes not judged)
  Leibniz                          gamma 0.0024, grad gamma 0.0006, JEBAR 0.0002, bottom pressure torque 0.0027; b'(z): 0.0004
  geostrophic                      |f z^ x U + int grad p dz| 2.4e-15 of |f U| 0.45: 0.003
  GridDiagnostics (reported)       max|dH| 9.8e-4 of 0.5, max|dU| 3.5e-8 of 1.9e-4, max|dV| 3.7e-8 of 1.9e-4"""
import pytest

import nupgcm_amd as npg
from tests import columns_ref as cr
from tests import integrals_ref as ir
from tests import sampling_ref as sr


@pytest.fixture(scope="module")
def arch():
    return npg.CPU()


@pytest.fixture(scope="module")
def bare(arch):
    return ir.bare_model(arch)


@pytest.fixture(scope="module")
def real(arch):
    return sr.bowl_model(arch, "bowl_surface_flux", nsteps=3)


def test_both_libraries_export_the_columns_entry_points():
    cr.check_exports()


def test_tiling_is_the_surfaces_tiling(bare):
    cr.check_tiling(bare)


def test_closed_form_p2(arch):
    cr.check_closed_form(arch)


def test_closed_form_p1_buoyancy(arch):
    cr.check_closed_form(arch, b_order=1)


def test_real_state_against_the_restatement(real):
    cr.check_real_state(real)


def test_grid_diagnostics_cross_check_and_streamfunction(real):
    cr.check_grid_diagnostics(real)


def test_leibniz_jebar_and_bottom_pressure_torque(arch):
    cr.check_leibniz(arch)


def test_geostrophic_flow_has_no_stress_residual(arch):
    cr.check_geostrophic(arch)


def test_edge_sizes_and_determinism(bare):
    cr.check_edges(bare)


def test_refusals_leave_the_outputs_untouched(bare):
    cr.check_refusals(bare)


def test_embedded_2d_model_is_refused(arch):
    cr.check_embedded_2d(arch)


def test_periodic_channel_seam(arch):
    cr.check_periodic(arch)


def test_recorder_as_on_plot(arch, tmp_path):
    cr.check_recorder(arch, tmp_path)
