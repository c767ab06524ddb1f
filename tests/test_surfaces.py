"""Maps on buoyancy surfaces (npg_surfaces_*) on the CPU() architecture - libnupgcm_host.so tiles the columns and scans
them with the same code as the device kernels (csrc/surfaces_core.h) - against a numpy brute force over all cells, closed-form roots and
nan_eval (tests/surfaces_ref.py).  No GPU.

Measured on the host library:
  tiling, bowl                     793 wet / 296 dry grid columns, at most 18 segments; 1092 / 63 vertex columns; |dz| <= 1.6e-15 against 1e-12
  tiling, channel basin            970 / 119 grid, 120 / 33 vertex, 496 / 32 edge-midpoint columns; min lambda at the midpoints -7.2e-16; no gaps
  B = z                            7525 crossings, 0.011 of 32 eps S_abs
  junctions                        96 interior vertices, each crossed once at its own z and once at the surface, error 0
  junctions, b' != 0               758 junctions, 3790 levels on and within 2 ulp of them: 0 counted twice, 0 of 283695 missed
  P2 monotone                      2124 crossings, < 0.001 of 1088 eps S_abs / |d_z B|; grad B 3.2e-15, u 4.7e-16 against 1e-11
  inversion                        -0.06: 572 one / 109 two (different segments); -0.1249: 36 one / 385 two (225 in one segment); 3.3e-15
  P1                               1214 crossings, 0.003 of 96 eps S_abs
  real state                       2794 crossings; u against nan_eval 0; residual in B 5.6e-16 against 9.3e-12; thickness 1.1e-16"""
import pytest

import nupgcm_amd as npg
from tests import integrals_ref as ir
from tests import sampling_ref as sr
from tests import surfaces_ref as ur


@pytest.fixture(scope="module")
def arch():
    return npg.CPU()


@pytest.fixture(scope="module")
def bare(arch):
    return ir.bare_model(arch)


@pytest.fixture(scope="module")
def real(arch):
    return sr.bowl_model(arch, "bowl_surface_flux", nsteps=3)


def test_both_libraries_export_the_surfaces_entry_points():
    ur.check_exports()


def test_tiling_against_the_brute_force_bowl(bare):
    ur.check_tiling_bowl(bare)


def test_tiling_against_the_brute_force_channel_basin(arch):
    ur.check_tiling_channel(arch)


def test_B_equals_z(bare):
    ur.check_B_equals_z(bare)


def test_a_crossing_on_a_junction_is_counted_once(bare):
    ur.check_junctions(bare)


def test_p2_exact_monotone_field(bare):
    ur.check_p2_monotone(bare)


def test_inversion_two_crossings(bare):
    ur.check_inversion(bare)


def test_p1_buoyancy(arch):
    ur.check_p1(arch)


def test_real_state_against_nan_eval(real):
    ur.check_real_state(real)


def test_edge_sizes_and_determinism(bare):
    ur.check_edges(bare)


def test_refusals_leave_the_outputs_untouched(bare):
    ur.check_refusals(bare)


def test_embedded_2d_model_is_refused(arch):
    ur.check_embedded_2d(arch)


def test_recorder_as_on_plot(arch, tmp_path):
    ur.check_recorder(arch, tmp_path)
