"""Isoneutral mixing of the passive tracers (nupgcm_amd.tracers.Isoneutral) on the CPU() architecture -
libnupgcm_host.so runs the same arithmetic as the device kernels (csrc/redi_core.h) - against the numpy restatement of
tests/redi_ref.py: the tensor tables and the floor / clip counts, K_iso entry by entry, the known answer K_iso B = 0, the level twin,
the right-hand side with the rotated tensor, three steps in the loop, refusals.  No GPU.

Every comparison uses the derived bound (terms of the sum) eps S_abs; figures are printed before they are asserted.

Measured on the host library: tables within 4.7e-2 of their bound, K_iso entries within 1.6e-2, |A_ij - A_ji| = 0 exactly, row sums
within 2.7e-3, |K_iso B| within 1.2e-3 of n eps sum_j |K_ij B_j| unclipped and 2e9 times it with clipping active."""
import ctypes

import pytest

import nupgcm_amd as npg
from nupgcm_amd import _lib as L
from tests import boundary_ref as br
from tests import helpers
from tests import interior_ref as itr
from tests import redi_ref as rr


@pytest.fixture(scope="module")
def arch():
    return npg.CPU()


@pytest.fixture(scope="module")
def mesh():
    return itr.bowl_mesh()


@pytest.fixture(scope="module")
def flux_model(arch, mesh):
    """bowl3D h = 0.1, P2, no Dirichlet nodes: 4 259 cells"""
    m = itr.light_model(arch, mesh)
    assert m.fe_data.mesh.ncell == 4259
    return m


@pytest.fixture(scope="module")
def diri_model(arch, mesh):
    return itr.light_model(arch, mesh, config="bowl_diri")


def test_both_libraries_export_the_entry_points():
    assert rr.NEW <= set(L.declared_symbols()) and "Isoneutral" in npg.__all__
    for path in (L.HOST_LIB_PATH, L.LIB_PATH):
        lib = ctypes.CDLL(path)
        assert not [s for s in rr.NEW if not hasattr(lib, s)], path


@pytest.mark.parametrize("kind", ["free", "both"])
def test_tables_counts_and_matrix_on_the_bowl(flux_model, kind):
    t, r, _, _ = rr.check_tables(flux_model, "bowl P2", kind)
    rr.check_matrix(flux_model, f"bowl P2 [{kind}]", t, r)


@pytest.mark.parametrize("kind", ["free", "both"])
def test_tables_counts_and_matrix_p1(arch, mesh, kind):
    m = itr.light_model(arch, mesh, b_order=1)
    t, r, _, _ = rr.check_tables(m, "bowl P1", kind)
    rr.check_matrix(m, f"bowl P1 [{kind}]", t, r)


def test_tables_counts_and_matrix_with_dirichlet_values(diri_model):
    t, r, _, _ = rr.check_tables(diri_model, "bowl_diri P2", "both")
    rr.check_matrix(diri_model, "bowl_diri P2 [both]", t, r)


@pytest.mark.parametrize("b_order", [2, 1])
def test_single_tetrahedron(arch, b_order):
    m = itr.light_model(arch, br.single_tet(arch).fe_data.mesh, b_order=b_order)
    assert m.fe_data.mesh.ncell == 1
    for kind in ("free", "all"):
        t, r, _, _ = rr.check_tables(m, f"single tetrahedron P{b_order}", kind)
        rr.check_matrix(m, f"single tetrahedron P{b_order} [{kind}]", t, r)


@pytest.mark.parametrize("b_order", [2, 1])
def test_channel_basin_rows_across_the_seam(arch, b_order):
    m, _ = br.channel_random(arch, b_order)
    t, r, _, _ = rr.check_tables(m, f"channel basin P{b_order}", "both")
    rr.check_matrix(m, f"channel basin P{b_order}", t, r)


def test_buoyancy_is_not_mixed(flux_model):
    rr.check_not_mixed(flux_model, "bowl_surface_flux P2")


def test_buoyancy_is_not_mixed_p1(arch, mesh):
    rr.check_not_mixed(itr.light_model(arch, mesh, b_order=1), "bowl_surface_flux P1")


def test_buoyancy_is_not_mixed_through_the_right_hand_side(diri_model):
    rr.check_not_mixed_rhs(diri_model, "bowl_diri P2")


@pytest.mark.parametrize("config", ["bowl_mixing", "bowl_diri"])
def test_level_matrix_is_the_engines_kh(arch, mesh, config):
    rr.check_level_matrix(itr.light_model(arch, mesh, config=config), config)


def test_level_twin_three_steps_with_the_convection_closure(arch):
    rr.check_level_twin(arch)


def test_rhs_with_dirichlet_values_and_background_gradient(arch, mesh):
    rr.check_rhs(itr.light_model(arch, mesh, config="bowl_mixing"), "bowl_mixing P2")


def test_rhs_p1(arch, mesh):
    rr.check_rhs(itr.light_model(arch, mesh, b_order=1, config="bowl_diri"), "bowl_diri P1")


def test_rhs_keeps_its_bits_with_the_mode_off(arch, mesh):
    rr.check_mode_off_bits(itr.light_model(arch, mesh, config="bowl_mixing"), "bowl_mixing P2")


@pytest.mark.parametrize("scheme", ["BDF2", "BDF1"])
def test_three_steps_in_the_loop(arch, scheme):
    rr.check_loop(arch, scheme)


def test_a_model_with_a_sponge_and_a_restoring_surface_is_accepted(arch):
    rr.check_forced_model_accepted(arch)


def test_refusals(arch, flux_model):
    flat = helpers.build_model("bowl_mixing", mesh="mesh_bowl2D_h0.1", nsteps=1, arch=arch)
    rr.check_refusals(flux_model, flat)
