"""Isoneutral mixing of the passive tracers on the GPU (libnupgcm_hip.so: k_redi_update / k_redi_matrix / k_tracers_local_iso,
DESIGN.md 30): the restatement, the bounds and the cases of tests/test_redi.py through the device library, and in addition the device
against the host library on the same tables, with that same bound (twice: two evaluations).  Shapes: 4 259 cells = 17 workgroups of
256 with a ragged last one and rows whose cell lists differ in length (P2 and P1), the single tetrahedron, the x-periodic channel basin
(rows that gather across the seam), a model with non-zero Dirichlet values.

Measured on the MI355X (ratios |err| / bound): tensor tables <= 4.7e-2 against the restatement and bit-identical to the host library's
on every mesh; floored / clipped counts equal; K_iso entries <= 1.5e-2 against the restatement and <= 7.1e-3 against the host library
(about half of the entries differ in the last bit: the DPP tree against the host's sequential sum over q); |A_ij - A_ji| = 0 exactly;
row sums <= 2.7e-3; |K_iso B| <= 2.1e-3 of n eps sum_j |K_ij B_j| unclipped, 2.0e9 .. 9.6e9 times it with clipping active; through
the right-hand side on bowl_diri 2.9e-4 unclipped, 1.5e10 clipped; K_iso(slope_max = 0, kappa_h) = NPG_MAT_KH bit for bit; level twin
||A_c (c_iso - c_plain)||_P 8.7e-17 .. 2.2e-16 against 1.5e-6 .. 1.9e-6 (the two CG residuals); right-hand side <= 5.4e-3 and
bit-identical to the host library's; conservation defect <= 2.7e-7 against 4.5e-7 .. 4.1e-6.  22 tests in 15 s."""
import pytest

import nupgcm_amd as npg
from tests import boundary_ref as br
from tests import helpers
from tests import interior_ref as itr
from tests import redi_ref as rr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def arch():
    return npg.GPU()


@pytest.fixture(scope="module")
def mesh():
    return itr.bowl_mesh()


@pytest.fixture(scope="module")
def flux_model(arch, mesh):
    m = itr.light_model(arch, mesh)
    assert m.fe_data.mesh.ncell == 4259                          # 17 workgroups of 256, a ragged last one
    return m


@pytest.fixture(scope="module")
def diri_model(arch, mesh):
    return itr.light_model(arch, mesh, config="bowl_diri")


def _tables_and_matrix(model, label, kind):
    host = rr.HostLibrary(model)
    t, r, _, _ = rr.check_tables(model, label, kind, against=host.tables)
    rr.check_matrix(model, f"{label} [{kind}]", t, r, against=host.matrix)


@pytest.mark.parametrize("kind", ["free", "both"])
def test_tables_counts_and_matrix_on_the_bowl(flux_model, kind):
    _tables_and_matrix(flux_model, "bowl P2", kind)


@pytest.mark.parametrize("kind", ["free", "both"])
def test_tables_counts_and_matrix_p1(arch, mesh, kind):
    _tables_and_matrix(itr.light_model(arch, mesh, b_order=1), "bowl P1", kind)


def test_tables_counts_and_matrix_with_dirichlet_values(diri_model):
    _tables_and_matrix(diri_model, "bowl_diri P2", "both")


@pytest.mark.parametrize("b_order", [2, 1])
def test_single_tetrahedron(arch, b_order):
    m = itr.light_model(arch, br.single_tet(arch).fe_data.mesh, b_order=b_order)
    assert m.fe_data.mesh.ncell == 1
    for kind in ("free", "all"):
        _tables_and_matrix(m, f"single tetrahedron P{b_order}", kind)


@pytest.mark.parametrize("b_order", [2, 1])
def test_channel_basin_rows_across_the_seam(arch, b_order):
    m, _ = br.channel_random(arch, b_order)
    _tables_and_matrix(m, f"channel basin P{b_order}", "both")


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
    m = itr.light_model(arch, mesh, config="bowl_mixing")
    rr.check_rhs(m, "bowl_mixing P2", against=rr.HostLibrary(m).rhs)


def test_rhs_p1(arch, mesh):
    m = itr.light_model(arch, mesh, b_order=1, config="bowl_diri")
    rr.check_rhs(m, "bowl_diri P1", against=rr.HostLibrary(m).rhs)


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
