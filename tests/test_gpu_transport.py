"""The tracers' transport operator as a matrix on the GPU (libnupgcm_hip.so: k_transport_velocity / k_transport_matrix /
k_transport_load): the restatement, the bounds and the cases of tests/test_transport.py through the device library, and
in addition the device against the host library on the same tables (velocity tables bit for bit; C and the loads within twice the
bound).  Shapes: 4 259 cells = 17 workgroups of 256 with a ragged last one and rows whose cell lists differ in length (P2 and P1),
the single tetrahedron, the x-periodic channel basin (rows that gather across the seam), models with non-zero Dirichlet values.

The measured worst |err| / bound of every check is in DESIGN.md 31."""
import pytest

import nupgcm_amd as npg
from tests import boundary_ref as br
from tests import helpers
from tests import interior_ref as itr
from tests import transport_ref as tp

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


@pytest.fixture(scope="module")
def p1_model(arch, mesh):
    return itr.light_model(arch, mesh, b_order=1, config="bowl_diri")


def _tables_and_matrix(model, label):
    tp.check_tables(model, label, against=tp.HostRaw(model))
    tp.check_matrix(model, label, against=tp.HostRaw(model))


def test_both_libraries_export_the_entry_points():
    tp.check_exports()


def test_velocity_tables_and_matrix_on_the_bowl(flux_model):
    _tables_and_matrix(flux_model, "bowl P2")


def test_velocity_tables_and_matrix_with_dirichlet_nodes(diri_model):
    _tables_and_matrix(diri_model, "bowl_diri P2")


def test_velocity_tables_and_matrix_p1(p1_model):
    _tables_and_matrix(p1_model, "bowl_diri P1")


@pytest.mark.parametrize("b_order", [2, 1])
def test_single_tetrahedron(arch, b_order):
    m = itr.light_model(arch, br.single_tet(arch).fe_data.mesh, b_order=b_order)
    assert m.fe_data.mesh.ncell == 1
    _tables_and_matrix(m, f"single tetrahedron P{b_order}")
    tp.check_twin(m, f"single tetrahedron P{b_order}")


@pytest.mark.parametrize("b_order", [2, 1])
def test_channel_basin_rows_across_the_seam(arch, b_order):
    m, _ = br.channel_random(arch, b_order)
    _tables_and_matrix(m, f"channel basin P{b_order}")


def test_a_linear_tracer_is_advected_exactly(flux_model):
    tp.check_linear_tracer(flux_model, "bowl P2")


def test_explicit_twin_with_dirichlet_values(diri_model):
    tp.check_twin(diri_model, "bowl_diri P2")


def test_explicit_twin_p1(p1_model):
    tp.check_twin(p1_model, "bowl_diri P1")


def test_loads_with_decay(diri_model):
    tp.check_load(diri_model, "bowl_diri P2", against=tp.HostRaw(diri_model))


def test_loads_p1(p1_model):
    tp.check_load(p1_model, "bowl_diri P1", against=tp.HostRaw(p1_model))


def test_ideal_age_equilibrium_and_step_algebra(arch):
    tt, _ = tp.check_ideal_age(arch)
    tp.check_step_algebra(arch, tt)


def test_decaying_tracer_equilibrium_without_dirichlet_nodes(arch):
    tp.check_decaying(arch)


def test_a_tracer_that_is_one_on_the_boundary_stays_one(arch, mesh):
    tp.check_constant(arch, mesh)


def test_transport_is_passive(arch):
    tp.check_passive(arch)


def test_refusals(arch, flux_model):
    flat = helpers.build_model("bowl_mixing", mesh="mesh_bowl2D_h0.1", nsteps=1, arch=arch)
    tp.check_refusals(flux_model, flat)
