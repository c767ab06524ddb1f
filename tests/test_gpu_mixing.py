"""Water-mass transformation by mixing (BuoyancyClasses.mixing) on the GPU (libnupgcm_hip.so: k_class_scan / k_classes_fold /
k_class_bin / k_classes_convert with the MixSampler): the restatement, the bounds and the cases of tests/test_mixing.py through the device library, and in
addition the device table against the host library's on the same state.  bowl3D h = 0.1 has 4259 = 16 x 256 + 163 cells (several
workgroups, a ragged last one), the 2-D bowl 173 (fewer than one workgroup).  Not reached at these sizes: the grid-stride wrap (more
than 1024 workgroups' worth of cells); the loop text is the census's (one kernel template for both samplers)."""
import pytest

import nupgcm_amd as npg
from tests import integrals_ref as ir
from tests import mixing_ref as mr
from tests import sampling_ref as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def arch():
    return npg.GPU()


@pytest.fixture(scope="module")
def flux_model(arch):
    """no Dirichlet b"""
    return sr.bowl_model(arch, "bowl_surface_flux", nsteps=3)


@pytest.fixture(scope="module")
def mix_model(arch):
    """N2 = 1 / alpha and Dirichlet b: B and b' bin differently, Dirichlet nodes count"""
    return sr.bowl_model(arch, "bowl_mixing", nsteps=3)


@pytest.fixture(scope="module")
def p1_model(arch):
    return sr.bowl_model(arch, "bowl_mixing", b_order=1, nsteps=3)


def channel(arch):
    """the small channel basin (periodic seam) with a random state"""
    model = sr.channel_model(arch)
    ir.random_state(model)
    return model


def test_table_against_the_restatement_bowl_p2(mix_model):
    assert mix_model.fe_data.mesh.ncell % 256 != 0 and mix_model.fe_data.mesh.ncell > 256
    mr.check_table(mix_model, "bowl P2")
    mr.check_device_against_host(mix_model, "bowl P2")
    mr.check_device_against_host(mix_model, "bowl P2 level 2", level=2)


def test_table_against_the_restatement_bowl_p1(p1_model):
    mr.check_table(p1_model, "bowl P1")
    mr.check_device_against_host(p1_model, "bowl P1")


def test_table_against_the_restatement_channel_basin(arch):
    model = channel(arch)
    mr.check_table(model, "channel basin")
    mr.check_device_against_host(model, "channel basin")


def test_table_against_the_restatement_embedded_2d(arch):
    model = ir.bowl2d_model(arch)
    assert model.fe_data.mesh.ncell < 256
    mr.check_table(model, "bowl 2-D")
    mr.check_device_against_host(model, "bowl 2-D")


def test_channel_0_is_the_census(mix_model, p1_model):
    mr.check_census_tie(mix_model, "bowl P2")
    mr.check_census_tie(p1_model, "bowl P1")


def test_sums_over_the_bins_equal_the_mesh_integrals(arch):
    mr.check_integrals_tie(mr.linear_kappa_model(arch), "bowl P1, kappa linear in x")


def test_closed_forms_and_closure_limits(flux_model):
    mr.check_closed_forms(flux_model, "bowl P2")


def test_scalars_equal_constant_tables(mix_model):
    mr.check_scalars_equal_tables(mix_model)


def test_determinism_and_the_shared_handle(mix_model):
    mr.check_determinism(mix_model)


def test_dropped_samples(flux_model, p1_model):
    mr.check_dropped(flux_model, "bowl P2")
    mr.check_dropped(p1_model, "bowl P1")


def test_shapes(mix_model):
    mr.check_shapes(mix_model, "bowl P2")


def test_refusals(flux_model):
    mr.check_refusals(flux_model)


def test_class_recorder_with_mixing_as_on_plot(arch, tmp_path):
    mr.check_recorder(lambda: sr.bowl_model(arch, "bowl_surface_flux"), tmp_path)
