"""The flow binned into (latitude band, buoyancy class) (nupgcm_amd.watermass) on the GPU (libnupgcm_hip.so: k_class_scan /
k_classes_fold / k_class_bin / k_classes_convert with the CensusSampler): the restatement, the bounds and the cases of tests/test_watermass.py through the
device library, and in addition the device table against the host library's on the same state.  bowl3D h = 0.1 has 4259 = 16 x 256 + 163
cells (several workgroups, a ragged last one), the 2-D bowl 173 (fewer than one workgroup)."""
import pytest

import nupgcm_amd as npg
from tests import integrals_ref as ir
from tests import sampling_ref as sr
from tests import watermass_ref as wr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def arch():
    return npg.GPU()


@pytest.fixture(scope="module")
def flux_model(arch):
    return sr.bowl_model(arch, "bowl_surface_flux", nsteps=3)


@pytest.fixture(scope="module")
def mix_model(arch):
    """N2 = 1 / alpha and Dirichlet b: B and b' bin differently, Dirichlet nodes count"""
    return sr.bowl_model(arch, "bowl_mixing", nsteps=3)


@pytest.fixture(scope="module")
def p1_model(arch):
    return sr.bowl_model(arch, "bowl_mixing", b_order=1, nsteps=3)


def channel(arch):
    """the small channel basin (periodic seam) with a random flow and its own buoyancy"""
    model = sr.channel_model(arch)
    b = model.b_vec.to_host()
    ir.random_state(model)
    model.b_vec.upload(b)
    return model


def test_table_against_the_restatement_bowl_p2(mix_model):
    assert mix_model.fe_data.mesh.ncell % 256 != 0 and mix_model.fe_data.mesh.ncell > 256
    wr.check_table(mix_model, "bowl P2")
    wr.check_device_against_host(mix_model, "bowl P2")
    wr.check_device_against_host(mix_model, "bowl P2 level 2", level=2)


def test_table_against_the_restatement_bowl_p1(p1_model):
    wr.check_table(p1_model, "bowl P1")
    wr.check_device_against_host(p1_model, "bowl P1")


def test_table_against_the_restatement_channel_basin(arch):
    model = channel(arch)
    wr.check_table(model, "channel basin")
    wr.check_device_against_host(model, "channel basin")


def test_table_against_the_restatement_embedded_2d(arch):
    model = ir.bowl2d_model(arch)
    assert model.fe_data.mesh.ncell < 256
    wr.check_table(model, "bowl 2-D")
    wr.check_device_against_host(model, "bowl 2-D")


def test_identities_against_the_mesh_integrals(mix_model, p1_model):
    wr.check_identities(mix_model, "bowl P2")
    wr.check_identities(p1_model, "bowl P1", p1=True)


def test_ties_at_an_edge(flux_model):
    wr.check_ties(flux_model)


def test_shapes(flux_model):
    wr.check_shapes(flux_model, "bowl P2")


def test_determinism_and_rezeroing(flux_model):
    wr.check_determinism(flux_model)


def test_dropped_samples(flux_model, p1_model):
    wr.check_dropped(flux_model, "bowl P2")
    wr.check_dropped(p1_model, "bowl P1")


def test_refusals(flux_model):
    wr.check_refusals(flux_model)
    wr.check_replicated_layout_refused(flux_model)


def test_class_recorder_as_on_plot(arch, tmp_path):
    wr.check_recorder(sr.bowl_model(arch, "bowl_surface_flux"), tmp_path)
