"""Passive tracers on the GPU (libnupgcm_hip.so: k_tracers_local / k_tracers_gather): the restatement, the bounds and the
cases of tests/test_tracers.py through the device library, and in addition the device against the host library on the same state and
the fp32 element mode against the existing advection kernel's own fp32 error.  Shapes: 4259 cells = 33 workgroups of 128 with a
ragged last one (P2 and P1), the 2-D mesh's 173 cells (one full workgroup and a ragged one, the embedded rule), the periodic channel.

Measured on the MI355X: every row within 4.2e-2 of its bound n eps S_abs; the twin bit-identical to npg_fe_evolution_rhs and c = b' to
the bit over 3 steps (bound 1.3e-6 .. 1.7e-6: the two CG residuals); device = host library on every row; fp32: max |err| / S_abs
1.18e-7 .. 1.69e-7 for the tracers against 1.35e-7 / 1.33e-7 for npg_fe_advection_rhs (allowed twice that); conservation defect
<= 1.4e-7 against 4.7e-7 .. 6.2e-7."""
import pytest

import nupgcm_amd as npg
from tests import helpers
from tests import sampling_ref as sr
from tests import tracers_ref as tr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def arch():
    return npg.GPU()


@pytest.fixture(scope="module")
def mixing(arch):
    model = helpers.build_model("bowl_mixing", nsteps=3, arch=arch)
    assert model.fe_data.mesh.ncell == 4259                      # several workgroups, a ragged last one
    return model


def test_rhs_against_the_restatement_with_the_dirichlet_lift(mixing):
    tr.check_rhs(mixing, "bowl_mixing P2", need_lift=True)


def test_rhs_against_the_restatement_p1(arch):
    tr.check_rhs(sr.bowl_model(arch, "bowl_mixing", b_order=1), "bowl_mixing P1", need_lift=True)


def test_rhs_against_the_restatement_without_dirichlet_nodes(arch):
    tr.check_rhs(sr.bowl_model(arch, "bowl_surface_flux"), "bowl_surface_flux P2")


@pytest.mark.parametrize("K", [1, 3])
def test_rhs_on_the_embedded_2d_mesh(arch, K):
    model = helpers.build_model("bowl_mixing", mesh="mesh_bowl2D_h0.1", nsteps=3, arch=arch)
    assert model.fe_data.mesh.ncell == 173
    tr.check_rhs(model, f"bowl_mixing 2-D K={K}", specs=tr.SPECS3[:K], need_lift=True)
    if K == 3:
        tr.check_device_against_host(model, "bowl_mixing 2-D")


@pytest.mark.parametrize("b_order", [2, 1])
def test_rhs_on_the_channel_basin(arch, b_order):
    tr.check_rhs(sr.channel_model(arch, b_order), f"channel basin P{b_order}")


@pytest.mark.parametrize("name,conv", [("bowl_mixing", (0.5, 0.1)), ("bowl_surface_flux", None)])
def test_twin_of_the_buoyancy(arch, name, conv):
    tr.check_twin(arch, name, conv)


def test_independence_and_fusion(mixing):
    tr.check_independence(mixing, "bowl_mixing P2")


def test_conservation_and_uniform_source(arch):
    tr.check_conservation(arch)


def test_refusals(mixing):
    tr.check_refusals(mixing)


def test_device_against_the_host_library(mixing):
    tr.check_device_against_host(mixing, "bowl_mixing P2")


def test_device_against_the_host_library_p1(arch):
    tr.check_device_against_host(sr.bowl_model(arch, "bowl_mixing", b_order=1), "bowl_mixing P1")


def test_fp32_element_mode_against_the_advection_kernel(mixing):
    tr.check_fp32(mixing, "bowl_mixing P2")


def test_tracers_are_passive_and_a_zero_tracer_stays_zero(arch):
    tr.check_passive(arch)
