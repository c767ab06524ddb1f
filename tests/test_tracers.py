"""Passive tracers (nupgcm_amd.tracers) on the CPU() architecture - libnupgcm_host.so runs the same per-cell arithmetic
as the device kernel (csrc/tracers_core.h) - against the numpy restatement of tests/tracers_ref.py: the right-hand side row by row on
every mesh family, the twin of b', independence of the tracers of one call, conservation, refusals, passivity.  No GPU.

Every comparison with the restatement uses the derived bound (terms in the row) eps S_abs of that row; figures are printed before
they are asserted.

Measured on the host library: every row within 4.2e-2 of its bound; the twin bit-identical to npg_fe_evolution_rhs and c = b' to the
bit over 3 steps (direct solves; bound 5.8e-16 .. 1.5e-13); conservation defect <= 2.8e-17 against 8.1e-13 .. 3.1e-12."""
import ctypes

import pytest

import nupgcm_amd as npg
from nupgcm_amd import _lib as L
from tests import helpers
from tests import integrals_ref as ir
from tests import sampling_ref as sr
from tests import tracers_ref as tr

NEW = {"npg_tracers_create", "npg_tracers_destroy", "npg_tracers_set", "npg_tracers_rhs"}


@pytest.fixture(scope="module")
def arch():
    return npg.CPU()


@pytest.fixture(scope="module")
def mixing(arch):
    """bowl3D h = 0.1, P2, Dirichlet b: 4259 cells"""
    return helpers.build_model("bowl_mixing", nsteps=3, arch=arch)


def test_both_libraries_export_the_tracer_entry_points():
    assert NEW <= set(L.declared_symbols())
    for path in (L.HOST_LIB_PATH, L.LIB_PATH):
        lib = ctypes.CDLL(path)
        assert not [s for s in NEW if not hasattr(lib, s)], path


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


@pytest.mark.parametrize("b_order", [2, 1])
def test_rhs_on_the_channel_basin(arch, b_order):
    """the periodic seam; no Dirichlet b: Gamma, S and the flux carry the tracers' differences"""
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


def test_tracers_are_passive_and_a_zero_tracer_stays_zero(arch):
    tr.check_passive(arch)
