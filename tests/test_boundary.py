"""Boundary integrals (nupgcm_amd.boundary) on the CPU() architecture - libnupgcm_host.so runs the same per-face
arithmetic as the device kernel (csrc/boundary_core.h) - against the numpy restatement of tests/boundary_ref.py, the closed boundary,
the divergence theorem on the discrete fields, closed forms, the project's load vectors and the energy identity with wind.  No GPU.

Measured on the host library (bound = n_faces n_q eps S_abs unless said otherwise; DESIGN.md 23 has the table):
  every channel vs the restatement   at most 1e-3 of the bound (largest: ch18 of the channel basin's bottom 5.7e-14 against 9.5e-11)
  one face's own integrals           at most 0.02 of 128 eps x the magnitude of its terms (up to 4.7 x 9 eps S_abs in the gradient channels)
  closed boundary                    sum n <= 3.7e-17 (bounds 2.6e-13 .. 2.2e-11); sum z n_z - V = -2.2e-16 (bowl), 3.1e-16 (channel basin)
  divergence theorem                 ch5 <= 1.5e-16 (bound 8.9e-12), ch7 <= 2.5e-18 (2.8e-13) on the channel basin
  closed forms                       <= 7.8e-16 against 3.9e-12 .. 3.9e-11
  load identities                    ch19 3.5e-18 (bound 3.9e-14), ch20 1.5e-20 (2.6e-14)
  energy identity with wind          bowl_wind 5.2e-18 against 2 |x'r| = 8.3e-18; channel basin 1.1e-18 against 3.4e-19 + 1e-14 (direct solves:
                                     r is rounding - boundary_ref.check_energy_identity says what is added and why)"""
import ctypes

import numpy as np
import pytest

import nupgcm_amd as npg
from nupgcm_amd import _lib as L
from tests import boundary_ref as br
from tests import integrals_ref as ir
from tests import sampling_ref as sr


@pytest.fixture(scope="module")
def arch():
    return npg.CPU()


@pytest.fixture(scope="module")
def flux_model(arch):
    return sr.bowl_model(arch, "bowl_surface_flux", nsteps=3)


@pytest.fixture(scope="module")
def wind_model(arch):
    return sr.bowl_model(arch, "bowl_wind", nsteps=3)


def test_exports():
    assert {"BoundaryIntegrals", "BoundaryFluxes", "BoundaryMaps", "BoundaryRecorder"} <= set(npg.__all__)
    assert br.NEW <= set(L.declared_symbols()) and L.NPG_NBND == br.NBND
    for path in (L.HOST_LIB_PATH, L.LIB_PATH):
        lib = ctypes.CDLL(path)
        assert not [s for s in br.NEW if not hasattr(lib, s)], path


@pytest.mark.parametrize("name,b_order", [("bowl_surface_flux", 2), ("bowl_surface_flux", 1), ("bowl_diri", 2), ("bowl_wind", 2)])
def test_every_channel_against_the_restatement(arch, flux_model, wind_model, name, b_order):
    model = {("bowl_surface_flux", 2): flux_model, ("bowl_wind", 2): wind_model}.get((name, b_order)) or sr.bowl_model(arch, name, b_order=b_order, nsteps=3)
    bi, raw, _ = br.check_channels(model, f"{name} P{b_order}")
    if name == "bowl_diri":                                                               # the Dirichlet lift: b' = y on the surface, not 0
        per_face = bi.compute_raw(faces=True)[1]
        assert np.abs(per_face[6, bi.face_group == bi.groups.index("surface")]).sum() > 0.1
    if name == "bowl_wind":
        assert raw[bi.groups.index("surface"), 19] != 0.0


@pytest.mark.parametrize("b_order", [2, 1])
def test_every_channel_on_the_channel_basin(arch, b_order):
    """periodic seam, function-valued nu: the full-stress traction; a random flow; and the model as it is - eddy closure on: NaN"""
    model, off = br.channel_random(arch, b_order)
    assert npg.BoundaryIntegrals(off).full_stress and npg.BoundaryIntegrals(off).viscous_available
    br.check_channels(off, f"channel basin P{b_order}")
    br.check_eddy_closure(model)                                                          # (its convection closure is on as well)


def test_every_channel_with_the_convection_closure(wind_model):
    v = br.convection_view(wind_model)
    bi, raw, _ = br.check_channels(v, "bowl_wind, convection closure")
    off, _ = npg.BoundaryIntegrals(wind_model).compute_raw()
    assert (raw[:, 18] != off[:, 18]).all() and np.array_equal(raw[:, :17], off[:, :17])  # the closure acts, and on kappa_v alone


def test_geometry_of_the_closed_boundary(arch, flux_model):
    br.check_geometry(flux_model, "bowl")
    br.check_geometry(br.channel_random(arch)[1], "channel basin", periodic=True)


@pytest.mark.parametrize("b_order", [2, 1])
def test_divergence_theorem_on_the_discrete_fields(arch, b_order):
    model = br.bare_model(arch, b_order=b_order)                                          # no Dirichlet tags: u . n is not 0 on the boundary
    ir.random_state(model)
    out = br.check_divergence_theorem(model, f"bowl without Dirichlet tags P{b_order}")
    assert out[5][1] > 0
    br.check_divergence_theorem(br.channel_random(arch, b_order)[1], f"channel basin P{b_order}")


def test_closed_forms(arch):
    br.check_closed_forms(arch)


def test_load_identities(wind_model, flux_model):
    br.check_load_identities(wind_model, flux_model)


def test_energy_identity_with_wind(arch, wind_model):
    br.check_energy_identity(wind_model, "bowl_wind after 3 steps")
    chan = sr.channel_model(arch)
    npg.invert(chan)
    br.check_energy_identity(chan, "channel basin, converged inversion")


def test_edge_sizes_through_the_mask(flux_model):
    br.check_edge_sizes(flux_model, "bowl_surface_flux")


def test_single_tetrahedron(arch):
    br.check_single_tet(arch)


def test_determinism(flux_model):
    br.check_determinism(flux_model)


def test_refusals(arch, flux_model):
    br.check_refusals(flux_model)
    br.check_2d_refused(arch)


def test_fluxes_and_maps(wind_model):
    br.check_fluxes_and_maps(wind_model)


def test_boundary_recorder_as_on_plot(arch, tmp_path):
    br.check_recorder(arch, tmp_path)
