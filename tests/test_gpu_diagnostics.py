"""The grid diagnostics on the MI355X (csrc/sample.hip: k_grid_integrals, k_grid_fold): the checks of tests/test_diagnostics.py on
GPU() - against the brute-force evaluator, against sample_to_grid + the host functions, closed forms, determinism and reuse, the
periodic seam, argument errors - and against the CPU() architecture's integrals of the same state (a child process: one process
runs on one architecture)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import nupgcm_amd as npg
from tests import diagnostics_ref as dr
from tests import sampling_ref as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def arch():
    return npg.GPU()


@pytest.fixture(scope="module")
def flux_model(arch):
    return sr.bowl_model(arch, "bowl_surface_flux", nsteps=3)


@pytest.fixture(scope="module")
def rest_model(arch):
    return sr.bowl_model(arch, "bowl_surface_flux")


def test_against_the_independent_evaluator(flux_model):
    dr.check_against_brute(flux_model, (24, 24, 24), exact_counts=True, label="GPU ")


def test_against_the_independent_evaluator_non_cubic(flux_model):
    dr.check_against_brute(flux_model, (19, 24, 31), exact_counts=False, label="GPU non-cubic ")


def test_against_sample_to_grid(flux_model):
    dr.check_against_sample_to_grid(flux_model, (24, 24, 24), label="GPU bowl P2 ")


def test_more_than_one_z_tile_and_x_chunk(flux_model):
    """nz > 256 (two z tiles per workgroup, the second with a tail) and nx not a multiple of the x chunk"""
    dr.check_against_sample_to_grid(flux_model, (21, 6, 300), label="GPU 21 x 6 x 300 ")


def test_at_rest(rest_model):
    dr.check_at_rest(rest_model)


@pytest.mark.parametrize("b_order", [2, 1])
def test_closed_forms(arch, b_order):
    dr.check_polynomial(arch, b_order)


def test_determinism_and_reuse(arch):
    dr.check_determinism_and_reuse(arch)


def test_periodic_channel_basin(arch):
    dr.check_periodic(arch)


def test_arguments(rest_model):
    dr.check_arguments(rest_model)


def test_cpu_and_gpu_architectures_agree(arch, tmp_path):
    """the CPU() architecture's state after three steps, loaded into a GPU() model: the same counts, and integrals within the
    bound of the comparison with the library's own samples"""
    out, state = str(tmp_path / "cpu.npz"), str(tmp_path / "state.npz")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "diagnostics_cpu_worker.py")
    subprocess.run([sys.executable, worker, "bowl_surface_flux", "2", out, state], check=True, timeout=600)
    z = np.load(out)
    model = sr.bowl_model(arch, "bowl_surface_flux", b_order=2)
    npg.set_state_from_file(model, state)
    r = npg.GridDiagnostics(model, 24, 24, 24).compute()
    assert np.array_equal(r.col[0], z["col"][0]) and np.array_equal(r.zon[0], z["zon"][0])
    Lx, Lz = r.x[-1] - r.x[0], r.z[-1] - r.z[0]
    sc, sz = z["scales_c"], z["scales_z"]
    everywhere = np.ones((24, 24), bool)
    dr._compare("CPU() vs GPU() columns", dr.COL[1:], r.col[1:], z["col"][1:], sc * Lz, (everywhere,) * 3, 1e-12)
    dr._compare("CPU() vs GPU() zonal lines", dr.ZON[1:], r.zon[1:], z["zon"][1:], sz * Lx, (everywhere,) * 5, 1e-12)
