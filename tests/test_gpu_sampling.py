"""Point sampling of the device-resident state on the MI355X (csrc/sample.hip: k_locate, k_sample) against the brute-force fp64
evaluator of tests/sampling_ref.py - the checks of tests/test_sampling.py on GPU() - and against the CPU() architecture's samples
of the same configuration (a child process: one process runs on one architecture)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import nupgcm_amd as npg
from tests import sampling_ref as sr

pytestmark = pytest.mark.gpu
CASES = [("bowl_surface_flux", 2), ("bowl_diri", 2), ("bowl_surface_flux", 1), ("bowl_diri", 1)]


@pytest.fixture(scope="module")
def arch():
    return npg.GPU()


@pytest.fixture(scope="module")
def models(arch):
    cache = {}

    def get(name, order, nsteps=3):
        if (name, order, nsteps) not in cache:
            cache[(name, order, nsteps)] = sr.bowl_model(arch, name, b_order=order, nsteps=nsteps)
        return cache[(name, order, nsteps)]
    return get


def test_location_against_brute_force(models):
    sr.check_location(models("bowl_surface_flux", 2))


def test_boundary_points_are_found(models):
    sr.check_boundary_slice(models("bowl_surface_flux", 2))


@pytest.mark.parametrize("name,b_order", CASES)
def test_values_against_the_host_evaluator(models, name, b_order):
    model = models(name, b_order)
    sr.compare_values(model, sr.box_points(model, 2500), label=f"GPU {name} P{b_order}")


@pytest.mark.parametrize("b_order", [2, 1])
def test_polynomial_exactness(arch, b_order):
    sr.check_polynomial(arch, b_order)


def test_nan_semantics_and_determinism(models):
    sr.check_nan_and_determinism(models("bowl_surface_flux", 2))


def test_periodic_mesh(arch):
    sr.check_periodic(arch)


def test_diagnostics(models):
    sr.check_diagnostics(models("bowl_surface_flux", 2, 0))


def test_run_hook(arch):
    sr.check_run_hook(arch)


@pytest.mark.parametrize("name,b_order", CASES[1:3])
def test_cpu_and_gpu_architectures_agree(arch, tmp_path, name, b_order):
    """the CPU() architecture's state after three steps, loaded into a GPU() model: same cells, and the values of the two
    architectures at the points of the comparison with the evaluator agree within its bounds"""
    out, state = str(tmp_path / "cpu.npz"), str(tmp_path / "state.npz")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sampling_cpu_worker.py")
    subprocess.run([sys.executable, worker, name, str(b_order), out, state], check=True, timeout=600)
    z = np.load(out)
    model = sr.bowl_model(arch, name, b_order=b_order)
    npg.set_state_from_file(model, state)
    loc = npg.PointLocator(model).locate(z["pts"])
    assert np.array_equal(loc.cells, z["cells"])
    ok = loc.valid
    for f, bound in (("u", 1e-11), ("p", 1e-11), ("b", 1e-11), ("grad_b", 1e-10)):
        got = npg.nan_eval(model, f, z["pts"], loc)
        assert np.array_equal(np.isnan(got), np.isnan(z[f]))
        err = np.abs(got[ok] - z[f][ok]).max() / np.abs(z[f][ok]).max()
        print(f"CPU() vs GPU() {name} P{b_order} {f}: {err:.2e} (bound {bound:.0e})")
        assert err <= bound
