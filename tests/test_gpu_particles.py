"""Particle tracking on the GPU (libnupgcm_hip.so: k_particles_advance): the checks and the bounds of
tests/test_particles.py through the device library - 2000 and 3000 particles are several workgroups with a ragged last one, a few
particles and none are less than one - and in addition the refusal of a partitioned locator handle and the CPU() architecture against
the GPU() one on the same state and seeds."""
import os
import subprocess
import sys

import numpy as np
import pytest

import nupgcm_amd as npg
from tests import integrals_ref as ir
from tests import particles_ref as pr
from tests import sampling_ref as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def arch():
    return npg.GPU()


@pytest.fixture(scope="module")
def bare(arch):
    return ir.bare_model(arch)


def test_rotation_against_the_closed_form_across_cells(bare):
    pr.check_rotation(bare)


def test_general_affine_flow_against_the_closed_form(bare):
    pr.check_general_affine(bare)


def test_leaving_the_mesh_where_the_brute_force_says(bare):
    pr.check_leaving(bare)


def test_time_blend_against_a_numpy_rk4(bare):
    pr.check_blend(bare)


@pytest.mark.parametrize("name,nsteps", [("bowl_surface_flux", 3), ("bowl_diri", 1)])
def test_real_state_against_nan_eval(arch, name, nsteps):
    pr.check_real_state(sr.bowl_model(arch, name, nsteps=nsteps), name)


def test_determinism(bare):
    pr.check_determinism(bare)


def test_periodic_seam(arch):
    pr.check_periodic(arch)


def test_tracker_as_on_plot(arch, tmp_path):
    pr.check_hook(arch, tmp_path)


def test_refusals_and_edge_cases(bare):
    assert hasattr(npg._lib.lib(), "npg_locator_create_cells")          # the partitioned handle is among the refusals here
    pr.check_refusals(bare)


def test_cpu_and_gpu_architectures_agree(arch, tmp_path):
    """the CPU() architecture's particles after 20 steps through its state after three timesteps, and the GPU()'s through the same
    state from the same seeds: the same status and cells, positions to 20 . 1e-12 . max|x| (the two compilers may contract
    differently)"""
    out, state = str(tmp_path / "cpu.npz"), str(tmp_path / "state.npz")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "particles_cpu_worker.py")
    subprocess.run([sys.executable, worker, "bowl_surface_flux", "3", out, state], check=True, timeout=600)
    z = np.load(out)
    model = sr.bowl_model(arch, "bowl_surface_flux")
    npg.set_state_from_file(model, state)
    tr = npg.ParticleTracker(model, z["seeds"], t0=float(z["t0"]), nsub=1)
    for _ in range(int(z["nsteps"])):
        tr.advance(float(z["h"]))
    got = tr.positions
    err, tol = np.abs(got - z["x"]).max(), int(z["nsteps"]) * 1e-12 * np.abs(z["seeds"]).max()
    print(f"CPU() vs GPU(): {int(z['nsteps'])} steps of h = {float(z['h']):.4e}, {int((tr.status == 0).sum())} alive; "
          f"max|x_gpu - x_cpu| = {err:.3e} (bound {tol:.1e})")
    assert np.array_equal(tr.status, z["status"]) and np.array_equal(tr.cells, z["cells"])
    assert np.array_equal(tr.t_lost, z["t_lost"], equal_nan=True)
    assert err <= tol
