"""Diffusing particles and reflecting walls on the GPU (libnupgcm_hip.so: k_particles_walk, k_particles_uniforms): the checks
and the bounds of tests/test_particles_walk.py through the device library - 1000 to 3000 particles are several workgroups with a ragged
last one - and in addition the refusal of a partitioned locator handle and the CPU() architecture against the GPU() one on the same
state, seeds and random numbers."""
import os
import subprocess
import sys

import numpy as np
import pytest

import nupgcm_amd as npg
from tests import integrals_ref as ir
from tests import particles_walk_ref as wr
from tests import sampling_ref as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def arch():
    return npg.GPU()


@pytest.fixture(scope="module")
def bare(arch):
    return ir.bare_model(arch)


def test_generator_against_the_numpy_philox(arch):
    wr.check_generator(arch)


def test_free_diffusion_exact_per_particle(bare):
    wr.check_free_diffusion(bare)


def test_linear_kappa_v_against_the_recurrence(bare):
    wr.check_linear_kappa(bare)


def test_flat_surface_reflects(bare):
    wr.check_flat_surface(bare)


def test_one_step_against_the_numpy_restatement_on_the_real_state(arch):
    wr.check_one_step(sr.bowl_model(arch, "bowl_surface_flux", nsteps=3))


def test_well_mixed_census(bare):
    wr.check_census(bare)


def test_periodic_seam_walked(arch):
    wr.check_periodic(arch)


def test_a_walk_that_cannot_be_finished_is_stuck(bare):
    wr.check_stuck(bare)


def test_determinism(bare):
    wr.check_determinism(bare)


def test_refusals_and_edge_cases(bare):
    assert hasattr(npg._lib.lib(), "npg_locator_create_cells")          # the partitioned handle is among the refusals here
    wr.check_refusals(bare)


def test_without_the_keywords_the_tracker_is_unchanged(bare):
    wr.check_opt_in(bare)


def test_tracker_with_diffusion_as_on_plot(arch, tmp_path):
    wr.check_hook(arch, tmp_path)


def test_cpu_and_gpu_architectures_agree(arch, tmp_path):
    """the CPU() architecture's diffusing particles after 20 steps through its state after three timesteps, and the GPU()'s through the
    same state from the same seeds with the same generator seed: the same status, cells, t_lost, wind and reflections, positions to
    20 . 1e-12 . max|x|"""
    out, state = str(tmp_path / "cpu.npz"), str(tmp_path / "state.npz")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "particles_walk_cpu_worker.py")
    subprocess.run([sys.executable, worker, "bowl_surface_flux", "3", out, state], check=True, timeout=600)
    z = np.load(out)
    model = sr.bowl_model(arch, "bowl_surface_flux")
    npg.set_state_from_file(model, state)
    kap = wr.vertex_table(model.fe_data.mesh, wr.KAPPA)
    tr = npg.ParticleTracker(model, z["seeds"], t0=float(z["t0"]), nsub=1, diffusion=(kap, kap, float(z["c_d"])), seed=int(z["seed"]))
    for _ in range(int(z["nsteps"])):
        tr.advance(float(z["h"]))
    got = tr.positions
    err, tol = np.abs(got - z["x"]).max(), int(z["nsteps"]) * 1e-12 * np.abs(z["seeds"]).max()
    print(f"CPU() vs GPU(), walk: {int(z['nsteps'])} steps of h = {float(z['h']):.4e}, {int((tr.status == 0).sum())} alive, "
          f"{int(tr.reflections.sum())} reflections; max|x_gpu - x_cpu| = {err:.3e} (bound {tol:.1e})")
    assert np.array_equal(tr.status, z["status"]) and np.array_equal(tr.cells, z["cells"])
    assert np.array_equal(tr.t_lost, z["t_lost"], equal_nan=True)
    assert np.array_equal(tr.wind, z["wind"]) and np.array_equal(tr.reflections, z["reflections"])
    assert err <= tol
