"""Maps on buoyancy surfaces on the GPU (libnupgcm_hip.so: k_surfaces_scan<10 | 4>, k_surfaces_fields): the checks and the
bounds of tests/test_surfaces.py through the device library - 1089 to 2244 columns are several workgroups with a ragged last one, and
the edge sizes run 1, 63, 64, 65 and 1000 columns - and in addition the refusal of a partitioned locator handle and the CPU()
architecture against the GPU() one on the same state."""
import os
import subprocess
import sys

import numpy as np
import pytest

import nupgcm_amd as npg
from tests import integrals_ref as ir
from tests import sampling_ref as sr
from tests import surfaces_ref as ur

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def arch():
    return npg.GPU()


@pytest.fixture(scope="module")
def bare(arch):
    return ir.bare_model(arch)


@pytest.fixture(scope="module")
def real(arch):
    return sr.bowl_model(arch, "bowl_surface_flux", nsteps=3)


def test_tiling_against_the_brute_force_bowl(bare):
    ur.check_tiling_bowl(bare)


def test_tiling_against_the_brute_force_channel_basin(arch):
    ur.check_tiling_channel(arch)


def test_B_equals_z(bare):
    ur.check_B_equals_z(bare)


def test_a_crossing_on_a_junction_is_counted_once(bare):
    ur.check_junctions(bare)


def test_p2_exact_monotone_field(bare):
    ur.check_p2_monotone(bare)


def test_inversion_two_crossings(bare):
    ur.check_inversion(bare)


def test_p1_buoyancy(arch):
    ur.check_p1(arch)


def test_real_state_against_nan_eval(real):
    ur.check_real_state(real)


def test_edge_sizes_and_determinism(bare):
    ur.check_edges(bare)


def test_refusals_leave_the_outputs_untouched(bare):
    assert hasattr(npg._lib.lib(), "npg_locator_create_cells")          # the partitioned handle is among the refusals here
    ur.check_refusals(bare)


def test_embedded_2d_model_is_refused(arch):
    ur.check_embedded_2d(arch)


def test_recorder_as_on_plot(arch, tmp_path):
    ur.check_recorder(arch, tmp_path)


def test_cpu_and_gpu_architectures_agree(arch, tmp_path):
    """the CPU() architecture's maps of its state after three timesteps, and the GPU()'s of the same state over the same columns and
    levels: the same tiling, the same ncross and status, z to 1e-12 max|z|"""
    out, state = str(tmp_path / "cpu.npz"), str(tmp_path / "state.npz")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "surfaces_cpu_worker.py")
    subprocess.run([sys.executable, worker, "bowl_surface_flux", "3", out, state], check=True, timeout=600)
    z = np.load(out)
    model = sr.bowl_model(arch, "bowl_surface_flux")
    npg.set_state_from_file(model, state)
    S = npg.BuoyancySurfaces(model, z["levels"], points=z["xy"])
    M = S.compute()
    on = z["ncross"] > 0
    scale = np.abs(z["z"][on]).max()
    ez, el = np.abs(M.z - z["z"])[on].max(), np.abs(M.z_low - z["z_low"])[on].max()
    eu = np.abs(M.u - z["u"])[on].max() / np.abs(z["u"][on]).max()
    print(f"CPU() vs GPU(), surfaces: {int(on.sum())} crossings on {len(z['levels'])} levels; max|z_gpu - z_cpu| = {ez:.3e}, z_low {el:.3e} "
          f"(bound {1e-12 * scale:.1e}), u {eu:.2e}")
    assert np.array_equal(S.nseg, z["nseg"]) and np.array_equal(M.z_top, z["z_top"], equal_nan=True) and np.array_equal(M.z_bot, z["z_bot"], equal_nan=True)
    assert np.array_equal(M.ncross, z["ncross"]) and np.array_equal(M.status, z["status"])
    assert on.sum() > 1000 and ez <= 1e-12 * scale and el <= 1e-12 * scale and eu <= 1e-11
    assert np.isnan(M.z[~on]).all()
