"""Column integrals on the GPU (libnupgcm_hip.so: k_column_segments<10 | 4>, k_column_fold): the checks and the bounds of
tests/test_columns.py through the device library - 2.8e3 columns and 2e4 segments are many workgroups with a ragged last one, and the
edge sizes run 1, 63, 64, 65 and 1000 columns - and in addition the refusal of a partitioned locator handle and the CPU()
architecture against the GPU() one on the same state, bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

import nupgcm_amd as npg
from tests import columns_ref as cr
from tests import integrals_ref as ir
from tests import sampling_ref as sr

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


def test_tiling_is_the_surfaces_tiling(bare):
    cr.check_tiling(bare)


def test_closed_form_p2(arch):
    cr.check_closed_form(arch)


def test_closed_form_p1_buoyancy(arch):
    cr.check_closed_form(arch, b_order=1)


def test_real_state_against_the_restatement(real):
    cr.check_real_state(real)


def test_grid_diagnostics_cross_check_and_streamfunction(real):
    cr.check_grid_diagnostics(real)


def test_leibniz_jebar_and_bottom_pressure_torque(arch):
    cr.check_leibniz(arch)


def test_geostrophic_flow_has_no_stress_residual(arch):
    cr.check_geostrophic(arch)


def test_edge_sizes_and_determinism(bare):
    cr.check_edges(bare)


def test_refusals_leave_the_outputs_untouched(bare):
    assert hasattr(npg._lib.lib(), "npg_locator_create_cells")          # the partitioned handle is among the refusals here
    cr.check_refusals(bare)


def test_embedded_2d_model_is_refused(arch):
    cr.check_embedded_2d(arch)


def test_periodic_channel_seam(arch):
    cr.check_periodic(arch)


def test_recorder_as_on_plot(arch, tmp_path):
    cr.check_recorder(arch, tmp_path)


def test_cpu_and_gpu_architectures_agree(arch, tmp_path):
    """the CPU() architecture's column integrals of its state after three timesteps, and the GPU()'s of the same state over the same
    columns: the same tiling, and every segment term, integral and end value bit for bit (no closure and no library function is read:
    both libraries run the lines of columns_core.h with contraction off)"""
    out, state = str(tmp_path / "cpu.npz"), str(tmp_path / "state.npz")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "columns_cpu_worker.py")
    subprocess.run([sys.executable, worker, "bowl_surface_flux", "3", out, state], check=True, timeout=600)
    z = np.load(out)
    model = sr.bowl_model(arch, "bowl_surface_flux")
    npg.set_state_from_file(model, state)
    CI = npg.ColumnIntegrals(model, points=z["xy"])
    for a, b in zip(CI.segments(), (z["ptr"], z["cell"], z["zt"], z["zb"])):
        assert np.array_equal(a, b)
    raw, seg = CI.compute_raw(segments=True)
    wet = ~np.isnan(z["raw"][0])
    diff = np.abs(raw - z["raw"])[:, wet]
    print(f"CPU() vs GPU(), columns: {int(wet.sum())} wet columns, {seg.shape[1]} segments; max|gpu - cpu| per channel: "
          + ", ".join(f"{d:.1e}" for d in diff.max(axis=1)) + f"; segment terms {np.abs(seg - z['seg']).max():.1e}")
    assert wet.sum() > 2000 and np.array_equal(seg, z["seg"]) and np.array_equal(raw, z["raw"], equal_nan=True)
