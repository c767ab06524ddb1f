"""The linearised model on the GPU (libnupgcm_hip.so: k_tangent_local + the engine's fixed-order gather): the checks of
tests/test_linearized.py through the device library behind the dense-inverse preconditioner, and in addition the device against the
host library on the same tables (bit for bit) and against the CPU() architecture's operator and modes (a child process: one process
runs on one architecture).  Shapes of the tangent load: 4 259 cells = 17 workgroups of 256 with a ragged last one and gather rows of
unequal length (P2 and P1), non-zero Dirichlet values, the single tetrahedron, the x-periodic channel basin (rows that gather across
the seam), the embedded 2-D bowl.  The largest eigenproblem is a 40-vector Krylov space on 5 864 unknowns.

No test reads the reference tree or provokes an error on the device: the refusals fail on the host, in argument checks."""
import os
import subprocess
import sys

import numpy as np
import pytest

import nupgcm_amd as npg
from tests import boundary_ref as br
from tests import helpers
from tests import interior_ref as itr
from tests import linearized_ref as lr

pytestmark = pytest.mark.gpu
DENSE = dict(preconditioner="dense_inverse")


@pytest.fixture(scope="module")
def arch():
    return npg.GPU()


@pytest.fixture(scope="module")
def mesh():
    return itr.bowl_mesh()


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    """the CPU() architecture's results, computed once"""
    out = str(tmp_path_factory.mktemp("linearized") / "cpu.npz")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "linearized_cpu_worker.py")
    subprocess.run([sys.executable, worker, out], check=True, timeout=600)
    z = np.load(out)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def wind_model(arch):
    return helpers.build_model("bowl_wind", nsteps=1, arch=arch, **DENSE)


def _case(cpu, prefix):
    return {k[len(prefix):]: v for k, v in cpu.items() if k.startswith(prefix)}


def test_both_libraries_export_the_entry_point():
    lr.check_exports()


@pytest.mark.parametrize("b_order", [2, 1])
def test_tangent_load_on_the_bowl(arch, mesh, b_order):
    m = itr.light_model(arch, mesh, b_order=b_order)
    assert m.fe_data.mesh.ncell == 4259                          # 17 workgroups of 256, a ragged last one
    lr.check_load(m, f"bowl P{b_order}", host=True)


def test_tangent_load_with_dirichlet_values(arch, mesh):
    m = itr.light_model(arch, mesh, config="bowl_diri")
    lr.check_load(m, "bowl_diri P2", host=True, N2=0.0)
    lr.check_dirichlet(m, itr.light_model(arch, mesh, config="bowl_diri", b_diri_vals=0.0), "bowl_diri P2")


@pytest.mark.parametrize("b_order", [2, 1])
def test_tangent_load_single_tetrahedron(arch, b_order):
    m = itr.light_model(arch, br.single_tet(arch).fe_data.mesh, b_order=b_order)
    assert m.fe_data.mesh.ncell == 1
    lr.check_load(m, f"single tetrahedron P{b_order}", host=True)


@pytest.mark.parametrize("b_order", [2, 1])
def test_tangent_load_across_the_periodic_seam(arch, b_order):
    m, _ = br.channel_random(arch, b_order)
    lr.check_load(m, f"channel basin P{b_order}", host=True)


def test_tangent_load_embedded_2d(arch):
    lr.check_load(lr.flat_model(arch, 0, **DENSE), "embedded 2-D bowl", host=True)


def test_apply_matches_the_cpu_architecture_after_three_steps(arch, cpu):
    model = helpers.build_model("bowl_mixing", nsteps=1, arch=arch, **DENSE)
    lr.check_derivative_against(model, _case(cpu, "d_mixing_"), "bowl_mixing after 3 steps")


def test_apply_matches_the_cpu_architecture_under_wind(wind_model, cpu):
    lr.check_derivative_against(wind_model, _case(cpu, "d_wind_"), "bowl_wind")


def test_apply_is_linear_for_tiny_perturbations(arch):
    lr.check_linearity(lr.flat_model(arch, 5, **DENSE), "2-D bowl")


def test_the_models_own_atol_would_drop_the_advective_part(arch):
    lr.check_atol_pitfall(lr.flat_model(arch, 5, **DENSE), "2-D bowl")


def test_linearisation_is_passive(arch):
    lr.check_passive(arch, "2-D bowl", **DENSE)


def test_diffusion_modes_match_eigsh(wind_model):
    lr.check_diffusion_modes(wind_model)


def test_eigenmodes_of_the_rest_state_match_the_dense_oracle(arch, cpu):
    lr.check_eigenmodes_against(arch, _case(cpu, "e_0_"), "2-D bowl at rest", **DENSE)


def test_eigenmodes_after_five_steps_match_the_dense_oracle(arch, cpu, tmp_path):
    _, em = lr.check_eigenmodes_against(arch, _case(cpu, "e_5_"), "2-D bowl after 5 steps", **DENSE)
    lr.check_modes_io(em, lr.flat_model(arch, 0, **DENSE), tmp_path)


def test_implicit_step_algebra(arch):
    _, lin = lr.eigen_case(arch, 5, **DENSE)
    lr.check_step(lin, "2-D bowl after 5 steps")


def test_refusals(arch):
    lr.check_refusals(helpers.build_model("bowl_mixing", mesh=lr.FLAT, nsteps=1, arch=arch, **DENSE))
