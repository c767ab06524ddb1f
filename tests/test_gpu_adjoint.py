"""The adjoint of the linearised model on the GPU (libnupgcm_hip.so: k_tangent_adjoint_local + the engine's fixed-order gather through
both inverted indices): the checks of tests/test_adjoint.py through the device library behind the dense-inverse
preconditioner (the transposed inversion builds its own from A'), and in addition the device against the host library on the same tables
(bit for bit) and against the CPU() architecture's oracle and left modes (a child process: one process runs on one architecture).
Shapes of the adjoint load: 4 259 cells = 17 workgroups of 256 with a ragged last one and rows of unequal length in both inverted
indices (P2 and P1), non-zero Dirichlet values, the single tetrahedron, the x-periodic channel basin (rows that gather across the
seam), the embedded 2-D bowl.  The matrix of the transpose is not built here: checks D and F stand for it.

No test reads the reference tree or provokes an error on the device: the refusals fail on the host, in argument checks."""
import os
import subprocess
import sys

import numpy as np
import pytest

import nupgcm_amd as npg
from tests import adjoint_ref as ar
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
    out = str(tmp_path_factory.mktemp("adjoint") / "cpu.npz")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "adjoint_cpu_worker.py")
    subprocess.run([sys.executable, worker, out], check=True, timeout=600)
    z = np.load(out)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def evolved(arch, cpu):
    """the CPU() run's 2-D bowl after 5 steps behind this architecture's inversions, with the CPU() run's oracle"""
    ref = _case(cpu, "e_5_")
    return ar.based_on(lr.flat_model(arch, 0, **DENSE), ref["bb"], ref["xb"]), ref


@pytest.fixture(scope="module")
def left_modes(evolved):
    """check F after 5 steps, once: the left modes serve check G too"""
    lin, ref = evolved
    assert ref["asym"] > 1e-6
    return ar.check_left_modes_against(lin, ref, "2-D bowl after 5 steps")[1]


def _case(cpu, prefix):
    return {k[len(prefix):]: v for k, v in cpu.items() if k.startswith(prefix)}


def test_both_libraries_export_the_entry_point():
    ar.check_exports()


@pytest.mark.parametrize("b_order", [2, 1])
def test_adjoint_load_on_the_bowl(arch, mesh, b_order):
    m = itr.light_model(arch, mesh, b_order=b_order)
    assert m.fe_data.mesh.ncell == 4259                          # 17 workgroups of 256, a ragged last one
    ar.check_load(m, f"bowl P{b_order}", host=True)
    ar.check_load_identity(m, f"bowl P{b_order}")


def test_adjoint_load_with_dirichlet_values(arch, mesh):
    m = itr.light_model(arch, mesh, config="bowl_diri")
    assert (lr.engine(m)._keep["bd"] != 0.0).any()
    ar.check_load(m, "bowl_diri P2", host=True, N2=0.0)
    ar.check_load_identity(m, "bowl_diri P2", N2=0.0)


@pytest.mark.parametrize("b_order", [2, 1])
def test_adjoint_load_single_tetrahedron(arch, b_order):
    m = itr.light_model(arch, br.single_tet(arch).fe_data.mesh, b_order=b_order)
    assert m.fe_data.mesh.ncell == 1
    ar.check_load(m, f"single tetrahedron P{b_order}", host=True)
    ar.check_load_identity(m, f"single tetrahedron P{b_order}")


@pytest.mark.parametrize("b_order", [2, 1])
def test_adjoint_load_across_the_periodic_seam(arch, b_order):
    m, _ = br.channel_random(arch, b_order)
    ar.check_load(m, f"channel basin P{b_order}", host=True)
    ar.check_load_identity(m, f"channel basin P{b_order}")


def test_adjoint_load_embedded_2d(arch):
    m = lr.flat_model(arch, 0, **DENSE)
    ar.check_load(m, "embedded 2-D bowl", host=True)
    ar.check_load_identity(m, "embedded 2-D bowl")


def test_operator_dot_identity_after_three_steps(arch, cpu):
    ref = _case(cpu, "d_mixing_")
    model = helpers.build_model("bowl_mixing", nsteps=1, arch=arch, **DENSE)
    ar.check_operator_identity(ar.based_on(model, ref["bb"], ref["xb"]), "bowl_mixing after 3 steps")


def test_operator_dot_identity_under_wind(arch, cpu):
    ref = _case(cpu, "d_wind_")
    model = helpers.build_model("bowl_wind", nsteps=1, arch=arch, **DENSE)
    ar.check_operator_identity(ar.based_on(model, ref["bb"], ref["xb"]), "bowl_wind")


def test_operator_dot_identity_behind_node_records(arch, cpu):
    """Diagonal(1 / h^3) and an A stored by node records, as the large meshes have it: the transposed inversion assembles a plain A once
    more.  The solves stop at rtol = 1e-6 here; the allowance is built from their true residuals, whatever they are."""
    ref = _case(cpu, "d_mixing_")
    model = helpers.build_model("bowl_mixing", nsteps=1, arch=arch, block_nodes=True)
    assert model.inversion.solver.A.paired and isinstance(model.inversion.solver.P, npg.Diagonal)
    lin = ar.based_on(model, ref["bb"], ref["xb"], rtol=1e-6)
    ar.check_operator_identity(lin, "bowl_mixing after 3 steps, node records, Diagonal")
    assert lin.adj_solver.P is model.inversion.solver.P           # the diagonal preconditioner is symmetric: the same object serves


def test_operator_dot_identity_on_the_2d_bowl(evolved):
    ar.check_operator_identity(evolved[0], "2-D bowl after 5 steps")


def test_left_modes_of_the_rest_state_match_the_dense_oracle(arch, cpu):
    ref = _case(cpu, "e_0_")
    ar.check_left_modes_against(ar.based_on(lr.flat_model(arch, 0, **DENSE), ref["bb"], ref["xb"]), ref, "2-D bowl at rest")


def test_left_modes_after_five_steps_match_the_dense_oracle(left_modes, tmp_path):
    ar.check_modes_side_io(left_modes, tmp_path)


def test_mode_pairs(evolved, left_modes, tmp_path):
    """the pairs from the left modes of the test above and right modes computed here (LinearizedModel.mode_pairs computes both: on
    CPU(), tests/test_adjoint.py)"""
    lin, ref = evolved
    right = lin.eigenmodes(int(ref["n"]), lr.DT_EIG)
    ar.check_pairs(npg.ModePairs.from_modes(right, left_modes, lin.mass_matrix_native()), ref, "2-D bowl after 5 steps", tmp_path)


def test_adjoint_step_algebra(evolved):
    ar.check_adjoint_step(evolved[0], "2-D bowl after 5 steps")


def test_the_adjoint_is_built_on_first_use(arch):
    ar.check_lazy(lr.flat_model(arch, 5, **DENSE))


def test_adjoint_calls_are_passive(arch):
    ar.check_passive(arch, "2-D bowl", **DENSE)


def test_refusals(arch):
    ar.check_refusals(helpers.build_model("bowl_mixing", mesh=lr.FLAT, nsteps=1, arch=arch, **DENSE))


def test_a_multigrid_preconditioned_model_refuses_the_adjoint(arch):
    ar.check_multigrid_refuses(arch)
