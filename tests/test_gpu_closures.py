"""The derivatives of the convection and eddy closures on the GPU (libnupgcm_hip.so: k_tangent_diffusion_local, k_tangent_eddy_local,
k_tangent_eddy_adjoint_local + the engine's fixed-order gathers): the loads of tests/test_closures.py through the device
library, against the extended-precision restatements and against the host library on the same tables (bit for bit); the tangent
operator and its adjoint behind the dense-inverse preconditioner against the CPU() architecture's results on the same base state (a
child process: one process runs on one architecture), the operator's dot identity, one small eigenproblem, passivity and refusals.
Shapes of the loads: 4 259 cells = 17 workgroups of 256 with a ragged last one (P2 and P1), non-zero Dirichlet values, the single
tetrahedron, the x-periodic channel basin (rows that gather across the seam), the embedded 2-D bowl; both stress forms.

No test reads the reference tree or provokes an error on the device: the refusals fail on the host, in argument checks."""
import os
import subprocess
import sys

import numpy as np
import pytest

import nupgcm_amd as npg
from tests import boundary_ref as br
from tests import closures_ref as cr
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
    out = str(tmp_path_factory.mktemp("closures") / "cpu.npz")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "closures_cpu_worker.py")
    subprocess.run([sys.executable, worker, out], check=True, timeout=600)
    z = np.load(out)
    return {k: z[k] for k in z.files}


def _case(cpu, prefix):
    return {k[len(prefix):]: v for k, v in cpu.items() if k.startswith(prefix)}


@pytest.fixture(scope="module")
def both(arch, cpu):
    """check F: the golden bowl with both closures on, linearised about the CPU() run's base state behind the dense inverse"""
    model = cr.closure_model(arch, True, True, run=False, **DENSE)
    return cr.check_against(model, _case(cpu, "f_"), "both closures, golden bowl after 2 steps")[0]


def test_both_libraries_export_the_entry_points():
    cr.check_exports()


@pytest.mark.parametrize("b_order", [2, 1])
def test_loads_on_the_bowl(arch, mesh, b_order):
    m = itr.light_model(arch, mesh, b_order=b_order)
    assert m.fe_data.mesh.ncell == 4259                          # 17 workgroups of 256, a ragged last one
    cr.check_loads(m, f"bowl P{b_order}", host=True)


def test_loads_with_dirichlet_values(arch, mesh):
    m = itr.light_model(arch, mesh, config="bowl_diri")
    assert (lr.engine(m)._keep["bd"] != 0.0).any()
    cr.check_loads(m, "bowl_diri P2", host=True, N2=0.0)


@pytest.mark.parametrize("b_order", [2, 1])
def test_loads_single_tetrahedron(arch, b_order):
    m = itr.light_model(arch, br.single_tet(arch).fe_data.mesh, b_order=b_order)
    assert m.fe_data.mesh.ncell == 1
    cr.check_loads(m, f"single tetrahedron P{b_order}", host=True)


def test_loads_across_the_periodic_seam(arch):
    m, _ = br.channel_random(arch, 2)
    cr.check_loads(m, "channel basin P2", host=True)


def test_loads_embedded_2d(arch):
    cr.check_loads(lr.flat_model(arch, 0, **DENSE), "embedded 2-D bowl", host=True)


def test_get_coeff_reads_back_what_was_set(arch, mesh):
    cr.check_get_coeff(itr.light_model(arch, mesh))


def test_apply_and_adjoint_match_the_cpu_architecture(both):
    assert both.closures == "tangent" and both.n_inversions > 1


def test_operator_dot_identity(both):
    cr.check_operator_identity(both, "both closures, golden bowl after 2 steps")


def test_eigenmodes_on_the_2d_bowl(arch, cpu):
    cr.check_eigenmodes_against(cr.flat_closure_model(arch, 0, **DENSE), _case(cpu, "g_"), "2-D bowl, both closures, after 5 steps")


def test_linearisation_is_passive(arch):
    cr.check_passive(arch, "2-D bowl", **DENSE)


def test_refusals(arch, mesh):
    cr.check_refusals(cr.closure_model(arch, True, True, mesh=lr.FLAT, nsteps=1, run=False, **DENSE))
    cr.check_unset_tables_refuse(itr.light_model(arch, mesh))


def test_vectors_of_another_context_are_refused(arch):
    cr.check_contexts_refuse(cr.closure_model(arch, True, True, mesh=lr.FLAT, nsteps=1, run=False, **DENSE))
