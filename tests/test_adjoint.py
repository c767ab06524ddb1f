"""The adjoint of the linearised model (nupgcm_amd.linearized) on the CPU() architecture - libnupgcm_host.so runs the
arithmetic of the device kernel (csrc/tangent_adjoint_core.h), the inversions and their transposes are sparse LU: the adjoint load
against the numpy restatement of tests/adjoint_ref.py and against the tangent load through the dot identity, the operator's dot
identity with its derived allowance, the whole transpose on the 2-D bowl, left modes against scipy's dense eig, ModePairs, the adjoint
step, passivity and refusals.  No GPU.

Figures are printed before they are asserted; the measured worst ratios are in DESIGN.md 34."""
import pytest

import nupgcm_amd as npg
from tests import adjoint_ref as ar
from tests import boundary_ref as br
from tests import helpers
from tests import interior_ref as itr
from tests import linearized_ref as lr


@pytest.fixture(scope="module")
def arch():
    return npg.CPU()


@pytest.fixture(scope="module")
def mesh():
    return itr.bowl_mesh()


@pytest.fixture(scope="module")
def evolved(arch):
    """the embedded 2-D bowl after 5 steps of bowl_mixing: its linearisation and its dense oracle with both sets of vectors"""
    model, lin = lr.eigen_case(arch, 5)
    return model, lin, ar.oracle_pairs(lin, lr.DT_EIG)


def _load_cases(arch, mesh):
    yield "bowl P2", itr.light_model(arch, mesh, b_order=2), 0.7
    yield "bowl P1", itr.light_model(arch, mesh, b_order=1), 0.7
    yield "bowl_diri P2", itr.light_model(arch, mesh, config="bowl_diri"), 0.0
    for b_order in (2, 1):
        yield f"single tetrahedron P{b_order}", itr.light_model(arch, br.single_tet(arch).fe_data.mesh, b_order=b_order), 0.7
        yield f"channel basin P{b_order}", br.channel_random(arch, b_order)[0], 0.7
    yield "embedded 2-D bowl", lr.flat_model(arch, 0), 0.7


def test_both_libraries_export_the_entry_point():
    ar.check_exports()


@pytest.mark.parametrize("b_order", [2, 1])
def test_adjoint_load_on_the_bowl(arch, mesh, b_order):
    m = itr.light_model(arch, mesh, b_order=b_order)
    assert m.fe_data.mesh.ncell == 4259                          # 17 workgroups of 256 on the device, a ragged last one
    ar.check_load(m, f"bowl P{b_order}")


def test_adjoint_load_with_dirichlet_values(arch, mesh):
    m = itr.light_model(arch, mesh, config="bowl_diri")
    assert (lr.engine(m)._keep["bd"] != 0.0).any()
    ar.check_load(m, "bowl_diri P2", N2=0.0)


@pytest.mark.parametrize("b_order", [2, 1])
def test_adjoint_load_single_tetrahedron(arch, b_order):
    m = itr.light_model(arch, br.single_tet(arch).fe_data.mesh, b_order=b_order)
    assert m.fe_data.mesh.ncell == 1
    ar.check_load(m, f"single tetrahedron P{b_order}")


@pytest.mark.parametrize("b_order", [2, 1])
def test_adjoint_load_across_the_periodic_seam(arch, b_order):
    m, _ = br.channel_random(arch, b_order)
    ar.check_load(m, f"channel basin P{b_order}")


def test_adjoint_load_embedded_2d(arch):
    ar.check_load(lr.flat_model(arch, 0), "embedded 2-D bowl")


def test_load_dot_identity_ties_the_adjoint_to_the_tangent(arch, mesh):
    worst = max(ar.check_load_identity(m, label, N2=N2) for label, m, N2 in _load_cases(arch, mesh))
    print(f"adjoint: worst ratio of the load's dot identity {worst:.3e}")


def test_operator_dot_identity_after_three_steps(arch):
    model, _, _, _ = lr.derivative_case(arch, "bowl_mixing", 3)
    ar.check_operator_identity(npg.LinearizedModel(model), "bowl_mixing after 3 steps")


def test_operator_dot_identity_under_wind(arch):
    model, _, _, _ = lr.derivative_case(arch, "bowl_wind", 0)
    ar.check_operator_identity(npg.LinearizedModel(model), "bowl_wind")


def test_the_whole_transpose_on_the_2d_bowl(evolved):
    _, lin, ref = evolved
    _, asym = ar.check_whole_transpose(lin, ref["J"], "2-D bowl after 5 steps")
    assert asym > 1e-6                                           # J is not symmetric: a symmetric shortcut cannot pass


def test_left_modes_of_the_rest_state_equal_the_right_ones(arch):
    _, lin = lr.eigen_case(arch, 0)
    ar.check_left_equals_right(lin, ar.oracle_pairs(lin, lr.DT_EIG), "2-D bowl at rest")


def test_left_modes_after_five_steps_match_the_dense_oracle(evolved, tmp_path):
    _, lin, ref = evolved
    assert ref["asym"] > 1e-6
    _, em = ar.check_left_modes(lin, ref, "2-D bowl after 5 steps")
    ar.check_modes_side_io(em, tmp_path)


def test_mode_pairs(evolved, tmp_path):
    _, lin, ref = evolved
    ar.check_pairs(lin.mode_pairs(int(ref["n"]), lr.DT_EIG), ref, "2-D bowl after 5 steps", tmp_path)


def test_adjoint_step_algebra(evolved):
    ar.check_adjoint_step(evolved[1], "2-D bowl after 5 steps")


def test_the_adjoint_is_built_on_first_use(arch):
    ar.check_lazy(lr.flat_model(arch, 5))


def test_adjoint_calls_are_passive(arch):
    ar.check_passive(arch, "2-D bowl")


def test_refusals(arch):
    ar.check_refusals(helpers.build_model("bowl_mixing", mesh=lr.FLAT, nsteps=1, arch=arch))
