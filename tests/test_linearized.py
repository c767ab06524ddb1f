"""The linearised model (nupgcm_amd.linearized) on the CPU() architecture - libnupgcm_host.so runs the arithmetic of the
device kernel (csrc/tangent_core.h), the inversions are sparse LU: the tangent load against the numpy restatement of
tests/linearized_ref.py, the operator against the central difference of the tendency the model already had, linearity under
atol = 0, passivity, the eigen-solver against scipy's eigsh and a dense eig, the algebra of the implicit step, refusals.  No GPU.

Figures are printed before they are asserted; the measured worst ratios are in DESIGN.md 33."""
import pytest

import nupgcm_amd as npg
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
    """the embedded 2-D bowl after 5 steps of bowl_mixing, with its linearisation, its dense oracle and its modes"""
    worst, em, ref = lr.check_eigenmodes(arch, 5, "2-D bowl after 5 steps")
    return worst, em, ref


def test_both_libraries_export_the_entry_point():
    lr.check_exports()


@pytest.mark.parametrize("b_order", [2, 1])
def test_tangent_load_on_the_bowl(arch, mesh, b_order):
    m = itr.light_model(arch, mesh, b_order=b_order)
    assert m.fe_data.mesh.ncell == 4259                          # 17 workgroups of 256 on the device, a ragged last one
    lr.check_load(m, f"bowl P{b_order}")


def test_tangent_load_with_dirichlet_values(arch, mesh):
    m = itr.light_model(arch, mesh, config="bowl_diri")
    lr.check_load(m, "bowl_diri P2", N2=0.0)
    lr.check_dirichlet(m, itr.light_model(arch, mesh, config="bowl_diri", b_diri_vals=0.0), "bowl_diri P2")


@pytest.mark.parametrize("b_order", [2, 1])
def test_tangent_load_single_tetrahedron(arch, b_order):
    m = itr.light_model(arch, br.single_tet(arch).fe_data.mesh, b_order=b_order)
    assert m.fe_data.mesh.ncell == 1
    lr.check_load(m, f"single tetrahedron P{b_order}")


@pytest.mark.parametrize("b_order", [2, 1])
def test_tangent_load_across_the_periodic_seam(arch, b_order):
    m, _ = br.channel_random(arch, b_order)
    lr.check_load(m, f"channel basin P{b_order}")


def test_tangent_load_embedded_2d(arch):
    lr.check_load(lr.flat_model(arch, 0), "embedded 2-D bowl")


def test_apply_is_the_derivative_of_the_tendency_after_three_steps(arch):
    lr.check_derivative(arch, "bowl_mixing", 3, "bowl_mixing after 3 steps")


def test_apply_is_the_derivative_of_the_tendency_under_wind(arch):
    lr.check_derivative(arch, "bowl_wind", 0, "bowl_wind")


def test_apply_is_linear_for_tiny_perturbations(arch):
    lr.check_linearity(lr.flat_model(arch, 5), "2-D bowl")


def test_linearisation_is_passive(arch):
    lr.check_passive(arch, "2-D bowl")


def test_diffusion_modes_match_eigsh(arch):
    lr.check_diffusion_modes(helpers.build_model("bowl_wind", nsteps=1, arch=arch))


def test_eigenmodes_of_the_rest_state_match_the_dense_oracle(arch):
    lr.check_eigenmodes(arch, 0, "2-D bowl at rest")


def test_eigenmodes_after_five_steps_match_the_dense_oracle(evolved):
    assert evolved[0] <= 1.0


def test_modes_save_load_and_as_b(arch, evolved, tmp_path):
    lr.check_modes_io(evolved[1], lr.flat_model(arch, 0), tmp_path)


def test_implicit_step_algebra(arch):
    _, lin = lr.eigen_case(arch, 5)
    lr.check_step(lin, "2-D bowl after 5 steps")


def test_refusals(arch):
    lr.check_refusals(helpers.build_model("bowl_mixing", mesh=lr.FLAT, nsteps=1, arch=arch))
