"""The derivatives of the convection and eddy closures in the linearised model (nupgcm_amd.linearized closures=) on the
CPU() architecture - libnupgcm_host.so runs the arithmetic of the device kernels (csrc/tangent_closures_core.h), the inversions are
sparse LU: the three loads against the extended-precision restatements of tests/closures_ref.py and their dot identities, the tangent
operator against Richardson's value of central differences of the nonlinear code that existed before it, the operator's dot identity,
one small eigenproblem, passivity and refusals.  No GPU.

Figures are printed before they are asserted; the measured worst ratios are in DESIGN.md 35."""
import pytest

import nupgcm_amd as npg
from tests import boundary_ref as br
from tests import closures_ref as cr
from tests import interior_ref as itr
from tests import linearized_ref as lr


@pytest.fixture(scope="module")
def arch():
    return npg.CPU()


@pytest.fixture(scope="module")
def mesh():
    return itr.bowl_mesh()


@pytest.fixture(scope="module")
def both(arch):
    """golden bowl, bowl_mixing after two BDF1 steps with both closures on: check D's model and its two linearisations"""
    return cr.check_derivative(arch, True, True, "both closures")


def test_both_libraries_export_the_entry_points():
    cr.check_exports()


@pytest.mark.parametrize("b_order", [2, 1])
def test_loads_on_the_bowl(arch, mesh, b_order):
    m = itr.light_model(arch, mesh, b_order=b_order)
    assert m.fe_data.mesh.ncell == 4259                          # 17 workgroups of 256 on the device, a ragged last one
    cr.check_loads(m, f"bowl P{b_order}")


def test_loads_with_dirichlet_values(arch, mesh):
    m = itr.light_model(arch, mesh, config="bowl_diri")
    assert (lr.engine(m)._keep["bd"] != 0.0).any()
    cr.check_loads(m, "bowl_diri P2", N2=0.0)


@pytest.mark.parametrize("b_order", [2, 1])
def test_loads_single_tetrahedron(arch, b_order):
    m = itr.light_model(arch, br.single_tet(arch).fe_data.mesh, b_order=b_order)
    assert m.fe_data.mesh.ncell == 1
    cr.check_loads(m, f"single tetrahedron P{b_order}")


def test_loads_across_the_periodic_seam(arch):
    m, _ = br.channel_random(arch, 2)
    cr.check_loads(m, "channel basin P2")


def test_loads_embedded_2d(arch):
    cr.check_loads(lr.flat_model(arch, 0), "embedded 2-D bowl")


def test_get_coeff_reads_back_what_was_set(arch, mesh):
    cr.check_get_coeff(itr.light_model(arch, mesh))


def test_tangent_is_the_derivative_with_convection(arch):
    cr.check_derivative(arch, True, False, "convection alone")


def test_tangent_is_the_derivative_with_the_eddy_closure(arch):
    cr.check_derivative(arch, False, True, "eddy alone")


def test_tangent_is_the_derivative_with_both(both):
    assert both[1].closures == "tangent" and both[2].closures == "frozen"


def test_operator_dot_identity(both):
    cr.check_operator_identity(both[1], "both closures, golden bowl after 2 steps")


def test_operator_dot_identity_frozen(both):
    cr.check_operator_identity(both[2], "both closures frozen, golden bowl after 2 steps")


def test_eigenmodes_on_the_2d_bowl(arch):
    cr.check_eigenmodes(arch, "2-D bowl, both closures, after 5 steps")


def test_step_and_pairs_work_on_top(arch):
    lin = npg.LinearizedModel(cr.flat_closure_model(arch), closures="tangent")
    lr.check_step(lin, "2-D bowl, both closures")
    mp = lin.mode_pairs(1, lr.DT_EIG)
    print(f"closures 2-D bowl: mode pair sigma {mp.sigma}, left {mp.sigma_left}, condition {mp.condition}")
    assert abs(mp.sigma[0] - mp.sigma_left[0]) <= 1e-6 * abs(mp.sigma[0])


def test_linearisation_is_passive(arch):
    cr.check_passive(arch, "2-D bowl")


def test_refusals(arch, mesh):
    cr.check_refusals(cr.closure_model(arch, True, True, mesh=lr.FLAT, nsteps=1, run=False))
    cr.check_unset_tables_refuse(itr.light_model(arch, mesh))
