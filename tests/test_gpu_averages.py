"""Time means and eddy co-moments on the GPU (libnupgcm_hip.so: k_tavg_comoments / k_tavg_means): the restatement, the
bounds and the cases of tests/test_averages.py through the device library, and in addition the device against the host library on the
same node table and samples - every entry identical (the kernels have only IEEE add, subtract and multiply in a fixed association).
The node counts cover several workgroups with a ragged last one (the bowl's P2 nodes), exactly 0, 1, 63, 64, 65, 255, 256, 257 nodes
through the mask, ten nodes (the single tetrahedron), the periodic seam of the channel basin and the embedded 2-D mesh, P2 and P1."""
import numpy as np
import pytest

import nupgcm_amd as npg
from tests import averages_ref as ar
from tests import boundary_ref as br
from tests import integrals_ref as ir
from tests import sampling_ref as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def arch():
    return npg.GPU()


@pytest.fixture(scope="module")
def bowl(arch):
    return ar.bowl_light(arch)


def test_exports():
    ar.check_exports()


def test_bits_on_the_bowl(bowl):
    nn = bowl.fe_data.mesh.nn
    assert nn > 2 * 256 and nn % 256 != 0                                                  # several workgroups, a ragged last one
    ar.check_bits(bowl, "bowl h = 0.1", against_host=True)


@pytest.mark.parametrize("n", ar.EDGE_COUNTS)
def test_bits_through_the_mask(bowl, n):
    mask = ar.masks(bowl.fe_data.mesh.nn)[n]
    assert mask.sum() == n
    ar.check_bits(bowl, f"mask of {n} nodes", mask, against_host=n in (0, 65, 257))


def test_single_tetrahedron(arch):
    tet = br.single_tet(arch)
    assert tet.fe_data.mesh.nn == 10
    ar.check_bits(tet, "single tetrahedron", against_host=True)
    ar.check_bits(br.bare_model(arch, tet.fe_data.mesh, b_order=1), "single tetrahedron P1", against_host=True)


@pytest.mark.parametrize("b_order", [2, 1])
def test_dirichlet_buoyancy(arch, b_order):
    ar.check_dirichlet(ar.bowl_light(arch, "bowl_wind", b_order), f"bowl_wind P{b_order}")
    if b_order == 1:
        ar.check_bits(ar.bowl_light(arch, "bowl_wind", b_order), f"bowl_wind P{b_order}", against_host=True)


@pytest.mark.parametrize("b_order", [2, 1])
def test_channel_basin(arch, b_order):
    model = sr.channel_model(arch, b_order)
    assert model.fe_data.mesh.periodic and model.averages is None
    ar.check_bits(model, f"channel basin P{b_order}", against_host=True)


def test_embedded_2d(arch):
    model = ar.bowl2d_light(arch)
    assert model.fe_data.mesh.dim == 2
    ar.check_bits(model, "bowl 2-D", against_host=True)


@pytest.mark.parametrize("offset", [0.0, 1.0])
def test_accuracy_of_the_recurrence(bowl, offset):
    ar.check_accuracy(bowl, "anomalies of order one" if offset == 0.0 else "anomalies 1e-6 of the mean", offset)


def test_phases(bowl):
    ar.check_phases(bowl, "bowl h = 0.1")


def test_every_and_means_only(bowl):
    ar.check_every(bowl)


def test_applied(arch):
    ar.check_applied(ir.bare_model(arch))


def test_run(arch, tmp_path):
    ar.check_run(arch, tmp_path)


def test_refusals(bowl):
    ar.check_refusals(bowl)
