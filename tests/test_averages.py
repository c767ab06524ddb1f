"""Time means and eddy co-moments (nupgcm_amd.averages) on the CPU() architecture - libnupgcm_host.so runs the same
per-node and per-entry arithmetic as the device kernels (csrc/tavg_core.h) - against the restatement of tests/averages_ref.py.  No GPU.

The means and the ten co-moments must be the numpy fp64 recurrence's to the bit; the recurrence is checked against a longdouble two-pass
result within each entry's own bound.  Measured on the host library, n = 50 (worst |err| / bound): anomalies of order one - means
0.010, co-moments 0.014; anomalies 1e-6 of the mean - means 0.068, co-moments 0.013; four merged bins of 16 samples - means 0.036,
co-moments 0.023.  The device gives the same figures: its entries are the host library's."""
import numpy as np
import pytest

import nupgcm_amd as npg
from tests import averages_ref as ar
from tests import boundary_ref as br
from tests import integrals_ref as ir
from tests import sampling_ref as sr


@pytest.fixture(scope="module")
def arch():
    return npg.CPU()


@pytest.fixture(scope="module")
def bowl(arch):
    return ar.bowl_light(arch)


def test_exports():
    ar.check_exports()


def test_bits_on_the_bowl(bowl):
    nn = bowl.fe_data.mesh.nn
    assert nn > 2 * 256 and nn % 256 != 0                                                  # several workgroups, a ragged last one
    ar.check_bits(bowl, "bowl h = 0.1")


@pytest.mark.parametrize("n", ar.EDGE_COUNTS)
def test_bits_through_the_mask(bowl, n):
    mask = ar.masks(bowl.fe_data.mesh.nn)[n]
    assert mask.sum() == n
    ar.check_bits(bowl, f"mask of {n} nodes", mask)


def test_single_tetrahedron(arch):
    tet = br.single_tet(arch)
    assert tet.fe_data.mesh.nn == 10
    ar.check_bits(tet, "single tetrahedron")
    ar.check_bits(br.bare_model(arch, tet.fe_data.mesh, b_order=1), "single tetrahedron P1")


@pytest.mark.parametrize("b_order", [2, 1])
def test_dirichlet_buoyancy(arch, b_order):
    ar.check_dirichlet(ar.bowl_light(arch, "bowl_wind", b_order), f"bowl_wind P{b_order}")


@pytest.mark.parametrize("b_order", [2, 1])
def test_channel_basin(arch, b_order):
    model = sr.channel_model(arch, b_order)
    assert model.fe_data.mesh.periodic and model.averages is None
    ar.check_bits(model, f"channel basin P{b_order}")


def test_embedded_2d(arch):
    model = ar.bowl2d_light(arch)
    assert model.fe_data.mesh.dim == 2
    ar.check_bits(model, "bowl 2-D")


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
