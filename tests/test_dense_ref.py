"""CPU guard of tests/dense_ref.py: the input generator, the extended-precision reference and the derived bounds, checked against
a numpy emulation of the fp32 and the scaled-fp16 storage at every size of the GPU test - so a bound that is wrong, or a matrix
on which the library would fall back from fp16 to fp32, shows without a GPU."""
import numpy as np
import pytest

from tests import dense_ref as dr


@pytest.mark.parametrize("n", dr.SIZES)
def test_emulated_storage_is_inside_the_bounds(n):
    c = dr.case(n)
    assert c.cond < 25.0
    assert c.R.shape[1] == 1 + len(dr.unit_columns(n)) and np.array_equal(np.argmax(c.R[:, 1:], axis=0), dr.unit_columns(n))
    assert dr.worst_ratio(c.Zref, c.Zref, c.bound32) == 0.0
    P = dr.probe_vectors(n)
    Y16 = dr.emulate_fp16(c.inv, np.hstack([c.R, P]))
    r32 = dr.worst_ratio(dr.emulate_fp32(c.inv, c.R), c.Zref, c.bound32)
    r16 = dr.worst_ratio(Y16[:, :c.R.shape[1]], c.Zref, c.bound16)
    print(f"n = {n}: cond {c.cond:.1f}, e_np {c.e_np:.2e}, error / bound: fp32 {r32:.3f}, fp16 {r16:.3f}")
    assert r32 <= 1.0 and r16 <= 1.0, (r32, r16)
    # the library's acceptance check keeps fp16 on these matrices
    for med, p99 in dr.acceptance_statistics(c.inv @ P, Y16[:, c.R.shape[1]:]):
        assert med <= 5e-3 and p99 <= 0.2, (med, p99)
    # a dropped column with r_j = O(1) is far outside either bound
    j = int(np.argmax(np.abs(c.R[:, 0]) * c.cs))
    Zd = (c.inv @ c.R[:, :1]) - c.inv[:, j:j + 1] * c.R[j, 0]
    assert dr.worst_ratio(Zd, c.Zref[:, :1], c.bound16[:, :1]) > 100.0


def test_the_bounds_are_tight():
    """halving either bound fails the emulation at the worst size: the bounds carry no slack to hide a kernel error in"""
    worst32 = worst16 = 0.0
    for n in (255, 513):
        c = dr.case(n)
        worst32 = max(worst32, dr.worst_ratio(dr.emulate_fp32(c.inv, c.R), c.Zref, c.bound32))
        worst16 = max(worst16, dr.worst_ratio(dr.emulate_fp16(c.inv, c.R), c.Zref, c.bound16))
    assert 0.5 < worst32 <= 1.0 and 0.5 < worst16 <= 1.0, (worst32, worst16)
