"""CPU tests of tests/records_ref.py: the synthetic record-form matrices, the reference product and its row-wise bound."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import records_ref as R


@pytest.fixture(scope="module")
def cases():
    return list(R.cpu_cases(np.random.default_rng(11)))


def test_every_case_has_the_structure_block_nodes_accepts(cases):
    for name, c in cases:
        A = c["A"]
        assert A.has_sorted_indices and A.shape[0] == A.shape[1], name
        assert R.accepts(A, c["nfull"], c["nsurf"]), name
        q, cn, T = R.block_table(A, c["nfull"], c["nsurf"])
        assert np.array_equal(T[:, 0], T[:, 4]) and np.array_equal(T[:, 1], -T[:, 3]), name        # bitwise, not within rtol
        both = (q < c["nfull"]) & (cn < c["nfull"])
        assert np.array_equal(T[both, 0], T[both, 8]), name


def test_ghost_cases_keep_the_structure_in_the_owned_columns():
    for lone in (False, True):
        c = R.ghost_case(lone, "benign", np.random.default_rng(3))
        m = c["A"].shape[0]
        assert c["A"].shape[1] == m + int(c["ncomp"].sum()) + int(lone)
        assert R.accepts(c["A"][:, :m].tocsr(), c["nfull"], c["nsurf"])


def test_every_refused_perturbation_violates_the_rule():
    c = R.refusal_base(np.random.default_rng(5))
    assert R.accepts(c["A"], c["nfull"], c["nsurf"])
    for kind in R.PERTURBATIONS_REFUSED:
        B = R.perturb_entry(c["A"], kind, c["nfull"], c["nsurf"], c["q"], c["c"])
        assert not R.accepts(B, c["nfull"], c["nsurf"]), kind
        assert abs(B - c["A"]).nnz > 0 or B.nnz != c["A"].nnz
    B = R.perturb_entry(c["A"], "yy_within", c["nfull"], c["nsurf"], c["q"], c["c"])
    assert R.accepts(B, c["nfull"], c["nsurf"]) and (B != c["A"]).nnz == 1


def test_scipy_product_is_inside_the_row_bound(cases):
    """the bound is not so tight that a correct fp64 product fails it: scipy's own, and one summed in reverse order"""
    for name, c in cases:
        A, x = c["A"], c["x"]
        for xx in (x, x.astype(np.float32).astype(np.float64)):
            worst = R.check_rows(A @ xx, A, xx)
            assert worst <= 1.0, name
            B = sp.csr_matrix((A.data[::-1], A.shape[1] - 1 - A.indices[::-1], np.r_[0, np.cumsum(np.diff(A.indptr)[::-1])]), shape=A.shape)
            assert R.check_rows((B @ xx[::-1])[::-1], A, xx) <= 1.0, name
        y0 = np.cos(np.arange(A.shape[0]))
        R.check_rows(-0.5 * (A @ x) + 2.0 * y0, A, x, alpha=-0.5, beta=2.0, y0=y0)


def test_cancelling_values_cancel():
    c = R.edge_case(170, 87, 64, "cancelling", np.random.default_rng(2))
    A, x = c["A"], c["x"]
    y, s = A @ x, R.abs_product(A, x)
    nbr = 3 * c["nfull"] + 2 * c["nsurf"]
    Ab = A[:, :nbr] @ x[:nbr]
    sb = R.abs_product(A[:, :nbr].tocsr(), x[:nbr])
    assert np.sum(np.abs(Ab[:nbr]) < 1e-12 * sb[:nbr]) >= 20                     # rows whose block part sums to ~0
    assert np.abs(A.data[A.data != 0]).max() / np.abs(A.data[A.data != 0]).min() > 1e10
    q, cn, T = R.block_table(A, c["nfull"], c["nsurf"])
    assert np.sum((T[:, 0] == 0) & (T[:, 1] != 0)) > 10                          # records with K == 0, C != 0
    assert np.abs(x.astype(np.float32)).max() < 3e38 and len(y) == len(s)


def test_reference_detects_one_wrong_short_row():
    c = R.edge_case(170, 87, 64, "benign", np.random.default_rng(2))
    A, x = c["A"], c["x"]
    y = A @ x
    i = int(np.argmin(np.where(R.abs_product(A, x) > 0, np.abs(y), np.inf)))
    y[i] *= 1 + 1e-12
    assert np.linalg.norm(y - A @ x) / np.linalg.norm(y) < 1e-13                 # the norm-wise check does not see it
    with pytest.raises(AssertionError):
        R.check_rows(y, A, x)


def test_expected_counts_on_hand_written_matrices():
    # one full node 0, one surface node 1, two rows behind: [x0 y0 z0 | x1 y1 | p0 p1]
    K, C_, k2, c2 = 2.0, 0.5, 3.0, 0.25
    rows = {0: {0: K, 1: C_, 3: k2, 4: c2, 5: 1.0}, 1: {0: -C_, 1: K, 3: -c2, 4: k2, 5: 1.0}, 2: {2: K, 5: 1.0},
            3: {3: 7.0, 4: 0.0, 6: 1.0}, 4: {3: 0.0, 4: 7.0},
            5: {0: 1.0, 2: 1.0, 3: 1.0}, 6: {6: 4.0}}
    A = sp.lil_matrix((7, 7))
    r, c, v = zip(*[(i, j, val) for i, row in rows.items() for j, val in row.items()])
    A = R._csr(r, c, v, (7, 7))
    assert R.accepts(A, 1, 1)
    # node records: (0,0) (0,1) (1,1) = 3; column records: (node 0, p0) [3 entries], (node 1, p1) [1 entry]: 2 records, 4 entries:
    # 56 bytes > 48 -> not used, the 4 entries stay CSR; coupling records: row p0 -> nodes 0 and 1 = 2; left: p1-p1
    assert R.expected_counts(A, 1, 1) == dict(nodes=2, records=3, coupling_records=2, csr_entries=5, column_records=False, coupling=True)
    assert R.expected_counts(A, 1, 1, coupling=False)["csr_entries"] == 8
    # two full nodes, one column behind, both with all three gradient entries: 2 column records for 6 entries (56 <= 72 bytes)
    rows = {0: {0: K, 1: C_, 3: k2, 4: c2, 6: 1.0}, 1: {0: -C_, 1: K, 3: -c2, 4: k2, 6: 1.0}, 2: {2: K, 5: k2, 6: 1.0},
            3: {3: K, 4: C_, 6: 2.0}, 4: {3: -C_, 4: K, 6: 2.0}, 5: {5: K, 6: 2.0}, 6: {}}
    r, c, v = zip(*[(i, j, val) for i, row in rows.items() for j, val in row.items()])
    A = R._csr(r, c, v, (7, 7))
    assert R.accepts(A, 2, 0)
    assert R.expected_counts(A, 2, 0) == dict(nodes=2, records=3, coupling_records=2, csr_entries=0, column_records=True, coupling=False)
    assert R.expected_counts(A, 2, 0, column_records=False) == dict(nodes=2, records=3, coupling_records=0, csr_entries=6,
                                                                   column_records=False, coupling=False)


def test_scramble_is_a_symmetric_permutation():
    c = R.edge_case(17, 9, 8, "benign", np.random.default_rng(1))
    B, node, comp, perm = R.scramble_dofs(c["A"], c["nfull"], c["nsurf"])
    assert sorted(perm) == list(range(c["A"].shape[0])) and (node >= 0).sum() == 3 * 17 + 2 * 9
    assert np.array_equal(B.toarray(), c["A"].toarray()[np.ix_(perm, perm)])
    assert np.array_equal(comp[:5], [0, 0, 0, 0, 0]) and node[3] == -1            # component-major, others interleaved
    x = c["x"]
    assert np.allclose(B @ x[perm], (c["A"] @ x)[perm], rtol=1e-12, atol=1e-9)


def test_full9_has_absent_pairs_and_no_kc_structure():
    rng = np.random.default_rng(4)
    c = R.edge_case(40, 25, 12, "benign", rng)
    nn = 65
    A9 = R.make_full9(40, 25, 12, R.edge_graph(nn), [[(q % 12, R._comps(q, 40))] for q in range(nn)], [[(r, R.ALL3)] for r in range(12)],
                      None, rng)
    assert not R.accepts(A9, 40, 25) and c["A"].shape == A9.shape
    q, cn, T = R.block_table(A9, 40, 25)
    assert np.isnan(T[:, [0, 1, 3, 4]]).any() and not np.isnan(T[q == cn][:, [0, 4]]).any()
