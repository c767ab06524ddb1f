"""Record and windowed sparse storage (csrc/csr.hip, spmv_device.h, spmv_window.h) on synthetic adversarial matrices.

Every product is compared ROW BY ROW with a long-double reference (tests/records_ref.py): |y_i - ref_i| <= (rowlen_i + 3) 2^-53
(|A||x|)_i, the bound of an fp64 sum of fp64 products in any order; rows without contributions must be exactly zero.  Every counter
is compared for equality with a count made from the scipy matrix.  All matrices are valid; every refusal is a documented one."""
import re

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

import nupgcm_amd as npg  # noqa: E402
from nupgcm_amd import _lib as L  # noqa: E402
from tests import records_ref as R  # noqa: E402

KNOBS = ("NPG_SPMV_COUPLING", "NPG_SPMV_COLUMN_RECORDS", "NPG_SPMV_WINDOW", "NPG_SPMV_WLANES", "NPG_SPMV_LANES", "NPG_WIN_SCALE",
         "NPG_WIN_BYTES", "NPG_WIN_ORDER", "NPG_WIN_ROWS", "NPG_WIN_DIAG", "NPG_WIN_UNCACHED")


@pytest.fixture(scope="module")
def arch():
    a = npg.GPU()
    a.ctx
    return a


@pytest.fixture(scope="module")
def wg_limit(arch):
    """workgroups of the gather-layout SpMV launch: min(tiles, 3 x the device's CUs) (launch_spmv_g32, csr.hip)"""
    return 3 * int(re.search(r"(\d+) CUs", arch.ctx.name()).group(1))


@pytest.fixture(autouse=True)
def clean_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def bit_equal(M, A):
    B = M.to_scipy_csr()
    return (np.array_equal(B.indptr, A.indptr) and np.array_equal(B.indices, A.indices) and
            np.array_equal(B.data.view(np.int64), A.data.view(np.int64)))


class Checks:
    """the references of one case, computed once: x as it is (npg_spmv) and rounded to fp32 (npg_spmv_gather32)"""

    def __init__(self, A, x, extra=None):
        self.A, self.x = A, x
        self.full = R.RowCheck(A, x)
        self.f32 = R.RowCheck(A, x.astype(np.float32).astype(np.float64))
        self.y0 = np.cos(np.arange(A.shape[0], dtype=float)) * 1e3
        self.extra = extra

    def products(self, arch, M, window, tag, gather=True):
        dx = npg.on_architecture(arch, self.x)
        self.full.check(M.mul(dx).to_host(), extra=self.extra, what=f"{tag} mul")
        dy = npg.on_architecture(arch, self.y0)
        M.mul(dx, dy, -0.75, 2.5)
        self.full.check(dy.to_host(), alpha=-0.75, beta=2.5, y0=self.y0, extra=None if self.extra is None else 0.75 * self.extra,
                        what=f"{tag} mul alpha beta")
        if not gather:
            return
        self.f32.check(M.mul_gather32(dx, windowed=False).to_host(), extra=self.extra, what=f"{tag} gather32 ordinary tiles")
        if window:
            self.f32.check(M.mul_gather32(dx, windowed=True).to_host(), extra=self.extra, what=f"{tag} gather32 windowed tiles")
        else:
            with pytest.raises(L.DeviceError):
                M.mul_gather32(dx, windowed=True)


def blocked(arch, c, monkeypatch, env=(), ghosts=True):
    for k, v in env:
        monkeypatch.setenv(k, v)
    try:
        M = npg.on_architecture(arch, c["A"])
        if ghosts and "first_col" in c:
            M.set_ghost_nodes(c["first_col"], c["ncomp"])
        ok = M.block_nodes(c["nfull"], c["nsurf"])
    finally:
        for k, v in env:
            monkeypatch.delenv(k)
    return M, ok


PLAIN = (("NPG_SPMV_COUPLING", "0"), ("NPG_SPMV_COLUMN_RECORDS", "0"))


def assert_counts(M, A, c, **kw):
    e = R.expected_counts(A, c["nfull"], c["nsurf"], **kw)
    assert M.storage() == (e["nodes"], e["records"], e["csr_entries"])
    assert M.coupling_records() == e["coupling_records"]
    return e


def run_case(arch, c, monkeypatch, want_window=None, extra=None, env=(), chk=None):
    """The four steps of every case: conversion, counters (equalities), the four products, and the products again for set_lanes in
    {4, 8, 16, 32} x NPG_SPMV_WLANES in {4, 8}; on the record form with all records and on the one built with NPG_SPMV_COUPLING=0
    and NPG_SPMV_COLUMN_RECORDS=0.  `env`: knobs set for every conversion.  Returns the window_info of the first handle."""
    A = c["A"]
    chk = chk or Checks(A, c["x"], extra)
    M, ok = blocked(arch, c, monkeypatch, env)
    assert ok
    e = assert_counts(M, A, c)
    info = M.window_info()
    window = info["tiles"] > 0
    if want_window is not None:
        assert window == want_window
    else:
        assert window == e["column_records"]          # a windowed set whenever the block rows are all records (and no cap is hit)
    chk.products(arch, M, window, "records")
    for wl in ("4", "8"):
        Mw, ok = blocked(arch, c, monkeypatch, env + (("NPG_SPMV_WLANES", wl),))
        assert ok and Mw.window_info() == info
        for lanes in (4, 8, 16, 32):
            Mw.set_lanes(lanes)
            chk.products(arch, Mw, window, f"wlanes {wl} lanes {lanes}")
    M0, ok = blocked(arch, c, monkeypatch, env + PLAIN)
    assert ok and M0.window_info()["tiles"] == 0
    assert_counts(M0, A, c, coupling=False, column_records=False)
    for lanes in (0, 4, 8, 16, 32):
        M0.set_lanes(lanes)
        chk.products(arch, M0, False, f"csr remainder, lanes {lanes}")
    return info


def rows_windowed(arch, c, monkeypatch, info, env=()):
    """whether the tiles behind the block rows are windowed tiles: NPG_WIN_ROWS=0 then changes what one product streams"""
    M, ok = blocked(arch, c, monkeypatch, env + (("NPG_WIN_ROWS", "0"),))
    assert ok
    Checks(c["A"], c["x"]).products(arch, M, True, "NPG_WIN_ROWS=0")
    return M.window_info()["bytes"] != info["bytes"]


# ---- A ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("values", R.VALUES)
@pytest.mark.parametrize("shape", R.EDGE_SHAPES)
def test_kinds_and_edges_of_the_block(arch, monkeypatch, shape, values):
    """Only surface nodes, only full nodes, one node of each kind, both kinds; 1, 2, 3 and 15 records per node (zero-record
    padding), whole tiles without column records (idle loads, the vlist sentinel), gradient entries in one row only.  A matrix
    without full nodes never gets column records (two entries of 12 bytes against a 28-byte record) and so no windowed set."""
    c = R.edge_case(*shape, values, np.random.default_rng(17))
    window = {(170, 87, 64): True, (255, 0, 3): True, (0, 257, 5): False, (0, 257, 0): False, (255, 0, 0): False}.get(shape)
    info = run_case(arch, c, monkeypatch, want_window=window)
    if shape == (170, 87, 64):
        assert info["tiles"] > info["block_tiles"] > 1


# ---- B ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("values", R.VALUES)
@pytest.mark.parametrize("N", R.HUB_N + [1025])
def test_hubs_at_the_window_caps(arch, monkeypatch, N, values):
    """A windowed tile lists its distinct column nodes, at most kWinNodes = 2 per lane of 512 (spmv_window.h): 1024.  A node's N
    records name N distinct nodes; the zero record that pads an odd list repeats the last column node and adds none, and N records
    are (N + 1) / 2 <= 1024 pairs (cap kWinPairs x 512) and 8 x 3 x 513 + 16 x 1025 bytes - far from the other limits
    (plan_window_tiles).  So N = 513 .. 1024 fills the second window-list slot (tid + 512), 1024 fits and 1025 is the
    first that does not: the matrix is still node-blocked but has NO windowed set."""
    c = R.hub_case(N, 0, values, np.random.default_rng(N))
    info = run_case(arch, c, monkeypatch, want_window=N <= 1024)
    assert (info["tiles"] > 0) == (N <= 1024)


@pytest.mark.parametrize("values", R.VALUES)
@pytest.mark.parametrize("G", [512, 513])
def test_gradient_columns_at_the_window_caps(arch, monkeypatch, G, values):
    """kWinCols = 1 column record per lane and one distinct other column per lane: 512 of each (cap_c and nv <= NT in
    plan_window_tiles); a node with 513 gradient columns leaves the matrix without a windowed set."""
    c = R.hub_case(0, G, values, np.random.default_rng(G))
    run_case(arch, c, monkeypatch, want_window=G <= 512)


# ---- C ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("values", R.VALUES)
@pytest.mark.parametrize("kind", ["block", "pp", "empty_run"])
def test_rows_behind_the_block_rows(arch, monkeypatch, kind, values):
    """Rows of coupling records only are windowed row tiles; rows that also hold entries behind the block, or a run of empty rows
    long enough for a tile without a column node, keep their ordinary tiles while the block rows stay windowed (both kinds of
    tile in one launch).  window_info does not say which kind the tiles behind the block are; NPG_WIN_ROWS=0 must give the same
    products either way."""
    c = R.rows_case(kind, values, np.random.default_rng(23))
    info = run_case(arch, c, monkeypatch, want_window=True)
    assert info["tiles"] > info["block_tiles"] > 0
    assert rows_windowed(arch, c, monkeypatch, info) == (kind == "block")


@pytest.mark.parametrize("values", R.VALUES)
def test_row_coupled_to_more_nodes_than_a_window_holds(arch, monkeypatch, values):
    """one row behind the block coupled to 1025 distinct nodes: no windowed row tiles, the block rows keep theirs"""
    c = R.hub_case(0, 0, values, np.random.default_rng(29), row_nodes=1025, nbehind=20)
    info = run_case(arch, c, monkeypatch, want_window=True)
    assert info["tiles"] > info["block_tiles"] > 0
    assert not rows_windowed(arch, c, monkeypatch, info)
    c = R.hub_case(0, 0, values, np.random.default_rng(29), row_nodes=1024, nbehind=20)          # one node fewer: windowed
    info = run_case(arch, c, monkeypatch, want_window=True)
    assert rows_windowed(arch, c, monkeypatch, info)


# ---- D ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many():
    """(matrix, its references) by (entries behind the block, values): built once"""
    rng = np.random.default_rng(31)
    out = {}
    for pp in (True, False):
        for v in R.VALUES:
            c = R.many_tiles_case(rng, 8000, pp=pp, values=v)
            out[pp, v] = (c, Checks(c["A"], c["x"]))
    return out


@pytest.mark.parametrize("values", R.VALUES)
@pytest.mark.parametrize("order,rows", [("0", "1"), ("1", "1"), ("2", "1"), ("0", "0")])
@pytest.mark.parametrize("pp", [True, False])
def test_workgroups_walk_several_tiles(arch, monkeypatch, many, wg_limit, pp, order, rows, values):
    """NPG_WIN_SCALE=0.25 and NPG_WIN_BYTES=8192 make 2 KiB tiles: more tiles than the launch has workgroups (min(tiles, 3 x CUs)),
    so a workgroup goes from tile to tile - block to block, block to row tile, row tile to the end - and hands the next tile's
    window on in registers.  8000 nodes: about 1100 block tiles, the smallest round size that clearly exceeds 3 x 256."""
    c, chk = many[pp, values]
    env = (("NPG_WIN_SCALE", "0.25"), ("NPG_WIN_BYTES", "8192"), ("NPG_WIN_ORDER", order), ("NPG_WIN_ROWS", rows))
    info = run_case(arch, c, monkeypatch, want_window=True, env=env, chk=chk)
    assert info["tiles"] > info["block_tiles"] > wg_limit


def test_gmres_on_many_small_tiles(arch, monkeypatch, many, wg_limit):
    """one solve (fp32 basis) with the gather-layout instance on the ordinary and on the windowed tiles: the stopping rule holds
    on the true residual formed with the scipy matrix.  Benign values only: they are the diagonally dominant instance a solve
    needs."""
    c = many[True, "benign"][0]
    A = c["A"]
    M, ok = blocked(arch, c, monkeypatch, (("NPG_WIN_SCALE", "0.25"), ("NPG_WIN_BYTES", "8192")))
    assert ok and M.window_info()["tiles"] > wg_limit
    y = A @ np.cos(np.arange(A.shape[1], dtype=float))
    for mode in (1, 2):
        ws = npg.GmresWorkspace(arch.ctx, A.shape[0], memory=20)
        ws.set_basis(32)
        ws.set_gather(mode)
        st = ws.solve(M, npg.on_architecture(arch, y), ws.x, npg.Diagonal(scalar=1 / 60.0))
        xs = ws.x.to_host()
        assert st["solved"] == 1 and st["niter"] <= 60, st
        assert np.linalg.norm((y - A @ xs) / 60.0) <= 1.5 * (1e-6 + 1e-6 * st["rnorm0"])


# ---- E ---------------------------------------------------------------------------------------------------------------------------
def test_record_form_that_does_not_fit_leaves_the_matrix_plain(arch, monkeypatch):
    """The structure holds, but the rows of one node do not fit an SpMV tile (2000 records x 3 components > 5824 slots).  Contract
    (include/nupgcm_hip.h): block_nodes returns False, no error, and the matrix is the plain matrix it was - bit for bit - and
    multiplies as before.  (One value set: nothing of the values is looked at before the refusal.)"""
    c = R.overlong_case("hub", np.random.default_rng(37))
    A = c["A"]
    assert R.accepts(A, c["nfull"], c["nsurf"])
    for env in ((), PLAIN, (("NPG_SPMV_WINDOW", "0"),)):
        M, ok = blocked(arch, c, monkeypatch, env)
        assert not ok
        assert M.storage() == (0, 0, A.nnz) and M.coupling_records() == 0 and M.window_info()["tiles"] == 0
        assert bit_equal(M, A)
        chk = Checks(A, c["x"])
        for lanes in (0, 4, 8, 16, 32):
            M.set_lanes(lanes)
            chk.products(arch, M, False, "after the refusal", gather=False)
    assert M.clone().to_scipy_csr().nnz == A.nnz                    # (a plain matrix again: it clones)


def test_tile_of_nodes_without_block_entries_has_no_windowed_set(arch, monkeypatch):
    """300 consecutive nodes whose rows hold gradient entries only: a windowed tile of them would list no column node.  Like every
    other limit of the windowed set this leaves the matrix node-blocked WITHOUT one (window_info: 0 tiles; the windowed product is
    an error); counters and products are those of the record form.  (Benign values: the case is about empty record lists.)"""
    c = R.overlong_case("no_block", np.random.default_rng(37))
    assert R.accepts(c["A"], c["nfull"], c["nsurf"])
    run_case(arch, c, monkeypatch, want_window=False)


# ---- F ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("values", R.VALUES)
@pytest.mark.parametrize("lone", [False, True])
def test_ghost_nodes(arch, monkeypatch, lone, values):
    """A rank's row block (n > m) in one process: npg_spmv_gather32 serves it without a halo (it fills the ghost nodes' slots of
    the gather-layout copy from x itself).  Ghost nodes with the {K, C} structure become node records of the windowed set, the one
    without its y column and the one that breaks the structure stay column records; rows behind the block whose ghost entries are
    all node components are windowed, one more ghost column that belongs to no node keeps them on ordinary tiles."""
    c = R.ghost_case(lone, values, np.random.default_rng(41))
    info = run_case(arch, c, monkeypatch, want_window=True)
    assert info["tiles"] > info["block_tiles"] > 0
    assert rows_windowed(arch, c, monkeypatch, info) == (not lone)
    # without the ghost-node table the same matrix keeps all ghost couplings as column records and its rows on ordinary tiles
    M, ok = blocked(arch, c, monkeypatch, ghosts=False)
    assert ok and M.window_info() != info and M.window_info()["tiles"] > M.window_info()["block_tiles"] > 0
    assert_counts(M, c["A"], c)
    Checks(c["A"], c["x"]).products(arch, M, True, "no ghost-node table")


# ---- G ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.PERTURBATIONS_REFUSED)
def test_refusals_leave_the_matrix_intact(arch, monkeypatch, kind):
    c = R.refusal_base(np.random.default_rng(43))
    B = R.perturb_entry(c["A"], kind, c["nfull"], c["nsurf"], c["q"], c["c"])
    assert not R.accepts(B, c["nfull"], c["nsurf"])
    M = npg.on_architecture(arch, B)
    assert not M.block_nodes(c["nfull"], c["nsurf"])
    assert M.storage() == (0, 0, B.nnz) and bit_equal(M, B)
    Checks(B, c["x"]).products(arch, M, False, kind, gather=False)


def test_mismatch_within_the_tolerance_is_accepted(arch, monkeypatch):
    """y-y differs from x-x by 0.5 rtol scale: accepted, and the record's ONE K (the x-x entry) then stands for the y-y entry too.
    The bound of node q's y row is widened by that: rtol scale_q |x| summed over the node's records (here one record differs)."""
    c = R.refusal_base(np.random.default_rng(43))
    rtol = 1e-12
    B = R.perturb_entry(c["A"], "yy_within", c["nfull"], c["nsurf"], c["q"], c["c"], rtol)
    q, nbr = c["q"], 3 * c["nfull"] + 2 * c["nsurf"]
    scale = np.abs(B[3 * q].toarray()[0, :nbr]).max()
    extra = np.zeros(B.shape[0])
    Bq = B[3 * q + 1].tocoo()
    extra[3 * q + 1] = rtol * scale * np.abs(c["x"][Bq.col[Bq.col < nbr]]).sum()
    run_case(arch, dict(c, A=B), monkeypatch, want_window=True, extra=extra)


# ---- H ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["edge", "rows"])
def test_block_nodes_dofs_in_a_scrambled_order(arch, monkeypatch, which):
    """component-major DoF order with the other unknowns interleaved and arbitrary node labels: products take and return the
    caller's order; the storage is that of the matrix in the library's own order.  (Benign values: npg_csr_block_nodes_dofs does
    not carry exact zeros over, and a record with K == 0 needs its explicit x-x entry.)"""
    rng = np.random.default_rng(47)
    c = R.edge_case(170, 87, 64, "benign", rng) if which == "edge" else R.rows_case("pp", "benign", rng)
    B, node, comp, perm = R.scramble_dofs(c["A"], c["nfull"], c["nsurf"])
    M, ok = blocked(arch, c, monkeypatch)
    assert ok
    S = npg.on_architecture(arch, B)
    assert S.block_nodes_dofs(node, comp)
    assert S.storage() == M.storage() and S.coupling_records() == M.coupling_records()
    assert S.window_info()["tiles"] == M.window_info()["tiles"] > 0
    chk = Checks(B, c["x"][perm])
    for lanes in (0, 4, 8, 16, 32):
        S.set_lanes(lanes)
        chk.products(arch, S, False, f"scrambled, lanes {lanes}", gather=False)
    # a scrambled matrix without the structure is handed back as it came
    Bad = R.scramble_dofs(R.perturb_entry(c["A"], "yx_sign", c["nfull"], c["nsurf"], 5, 6), c["nfull"], c["nsurf"])[0]
    S2 = npg.on_architecture(arch, Bad)
    assert not S2.block_nodes_dofs(node, comp) and bit_equal(S2, Bad)
    Checks(Bad, c["x"][perm]).products(arch, S2, False, "refused, scrambled", gather=False)


# ---- I ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("values", R.VALUES)
@pytest.mark.parametrize("shape", [(0, 257, 0), (255, 0, 0), (1, 1, 1), (170, 87, 64)])
def test_full_node_records_with_absent_pairs(arch, monkeypatch, shape, values):
    """npg_csr_pack_nodes on nine-value node pairs with structurally absent component pairs, on the node graphs, gradient and
    divergence lists of group A; the companion follows combine, gather_values and zero_values of the plain matrix."""
    nfull, nsurf, nbehind = shape
    rng = np.random.default_rng(53)
    base = R.edge_case(*shape, "benign", rng)
    nn = nfull + nsurf
    A9 = R.make_full9(nfull, nsurf, nbehind, base["graph"], base["grad"], base["div"], None, rng, values=values)
    x = base["x"]
    M = npg.on_architecture(arch, A9)
    if nn > 2:
        assert not M.block_nodes(nfull, nsurf) and bit_equal(M, A9)
    assert M.pack_nodes(nfull, nsurf)
    assert bit_equal(M, A9)
    assert M.storage() == (0, 0, A9.nnz)           # (the matrix itself stays plain: the records are its companion's)
    chk = Checks(A9, x)
    for lanes in (0, 4, 8, 16, 32):
        M.set_lanes(lanes)
        chk.products(arch, M, False, f"packed, lanes {lanes}", gather=False)
    # combine: M = 2 X - 0.5 (Y + Z) on the shared pattern
    mats = []
    for k in range(3):
        V = A9.copy()
        V.data[:] = rng.standard_normal(V.nnz)
        mats.append(V)
    X, Y, Z = (npg.on_architecture(arch, V) for V in mats)
    M.combine(2.0, X, -0.5, Y, Z)
    A2 = M.to_scipy_csr()          # (the device's own rounding of the combination; the pattern must be untouched)
    assert np.array_equal(A2.indptr, A9.indptr) and np.array_equal(A2.indices, A9.indices)
    assert np.allclose(A2.data, 2.0 * mats[0].data - 0.5 * (mats[1].data + mats[2].data), rtol=1e-14, atol=1e-15)
    Checks(A2, x).products(arch, M, False, "after combine", gather=False)
    # gather_values: the entries reversed
    idx = np.arange(A9.nnz - 1, -1, -1, dtype=np.int64)
    M.gather_values(X, npg.architectures.DeviceIndex(arch.ctx, idx, A9.nnz))
    A3 = A9.copy()
    A3.data[:] = mats[0].data[idx]
    assert bit_equal(M, A3)
    Checks(A3, x).products(arch, M, False, "after gather_values", gather=False)
    L.check(L.lib().npg_csr_zero_values(M.h))
    y = M.mul(npg.on_architecture(arch, x)).to_host()
    assert np.all(y == 0.0)
