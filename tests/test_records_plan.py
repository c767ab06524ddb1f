"""The host planner of the record storage (csrc/csr_records_core.h) without a GPU: tests/records_plan_main.cpp is compiled with
g++ under AddressSanitizer and UBSan and run as a child process on the cases of tests/records_ref.py.  Checked: the outcome against
records_ref.accepts, the counters against records_ref.expected_counts, the matrix rebuilt from the plan bit for bit, the padding,
and the windowed plan's indices, coverage and caps."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from tests import records_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ACCEPTED, NOT_THE_STRUCTURE, NODE_DOES_NOT_FIT, ROW_DOES_NOT_FIT = range(4)
# caps of a windowed tile (csrc/spmv_window.h: 512 threads, kWinPairs = 2, kWinCols = 1, kWinNodes = 2; csrc/spmv_device.h: kTileNnz)
NT, WIN_PAIRS, WIN_COLS, WIN_NODES, TILE_ROWS = 512, 2, 1, 2, 256
DTYPES = {"i64": np.int64, "i32": np.int32, "f64": np.float64, "u16": np.uint16}


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/records_plan_main.cpp")
    exe = str(tmp_path_factory.mktemp("records_plan") / "records_plan_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                    os.path.join(HERE, "records_plan_main.cpp"), "-o", exe], check=True)
    return exe


def plan(planner, d, A, nfull, nsurf, full=False, ghosts=None, **switches):
    """run the planner on A in directory d; returns (meta, arrays)"""
    A = sp.csr_matrix(A)
    shutil.rmtree(d, ignore_errors=True)
    os.makedirs(d)
    A.indptr.astype("<i8").tofile(os.path.join(d, "rowptr.i64"))
    A.indices.astype("<i4").tofile(os.path.join(d, "col.i32"))
    A.data.astype("<f8").tofile(os.path.join(d, "val.f64"))
    if ghosts is not None:
        ghosts[0].astype("<i4").tofile(os.path.join(d, "gn_col.i32"))
        ghosts[1].astype("<i4").tofile(os.path.join(d, "gn_ncomp.i32"))
    meta = dict(m=A.shape[0], n=A.shape[1], nfull=nfull, nsurf=nsurf, rtol=1e-12, full=int(full), window=1, column_records=1,
                coupling=1, win_rows=1, win_bytes=0, win_scale=1.0, win_order=0, num_cu=256)
    meta.update(switches)
    with open(os.path.join(d, "meta.txt"), "w") as f:
        for k, v in meta.items():
            f.write(f"{k} {v!r}\n")
    subprocess.run([planner, d], check=True)            # (a sanitizer report ends the child with a non-zero status)
    out = {}
    with open(os.path.join(d, "out_meta.txt")) as f:
        for line in f:
            k, v = line.split()
            out[k] = int(v)
    arr = {}
    for name in os.listdir(d):
        if name.startswith("out_") and name != "out_meta.txt":
            base, ext = name[4:].rsplit(".", 1)
            arr[base] = np.fromfile(os.path.join(d, name), dtype=DTYPES[ext])
    return out, arr


# ---- the reconstruction rule, from the layouts documented in csrc/common.h (npg_csr) ----------------------------------------------
def lists(offsets, lengths=None):
    """(owner, index) of every record of the lists offsets[i] .. offsets[i] + lengths[i] (default: the whole list)"""
    n = np.diff(offsets) if lengths is None else np.asarray(lengths, np.int64)
    owner = np.repeat(np.arange(len(n)), n)
    idx = np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n) + np.repeat(offsets[:-1], n)
    return owner, idx


def rebuild_block(a, m, n, nfull, nsurf, colrec, coupling):
    """(rows, cols, vals) of the matrix a {K, C} plan stands for: node records (x-x = y-y = K, x-y = C, y-x = -C, z-z = K between
    full nodes), column records, coupling records and the CSR remainder; the padding records are left out"""
    nbr = 3 * nfull + 2 * nsurf
    q, e = lists(a["prow"], a["plen"])
    c = a["pcol"][e].astype(np.int64)
    K, C = a["pkc"][2 * e], a["pkc"][2 * e + 1]
    fq, fc = R.first_dof(q, nfull), R.first_dof(c, nfull)
    both = (q < nfull) & (c < nfull)
    rows = [fq, fq, fq + 1, fq + 1, fq[both] + 2]
    cols = [fc, fc + 1, fc, fc + 1, fc[both] + 2]
    vals = [K, C, -C, K, K[both]]
    if colrec:
        q, e = lists(a["grow"])
        fq, full = R.first_dof(q, nfull), q < nfull
        assert np.all(a["gz"][e][~full] == 0.0)
        rows += [fq, fq + 1, fq[full] + 2]
        cols += [a["gcol"][e], a["gcol"][e], a["gcol"][e][full]]
        vals += [a["gxy"][2 * e], a["gxy"][2 * e + 1], a["gz"][e][full]]
    if coupling:
        r, e = lists(a["drow"], a["dlen"])
        c = a["dcol"][e].astype(np.int64)
        fc, full = R.first_dof(c, nfull), c < nfull
        assert np.all(a["dz"][e][~full] == 0.0)
        rows += [nbr + r, nbr + r, nbr + r[full]]
        cols += [fc, fc + 1, fc[full] + 2]
        vals += [a["dxy"][2 * e], a["dxy"][2 * e + 1], a["dz"][e][full]]
    r, e = lists(a["rowptr"])
    rows.append(r)
    cols.append(a["col"][e])
    vals.append(a["val"][e])
    return (np.concatenate([np.asarray(x, np.int64) for x in rows]), np.concatenate([np.asarray(x, np.int64) for x in cols]),
            np.concatenate(vals))


def assert_same_matrix(A, rows, cols, vals):
    """every entry of A is in the rebuilt matrix with the same bits, once; what the rebuilt matrix holds beside them is +0.0 (the
    slots of a record whose entry is absent)"""
    A = sp.csr_matrix(A).tocoo()
    n = A.shape[1]
    key = rows * n + cols
    order = np.argsort(key, kind="stable")
    key, vals = key[order], vals[order]
    assert np.all(np.diff(key) > 0), "the plan stores an entry twice"
    akey = A.row.astype(np.int64) * n + A.col
    pos = np.searchsorted(key, akey)
    assert np.all(pos < len(key)) and np.array_equal(key[np.minimum(pos, len(key) - 1)], akey), "an entry of the matrix is not in the plan"
    assert np.array_equal(vals[pos].view(np.int64), A.data.view(np.int64)), "an entry differs in its bits"
    rest = np.ones(len(key), bool)
    rest[pos] = False
    assert np.all(vals[rest].view(np.int64) == 0), "the plan holds a value the matrix does not"


def check_padding(a, meta):
    for off, ln, zero, col in (("prow", "plen", ("pkc", 2), "pcol"),) + ((("drow", "dlen", ("dxy", 2), "dcol"),) if meta["coupling"] else ()):
        n = np.diff(a[off])
        pad = n - a[ln]
        assert np.all((pad == 0) | (pad == 1))
        if meta["padded"]:
            assert np.all(n % 2 == 0), f"{off}: a list the kernels take in pairs has an odd length"
            assert np.array_equal(pad, a[ln] % 2)
        else:
            assert np.all(pad == 0)
        e = a[off][1:][pad == 1] - 1                    # the padding records: exactly those beyond the unpadded length
        name, w = zero
        assert np.all(a[name].reshape(-1, w)[e] == 0.0) and np.array_equal(a[col][e], a[col][e - 1])
        if off == "drow":
            assert np.all(a["dz"][e] == 0.0)


def tiles_of(a, name):
    t = a[name].reshape(-1, 10)
    return [dict(zip(("base", "pbase", "r0", "nrows", "n", "npe", "woff", "voff", "nw", "nv"), map(int, row))) for row in t]


def check_window(a, meta, m, nfull, nsurf):
    nnode, nbr = nfull + nsurf, 3 * nfull + 2 * nsurf
    prow, grow = (a["wprow"], a["wgrow"]) if meta["win_own"] else (a["prow"], a["grow"])
    pcol, gcol = (a["wpcol"], a["wgcol"]) if meta["win_own"] else (a["pcol"], a["gcol"])
    drow, dcol = (a["wdrow"], a["wdcol"]) if meta["win_rows_own"] else (a["drow"], a["dcol"])
    assert np.all(np.diff(prow) % 2 == 0) and meta["win_nw_rec"] == prow[-1] and meta["win_nw_grec"] == len(gcol)
    assert len(a["pkc2"]) == 2 * len(pcol) == 4 * meta["win_npairs"] and len(a["widx"]) == len(pcol) and len(a["gidx"]) == len(gcol)
    assert a["vlist"][-1] == nbr                        # the sentinel
    tiles = tiles_of(a, "wtiles")
    ni = meta["win_ninterior"]
    covered = np.zeros(m, np.int64)
    nrow_tiles = 0
    for part in (tiles[:ni], tiles[ni:]):
        blk = [t for t in part if t["r0"] < nbr]
        assert all(x["r0"] < y["r0"] for x, y in zip(blk, blk[1:])), "block tiles out of order within a pass"
        beh = [t for t in part if t["r0"] >= nbr]
        assert all(x["r0"] < y["r0"] for x, y in zip(beh, beh[1:]))
    for t in tiles:
        covered[t["r0"]:t["r0"] + t["nrows"]] += 1
        if t["r0"] < nbr:
            ncomp = 3 if t["r0"] < 3 * nfull else 2
            q0, q1 = int(R.node_of_col(t["r0"], nfull)), int(R.node_of_col(t["r0"] + t["nrows"] - 1, nfull)) + 1
            assert t["nrows"] == ncomp * (q1 - q0) and t["pbase"] == prow[q0] and t["npe"] == prow[q1] - prow[q0]
            assert t["base"] == grow[q0] and t["n"] == grow[q1] - grow[q0]
            e = np.arange(t["pbase"], t["pbase"] + t["npe"])
            assert t["nw"] > 0 and np.all(a["widx"][e] < t["nw"]) and np.array_equal(a["wlist"][t["woff"] + a["widx"][e].astype(np.int64)], pcol[e])
            g = np.arange(t["base"], t["base"] + t["n"])
            assert np.all(a["gidx"][g] < max(t["nv"], 1) if len(g) else True)
            assert np.array_equal(a["vlist"][t["voff"] + a["gidx"][g].astype(np.int64)], gcol[g])
            np_, ng = t["npe"] // 2, t["n"]
            assert t["nrows"] <= TILE_ROWS and np_ <= WIN_PAIRS * NT and ng <= WIN_COLS * NT and t["nw"] <= WIN_NODES * NT and t["nv"] <= NT
            assert 8 * ((ncomp * (np_ + ng) + 1) & ~1) + 16 * t["nw"] + 4 * t["nv"] <= 8 * R.TILE_SLOTS
            w = a["wbk"].reshape(-1, 2)[q0:q1]
            assert np.array_equal(w[:, 0], grow[q0 + 1:q1 + 1] - grow[q0]) and np.array_equal(w[:, 1], (prow[q0 + 1:q1 + 1] - prow[q0]) // 2)
        elif t["nw"] > 0:
            nrow_tiles += 1
            r0, r1 = t["r0"] - nbr, t["r0"] - nbr + t["nrows"]
            assert t["pbase"] == drow[r0] and t["npe"] == drow[r1] - drow[r0] and t["n"] == 0
            e = np.arange(t["pbase"], t["pbase"] + t["npe"])
            assert np.all(a["dwidx"][e] < t["nw"]) and np.array_equal(a["wlist"][t["woff"] + a["dwidx"][e].astype(np.int64)], dcol[e])
            assert t["nrows"] <= TILE_ROWS // 2 and t["npe"] // 2 <= WIN_PAIRS * NT and t["nw"] <= WIN_NODES * NT
            assert np.array_equal(a["dbk"][r0:r1], (drow[r0 + 1:r1 + 1] - drow[r0]) // 2)
    assert np.all(covered == 1), "the windowed set does not cover every row exactly once"
    assert nrow_tiles == meta["win_nrow_tiles"]
    if nrow_tiles:
        assert np.all(np.diff(drow) % 2 == 0) and len(a["dxy2"]) == 2 * len(dcol) == 4 * meta["win_ndpairs"] and meta["win_nw_drec"] == len(dcol)


def check_block_case(planner, d, c, window=None):
    A, nfull, nsurf = sp.csr_matrix(c["A"]), c["nfull"], c["nsurf"]
    ghosts = (c["first_col"], c["ncomp"]) if "first_col" in c else None
    accepted = R.accepts(A, nfull, nsurf)
    for switches in (dict(), dict(coupling=0, column_records=0), dict(window=0)):
        meta, a = plan(planner, d, A, nfull, nsurf, ghosts=ghosts, **switches)
        assert (meta["outcome"] != NOT_THE_STRUCTURE) == accepted
        if meta["outcome"] != ACCEPTED:
            return meta
        on = not ("coupling" in switches)
        e = R.expected_counts(A, nfull, nsurf, coupling=on, column_records=on)
        assert (len(a["plen"]), meta["nrec_real"], len(a["col"])) == (e["nodes"], e["records"], e["csr_entries"])
        assert meta["ndrec_real"] + len(a["gcol"]) == e["coupling_records"]
        assert (meta["colrec"], meta["coupling"]) == (int(e["column_records"]), int(e["coupling"]))
        assert meta["padded"] == int(switches.get("window", 1))
        check_padding(a, meta)
        assert_same_matrix(A, *rebuild_block(a, A.shape[0], A.shape[1], nfull, nsurf, meta["colrec"], meta["coupling"]))
        assert meta["tiles_fit"] == ACCEPTED
        if not switches:
            first = meta
            if window is not None:
                assert meta["win_present"] == int(window)
            if meta["win_present"]:
                assert not meta["win_overflow"]
                check_window(a, meta, A.shape[0], nfull, nsurf)
        else:
            assert not meta["win_present"]
    return first


@pytest.mark.parametrize("values", R.VALUES)
@pytest.mark.parametrize("shape", R.EDGE_SHAPES)
def test_edge_shapes(planner, tmp_path, shape, values):
    window = {(170, 87, 64): True, (255, 0, 3): True, (0, 257, 5): False, (0, 257, 0): False, (255, 0, 0): False}.get(shape)
    check_block_case(planner, str(tmp_path / "c"), R.edge_case(*shape, values, np.random.default_rng(17)), window)


@pytest.mark.parametrize("values", R.VALUES)
@pytest.mark.parametrize("N", [512, 513, 1024, 1025])
def test_hubs_at_the_window_caps(planner, tmp_path, N, values):
    """a node's N records name N distinct nodes: 2 x 512 fit a windowed tile, 1025 leave the matrix without a windowed set"""
    check_block_case(planner, str(tmp_path / "c"), R.hub_case(N, 0, values, np.random.default_rng(N)), N <= WIN_NODES * NT)


@pytest.mark.parametrize("values", R.VALUES)
@pytest.mark.parametrize("G", [512, 513])
def test_gradient_columns_at_the_window_caps(planner, tmp_path, G, values):
    check_block_case(planner, str(tmp_path / "c"), R.hub_case(0, G, values, np.random.default_rng(G)), G <= WIN_COLS * NT)


@pytest.mark.parametrize("values", R.VALUES)
@pytest.mark.parametrize("kind", ["block", "pp", "empty_run"])
def test_rows_behind_the_block_rows(planner, tmp_path, kind, values):
    """rows of coupling records only become windowed row tiles; entries behind the block or a long run of empty rows keep them on
    ordinary tiles"""
    meta = check_block_case(planner, str(tmp_path / "c"), R.rows_case(kind, values, np.random.default_rng(23)), True)
    assert (meta["win_nrow_tiles"] > 0) == (kind == "block")


@pytest.mark.parametrize("values", R.VALUES)
@pytest.mark.parametrize("lone", [False, True])
def test_ghost_nodes(planner, tmp_path, lone, values):
    """ghost nodes with the structure become node records of the windowed set; a ghost column that belongs to no node keeps the rows
    behind the block on ordinary tiles"""
    c = R.ghost_case(lone, values, np.random.default_rng(41))
    meta = check_block_case(planner, str(tmp_path / "c"), c, True)
    assert meta["win_own"] and meta["win_rows_own"] == int(not lone) and (meta["win_nrow_tiles"] > 0) == (not lone)
    # the set's own records stand for the same matrix: node records on ghost nodes rebuilt as entries on their columns
    _, a = plan(planner, str(tmp_path / "c"), c["A"], c["nfull"], c["nsurf"], ghosts=(c["first_col"], c["ncomp"]))
    nnode, m = c["nfull"] + c["nsurf"], c["A"].shape[0]
    q, e = lists(a["wprow"])
    cn = a["wpcol"][e].astype(np.int64)
    k2, P = a["pkc2"], len(a["wpcol"]) // 2
    pkc = np.empty(2 * len(a["wpcol"]))
    pkc.reshape(-1, 4)[:, :2] = k2[:2 * P].reshape(-1, 2)
    pkc.reshape(-1, 4)[:, 2:] = k2[2 * P:].reshape(-1, 2)
    pad = np.zeros(len(cn), bool)                       # (a node's column nodes are distinct: a repeated one is the padding record)
    pad[1:] = (q[1:] == q[:-1]) & (cn[1:] == cn[:-1])
    assert np.all(pkc.reshape(-1, 2)[e[pad]] == 0.0)
    gh = (cn >= nnode) & ~pad
    assert gh.sum() > 0 and np.all(cn[gh] - nnode < len(c["first_col"]))
    g = cn[gh] - nnode
    fq, fc, full = R.first_dof(q[gh], c["nfull"]), c["first_col"][g].astype(np.int64), (q[gh] < c["nfull"]) & (c["ncomp"][g] == 3)
    K, C = pkc[2 * e[gh]], pkc[2 * e[gh] + 1]
    rows = np.concatenate([fq, fq, fq + 1, fq + 1, fq[full] + 2])
    cols = np.concatenate([fc, fc + 1, fc, fc + 1, fc[full] + 2])
    vals = np.concatenate([K, C, -C, K, K[full]])
    ng = len(a["wgcol"])
    qg, eg = lists(a["wgrow"])
    fqg, fullg = R.first_dof(qg, c["nfull"]), qg < c["nfull"]
    rows = np.concatenate([rows, fqg, fqg + 1, fqg[fullg] + 2])
    cols = np.concatenate([cols, a["wgcol"][eg], a["wgcol"][eg], a["wgcol"][eg][fullg]])
    vals = np.concatenate([vals, a["wgval"][2 * eg], a["wgval"][2 * eg + 1], a["wgval"][2 * ng + eg][fullg]])
    nbr = 3 * c["nfull"] + 2 * c["nsurf"]
    sub = sp.csr_matrix(c["A"])[:nbr].tocoo()
    keep = sub.col >= nbr
    assert_same_matrix(sp.coo_matrix((sub.data[keep], (sub.row[keep], sub.col[keep])), shape=c["A"].shape), rows, cols, vals)


@pytest.mark.parametrize("kind", ["hub", "no_block"])
def test_overlong(planner, tmp_path, kind):
    """a node with 2000 records fits no tile (no error: an outcome); 300 nodes without block entries leave no windowed set"""
    meta = check_block_case(planner, str(tmp_path / "c"), R.overlong_case(kind, np.random.default_rng(37)), False if kind == "no_block" else None)
    assert meta["outcome"] == (NODE_DOES_NOT_FIT if kind == "hub" else ACCEPTED)


@pytest.mark.parametrize("kind", R.PERTURBATIONS_REFUSED)
def test_refusals(planner, tmp_path, kind):
    c = R.refusal_base(np.random.default_rng(43))
    assert check_block_case(planner, str(tmp_path / "c"), c, True)["outcome"] == ACCEPTED
    B = R.perturb_entry(c["A"], kind, c["nfull"], c["nsurf"], c["q"], c["c"])
    assert not R.accepts(B, c["nfull"], c["nsurf"])
    assert check_block_case(planner, str(tmp_path / "c"), dict(c, A=B))["outcome"] == NOT_THE_STRUCTURE


@pytest.mark.parametrize("values", R.VALUES)
@pytest.mark.parametrize("shape", [(0, 257, 0), (255, 0, 0), (1, 1, 1), (170, 87, 64)])
def test_full_node_records(planner, tmp_path, shape, values):
    """plan_full_records: every entry of the matrix is referenced exactly once, from the slot that stands for its row and column"""
    nfull, nsurf, nbehind = shape
    rng = np.random.default_rng(53)
    base = R.edge_case(*shape, "benign", rng)
    A = sp.csr_matrix(R.make_full9(nfull, nsurf, nbehind, base["graph"], base["grad"], base["div"], None, rng, values=values))
    meta, a = plan(planner, str(tmp_path / "c"), A, nfull, nsurf, full=True)
    assert meta["outcome"] == ACCEPTED
    nbr = 3 * nfull + 2 * nsurf
    n9, ng, nd = len(a["pcol"]), len(a["gcol"]), len(a["dcol"])
    assert (len(a["map9"]), len(a["mapg"]), len(a["mapd"]), len(a["maprem"])) == (9 * n9, 3 * ng, 3 * nd, len(a["col"]))
    q, e = lists(a["prow"])
    fq, fc = R.first_dof(q, nfull), R.first_dof(a["pcol"][e].astype(np.int64), nfull)
    rows, cols, pos = [], [], []
    for s9 in range(9):
        rows.append(fq + s9 // 3)
        cols.append(fc + s9 % 3)
        pos.append(a["map9"][(s9 & ~1) * n9 + 2 * e + (s9 & 1)] if s9 < 8 else a["map9"][8 * n9 + e])
    q, e = lists(a["grow"])
    r, ed = lists(a["drow"])
    fq, fc = R.first_dof(q, nfull), R.first_dof(a["dcol"][ed].astype(np.int64), nfull)
    for k in range(3):
        rows += [fq + k, nbr + r]
        cols += [a["gcol"][e].astype(np.int64), fc + k]
        pos += [a["mapg"][2 * e + k] if k < 2 else a["mapg"][2 * ng + e], a["mapd"][2 * ed + k] if k < 2 else a["mapd"][2 * nd + ed]]
    r, e = lists(a["rowptr"])
    assert np.all(r >= nbr)
    rows.append(r)
    cols.append(a["col"][e].astype(np.int64))
    pos.append(a["maprem"][e])
    rows, cols, pos = (np.concatenate([np.asarray(x, np.int64) for x in v]) for v in (rows, cols, pos))
    used = pos >= 0
    assert np.array_equal(np.sort(pos[used]), np.arange(A.nnz)), "every entry once"
    C = A.tocoo()              # (canonical CSR: position k is entry k)
    assert np.array_equal(C.row[pos[used]], rows[used]) and np.array_equal(C.col[pos[used]], cols[used])
