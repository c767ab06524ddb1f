"""Synthetic matrices in the record forms' ordering, and a high-precision reference for products with them.

The record storage of csrc/csr.hip (npg_csr_block_nodes, npg_csr_pack_nodes, the windowed tile set) is otherwise only exercised
by finite-element matrices, which all look alike.  Here a matrix is built from a node graph chosen by the test - hubs, nodes with
one record, nodes without gradient columns, empty rows behind the block - in the ordering the library expects:

    rows / columns  [ 3 nfull (x, y, z of every full node) | 2 nsurf (x, y of every surface node) | nbehind other unknowns ]

Pure numpy / scipy: nothing here needs a GPU.
"""
import numpy as np
import scipy.sparse as sp

U53 = 2.0 ** -53
TILE_SLOTS = 5824          # LDS product slots of one SpMV tile (kTileNnz, csrc/spmv_device.h)


# ---- ordering ------------------------------------------------------------------------------------------------------------------
def first_dof(q, nfull):
    q = np.asarray(q)
    return np.where(q < nfull, 3 * q, 3 * nfull + 2 * (q - nfull))


def node_of_col(c, nfull):
    c = np.asarray(c)
    nf3 = 3 * nfull
    return np.where(c < nf3, c // 3, nfull + (c - nf3) // 2)


def comp_of_col(c, nfull):
    c = np.asarray(c)
    nf3 = 3 * nfull
    return np.where(c < nf3, c % 3, (c - nf3) % 2)


def _csr(rows, cols, vals, shape):
    A = sp.coo_matrix((np.asarray(vals, float), (np.asarray(rows, np.int64), np.asarray(cols, np.int64))), shape=shape).tocsr()
    A.sort_indices()                # (explicit zeros are kept: a record with K == 0 still has its x-x entry)
    return A


# ---- values ----------------------------------------------------------------------------------------------------------------------
def draw(values, rng, n):
    """n values: 'benign' standard normal; 'cancelling' signed magnitudes 1e-6 .. 1e6"""
    if values == "benign":
        return rng.standard_normal(n)
    return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6, 6, n)


def input_vector(n, rng):
    """an input inside fp32 range with entries of very different size"""
    return rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)


# ---- generator -------------------------------------------------------------------------------------------------------------------
def make_blocked(nfull, nsurf, nbehind, node_graph, grad, div, pp, values, rng, x=None):
    """A matrix with the {K, C} node structure.

    node_graph[q]: the column nodes row node q couples to (distinct).  For each pair the SAME double K goes into x-x, y-y and
                   (both nodes full) z-z, C into x-y and -C into y-x.
    grad[q]:       [(j, comps)]: column 3 nfull + 2 nsurf + j holds an entry in the rows `comps` (subset of (0, 1, 2)) of node q
    div[r]:        [(c, comps)]: row r behind the block holds entries in the components `comps` of column node c
    pp:            nbehind x nbehind sparse block (or None)
    values:        'benign' | 'cancelling'.  'cancelling' needs x: every third node's diagonal K is then set so that the block part
                   of its x row sums to zero against x, and every fifth record has K == 0 with C != 0.
    """
    nnode = nfull + nsurf
    nbr = 3 * nfull + 2 * nsurf
    m = nbr + nbehind
    assert len(node_graph) == nnode and len(grad) == nnode and len(div) == nbehind
    qs = np.repeat(np.arange(nnode), [len(g) for g in node_graph]).astype(np.int64)
    cs = np.fromiter((c for g in node_graph for c in g), np.int64, len(qs))
    K = draw(values, rng, len(qs))
    Cc = draw(values, rng, len(qs))
    if values == "cancelling":
        K[4::5] = 0.0
        assert x is not None
        fq, fc = first_dof(qs, nfull), first_dof(cs, nfull)
        term = K * x[fc] + Cc * x[fc + 1]
        for q in range(0, nnode, 3):
            sel = np.flatnonzero(qs == q)
            d = sel[cs[sel] == q]
            if len(d) == 1 and x[fq[d[0]]] != 0.0:
                rest = term[sel].sum() - K[d[0]] * x[fc[d[0]]]
                K[d[0]] = -rest / x[fc[d[0]]]
    fq, fc = first_dof(qs, nfull), first_dof(cs, nfull)
    both = (qs < nfull) & (cs < nfull)
    rows = [fq, fq, fq + 1, fq + 1, fq[both] + 2]
    cols = [fc, fc + 1, fc, fc + 1, fc[both] + 2]
    vals = [K, Cc, -Cc, K, K[both]]
    gr, gc = [], []
    for q in range(nnode):
        for j, comps in grad[q]:
            for a in comps:
                assert a < (3 if q < nfull else 2)
                gr.append(int(first_dof(q, nfull)) + a)
                gc.append(nbr + j)
    rows.append(np.asarray(gr, np.int64))
    cols.append(np.asarray(gc, np.int64))
    vals.append(draw(values, rng, len(gr)))
    dr, dc = [], []
    for r in range(nbehind):
        for c, comps in div[r]:
            for a in comps:
                assert a < (3 if c < nfull else 2)
                dr.append(nbr + r)
                dc.append(int(first_dof(c, nfull)) + a)
    rows.append(np.asarray(dr, np.int64))
    cols.append(np.asarray(dc, np.int64))
    vals.append(draw(values, rng, len(dr)))
    if pp is not None:
        P = sp.coo_matrix(pp)
        rows.append(P.row.astype(np.int64) + nbr)
        cols.append(P.col.astype(np.int64) + nbr)
        vals.append(draw(values, rng, P.nnz))
    return _csr(np.concatenate(rows), np.concatenate(cols), np.concatenate(vals), (m, m))


def banded_graph(nnode, half, rng=None, extra=0):
    """node q couples to q - half .. q + half (clipped) and to `extra` random far nodes"""
    g = []
    for q in range(nnode):
        s = set(range(max(0, q - half), min(nnode, q + half + 1)))
        if extra:
            s.update(int(c) for c in rng.integers(0, nnode, extra))
        g.append(sorted(s))
    return g


def _edit(A, delete=(), add=()):
    """A without the entries `delete` [(i, j)] and with the entries `add` [(i, j, v)]"""
    C = A.tocoo()
    keep = np.ones(C.nnz, bool)
    for i, j in delete:
        hit = (C.row == i) & (C.col == j)
        assert hit.sum() == 1
        keep &= ~hit
    r = np.concatenate([C.row[keep], np.asarray([a[0] for a in add], np.int64)])
    c = np.concatenate([C.col[keep], np.asarray([a[1] for a in add], np.int64)])
    v = np.concatenate([C.data[keep], np.asarray([a[2] for a in add], float)])
    return _csr(r, c, v, A.shape)


PERTURBATIONS_REFUSED = ("yy_off", "yx_sign", "missing_zz", "extra_z", "lone_xx", "pair_on_second")


def perturb_entry(A, kind, nfull, nsurf, q, c, rtol=1e-12):
    """Break (or, 'yy_within', bend within the tolerance) the structure of the coupling of FULL nodes q -> c (an existing pair)."""
    assert q < nfull and c < nfull and q != c
    rx, cx = 3 * q, 3 * c
    nbr = 3 * nfull + 2 * nsurf
    row = A[rx].tocoo()
    scale = np.abs(row.data[row.col < nbr]).max()
    K, Cc = A[rx, cx], A[rx, cx + 1]
    if kind in ("yy_off", "yy_within"):
        d = (2.0 if kind == "yy_off" else 0.5) * rtol * scale
        assert K + d != K
        return _edit(A, [(rx + 1, cx + 1)], [(rx + 1, cx + 1, K + d)])
    if kind == "yx_sign":
        assert Cc != 0.0
        return _edit(A, [(rx + 1, cx)], [(rx + 1, cx, Cc)])
    if kind == "missing_zz":
        return _edit(A, [(rx + 2, cx + 2)])
    if kind == "extra_z":
        return _edit(A, [], [(rx + 2, cx, 0.5)])
    if kind == "lone_xx":
        return _edit(A, [(rx, cx + 1)])
    if kind == "pair_on_second":        # the x row's pair sits on (y_c, z_c) instead of (x_c, y_c)
        return _edit(A, [(rx, cx)], [(rx, cx + 2, K)])
    raise ValueError(kind)


# ---- the acceptance rule of npg_csr_block_nodes, restated from the header comment ------------------------------------------------
def block_table(A, nfull, nsurf):
    """(q, c, T): the coupled node pairs of the block and their 3 x 3 entries T[p, 3 a + b] = A[comp a of q, comp b of c], NaN: absent"""
    nbr = 3 * nfull + 2 * nsurf
    C = A.tocoo()
    sel = (C.row < nbr) & (C.col < nbr)
    r, c, v = C.row[sel].astype(np.int64), C.col[sel].astype(np.int64), C.data[sel]
    q, a = node_of_col(r, nfull), comp_of_col(r, nfull)
    cn, b = node_of_col(c, nfull), comp_of_col(c, nfull)
    key, inv = np.unique(q * (nfull + nsurf + 1) + cn, return_inverse=True)
    T = np.full((len(key), 9), np.nan)
    T[inv, 3 * a + b] = v
    return key // (nfull + nsurf + 1), key % (nfull + nsurf + 1), T


def accepts(A, nfull, nsurf, rtol=1e-12):
    """Header of npg_csr_block_nodes: node q couples to node c through ONE K (the x-x, y-y and - between full nodes - z-z entries)
    and ONE C (x-y entry, -C for y-x), nothing else of the block is stored, checked entry by entry within rtol times the scale of
    the node's x row."""
    nbr = 3 * nfull + 2 * nsurf
    q, c, T = block_table(A, nfull, nsurf)
    if len(q) == 0:
        return True
    both = (q < nfull) & (c < nfull)
    present = ~np.isnan(T)
    want = np.zeros_like(present)
    want[:, [0, 1, 3, 4]] = True
    want[both, 8] = True
    if not np.array_equal(present, want):
        return False
    absA = abs(A).tocsr()[:, :nbr]
    scale_row = np.asarray(absA.max(axis=1).todense()).ravel() if absA.nnz else np.zeros(A.shape[0])
    tol = rtol * scale_row[first_dof(q, nfull)]
    ok = (np.abs(T[:, 4] - T[:, 0]) <= tol) & (np.abs(T[:, 3] + T[:, 1]) <= tol)
    ok[both] &= np.abs(T[both, 8] - T[both, 0]) <= tol[both]
    return bool(ok.all())


# ---- counters --------------------------------------------------------------------------------------------------------------------
def expected_counts(A, nfull, nsurf, coupling=True, column_records=True):
    """What npg_csr_storage / npg_csr_coupling_records report after npg_csr_block_nodes (include/nupgcm_hip.h): block nodes, node
    records (one per coupled node pair), 28-byte records (one per (row behind the block, column node) + one per (node, column
    outside the block)) and the entries left as plain CSR.  The zero records that pad a list to an even count are NOT counted.
    Column records are used when they are fewer bytes than the entries they replace (28 per record against 12 per entry);
    coupling records unless a row behind the block would not fit a tile with them.  coupling / column_records = False: the
    NPG_SPMV_COUPLING=0 / NPG_SPMV_COLUMN_RECORDS=0 builds."""
    nnode, nbr = nfull + nsurf, 3 * nfull + 2 * nsurf
    C = A.tocoo()
    r, c = C.row.astype(np.int64), C.col.astype(np.int64)
    blk_r, blk_c = r < nbr, c < nbr
    q = node_of_col(np.where(blk_r, r, 0), nfull)
    cn = node_of_col(np.where(blk_c, c, 0), nfull)
    s = blk_r & blk_c
    records = len(np.unique(q[s] * (nnode + 1) + cn[s]))
    s = blk_r & ~blk_c
    ngrec, g_entries = len(np.unique(q[s] * A.shape[1] + c[s])), int(s.sum())
    colrec = column_records and ngrec > 0 and 28 * ngrec <= 12 * g_entries
    s = ~blk_r & blk_c
    ndrec, d_entries = len(np.unique(r[s] * (nnode + 1) + cn[s])), int(s.sum())
    rest = int((~blk_r & ~blk_c).sum())
    if coupling and A.shape[0] > nbr:
        per_row = np.bincount(np.unique(r[s] * (nnode + 1) + cn[s]) // (nnode + 1), minlength=A.shape[0])[nbr:]
        rest_row = np.bincount(r[~blk_r & ~blk_c], minlength=A.shape[0])[nbr:]
        coupling = bool(np.all(per_row + (per_row & 1) + rest_row <= TILE_SLOTS))
    else:
        coupling = False
    return dict(nodes=nnode, records=records, coupling_records=(ndrec if coupling else 0) + (ngrec if colrec else 0),
                csr_entries=rest + (0 if coupling else d_entries) + (0 if colrec else g_entries), column_records=colrec,
                coupling=coupling and ndrec > 0)


# ---- reference product and its bound ----------------------------------------------------------------------------------------------
def _rowsum(indptr, v):
    out = np.zeros(len(indptr) - 1, v.dtype)
    nz = np.diff(indptr) > 0
    if nz.any():
        out[nz] = np.add.reduceat(v, indptr[:-1][nz])
    return out


def ref_product(A, x):
    """A x with every product and every row sum in np.longdouble (64-bit significand on x86: error below rowlen 2^-64 |A||x|)"""
    A = sp.csr_matrix(A)
    assert np.finfo(np.longdouble).nmant >= 63
    v = A.data.astype(np.longdouble) * np.asarray(x, float)[A.indices].astype(np.longdouble)
    return _rowsum(A.indptr, v)


def abs_product(A, x):
    A = sp.csr_matrix(A)
    return _rowsum(A.indptr, np.abs(A.data) * np.abs(np.asarray(x, float)[A.indices]))


def row_bound(A, x):
    """(rowlen_i + 3) 2^-53 (|A||x|)_i: the bound on an fp64 sum of rowlen_i fp64 products in ANY order (one rounding per product,
    rowlen - 1 per sum: rowlen u to first order), with room for the three roundings of y = alpha (A x) + beta y.  Derived, not
    measured."""
    A = sp.csr_matrix(A)
    return (np.diff(A.indptr) + 3) * U53 * abs_product(A, x)


class RowCheck:
    """reference and bound of one (A, x), computed once: check(y) for y = alpha A x + beta y0"""

    def __init__(self, A, x):
        self.A, self.x = sp.csr_matrix(A), np.asarray(x, float)
        self.ref, self.bound, self.abs = ref_product(A, x), row_bound(A, x), abs_product(A, x)
        self.len3 = np.diff(self.A.indptr) + 3

    def check(self, y, alpha=1.0, beta=0.0, y0=None, extra=None, what=""):
        ref, bound = alpha * self.ref, abs(alpha) * self.bound
        if beta != 0.0:
            ref = ref + np.longdouble(beta) * y0.astype(np.longdouble)
            bound = bound + self.len3 * U53 * abs(beta) * np.abs(y0)
        if extra is not None:
            bound = bound + extra
        err = np.abs(y.astype(np.longdouble) - ref).astype(float)
        bad = np.flatnonzero(~(err <= bound))
        assert len(bad) == 0, f"{what}: {len(bad)} rows outside the row-wise bound, first {bad[:5]}: err {err[bad[:5]]}, bound {bound[bad[:5]]}"
        if beta == 0.0 and extra is None:
            assert np.all(y[self.abs == 0.0] == 0.0), f"{what}: a row without contributions is not exactly zero"
        return float(np.max(err / np.where(bound > 0, bound, 1.0))) if len(err) else 0.0


def check_rows(y, A, x, alpha=1.0, beta=0.0, y0=None, extra=None):
    """row-wise: |y_i - ref_i| <= bound_i for every i, exact zeros where |A||x| is zero; returns the worst ratio"""
    return RowCheck(A, x).check(y, alpha, beta, y0, extra)


# ---- ghost columns, nine-value pairs, scrambled orders ----------------------------------------------------------------------------
def with_ghosts(A, nfull, nsurf, ghosts, div_ghost, lone, values, rng):
    """A (m x m) with ghost columns [m, n) appended.  ghosts: [(ncomp, kind, [row nodes])], kind 'ok' (the {K, C} structure),
    'no_y' (the ghost node's y column holds nothing), 'broken' (y-y differs from x-x).  div_ghost: [(row behind the block, ghost,
    comps)].  lone: rows behind the block that hold an entry in one more ghost column that belongs to no node.
    Returns (A_ext, first_col, ncomp) for npg_csr_set_ghost_nodes."""
    m = A.shape[0]
    nbr = 3 * nfull + 2 * nsurf
    C = A.tocoo()
    r, c, v = [C.row.astype(np.int64)], [C.col.astype(np.int64)], [C.data]
    first_col, ncomp, col = [], [], m
    for nc, kind, rows in ghosts:
        first_col.append(col)
        ncomp.append(nc)
        for q in rows:
            fq, full = int(first_dof(q, nfull)), q < nfull
            K, Cc = draw(values, rng, 2)
            e = [(fq, col, K), (fq, col + 1, Cc), (fq + 1, col, -Cc), (fq + 1, col + 1, K * 1.5 if kind == "broken" else K)]
            if full and nc == 3:
                e.append((fq + 2, col + 2, K))
            if kind == "no_y":
                e = [t for t in e if t[1] != col + 1]
            for i, j, val in e:
                r.append([i]); c.append([j]); v.append([val])
        col += nc
    for row, g, comps in div_ghost:
        for a in comps:
            r.append([nbr + row]); c.append([first_col[g] + a]); v.append(draw(values, rng, 1))
    if lone:
        for row in lone:
            r.append([nbr + row]); c.append([col]); v.append(draw(values, rng, 1))
        col += 1
    Ae = _csr(np.concatenate(r), np.concatenate(c), np.concatenate(v), (m, col))
    return Ae, np.asarray(first_col, np.int32), np.asarray(ncomp, np.int32)


def make_full9(nfull, nsurf, nbehind, node_graph, grad, div, pp, rng, absent=0.3, values="benign"):
    """nine independent values per coupled node pair (no {K, C} structure), each component pair structurally absent with
    probability `absent` (the diagonal entries always present) - for npg_csr_pack_nodes"""
    A = make_blocked(nfull, nsurf, nbehind, node_graph, grad, div, pp, "benign", rng)
    A.data[:] = draw(values, rng, A.nnz)
    nbr = 3 * nfull + 2 * nsurf
    nnode = nfull + nsurf
    rows, cols = [], []
    for q in range(nnode):
        fq, nq = int(first_dof(q, nfull)), 3 if q < nfull else 2
        for cnode in node_graph[q]:
            fc, ncn = int(first_dof(cnode, nfull)), 3 if cnode < nfull else 2
            for a in range(nq):
                for b in range(ncn):
                    if (q == cnode and a == b) or rng.random() >= absent:
                        rows.append(fq + a)
                        cols.append(fc + b)
    C = A.tocoo()
    keep = ~((C.row < nbr) & (C.col < nbr))
    r = np.concatenate([C.row[keep], np.asarray(rows, np.int64)])
    c = np.concatenate([C.col[keep], np.asarray(cols, np.int64)])
    v = np.concatenate([C.data[keep], draw(values, rng, len(rows))])
    return _csr(r, c, v, A.shape)


def scramble_dofs(A, nfull, nsurf):
    """(P A P^T, node_of_dof, comp_of_dof): component-major order - all x, then the other unknowns interleaved one after every
    third DoF, all y, all z - with arbitrary non-negative node labels; perm[i] = index in A of row i of the result"""
    nnode, nbr, m = nfull + nsurf, 3 * nfull + 2 * nsurf, A.shape[0]
    f = first_dof(np.arange(nnode), nfull)
    vel = [(int(f[q]) + a, q, a) for a in range(3) for q in range(nnode) if a < (3 if q < nfull else 2)]
    others = list(range(nbr, m))
    order, node, comp = [], [], []
    for k, (i, q, a) in enumerate(vel):
        order.append(i); node.append(7 * q + 3); comp.append(a)
        if k % 3 == 2 and others:
            order.append(others.pop(0)); node.append(-1); comp.append(0)
    for i in others:
        order.append(i); node.append(-1); comp.append(0)
    perm = np.asarray(order, np.int64)
    B = sp.csr_matrix(A)[perm][:, perm].tocsr()
    B.sort_indices()
    return B, np.asarray(node, np.int64), np.asarray(comp, np.int32), perm


# ---- the cases (shared by the CPU tests of this module and the GPU tests) ---------------------------------------------------------
ALL3 = (0, 1, 2)


def _comps(q, nfull):
    return ALL3 if q < nfull else (0, 1)


def edge_graph(nnode):
    """record counts per node cycling through 1 (diagonal only), 2, 3 and 15"""
    return [sorted({(q + k) % nnode for k in range(min((1, 2, 3, 15)[q % 4], nnode))}) for q in range(nnode)]


def edge_case(nfull, nsurf, nbehind, values, rng, pp=None):
    """group A: both / one / hardly any kind of node; the middle third of the nodes without any gradient column (whole tiles
    without column records), every eighth node with a gradient entry in only one of its rows; rows behind the block with 0, 1, 3
    and 2 (surface nodes only, x component only: d_z = d_y = 0) coupling records"""
    nnode = nfull + nsurf
    grad = [[] for _ in range(nnode)]
    if nbehind:
        for q in range(nnode):
            if nnode // 3 <= q < 2 * nnode // 3:
                continue
            if q % 8 == 4:
                grad[q] = [(q % nbehind, (1,))]
            else:
                grad[q] = [(j, _comps(q, nfull)) for j in sorted({q % nbehind, (q + 1) % nbehind, (3 * q) % nbehind})]
    div = []
    for r in range(nbehind):
        k = r % 4
        if k == 0:
            div.append([])
        elif k == 1:
            div.append([(r % nnode, _comps(r % nnode, nfull))])
        elif k == 2:
            div.append([(c, _comps(c, nfull)) for c in sorted({r % nnode, (r + 7) % nnode, (5 * r) % nnode})])
        else:
            cs = sorted({nfull + r % nsurf, nfull + (r + 3) % nsurf}) if nsurf else sorted({r % nnode, (r + 3) % nnode})
            div.append([(c, (0,)) for c in cs])
    n = 3 * nfull + 2 * nsurf + nbehind
    x = input_vector(n, rng)
    A = make_blocked(nfull, nsurf, nbehind, edge_graph(nnode), grad, div, pp, values, rng, x)
    return dict(A=A, nfull=nfull, nsurf=nsurf, x=x, graph=edge_graph(nnode), grad=grad, div=div)


HUB_NODES = 1100          # 550 full + 550 surface nodes, banded, plus hubs


def hub_case(N, G, values, rng, row_nodes=0, nbehind=600, hub_full=10, hub_surf=560):
    """group B: a banded matrix with one hub of each kind coupled to N distinct column nodes (itself included; N = 0: no hub), the
    full hub with G gradient columns (0: one like every full node); row_nodes > 0: row 3 behind the block coupled to that many
    distinct nodes"""
    nfull = nsurf = HUB_NODES // 2
    nnode = nfull + nsurf
    graph = banded_graph(nnode, 2)
    for hub in ((hub_full, hub_surf) if N else ()):
        others = [c for c in np.unique(np.linspace(0, nnode - 1, N + 8).astype(int)) if c != hub][:N - 1]
        graph[hub] = sorted(set(others) | {hub})
        assert len(graph[hub]) == N
    grad = [[(q % nbehind, ALL3)] if q < nfull else [] for q in range(nnode)]
    if G:
        grad[hub_full] = [(j, ALL3) for j in range(G)]
    div = [[(r % nnode, _comps(r % nnode, nfull))] for r in range(nbehind)]
    if row_nodes:
        div[3] = [(c, _comps(c, nfull)) for c in range(row_nodes)]
    n = 3 * nfull + 2 * nsurf + nbehind
    x = input_vector(n, rng)
    A = make_blocked(nfull, nsurf, nbehind, graph, grad, div, None, values, rng, x)
    return dict(A=A, nfull=nfull, nsurf=nsurf, x=x)


def rows_case(kind, values, rng):
    """group C: the rows behind the block rows.  'block': entries in block columns only (1, 3, 2 surface-only, 0 and 4 records per
    row); 'pp': every seventh row also holds entries of the block behind the block; 'empty_run': 300 consecutive empty rows"""
    nfull, nsurf, nbehind = 120, 80, 420
    nnode = nfull + nsurf
    grad = [[(q % nbehind, ALL3)] if q < nfull else [] for q in range(nnode)]
    div = []
    for r in range(nbehind):
        k = r % 5
        if kind == "empty_run" and 60 <= r < 360:
            div.append([])
        elif k == 0:
            div.append([(r % nnode, _comps(r % nnode, nfull))])
        elif k == 1:
            div.append([(c, _comps(c, nfull)) for c in sorted({r % nnode, (r + 9) % nnode, (7 * r) % nnode})])
        elif k == 2:
            div.append([(c, (0, 1)) for c in sorted({nfull + r % nsurf, nfull + (r + 5) % nsurf})])
        elif k == 3:
            div.append([])
        else:
            div.append([(c, _comps(c, nfull)) for c in sorted({(r + j * 11) % nnode for j in range(4)})])
    pp = None
    if kind == "pp":
        idx = np.arange(0, nbehind, 7)
        pp = sp.coo_matrix((np.ones(2 * len(idx)), (np.r_[idx, idx], np.r_[idx, (idx + 1) % nbehind])), shape=(nbehind, nbehind))
    n = 3 * nfull + 2 * nsurf + nbehind
    x = input_vector(n, rng)
    A = make_blocked(nfull, nsurf, nbehind, banded_graph(nnode, 2), grad, div, pp, values, rng, x)
    return dict(A=A, nfull=nfull, nsurf=nsurf, x=x)


def many_tiles_case(rng, nnode=8000, pp=True, values="benign"):
    """group D: about 14 banded neighbours and 2 random far ones per node; 'benign' values are made diagonally dominant (the GMRES
    solve)"""
    nfull = nsurf = nnode // 2
    nbehind = nnode // 4
    graph = banded_graph(nnode, 7, rng, extra=2)
    grad = [[(q % nbehind, _comps(q, nfull))] for q in range(nnode)]
    div = [[(c, _comps(c, nfull)) for c in sorted({r % nnode, (4 * r + 1) % nnode, (r + nnode // 2) % nnode})] for r in range(nbehind)]
    P = sp.identity(nbehind, format="coo") if pp else None
    n = 3 * nfull + 2 * nsurf + nbehind
    x = input_vector(n, rng)
    A = make_blocked(nfull, nsurf, nbehind, graph, grad, div, P, values, rng, x)
    if values != "benign":
        return dict(A=A, nfull=nfull, nsurf=nsurf, x=x)
    nbr = 3 * nfull + 2 * nsurf
    A = A.tolil()                   # K of every node's own record (x-x, y-y, z-z alike) and the block behind the block
    for i in range(nbr + (nbehind if pp else 0)):
        A[i, i] = 60.0
    A = A.tocsr()
    A.sort_indices()
    return dict(A=A, nfull=nfull, nsurf=nsurf, x=input_vector(A.shape[1], rng))


def overlong_case(kind, rng):
    """group E: matrices with the structure whose record form does not fit.  'hub': a full node with 2000 neighbours (three product
    slots per record: more than one tile holds); 'no_block': 300 consecutive full nodes whose rows hold gradient entries only - a
    windowed tile without a single column node"""
    nfull, nsurf, nbehind = 1100, 1000, 64
    nnode = nfull + nsurf
    graph = banded_graph(nnode, 1)
    if kind == "hub":
        graph[7] = list(range(2000))
    else:
        for q in range(400, 700):
            graph[q] = []
    grad = [[(q % nbehind, ALL3)] if q < nfull else [] for q in range(nnode)]
    div = [[(r, ALL3)] for r in range(nbehind)]
    A = make_blocked(nfull, nsurf, nbehind, graph, grad, div, sp.identity(nbehind), "benign", rng)
    return dict(A=A, nfull=nfull, nsurf=nsurf, x=input_vector(A.shape[1], rng))


def refusal_base(rng):
    nfull, nsurf, nbehind = 60, 40, 30
    nnode = nfull + nsurf
    grad = [[(q % nbehind, ALL3)] if q < nfull else [] for q in range(nnode)]
    div = [[(r, ALL3)] for r in range(nbehind)]
    A = make_blocked(nfull, nsurf, nbehind, banded_graph(nnode, 2), grad, div, sp.identity(nbehind), "benign", rng)
    return dict(A=A, nfull=nfull, nsurf=nsurf, x=input_vector(A.shape[1], rng), q=5, c=6)


def ghost_case(lone, values, rng):
    """group F: a rank's row block with ghost nodes of 3 and of 2 components, one without its y column, one that breaks {K, C}; rows
    behind the block with entries on ghost node components (and, `lone`, on a ghost column that belongs to no node)"""
    base = edge_case(90, 60, 40, values, rng)
    nfull, nsurf = base["nfull"], base["nsurf"]
    ghosts = [(3, "ok", [0, 1, 2, 95]), (2, "ok", [3, 100, 101]), (3, "no_y", [4, 5]), (3, "broken", [6, 7]), (2, "ok", [149])]
    div_ghost = [(1, 0, ALL3), (1, 1, (0, 1)), (5, 4, (1,)), (8, 2, (0, 2))]
    A, first_col, ncomp = with_ghosts(base["A"], nfull, nsurf, ghosts, div_ghost, [9, 13] if lone else [], values, rng)
    return dict(A=A, nfull=nfull, nsurf=nsurf, x=input_vector(A.shape[1], rng), first_col=first_col, ncomp=ncomp)


EDGE_SHAPES = [(0, 257, 0), (255, 0, 0), (1, 1, 1), (170, 87, 64), (255, 0, 3), (0, 257, 5)]
HUB_N = [511, 512, 513, 1023, 1024]
VALUES = ["cancelling", "benign"]


def cpu_cases(rng):
    """every {K, C} case the GPU tests use (name, case)"""
    for v in VALUES:
        for s in EDGE_SHAPES:
            yield f"edge{s}-{v}", edge_case(*s, v, rng)
        for k in ("block", "pp", "empty_run"):
            yield f"rows-{k}-{v}", rows_case(k, v, rng)
    for N in HUB_N + [1025]:
        yield f"hub{N}", hub_case(N, 0, "benign", rng)
    for G in (512, 513):
        yield f"grad{G}", hub_case(0, G, "cancelling", rng)
    yield "row1025", hub_case(0, 0, "benign", rng, row_nodes=1025, nbehind=20)
    yield "many", many_tiles_case(rng, 2000)
    yield "many-rows", many_tiles_case(rng, 2000, pp=False)
    for k in ("hub", "no_block"):
        yield f"overlong-{k}", overlong_case(k, rng)
    yield "refusal-base", refusal_base(rng)
