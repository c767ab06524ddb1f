// Record storage of the velocity block, planned on the host: WHAT the record form of a matrix is - node records, column records,
// coupling records, the CSR remainder, the windowed tile set - as plain host arrays in the layouts the kernels read (common.h,
// spmv_device.h, spmv_window.h).  Standard library only: csr.hip uploads a plan into a candidate handle and commits it; the CPU test
// (tests/records_plan_main.cpp) compiles this header alone, under a sanitizer.  Nothing here reads the environment.
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cmath>
#include <cstdint>
#include <vector>

namespace npg {

// THE ordering of a node-blocked matrix: rows / columns [ 3 nfull (x, y, z of every full node) | 2 nsurf (x, y of every surface
// node) | the rest ]
struct NodeOrder {
    int64_t nfull = 0, nsurf = 0;
    int64_t nnode() const { return nfull + nsurf; }
    int64_t block_rows() const { return 3 * nfull + 2 * nsurf; }
    int ncomp(int64_t q) const { return q < nfull ? 3 : 2; }
    int64_t first(int64_t q) const { return q < nfull ? 3 * q : 3 * nfull + 2 * (q - nfull); }                  // first DoF of node q
    int64_t node_of(int64_t c) const { return c < 3 * nfull ? c / 3 : nfull + (c - 3 * nfull) / 2; }            // c < block_rows()
};

// limits of one tile; the defaults are the kernels' constants (csr.hip asserts the equalities)
struct RecordCaps {
    int tile_slots = 5824;      // kTileNnz: LDS product slots of an ordinary tile
    int tile_rows = 256;        // kTileRows
    int win_threads = 512;      // threads of the windowed kernels
    int win_pairs = 2, win_cols = 1, win_nodes = 2;      // kWinPairs, kWinCols, kWinNodes: per lane of a windowed tile
};

// the environment switches of a conversion, read once by the caller (record_switches(), csr.hip)
struct RecordSwitches {
    bool window = true;             // NPG_SPMV_WINDOW=0: no windowed tile set, no padding of record lists
    bool column_records = true;     // NPG_SPMV_COLUMN_RECORDS=0
    bool coupling = true;           // NPG_SPMV_COUPLING=0
    bool win_rows = true;           // NPG_WIN_ROWS=0: ordinary tiles for the rows behind the block rows
    int64_t win_bytes = 0;          // NPG_WIN_BYTES, at least 8192 (0: not set): smaller windowed tiles
    double win_scale = 1.0;         // NPG_WIN_SCALE (> 0): all caps of a windowed tile scaled, clamped to [0.25, 1]
    int win_order = 0;              // NPG_WIN_ORDER
    int wlanes = 0;                 // NPG_SPMV_WLANES: 8 or 4 (0: not set)
};

// a sorted CSR matrix on the host (val may be null where only positions are wanted)
struct HostCsr {
    int64_t m = 0, n = 0;
    const int64_t *rowptr = nullptr;
    const int32_t *col = nullptr;
    const double *val = nullptr;
};

// THE walk over a node-ordered matrix.  Per row node q (rows first(q) .. + ncomp): its coupled column nodes in ascending order, each
// with the source positions src[3 a + b] of A[comp a of q, comp b of c] (-1: absent); then its columns outside the block in
// ascending order, each with the positions src[a] in the node's rows.  Per row r behind the block rows: its column nodes with the
// positions src[b] of the components, then the position where the rest of the row (columns outside the block) starts.
// Visitor: begin_node(q), bool node_record(q, c, src[9]) (false: stop, the walk returns false), column_record(q, col, src[3]),
// end_node(q), coupling_record(r, c, src[3]), end_row(r, rest_begin).
template <class V>
bool walk_records(const HostCsr &A, const NodeOrder &o, V &&v) {
    const int64_t nbr = o.block_rows(), nnode = o.nnode();
    const int64_t *rp = A.rowptr;
    const int32_t *col = A.col;
    for (int64_t q = 0; q < nnode; ++q) {
        const int nc = o.ncomp(q);
        const int64_t rx = o.first(q);
        int64_t it[3] = {0, 0, 0}, en[3] = {0, 0, 0};
        for (int a = 0; a < nc; ++a) {
            it[a] = rp[rx + a];
            en[a] = rp[rx + a + 1];
        }
        v.begin_node(q);
        for (;;) {                                    // block columns, node by node (rows are sorted: block columns come first)
            int64_t c0 = nbr;                         // the smallest block column left in the node's rows: its node comes next
            for (int a = 0; a < nc; ++a)
                if (it[a] < en[a]) c0 = std::min<int64_t>(c0, col[it[a]]);
            if (c0 == nbr) break;
            int64_t src[9] = {-1, -1, -1, -1, -1, -1, -1, -1, -1};
            const int64_t cn = o.node_of(c0), f = o.first(cn), f1 = f + o.ncomp(cn);
            for (int a = 0; a < nc; ++a)
                while (it[a] < en[a] && col[it[a]] < f1) {
                    src[3 * a + (int)(col[it[a]] - f)] = it[a];
                    ++it[a];
                }
            if (!v.node_record(q, cn, src)) return false;
        }
        for (;;) {                                    // what is left: columns outside the block, one record per column
            int64_t mc = INT64_MAX;
            for (int a = 0; a < nc; ++a)
                if (it[a] < en[a]) mc = std::min<int64_t>(mc, col[it[a]]);
            if (mc == INT64_MAX) break;
            int64_t src[3] = {-1, -1, -1};
            for (int a = 0; a < nc; ++a)
                if (it[a] < en[a] && col[it[a]] == mc) src[a] = it[a]++;
            v.column_record(q, mc, src);
        }
        v.end_node(q);
    }
    for (int64_t r = nbr; r < A.m; ++r) {
        int64_t k = rp[r];
        while (k < rp[r + 1] && col[k] < nbr) {
            const int64_t cn = o.node_of(col[k]), f = o.first(cn), f1 = f + o.ncomp(cn);
            int64_t src[3] = {-1, -1, -1};
            for (; k < rp[r + 1] && col[k] < f1; ++k) src[col[k] - f] = k;
            v.coupling_record(r, cn, src);
        }
        v.end_row(r, k);
    }
    return true;
}

enum class PlanOutcome { accepted, not_the_structure, node_does_not_fit, row_does_not_fit };

// The {K, C} record form (npg_csr_block_nodes).  Layouts as uploaded: pkc = {K, C} per node record; gxy / gz = (a_x, a_y) pairs and
// a_z per column record; dxy / dz the same per coupling record; rowptr / col / val = the CSR remainder.  With `padded` every node's
// and every row's record list has an even length: the records beyond the unpadded length plen[q] / dlen[r] are zero records that
// repeat the list's last column node.  Without column records grow / gcol / gxy / gz are empty and the block rows keep what they
// hold outside the block in the remainder; without coupling records drow / dcol / dxy / dz are empty likewise.
struct RecordPlan {
    PlanOutcome outcome = PlanOutcome::not_the_structure;
    NodeOrder order;
    int64_t m = 0, n = 0;
    bool padded = false, colrec = false, coupling = false;
    std::vector<int64_t> prow, grow, drow, rowptr;
    std::vector<int32_t> pcol, gcol, dcol, col;
    std::vector<double> pkc, gxy, gz, dxy, dz, val;
    std::vector<int32_t> plen, dlen;            // unpadded length of node q's / row r's record list
    int64_t nrec_real = 0, ndrec_real = 0;      // records without the padding
};

// Acceptance (header of npg_csr_block_nodes, restated in tests/records_ref.py::accepts): between node q and column node c EXACTLY
// the entries x-x, x-y, y-x, y-y and - both nodes full - z-z are stored, with y-y = x-x = K, y-x = -(x-y) = -C and z-z = K within
// rtol times the largest magnitude among the block entries of q's x row.
// tile_slots: a node whose rows, or a row with coupling records that, would not fit one tile is no error: the outcome says so.
inline RecordPlan plan_block_records(const HostCsr &A, const NodeOrder &o, double rtol, const RecordSwitches &sw, int tile_slots) {
    struct Visitor {
        const HostCsr &A;
        const NodeOrder &o;
        RecordPlan &p;
        const double rtol;
        const int tile_slots;
        const bool pad;
        double tol;
        bool row_fits;              // coupling records are wanted and every row so far fits a tile with them
        int64_t outside;            // entries of the block rows outside the block columns
        double at(int64_t k) const { return k < 0 ? 0.0 : A.val[k]; }
        void begin_node(int64_t q) {
            const int64_t rx = o.first(q), nbr = o.block_rows();
            double scale = 0.0;
            for (int64_t k = A.rowptr[rx]; k < A.rowptr[rx + 1] && A.col[k] < nbr; ++k) scale = std::max(scale, std::fabs(A.val[k]));
            tol = rtol * scale;
        }
        bool node_record(int64_t q, int64_t c, const int64_t *src) {
            const bool zz = q < o.nfull && c < o.nfull;
            for (int s = 0; s < 9; ++s)
                if ((src[s] >= 0) != (s == 0 || s == 1 || s == 3 || s == 4 || (s == 8 && zz))) return false;
            const double K = A.val[src[0]], C = A.val[src[1]];
            if (std::fabs(A.val[src[4]] - K) > tol || std::fabs(A.val[src[3]] + C) > tol) return false;
            if (zz && std::fabs(A.val[src[8]] - K) > tol) return false;
            p.pcol.push_back((int32_t)c);
            p.pkc.push_back(K);
            p.pkc.push_back(C);
            return true;
        }
        void column_record(int64_t, int64_t col, const int64_t *src) {
            p.gcol.push_back((int32_t)col);
            p.gxy.push_back(at(src[0]));
            p.gxy.push_back(at(src[1]));
            p.gz.push_back(at(src[2]));
            outside += (src[0] >= 0) + (src[1] >= 0) + (src[2] >= 0);
        }
        void end_node(int64_t q) {
            const int64_t len = (int64_t)p.pcol.size() - p.prow[q];
            p.plen[q] = (int32_t)len;
            p.nrec_real += len;
            if (pad && (len & 1)) {                  // zero record on the node's last column node
                p.pcol.push_back(p.pcol.back());
                p.pkc.push_back(0.0);
                p.pkc.push_back(0.0);
            }
            p.prow[q + 1] = (int64_t)p.pcol.size();
            p.grow[q + 1] = (int64_t)p.gcol.size();
        }
        void coupling_record(int64_t, int64_t c, const int64_t *src) {
            if (!row_fits) return;
            p.dcol.push_back((int32_t)c);
            p.dxy.push_back(at(src[0]));
            p.dxy.push_back(at(src[1]));
            p.dz.push_back(at(src[2]));
        }
        void end_row(int64_t r, int64_t rest) {
            if (!row_fits) return;
            const int64_t i = r - o.block_rows();
            int64_t len = (int64_t)p.dcol.size() - p.drow[i];
            p.dlen[i] = (int32_t)len;
            p.ndrec_real += len;
            if (pad && (len & 1)) {                  // zero record on the row's last column node (windowed tiles take records in pairs)
                p.dcol.push_back(p.dcol.back());
                p.dxy.push_back(0.0);
                p.dxy.push_back(0.0);
                p.dz.push_back(0.0);
                ++len;
            }
            p.drow[i + 1] = (int64_t)p.dcol.size();
            if (len + (A.rowptr[r + 1] - rest) > tile_slots) row_fits = false;
        }
    };
    RecordPlan p;
    p.order = o;
    p.m = A.m;
    p.n = A.n;
    p.padded = sw.window;
    const int64_t nnode = o.nnode(), nbr = o.block_rows(), nnz = A.rowptr[A.m];
    p.prow.assign((size_t)nnode + 1, 0);
    p.grow.assign((size_t)nnode + 1, 0);
    p.plen.assign((size_t)nnode, 0);
    p.drow.assign((size_t)(A.m - nbr) + 1, 0);
    p.dlen.assign((size_t)(A.m - nbr), 0);
    p.pcol.reserve((size_t)nnz / 5);
    p.pkc.reserve((size_t)nnz / 5 * 2);
    Visitor v{A, o, p, rtol, tile_slots, sw.window, 0.0, sw.coupling, 0};
    if (!walk_records(A, o, v)) return p;
    // column records pay when they replace more than 28 / 12 entries each
    p.colrec = sw.column_records && !p.gcol.empty() && 28 * (int64_t)p.gcol.size() <= 12 * v.outside;
    if (!p.colrec) {
        p.grow.clear();
        p.gcol.clear();
        p.gxy.clear();
        p.gz.clear();
    }
    // rows behind the block rows: coupling records unless switched off, or a row would not fit a tile that way, or there are none
    p.coupling = A.m > nbr && v.row_fits && !p.dcol.empty();
    if (!p.coupling) {
        p.drow.clear();
        p.dlen.clear();
        p.dcol.clear();
        p.dxy.clear();
        p.dz.clear();
        p.ndrec_real = 0;
    }
    // the CSR remainder: what the block rows hold outside the block (without column records), what the rows behind them hold
    // outside the block columns (with coupling records) or altogether
    p.rowptr.assign((size_t)A.m + 1, 0);
    p.col.reserve((size_t)nnz / 2);
    p.val.reserve((size_t)nnz / 2);
    for (int64_t r = 0; r < A.m; ++r) {
        const bool skip_block = r < nbr || p.coupling;
        if (!(r < nbr && p.colrec))
            for (int64_t k = A.rowptr[r]; k < A.rowptr[r + 1]; ++k) {
                if (skip_block && A.col[k] < nbr) continue;
                p.col.push_back(A.col[k]);
                p.val.push_back(A.val[k]);
            }
        p.rowptr[r + 1] = (int64_t)p.col.size();
    }
    // the rows of one node share a tile: records (one product slot per component) + what they keep in the remainder
    for (int64_t q = 0; q < nnode; ++q) {
        const int64_t rx = o.first(q);
        const int64_t slots = p.rowptr[rx + o.ncomp(q)] - p.rowptr[rx] +
                              o.ncomp(q) * (p.prow[q + 1] - p.prow[q] + (p.colrec ? p.grow[q + 1] - p.grow[q] : 0));
        if (slots > tile_slots) {
            p.outcome = PlanOutcome::node_does_not_fit;
            return p;
        }
    }
    p.outcome = PlanOutcome::accepted;
    return p;
}

// FULL node records (npg_csr_pack_nodes): the same split carrying source positions in the stream layouts of pk9 / gval / dval / val
// - map9: (a_2k, a_2k+1) pairs as four 16-byte streams, a_8 as one 8-byte stream; mapg / mapd: [2 n] pairs, then [n] third values.
struct PackPlan {
    PlanOutcome outcome = PlanOutcome::accepted;
    std::vector<int64_t> prow, grow, drow, rowptr;
    std::vector<int32_t> pcol, gcol, dcol, col;
    std::vector<int64_t> map9, mapg, mapd, maprem;
};

inline PackPlan plan_full_records(const HostCsr &A, const NodeOrder &o, int tile_slots) {
    struct Visitor {
        const HostCsr &A;
        const NodeOrder &o;
        PackPlan &p;
        const int tile_slots;
        std::vector<int64_t> m9, mg3, md3;          // source positions, record-major (re-laid below)
        void begin_node(int64_t) {}
        bool node_record(int64_t, int64_t c, const int64_t *src) {
            p.pcol.push_back((int32_t)c);
            m9.insert(m9.end(), src, src + 9);
            return true;
        }
        void column_record(int64_t, int64_t col, const int64_t *src) {
            p.gcol.push_back((int32_t)col);
            mg3.insert(mg3.end(), src, src + 3);
        }
        void end_node(int64_t q) {
            p.prow[q + 1] = (int64_t)p.pcol.size();
            p.grow[q + 1] = (int64_t)p.gcol.size();
            if (o.ncomp(q) * ((p.prow[q + 1] - p.prow[q]) + (p.grow[q + 1] - p.grow[q])) > tile_slots) p.outcome = PlanOutcome::node_does_not_fit;
        }
        void coupling_record(int64_t, int64_t c, const int64_t *src) {
            p.dcol.push_back((int32_t)c);
            md3.insert(md3.end(), src, src + 3);
        }
        void end_row(int64_t r, int64_t rest) {
            const int64_t i = r - o.block_rows();
            p.drow[i + 1] = (int64_t)p.dcol.size();
            for (int64_t k = rest; k < A.rowptr[r + 1]; ++k) {
                p.col.push_back(A.col[k]);
                p.maprem.push_back(k);
            }
            p.rowptr[r + 1] = (int64_t)p.col.size();
            if ((p.drow[i + 1] - p.drow[i]) + (A.rowptr[r + 1] - rest) > tile_slots) p.outcome = PlanOutcome::row_does_not_fit;
        }
    };
    PackPlan p;
    const int64_t nnode = o.nnode(), nbr = o.block_rows();
    p.prow.assign((size_t)nnode + 1, 0);
    p.grow.assign((size_t)nnode + 1, 0);
    p.drow.assign((size_t)(A.m - nbr) + 1, 0);
    p.rowptr.assign((size_t)A.m + 1, 0);
    Visitor v{A, o, p, tile_slots, {}, {}, {}};
    walk_records(A, o, v);
    if (p.outcome != PlanOutcome::accepted) return p;
    const int64_t n9 = (int64_t)p.pcol.size(), ng = (int64_t)p.gcol.size(), nd = (int64_t)p.dcol.size();
    p.map9.resize((size_t)9 * n9);
    p.mapg.resize((size_t)3 * ng);
    p.mapd.resize((size_t)3 * nd);
    for (int64_t e = 0; e < n9; ++e) {
        for (int s9 = 0; s9 < 8; ++s9) p.map9[(size_t)(s9 & ~1) * n9 + 2 * e + (s9 & 1)] = v.m9[(size_t)9 * e + s9];
        p.map9[(size_t)8 * n9 + e] = v.m9[(size_t)9 * e + 8];
    }
    for (int64_t e = 0; e < ng; ++e) {
        p.mapg[2 * e] = v.mg3[3 * e];
        p.mapg[2 * e + 1] = v.mg3[3 * e + 1];
        p.mapg[2 * ng + e] = v.mg3[3 * e + 2];
    }
    for (int64_t e = 0; e < nd; ++e) {
        p.mapd[2 * e] = v.md3[3 * e];
        p.mapd[2 * e + 1] = v.md3[3 * e + 1];
        p.mapd[2 * nd + e] = v.md3[3 * e + 2];
    }
    return p;
}

// ---- ordinary tiles ---------------------------------------------------------------------------------------------------------------
// one tile on the host: the fields of TileDesc / WTileDesc (common.h)
struct PlanTile {
    int64_t base = 0, pbase = 0;
    int32_t r0 = 0, nrows = 0, n = 0, npe = 0;
    int32_t woff = 0, voff = 0, nw = 0, nv = 0;
};

// what tile_boundaries reads of a matrix: remainder row offsets and the record offsets (null: no such records)
struct TileInput {
    int64_t m = 0;
    NodeOrder order;
    const int64_t *rowptr = nullptr, *prow = nullptr, *grow = nullptr, *drow = nullptr;
    int num_cu = 1;
};

// Row tiles for the CSR-stream kernels: consecutive whole rows (whole nodes in the block rows), at most tile_slots LDS product
// slots and max_rows rows per tile; small matrices get about one tile per CU.  accepted, or which kind of row did not fit.
inline PlanOutcome plan_tile_boundaries(const TileInput &A, int tile_slots, int max_rows, int tile_rows, std::vector<int32_t> &tp) {
    const int64_t m = A.m;
    const NodeOrder &o = A.order;
    const int64_t *rp = A.rowptr, *pp = o.nnode() ? A.prow : nullptr, *dp = A.drow, *gp = A.grow;
    const int64_t nf3 = 3 * o.nfull, nbr = o.block_rows();
    const int64_t slots_total = rp[m] + (pp ? 3 * pp[o.nfull] + 2 * (pp[o.nnode()] - pp[o.nfull]) : 0) + (dp ? dp[m - nbr] : 0) +
                                (gp ? 3 * gp[o.nfull] + 2 * (gp[o.nnode()] - gp[o.nfull]) : 0);
    int64_t target = slots_total / (int64_t)A.num_cu;
    target = std::min<int64_t>(tile_slots, std::max<int64_t>(1024, target)); // >= 1 tile per CU on small matrices
    // LDS product slots of rows [a, b): their CSR entries + one per component per record (a, b on node boundaries of
    // one kind inside the block rows)
    auto slots = [&](int64_t a, int64_t b) {
        int64_t s = rp[b] - rp[a];
        if (pp && a < nbr) s += (a < nf3 ? 3 : 2) * (pp[o.node_of(b)] - pp[o.node_of(a)]);
        if (gp && a < nbr) s += (a < nf3 ? 3 : 2) * (gp[o.node_of(b)] - gp[o.node_of(a)]);
        if (dp && a >= nbr) s += dp[b - nbr] - dp[a - nbr];
        return s;
    };
    const int64_t max_rows_rec = std::min<int64_t>(max_rows, tile_rows / 2);      // TileLds::prp
    tp.clear();
    tp.push_back(0);
    int64_t r = 0;
    while (r < m) {
        const bool inblk = r < nbr;
        const int64_t step = !inblk ? 1 : (r < nf3 ? 3 : 2), lim = !inblk ? m : (r < nf3 ? nf3 : nbr);
        int64_t r1 = r + step;
        const int64_t mr = (!inblk && dp) ? max_rows_rec : max_rows;
        while (r1 < lim && r1 + step - r <= mr && slots(r, r1 + step) <= target) r1 += step;
        if (inblk && slots(r, r1) > tile_slots) return PlanOutcome::node_does_not_fit;
        if (!inblk && dp && slots(r, r1) > tile_slots) return PlanOutcome::row_does_not_fit;
        tp.push_back((int32_t)r1);
        r = r1;
    }
    return PlanOutcome::accepted;
}

// the descriptors of the tiles tp[t] .. tp[t + 1]: (base, n) = a tile's CSR entries or - block rows with column records - its column
// records; (pbase, npe) = its node records or - rows behind the block rows - its coupling records
inline std::vector<PlanTile> plan_tiles(const TileInput &A, const std::vector<int32_t> &tp) {
    const NodeOrder &o = A.order;
    const int64_t nbr = o.block_rows();
    std::vector<PlanTile> td(tp.size() - 1);
    for (size_t t = 0; t + 1 < tp.size(); ++t) {
        const int64_t r0 = tp[t], r1 = tp[t + 1];
        PlanTile &q = td[t];
        q.r0 = (int32_t)r0;
        q.nrows = (int32_t)(r1 - r0);
        q.base = A.rowptr[r0];
        q.n = (int32_t)(A.rowptr[r1] - A.rowptr[r0]);
        if (r0 < nbr) {
            q.pbase = A.prow[o.node_of(r0)];
            q.npe = (int32_t)(A.prow[o.node_of(r1)] - q.pbase);
            if (A.grow) {
                q.base = A.grow[o.node_of(r0)];
                q.n = (int32_t)(A.grow[o.node_of(r1)] - q.base);
            }
        } else if (A.drow) {
            q.pbase = A.drow[r0 - nbr];
            q.npe = (int32_t)(A.drow[r1 - nbr] - q.pbase);
        }
    }
    return td;
}

// ---- the windowed tile set (spmv_window.h) ------------------------------------------------------------------------------------------
// A second tiling of the block rows whose tiles are sized by what they need in LDS - pair-summed products, column-record products,
// the window of distinct column nodes (16 B each) and of distinct other columns (4 B each) - followed by the tiles of the rows
// behind the block rows: windowed too where all they hold is coupling records, else the ordinary tiles.
struct GhostNodes {            // npg_csr_set_ghost_nodes: ghost columns [col[g], col[g] + ncomp[g]) are ONE node of a neighbour
    std::vector<int32_t> col, ncomp;
    int64_t count() const { return (int64_t)col.size(); }
};

struct WindowPlan {
    bool present = false;       // false: the matrix gets no windowed set (an ordinary outcome: some node's rows fit no windowed tile)
    bool overflow = false;      // the window lists exceed int32 offsets (an error)
    std::vector<PlanTile> tiles;            // final order: per pass (without / with ghost columns) block tiles and tiles of the other rows
    int32_t ninterior = 0, nrow_tiles = 0, wlanes = 8;
    std::vector<uint16_t> widx, gidx, dwidx;        // window index of every node / column / coupling record of the set
    std::vector<int32_t> wlist, vlist;              // per-tile lists of distinct column nodes / other columns (vlist ends in a sentinel)
    std::vector<int32_t> wbk, dbk;                  // tile-local end offsets: [nnode][2] column records / record pairs; pairs per row behind
    std::vector<double> pkc2, dxy2;                 // {K, C} / (d_x, d_y) split by position in the record pair: [pairs] firsts, [pairs] seconds
    int64_t npairs = 0, ndpairs = 0;
    bool own = false, rows_own = false;             // ghost nodes were converted: the set has its own column-record values / d_z
    std::vector<double> wgval, wdz;                 // [2 nw_grec] (a_x, a_y), [nw_grec] a_z ; d_z of the set's own coupling records
    std::vector<int32_t> gslot;                     // per ghost column: float position of its node slot in the gather-layout copy, -1
    int64_t nw_rec = 0, nw_grec = 0, nw_drec = 0;   // padded node records, column records, padded coupling records of the set
    // the set's own record lists where ghost nodes were converted (own: block rows; rows_own: rows behind them), else the plan's;
    // the offsets and columns are not uploaded (the tiles and window indices stand for them)
    std::vector<int64_t> prow, grow, drow;
    std::vector<int32_t> pcol, gcol, dcol;
};

namespace winplan {

// stage 1: the block rows' records of the set - the plan's, or (ghost nodes) its own lists in which the column records of a row
// node on the components of ONE ghost node that carry the {K, C} structure (A[x_q,x_c] = A[y_q,y_c] = A[z_q,z_c] = K,
// A[x_q,y_c] = -A[y_q,x_c] = C, nothing else, within 1e-12 of the node's largest |K|) are a node record with column node nnode + g
struct BlockRecords {
    bool own = false;
    std::vector<int64_t> prow, grow;
    std::vector<int32_t> pcol, gcol;
    std::vector<double> pkc, gxy, gz;
    std::vector<int32_t> gnode, gcomp;        // per ghost column: its ghost node (-1: none) and component
};

inline BlockRecords convert_ghost_nodes(const RecordPlan &P, const GhostNodes &gn) {
    BlockRecords b;
    const NodeOrder &o = P.order;
    const int64_t nnode = o.nnode(), m = P.m;
    b.gnode.assign((size_t)std::max<int64_t>(P.n - m, 0), -1);
    b.gcomp.assign(b.gnode.size(), 0);
    if (gn.count() == 0) return b;
    for (int64_t g = 0; g < gn.count(); ++g)
        for (int a = 0; a < gn.ncomp[(size_t)g]; ++a) {
            b.gnode[(size_t)(gn.col[(size_t)g] - m + a)] = (int32_t)g;
            b.gcomp[(size_t)(gn.col[(size_t)g] - m + a)] = a;
        }
    b.prow.assign((size_t)nnode + 1, 0);
    b.grow.assign((size_t)nnode + 1, 0);
    int64_t converted = 0;
    auto keep = [&](int64_t e) {
        b.gcol.push_back(P.gcol[e]);
        b.gxy.push_back(P.gxy[2 * e]);
        b.gxy.push_back(P.gxy[2 * e + 1]);
        b.gz.push_back(P.gz[e]);
    };
    for (int64_t q = 0; q < nnode; ++q) {
        const bool qfull = q < o.nfull;
        const int64_t pe = P.prow[q] + P.plen[q];            // the node's own records, without the padding (re-made below)
        double scale_q = 0.0;
        for (int64_t e = P.prow[q]; e < pe; ++e) {
            b.pcol.push_back(P.pcol[e]);
            b.pkc.push_back(P.pkc[2 * e]);
            b.pkc.push_back(P.pkc[2 * e + 1]);
            scale_q = std::max(scale_q, std::fabs(P.pkc[2 * e]));
        }
        const double tol = 1e-12 * scale_q;
        // column records, ascending columns: the components of a ghost node are adjacent
        for (int64_t e = P.grow[q]; e < P.grow[q + 1];) {
            const int64_t m0 = P.gcol[e];
            const int32_t g = m0 >= m ? b.gnode[(size_t)(m0 - m)] : -1;
            if (g < 0 || b.gcomp[(size_t)(m0 - m)] != 0) {
                keep(e++);
                continue;
            }
            // the node pair's table t[3 a + c] = A[comp a of q, comp c of the ghost node] (absent: 0) from the records of columns
            // m0 (x), m0 + 1 (y)[, m0 + 2 (z)]
            const int nc = gn.ncomp[(size_t)g];
            double t[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            int64_t e1 = e;
            for (; e1 < P.grow[q + 1] && P.gcol[e1] < m0 + nc; ++e1) {
                const int c = (int)(P.gcol[e1] - m0);
                t[c] = P.gxy[2 * e1];
                t[3 + c] = P.gxy[2 * e1 + 1];
                t[6 + c] = P.gz[e1];
            }
            const double K = t[0], C = t[1];
            bool ok = std::fabs(t[4] - K) <= tol && std::fabs(t[3] + C) <= tol && std::fabs(t[6]) <= tol && std::fabs(t[7]) <= tol;
            if (nc == 3) ok = ok && std::fabs(t[2]) <= tol && std::fabs(t[5]) <= tol && (!qfull || std::fabs(t[8] - K) <= tol);
            if (ok) {
                b.pcol.push_back((int32_t)(nnode + g));
                b.pkc.push_back(K);
                b.pkc.push_back(C);
                ++converted;
            } else {
                for (int64_t k = e; k < e1; ++k) keep(k);
            }
            e = e1;
        }
        if (((int64_t)b.pcol.size() - b.prow[q]) & 1) {            // zero record on the node's last column node
            b.pcol.push_back(b.pcol.back());
            b.pkc.push_back(0.0);
            b.pkc.push_back(0.0);
        }
        b.prow[q + 1] = (int64_t)b.pcol.size();
        b.grow[q + 1] = (int64_t)b.gcol.size();
    }
    b.own = converted > 0;
    return b;
}

// the limits every stage shares
struct Limits {
    int NT = 512;
    int64_t hard = 0, soft = 0, cap_p = 0, cap_c = 0, total = 0;
};

// the record lists a stage tiles: offsets and column (node) of every record
struct Lists {
    const std::vector<int64_t> &prow, &grow;
    const std::vector<int32_t> &pcol, &gcol;
};

// per-tile distinct columns by stamps: stamp[c] == T while tile T is open and holds c; pos[c] = its index in the tile's sorted list
struct Stamps {
    std::vector<int32_t> stampW, stampV, posW, posV;
};

// stage 2: the block tiles - greedy growth node by node under the LDS caps.  false: no windowed set.
inline bool block_tiles(const NodeOrder &o, int64_t m, const Lists &L, const Limits &lim, const RecordCaps &caps, Stamps &st, WindowPlan &w,
                        std::vector<PlanTile> &blk, std::vector<char> &ghost) {
    const int64_t nnode = o.nnode(), nfull = o.nfull;
    const int NT = lim.NT;
    const std::vector<int64_t> &prow = L.prow, &grow = L.grow;
    const std::vector<int32_t> &pcol = L.pcol, &gcol = L.gcol;
    w.widx.assign(pcol.size(), 0);
    w.gidx.assign(gcol.size(), 0);
    w.wbk.assign((size_t)2 * nnode, 0);
    std::vector<int32_t> tw, tv, nwl, nvl;
    auto bytes_of = [](int ncomp, int64_t np, int64_t ng, int64_t nw, int64_t nv) {
        const int64_t slots = ncomp * (np + ng);
        return 8 * ((slots + 1) & ~(int64_t)1) + 16 * nw + 4 * nv;
    };
    for (int kind = 0; kind < 2; ++kind) {
        const int64_t lo = kind ? nfull : 0, hi = kind ? nnode : nfull;
        const int ncomp = kind ? 2 : 3;
        int64_t q = lo;
        while (q < hi) {
            const int32_t T = (int32_t)blk.size();
            tw.clear();
            tv.clear();
            int64_t np = 0, ng = 0, qe = q;
            while (qe < hi) {
                nwl.clear();
                nvl.clear();
                for (int64_t e = prow[qe]; e < prow[qe + 1]; ++e)
                    if (st.stampW[pcol[e]] != T) {
                        st.stampW[pcol[e]] = T;
                        nwl.push_back(pcol[e]);
                    }
                for (int64_t e = grow[qe]; e < grow[qe + 1]; ++e)
                    if (st.stampV[gcol[e]] != T) {
                        st.stampV[gcol[e]] = T;
                        nvl.push_back(gcol[e]);
                    }
                const int64_t np2 = np + (prow[qe + 1] - prow[qe]) / 2, ng2 = ng + (grow[qe + 1] - grow[qe]);
                const int64_t nw2 = (int64_t)(tw.size() + nwl.size()), nv2 = (int64_t)(tv.size() + nvl.size());
                const int64_t by = bytes_of(ncomp, np2, ng2, nw2, nv2);
                const bool shape = (qe + 1 - q) * ncomp <= caps.tile_rows && np2 <= lim.cap_p && ng2 <= lim.cap_c &&
                                   nw2 <= (int64_t)caps.win_nodes * NT && nv2 <= NT;
                if (qe == q && !(shape && by <= lim.hard)) return false;       // one node's rows do not fit: no windowed set
                if (qe > q && !(shape && by <= lim.soft)) {
                    for (int32_t c : nwl) st.stampW[c] = -1;
                    for (int32_t c : nvl) st.stampV[c] = -1;
                    break;
                }
                tw.insert(tw.end(), nwl.begin(), nwl.end());
                tv.insert(tv.end(), nvl.begin(), nvl.end());
                np = np2;
                ng = ng2;
                ++qe;
            }
            std::sort(tw.begin(), tw.end());
            std::sort(tv.begin(), tv.end());
            for (size_t i = 0; i < tw.size(); ++i) st.posW[tw[i]] = (int32_t)i;
            for (size_t i = 0; i < tv.size(); ++i) st.posV[tv[i]] = (int32_t)i;
            for (int64_t e = prow[q]; e < prow[qe]; ++e) w.widx[e] = (uint16_t)st.posW[pcol[e]];
            for (int64_t e = grow[q]; e < grow[qe]; ++e) w.gidx[e] = (uint16_t)st.posV[gcol[e]];
            for (int64_t k = q; k < qe; ++k) {
                w.wbk[2 * k] = (int32_t)(grow[k + 1] - grow[q]);
                w.wbk[2 * k + 1] = (int32_t)((prow[k + 1] - prow[q]) >> 1);
            }
            PlanTile d;
            d.r0 = (int32_t)o.first(q);
            d.nrows = (int32_t)((qe - q) * ncomp);
            d.base = grow[q];
            d.n = (int32_t)ng;
            d.pbase = prow[q];
            d.npe = (int32_t)(2 * np);
            d.woff = (int32_t)w.wlist.size();
            d.nw = (int32_t)tw.size();
            d.voff = (int32_t)w.vlist.size();
            d.nv = (int32_t)tv.size();
            if (d.nw == 0) return false;        // a tile of nodes without any entry in the block columns: no windowed set
            w.wlist.insert(w.wlist.end(), tw.begin(), tw.end());
            w.vlist.insert(w.vlist.end(), tv.begin(), tv.end());
            blk.push_back(d);
            ghost.push_back((!tv.empty() && tv.back() >= m) || tw.back() >= nnode);   // (ghost columns; ghost nodes as record columns)
            q = qe;
        }
    }
    return true;
}

// stage 3a: a rank's row block with ghost nodes - what the rows behind the block rows hold on ghost columns is CSR remainder for
// the ordinary tiles; for THIS tile set the entries on a ghost node's components become one coupling record {nnode + g, d_x, d_y,
// d_z} behind the row's owned-node records.  false: some remaining entry is no node component (ordinary tiles for these rows).
struct RowRecords {
    std::vector<int64_t> drow;
    std::vector<int32_t> dcol;
    std::vector<double> dxy, dz;
};

inline bool convert_ghost_rows(const RecordPlan &P, const BlockRecords &b, RowRecords &rr) {
    const int64_t nbr = P.order.block_rows(), nnode = P.order.nnode(), nbehind = P.m - nbr, m = P.m;
    rr.drow.assign((size_t)nbehind + 1, 0);
    for (int64_t r = 0; r < nbehind; ++r) {
        for (int64_t e = P.drow[r]; e < P.drow[r] + P.dlen[r]; ++e) {          // (without the padding: re-made below)
            rr.dcol.push_back(P.dcol[e]);
            rr.dxy.push_back(P.dxy[2 * e]);
            rr.dxy.push_back(P.dxy[2 * e + 1]);
            rr.dz.push_back(P.dz[e]);
        }
        int32_t cur = -1;
        for (int64_t k = P.rowptr[nbr + r]; k < P.rowptr[nbr + r + 1]; ++k) {
            const int64_t m0 = P.col[k];
            const int32_t g = m0 >= m ? b.gnode[(size_t)(m0 - m)] : -1;
            if (g < 0) return false;
            if (g != cur) {
                rr.dcol.push_back((int32_t)(nnode + g));
                rr.dxy.push_back(0.0);
                rr.dxy.push_back(0.0);
                rr.dz.push_back(0.0);
                cur = g;
            }
            const int a = b.gcomp[(size_t)(m0 - m)];
            if (a == 2) rr.dz.back() = P.val[k];
            else rr.dxy[rr.dxy.size() - 2 + a] = P.val[k];
        }
        if (((int64_t)rr.dcol.size() - rr.drow[r]) & 1) {
            rr.dcol.push_back(rr.dcol.back());
            rr.dxy.push_back(0.0);
            rr.dxy.push_back(0.0);
            rr.dz.push_back(0.0);
        }
        rr.drow[r + 1] = (int64_t)rr.dcol.size();
    }
    return true;
}

// stage 3b: the rows behind the block rows (the divergence rows) as windowed tiles - two adjacent records of a row per lane, at
// most win_pairs pairs per lane and win_nodes distinct column nodes per lane: small tiles, one dependent chain each.
// Leaves rowt empty (and the lists as they were) when some row does not fit or a run of rows names no column node.
inline void row_tiles(int64_t nbr, int64_t nnode, const std::vector<int64_t> &drow, const std::vector<int32_t> &dcol, const Limits &lim,
                      const RecordCaps &caps, size_t nblk, Stamps &st, WindowPlan &w, std::vector<PlanTile> &rowt, std::vector<char> &rghost) {
    const int64_t nbehind = (int64_t)drow.size() - 1;
    const int NT = lim.NT;
    w.dwidx.assign(dcol.size(), 0);
    w.dbk.assign((size_t)nbehind, 0);
    int64_t cap_pairs = lim.cap_p;
    {       // small matrices: about as many tiles as the block rows got per byte
        const int64_t want = std::max<int64_t>(1, (int64_t)nblk * (drow[nbehind] * 28) / std::max<int64_t>(1, lim.total * 3));
        cap_pairs = std::min<int64_t>(cap_pairs, std::max<int64_t>(64, drow[nbehind] / 2 / want));
    }
    std::vector<int32_t> tw, nwl;
    int64_t r = 0;
    bool ok = true;
    const size_t wlist_blk = w.wlist.size();
    while (r < nbehind && ok) {
        const int32_t T = (int32_t)(nblk + rowt.size());
        tw.clear();
        int64_t np = 0, re = r;
        while (re < nbehind) {
            nwl.clear();
            for (int64_t e = drow[re]; e < drow[re + 1]; ++e)
                if (st.stampW[dcol[e]] != T) {
                    st.stampW[dcol[e]] = T;
                    nwl.push_back(dcol[e]);
                }
            const int64_t np2 = np + (drow[re + 1] - drow[re]) / 2, nw2 = (int64_t)(tw.size() + nwl.size());
            const bool hardfit = re + 1 - r <= caps.tile_rows / 2 && np2 <= (int64_t)caps.win_pairs * NT && nw2 <= (int64_t)caps.win_nodes * NT &&
                                 8 * ((np2 + 1) & ~(int64_t)1) + 16 * nw2 <= lim.hard;
            if (re == r && !hardfit) {
                ok = false;
                break;
            }
            if (re > r && !(hardfit && np2 <= cap_pairs)) {
                for (int32_t c : nwl) st.stampW[c] = -1;
                break;
            }
            tw.insert(tw.end(), nwl.begin(), nwl.end());
            np = np2;
            ++re;
        }
        if (!ok) break;
        std::sort(tw.begin(), tw.end());
        for (size_t i = 0; i < tw.size(); ++i) st.posW[tw[i]] = (int32_t)i;
        for (int64_t e = drow[r]; e < drow[re]; ++e) w.dwidx[e] = (uint16_t)st.posW[dcol[e]];
        for (int64_t k = r; k < re; ++k) w.dbk[k] = (int32_t)((drow[k + 1] - drow[r]) >> 1);
        PlanTile d;
        d.r0 = (int32_t)(nbr + r);
        d.nrows = (int32_t)(re - r);
        d.pbase = drow[r];
        d.npe = (int32_t)(2 * np);
        d.woff = (int32_t)w.wlist.size();
        d.nw = (int32_t)tw.size();
        d.voff = (int32_t)w.vlist.size();
        if (d.nw == 0) {            // (a block of empty rows: nothing to window)
            ok = false;
            break;
        }
        w.wlist.insert(w.wlist.end(), tw.begin(), tw.end());
        rowt.push_back(d);
        rghost.push_back(tw.back() >= nnode);
        r = re;
    }
    if (!ok) {          // (ordinary tiles for these rows: the lists of the row tiles made so far go with them)
        rowt.clear();
        rghost.clear();
        w.wlist.resize(wlist_blk);
    }
}

// stage 4: the final order.  Per pass (tiles without / with ghost columns): a = block tiles, b = tiles of the rows behind them -
// windowed (rowt), or the ordinary ones as build_tiles made and ordered them.  order 0 = a then b; 1 = b then a; 2 = b spread
// evenly among a.
inline void order_tiles(const std::vector<PlanTile> &blk, const std::vector<char> &ghost, const std::vector<PlanTile> &rowt,
                        const std::vector<char> &rghost, const std::vector<PlanTile> &ordinary, int32_t ordinary_interior, int64_t nbr,
                        int order, WindowPlan &w) {
    w.tiles.reserve(blk.size() + ordinary.size() + rowt.size());
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<PlanTile> a, b;
        for (size_t t = 0; t < blk.size(); ++t)
            if ((ghost[t] != 0) == (pass == 1)) a.push_back(blk[t]);
        if (!rowt.empty()) {
            for (size_t t = 0; t < rowt.size(); ++t)
                if ((rghost[t] != 0) == (pass == 1)) b.push_back(rowt[t]);
        } else {
            for (size_t t = 0; t < ordinary.size(); ++t)
                if (ordinary[t].r0 >= nbr && ((int32_t)t >= ordinary_interior) == (pass == 1)) b.push_back(ordinary[t]);
        }
        if (order == 1) {
            w.tiles.insert(w.tiles.end(), b.begin(), b.end());
            w.tiles.insert(w.tiles.end(), a.begin(), a.end());
        } else if (order == 2 && !b.empty()) {
            size_t ib = 0;
            for (size_t ia = 0; ia < a.size(); ++ia) {
                while (ib < b.size() && ib * a.size() <= ia * b.size()) w.tiles.push_back(b[ib++]);
                w.tiles.push_back(a[ia]);
            }
            while (ib < b.size()) w.tiles.push_back(b[ib++]);
        } else {
            w.tiles.insert(w.tiles.end(), a.begin(), a.end());
            w.tiles.insert(w.tiles.end(), b.begin(), b.end());
        }
        if (pass == 0) w.ninterior = (int32_t)w.tiles.size();
    }
}

// values of a record list split by position in the record pair: [pairs] firsts, then [pairs] seconds - a lane's two 16-byte loads
// are then each part of a fully contiguous stream (the interleaved list gives 32-byte strides)
inline std::vector<double> split_pairs(const std::vector<double> &v2, size_t nrec) {
    const size_t P = nrec / 2;
    std::vector<double> s(4 * P);
    for (size_t pr = 0; pr < P; ++pr) {
        s[2 * pr] = v2[4 * pr];
        s[2 * pr + 1] = v2[4 * pr + 1];
        s[2 * P + 2 * pr] = v2[4 * pr + 2];
        s[2 * P + 2 * pr + 1] = v2[4 * pr + 3];
    }
    return s;
}

}  // namespace winplan

// ordinary: the matrix's ordinary tiles in their final order (their first ordinary_interior read no ghost column)
inline WindowPlan plan_window_tiles(const RecordPlan &P, const GhostNodes &gn, int num_cu, const std::vector<PlanTile> &ordinary,
                                    int32_t ordinary_interior, const RecordSwitches &sw, const RecordCaps &caps = RecordCaps()) {
    using namespace winplan;
    WindowPlan w;
    const NodeOrder &o = P.order;
    const int64_t nnode = o.nnode(), nfull = o.nfull, nbr = o.block_rows(), nbehind = P.m - nbr;
    if (nnode == 0 || !P.colrec || !P.padded) return w;
    BlockRecords b = convert_ghost_nodes(P, gn);
    w.own = b.own;
    const Lists L{b.own ? b.prow : P.prow, b.own ? b.grow : P.grow, b.own ? b.pcol : P.pcol, b.own ? b.gcol : P.gcol};
    const std::vector<double> &pkc = b.own ? b.pkc : P.pkc;
    const int64_t nwin_nodes = nnode + (b.own ? gn.count() : 0);
    Limits lim;
    lim.NT = caps.win_threads;
    lim.hard = 8 * (int64_t)caps.tile_slots;
    if (sw.win_bytes) lim.hard = std::min<int64_t>(lim.hard, sw.win_bytes);    // tuning: smaller tiles
    const double scale = std::min(1.0, std::max(0.25, sw.win_scale));       // all caps of a tile scaled
    lim.hard = (int64_t)(scale * (double)lim.hard);
    lim.cap_p = (int64_t)(scale * caps.win_pairs * lim.NT);
    lim.cap_c = (int64_t)(scale * caps.win_cols * lim.NT);
    // small matrices: about one tile per CU (as plan_tile_boundaries does)
    lim.total = 8 * (3 * (L.prow[nfull] / 2 + L.grow[nfull]) + 2 * ((L.prow[nnode] - L.prow[nfull]) / 2 + L.grow[nnode] - L.grow[nfull]));
    lim.soft = std::min<int64_t>(lim.hard, std::max<int64_t>(8 * 1024, lim.total / std::max(1, num_cu)));
    Stamps st;
    st.stampW.assign((size_t)nwin_nodes, -1);
    st.posW.assign((size_t)nwin_nodes, 0);
    st.stampV.assign((size_t)P.n, -1);
    st.posV.assign((size_t)P.n, 0);
    std::vector<PlanTile> blk, rowt;
    std::vector<char> ghost, rghost;
    if (!block_tiles(o, P.m, L, lim, caps, st, w, blk, ghost)) return WindowPlan();
    RowRecords rr;
    w.rows_own = b.own && sw.win_rows && P.coupling && nbehind > 0 && P.n > P.m && convert_ghost_rows(P, b, rr);
    const std::vector<int64_t> &drow = w.rows_own ? rr.drow : P.drow;
    const std::vector<int32_t> &dcol = w.rows_own ? rr.dcol : P.dcol;
    const std::vector<double> &dxy = w.rows_own ? rr.dxy : P.dxy;
    if (sw.win_rows && P.coupling && nbehind > 0 && ((P.rowptr[P.m] - P.rowptr[nbr] == 0 && P.n == P.m) || w.rows_own))
        row_tiles(nbr, nnode, drow, dcol, lim, caps, blk.size(), st, w, rowt, rghost);
    w.vlist.push_back((int32_t)nbr);           // sentinel: a tile without such columns still reads one entry at its offset
    if (!(w.wlist.size() < (size_t)INT32_MAX && w.vlist.size() < (size_t)INT32_MAX)) {
        w.overflow = true;
        return w;
    }
    order_tiles(blk, ghost, rowt, rghost, ordinary, ordinary_interior, nbr, sw.win_order, w);
    w.pkc2 = split_pairs(pkc, L.pcol.size());
    w.npairs = (int64_t)(L.pcol.size() / 2);
    w.nrow_tiles = (int32_t)rowt.size();
    if (!rowt.empty()) {
        w.dxy2 = split_pairs(dxy, dcol.size());
        w.ndpairs = (int64_t)(dcol.size() / 2);
        w.nw_drec = (int64_t)dcol.size();
        if (w.rows_own) {
            w.wdz = std::move(rr.dz);
            w.drow = std::move(rr.drow);
            w.dcol = std::move(rr.dcol);
        }
    } else {
        w.dwidx.clear();
        w.dbk.clear();
        w.rows_own = false;
    }
    if (b.own) {
        w.wgval.resize(3 * b.gz.size());
        std::copy(b.gxy.begin(), b.gxy.end(), w.wgval.begin());
        std::copy(b.gz.begin(), b.gz.end(), w.wgval.begin() + (std::ptrdiff_t)b.gxy.size());
        // where the halo unpack stores a ghost column's float beside its place behind the owned entries: its node's 4-float slot
        w.gslot.assign((size_t)(P.n - P.m), -1);
        for (int64_t g = 0; g < gn.count(); ++g)
            for (int a = 0; a < gn.ncomp[(size_t)g]; ++a) w.gslot[(size_t)(gn.col[(size_t)g] - P.m + a)] = (int32_t)(4 * (nnode + g) + a);
    }
    w.nw_grec = (int64_t)L.gcol.size();
    w.nw_rec = L.prow[nnode];
    // lanes per node in the segmented sums of a windowed tile (a lane takes two slots per trip): measured on bowl3D h = 0.02
    // (14 pair slots + 8 column-record slots per row, 64 nodes per tile) 8 lanes 136.9 us per product against 142.6 with 4
    const double mean = (double)(L.prow[nnode] / 2 + L.grow[nnode]) / (double)nnode;
    w.wlanes = sw.wlanes ? sw.wlanes : (mean <= 12 ? 4 : 8);
    if (b.own) {
        w.prow = std::move(b.prow);
        w.grow = std::move(b.grow);
        w.pcol = std::move(b.pcol);
        w.gcol = std::move(b.gcol);
    }
    w.present = true;
    return w;
}

}  // namespace npg
