// Interior buoyancy forcing (npg_interior_*): a volume source Q(x, t) and a sponge gamma(x) (b*(x, t) - b) of the buoyancy
// equation - the volume counterpart of forcing_core.h.  The arithmetic shared by the device kernels (interior.hip) and the host library
// (csrc_host/nupgcm_host.cpp), with the plan both build at create and the argument checks of the entry points: GPU() and CPU() evaluate
// the same expressions in the same order.  Always fp64 (npg_fe_set_precision does not apply).
//
// The handle holds the KEPT cells only (ascending cell ids): kept cell kc is cell cell[kc] of the engine.  The points are the engine's
// own volume rule - the rule NPG_MAT_M is assembled with: qw[q] wdet(c) at the points whose shape values are Nb[NB q + i] - so a
// constant gamma gives gamma M up to rounding.  Tables are component-major [key][point][kept cell]: a wave of consecutive kept cells
// reads unit stride.  The value of a series at a point is
//   v = a                          (w == 0: the second keyframe is not read)
//   v = (1 - w) a + w b            a = keyframe key, b = keyframe key + 1 (or 0 behind the last: the periodic wrap); w from the host
// Series: 0 Q, 1 b* (with the static gamma [point][kept cell]).  b_D(q) = sum_i Nb_i(q) bd_i over the cell's DIRICHLET nodes, bd_i
// their values from the engine's table (CellView::b): the Dirichlet columns of R, lifted into the load.
//   pass 1   loc[k][kc] = sum_q ((qw_q wdet) (Q_q + gamma_q (b*_q - b_D(q)))) Nb_k(q)      one kept cell per lane
//   pass 2   out[r] = sum_{slots of r} loc[slot]      the slots of a row in (kept cell, local node) order; rows without slots: 0
//   matrix   R[e] = sum_{slots (kc, i, j) of e} sum_q ((qw_q wdet) gamma_q) (Nb_i(q) Nb_j(q))     e over the entries some kept cell
//            touches, slots in (kept cell, i, j) order; rows and columns with a Dirichlet code take no part
//   budget   acc[0] += w, acc[1] += w Q_q, acc[2] += w (gamma_q (b*_q - b(q)))     w = qw_q wdet, b(q) from the state, Dirichlet nodes included
// One order of every sum, no atomics: the same bits on every call.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "cell_view.h"

namespace npg {

constexpr int kItrNSeries = 2;      // Q, b*
constexpr int kItrNBudget = 3;      // volume, source, restoring
constexpr int kItrChunk = 256;      // kept cells per partial row of the host library's budget (a constant: not the thread count)
#ifndef NPG_ITR_BLOCK
#define NPG_ITR_BLOCK 256
#endif

// what the kernels read beside the engine's tables ([key][point][kept cell] tables; device pointers in the device library)
struct ItrCells {
    int64_t nkept;
    int nq;
    const int32_t *cell;                  // [nkept] ascending cell ids
    const double *ser[kItrNSeries];       // [nkey][nq][nkept] or null
    const double *gamma;                  // [nq][nkept] or null
    int32_t nkey[kItrNSeries], key[kItrNSeries];
    double w[kItrNSeries];
    NPG_HD bool has(int c) const { return ser[c] != nullptr; }
    NPG_HD double at(int c, int q, int64_t kc) const {
        const size_t nk = (size_t)nkept;
        const double a = ser[c][((size_t)key[c] * nq + q) * nk + kc];
        if (w[c] == 0.0) return a;
        const int32_t k1 = key[c] + 1 < nkey[c] ? key[c] + 1 : 0;
        const double b = ser[c][((size_t)k1 * nq + q) * nk + kc];
        return (1.0 - w[c]) * a + w[c] * b;
    }
    NPG_HD double g(int q, int64_t kc) const { return gamma[(size_t)q * (size_t)nkept + kc]; }
    NPG_HD bool restoring() const { return has(1) && gamma != nullptr; }
};

// pass 1 of kept cell kc: loc[k nkept + kc].  S: the shape tables qw[q], Nb[NB q + i]; V: the engine's cell tables (cell_view.h)
template <int NB, class S, class V>
NPG_HD void itr_cell_load(const S &s, const V &view, const ItrCells &t, int64_t kc, double *loc) {
    const int64_t c = t.cell[kc];
    const double wdet = view.wdet(c);
    const bool hq = t.has(0), hr = t.restoring();
    double bd[NB], acc[NB];
NPG_UNROLL
    for (int i = 0; i < NB; ++i) {
        bd[i] = view.cb(i, c) < 0 ? view.b(nullptr, i, c) : 0.0;      // the Dirichlet nodes' values; a free node takes no part in b_D
        acc[i] = 0.0;
    }
    for (int q = 0; q < t.nq; ++q) {
        double x = hq ? t.at(0, q, kc) : 0.0;
        if (hr) {
            double bdq = 0.0;
NPG_UNROLL
            for (int i = 0; i < NB; ++i) bdq += s.Nb[q * NB + i] * bd[i];
            x = x + t.g(q, kc) * (t.at(1, q, kc) - bdq);
        }
        const double wv = (s.qw[q] * wdet) * x;
NPG_UNROLL
        for (int k = 0; k < NB; ++k) acc[k] += wv * s.Nb[q * NB + k];
    }
NPG_UNROLL
    for (int k = 0; k < NB; ++k) loc[(size_t)k * (size_t)t.nkept + kc] = acc[k];
}

// pass 2 of buoyancy row r
NPG_HD void itr_gather_row(int64_t r, const int32_t *ptr, const int32_t *slot, const double *loc, double *out) {
    const int32_t lo = ptr[r], hi = ptr[r + 1];
    double s = 0.0;
    for (int32_t i = lo; i < hi; ++i) s += loc[slot[i]];
    out[r] = hi > lo ? s : 0.0;
}

// entry e of R: its slots (kept cell, code = i NB + j) added in order
template <int NB, class S, class V>
NPG_HD double itr_matrix_entry(const S &s, const V &view, const ItrCells &t, const int32_t *eptr, const int32_t *ecell, const uint8_t *ecode,
                               int64_t e) {
    double sum = 0.0;
    for (int32_t i = eptr[e]; i < eptr[e + 1]; ++i) {
        const int64_t kc = ecell[i];
        const int a = ecode[i] / NB, b = ecode[i] % NB;
        const double wdet = view.wdet(t.cell[kc]);
        double m = 0.0;
        for (int q = 0; q < t.nq; ++q) m += ((s.qw[q] * wdet) * t.g(q, kc)) * (s.Nb[q * NB + a] * s.Nb[q * NB + b]);
        sum += m;
    }
    return sum;
}

// what kept cell kc adds to the three integrals: volume, int Q, int gamma (b* - b) for the state xb
template <int NB, class S, class V>
NPG_HD void itr_cell_budget(const S &s, const V &view, const ItrCells &t, const double *xb, int64_t kc, double acc[kItrNBudget]) {
    const int64_t c = t.cell[kc];
    const double wdet = view.wdet(c);
    const bool hq = t.has(0), hr = t.restoring();
    double b[NB];
NPG_UNROLL
    for (int i = 0; i < NB; ++i) b[i] = view.b(xb, i, c);
    for (int q = 0; q < t.nq; ++q) {
        const double w = s.qw[q] * wdet;
        acc[0] += w;
        if (hq) acc[1] += w * t.at(0, q, kc);
        if (hr) {
            double bq = 0.0;
NPG_UNROLL
            for (int i = 0; i < NB; ++i) bq += s.Nb[q * NB + i] * b[i];
            acc[2] += w * (t.g(q, kc) * (t.at(1, q, kc) - bq));
        }
    }
}

// The plan of a handle, built on the host at create by both libraries: the slots of pass 2 and of the matrix.
struct ItrPlan {
    int nb = 10;                          // buoyancy nodes per cell
    std::vector<int32_t> gptr, gslot;     // [n_b + 1], [nslot]: positions in loc
    std::vector<int32_t> eptr, ecell;     // [nent + 1], [nmslot]
    std::vector<uint8_t> ecode;           // [nmslot]
    std::vector<int64_t> epos;            // [nent]: the entry's position in the values of a matrix with the pattern
    bool has_pattern = false;
    int64_t pat_m = 0, pat_nnz = 0;
};

// npg_interior_create's validation and plan, for both libraries: "" or what is wrong (nothing has been allocated or launched yet).
// V: the engine's DoF codes (a CellView over HOST memory); rowptr / col: the "b" pattern on the host, or null (no matrix R).
template <class V>
inline std::string itr_build_plan(const V &view, int64_t n_b, int64_t nkept, const int32_t *cells, int64_t pat_m, const int64_t *rowptr,
                                  const int32_t *col, ItrPlan &pl) {
    const int nb = pl.nb = view.nb;
    if (nb != 10 && nb != 4) return "npg_interior_create: the engine's buoyancy space must have 10 or 4 nodes per cell";
    if (nkept < 0 || nkept > view.ncell) return msgf("npg_interior_create: nkept must be 0 .. ncell = %lld, got %lld", (long long)view.ncell, (long long)nkept);
    if ((int64_t)nb * nb * nkept > INT32_MAX) return "npg_interior_create: more than 2^31 - 1 slots";
    if (nkept > 0 && !cells) return "npg_interior_create: NULL cell table";
    if (n_b + 1 > INT32_MAX) return "npg_interior_create: more than 2^31 - 2 rows";
    for (int64_t k = 0; k < nkept; ++k) {
        if (cells[k] < 0 || cells[k] >= view.ncell) return msgf("npg_interior_create: kept cell %lld: cell %d is out of range", (long long)k, cells[k]);
        if (k > 0 && cells[k] <= cells[k - 1]) return msgf("npg_interior_create: kept cell %lld: the cell ids must be strictly ascending", (long long)k);
    }
    if (rowptr && pat_m != n_b) return msgf("npg_interior_create: the pattern has %lld rows, the buoyancy has %lld unknowns", (long long)pat_m, (long long)n_b);
    // pass 2: count, offsets, fill - kept cells ascending, local node ascending: a row's slots are sorted by (kept cell, local node)
    pl.gptr.assign((size_t)n_b + 1, 0);
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<int32_t> next;
        if (pass) {
            for (int64_t r = 0; r < n_b; ++r) pl.gptr[(size_t)r + 1] += pl.gptr[(size_t)r];
            pl.gslot.assign((size_t)pl.gptr[(size_t)n_b], 0);
            next.assign(pl.gptr.begin(), pl.gptr.end() - 1);
        }
        for (int64_t kc = 0; kc < nkept; ++kc)
            for (int k = 0; k < nb; ++k) {
                const int32_t r = view.cb(k, cells[kc]);
                if (r < 0) continue;
                if (r >= n_b) return msgf("npg_interior_create: kept cell %lld: a DoF code is out of range", (long long)kc);
                if (!pass) ++pl.gptr[(size_t)r + 1];
                else pl.gslot[(size_t)next[(size_t)r]++] = (int32_t)((int64_t)k * nkept + kc);
            }
    }
    // the matrix: (position, kept cell, code) of every pair of free nodes, sorted by (position, kept cell, code)
    pl.has_pattern = rowptr != nullptr;
    pl.eptr.assign(1, 0);
    pl.ecell.clear(), pl.ecode.clear(), pl.epos.clear();
    if (!rowptr) return "";
    pl.pat_m = pat_m, pl.pat_nnz = rowptr[pat_m];
    // a counting sort by position: the slots are generated in (kept cell, i, j) order and keep it inside an entry
    std::vector<int64_t> posv;
    posv.reserve((size_t)nkept * nb * nb);
    std::vector<int32_t> cnt((size_t)pl.pat_nnz, 0);
    for (int64_t kc = 0; kc < nkept; ++kc)
        for (int i = 0; i < nb; ++i) {
            const int32_t ri = view.cb(i, cells[kc]);
            if (ri < 0) continue;
            const int32_t *b = col + rowptr[ri], *e = col + rowptr[ri + 1];
            for (int j = 0; j < nb; ++j) {
                const int32_t cj = view.cb(j, cells[kc]);
                if (cj < 0) continue;
                const int32_t *p = std::lower_bound(b, e, cj);
                if (p == e || *p != cj)
                    return msgf("npg_interior_create: kept cell %lld: entry (%d, %d) is not in the pattern", (long long)kc, ri, cj);
                posv.push_back((int64_t)(p - col));
                ++cnt[(size_t)(p - col)];
            }
        }
    pl.eptr.clear();
    int32_t run = 0;
    for (int64_t pos = 0; pos < pl.pat_nnz; ++pos) {
        const int32_t n = cnt[(size_t)pos];
        if (n == 0) continue;
        pl.epos.push_back(pos);
        pl.eptr.push_back(run);
        cnt[(size_t)pos] = run;             // from here on: where the entry's next slot goes
        run += n;
    }
    pl.eptr.push_back(run);
    pl.ecell.assign(posv.size(), 0), pl.ecode.assign(posv.size(), 0);
    size_t s = 0;
    for (int64_t kc = 0; kc < nkept; ++kc)
        for (int i = 0; i < nb; ++i) {
            if (view.cb(i, cells[kc]) < 0) continue;
            for (int j = 0; j < nb; ++j) {
                if (view.cb(j, cells[kc]) < 0) continue;
                const int32_t dst = cnt[(size_t)posv[s++]]++;
                pl.ecell[(size_t)dst] = (int32_t)kc, pl.ecode[(size_t)dst] = (uint8_t)(i * nb + j);
            }
        }
    return "";
}

// a table [n][nq][nkept] of npg_interior_set_series / set_gamma: finite, gamma >= 0
inline std::string check_interior_table(const char *who, const double *table, int64_t n, int nq, int64_t nkept, bool nonneg) {
    for (int64_t i = 0; i < n * nq * nkept; ++i) {
        if (!std::isfinite(table[i]) || (nonneg && table[i] < 0.0))
            return msgf("%s: the table is %s at keyframe %lld, point %d of kept cell %lld", who, std::isfinite(table[i]) ? "negative" : "not finite",
                        (long long)(i / (nq * nkept)), (int)((i / nkept) % nq), (long long)(i % nkept));
    }
    return "";
}

inline std::string check_interior_set_series(bool handle, int which, int nkey, const double *tables, int nq, int64_t nkept) {
    if (!handle) return "npg_interior_set_series: NULL argument";
    if (which < 0 || which >= kItrNSeries) return msgf("npg_interior_set_series: which must be NPG_ITR_SOURCE or NPG_ITR_TARGET, got %d", which);
    if (tables && nkey < 1) return msgf("npg_interior_set_series: nkey must be >= 1, got %d", nkey);
    return tables ? check_interior_table("npg_interior_set_series", tables, nkey, nq, nkept, false) : "";
}

inline std::string check_interior_set_gamma(bool handle, const double *table, int nq, int64_t nkept) {
    if (!handle) return "npg_interior_set_gamma: NULL argument";
    return table ? check_interior_table("npg_interior_set_gamma", table, 1, nq, nkept, true) : "";
}

// the (key, w) pairs of npg_interior_apply / npg_interior_budget
inline std::string check_interior_keys(const char *who, const int32_t *key, const double *w, const int32_t nkey[kItrNSeries]) {
    if (!key || !w) return msgf("%s: NULL argument", who);
    for (int c = 0; c < kItrNSeries; ++c) {
        if (nkey[c] == 0) continue;
        if (key[c] < 0 || key[c] >= nkey[c]) return msgf("%s: series %d: key %d is outside its %d keyframes", who, c, key[c], nkey[c]);
        if (!(w[c] >= 0.0 && w[c] <= 1.0)) return msgf("%s: series %d: the weight must be in [0, 1], got %g", who, c, w[c]);
    }
    return "";
}

inline std::string check_interior_apply(bool handles, const int32_t *key, const double *w, const int32_t nkey[kItrNSeries], int64_t n_b,
                                        int64_t out_n, bool one_ctx) {
    if (!handles) return "npg_interior_apply: NULL argument";
    const std::string err = check_interior_keys("npg_interior_apply", key, w, nkey);
    if (!err.empty()) return err;
    if (out_n != n_b) return msgf("npg_interior_apply: rhs_src_out has %lld entries, expected %lld", (long long)out_n, (long long)n_b);
    if (!one_ctx) return "npg_interior_apply: arguments of different contexts";
    return "";
}

inline std::string check_interior_matrix(bool handles, bool has_pattern, bool has_gamma, bool same_pattern) {
    if (!handles) return "npg_interior_matrix: NULL argument";
    if (!has_pattern) return "npg_interior_matrix: the handle was created without a pattern";
    if (!has_gamma) return "npg_interior_matrix: no gamma table (npg_interior_set_gamma)";
    if (!same_pattern) return "npg_interior_matrix: R must be a plain-CSR matrix with the pattern given at create";
    return "";
}

inline std::string check_interior_budget(bool handles, const int32_t *key, const double *w, const int32_t nkey[kItrNSeries], int64_t n_b,
                                         int64_t b_n, int64_t out_n, bool one_ctx) {
    if (!handles) return "npg_interior_budget: NULL argument";
    const std::string err = check_interior_keys("npg_interior_budget", key, w, nkey);
    if (!err.empty()) return err;
    if (b_n != n_b) return msgf("npg_interior_budget: the buoyancy vector has %lld entries, expected %lld", (long long)b_n, (long long)n_b);
    if (out_n < kItrNBudget) return msgf("npg_interior_budget: out holds %lld doubles, needs %d", (long long)out_n, kItrNBudget);
    if (!one_ctx) return "npg_interior_budget: arguments of different contexts";
    return "";
}

}  // namespace npg
