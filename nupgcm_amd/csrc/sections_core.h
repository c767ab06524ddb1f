// Transports through SECTIONS (npg_sections_*): planes that cut the mesh, binned in two in-plane coordinates.  The plan
// (host code, plain C++), the per-piece arithmetic and the fold order, shared by the device library (sections.hip) and the host library
// (csrc_host/nupgcm_host.cpp): GPU() and CPU() build the same plan and evaluate the same expressions in the same order, piece by piece
// and bin by bin.  Always fp64 (npg_fe_set_precision does not apply).
//
// A section is a frame {origin o, unit normal n, in-plane unit axes e1, e2} (12 doubles; mutually orthogonal to 1e-12, any handedness)
// and two strictly increasing edge arrays, edges1[0 .. n1] and edges2[0 .. n2], whose first / last entry may be -inf / +inf.  Bin (i, j)
// is half-open: edges1[i] <= (x - o) . e1 < edges1[i + 1] and edges2[j] <= (x - o) . e2 < edges2[j + 1]; nothing outside the edges counts.
// Bins are numbered section by section, (i, j) row-major.
//
// THE CUT RULE.  d_k = ((x0 - o0) n0 + (x1 - o1) n1) + (x2 - o2) n2 at a cell's OWN four vertices (sec_dot: one association, no
// contraction - both libraries are built with -ffp-contract=off).  A vertex is below iff d < 0; d == 0 counts as above.  1 or 3 vertices
// below give a triangle, 2 a quadrilateral, 0 or 4 nothing.  The corners lie on the edges (a, b) with d_a < 0 <= d_b at
// t = d_a / (d_a - d_b) from the below vertex: barycentrics lambda_a = 1 - t, lambda_b = t.  So a mesh face lying in the plane is counted
// by exactly one of its two cells (the one whose fourth vertex is below), and a vertex or an edge on the plane gives pieces without
// area, which are dropped.
//
// CLIPPING.  Sutherland-Hodgman with the same half-open rule, first against the edges1 bins the polygon reaches, then against the edges2
// bins: a corner is inside the lower edge E iff s >= E, inside the upper edge iff s < E.  A crossing of E between two corners is formed
// from the corner with s < E (L) to the corner with s >= E (H) whichever way round the polygon is walked - both bins that share E get the
// same point: t = (E - s_L) / (s_H - s_L), every barycentric and the other in-plane coordinate lambda_L + t (lambda_H - lambda_L), the
// clipped coordinate E itself.  No crossing is ever formed with an infinite edge.  Each clipped polygon is fan-triangulated from its
// first corner; a triangle's area is half the norm of the cross product of its corners' physical coordinates
// x = ((lambda_0 X_0 + lambda_1 X_1) + lambda_2 X_2) + lambda_3 X_3; triangles whose area is not > 0 are dropped.
//
// A PIECE is (cell, bin, 3 corners x 4 barycentrics, area).  Pieces are ordered by (global bin, cell, index within the cell and bin);
// bin_ptr[nbin + 1] delimits the bins.  The planner is single-threaded: a pure function of its arguments.
//
// THE ARITHMETIC (section_piece).  The six points of the symmetric degree-4 triangle rule (weights summing to 1), point q at
// lambda_m = (mu_q0 L_0m + mu_q1 L_1m) + mu_q2 L_2m of the corners' barycentrics L; the P2 basis and its derivatives on the fly in the
// order of fe.p2_tables (vertices, then the edges (0,1) (0,2) (1,2) (0,3) (1,3) (2,3)); every sum over basis functions ascending from 0.0.
// The measure is w_q area.  term[k], the piece's NPG_NSEC = 14 raw channels (model prefactors are the caller's):
//
//    0  1                         1  u . n                    2  b'                         3  b' u . n
//    4  z u . n                   5  p                        6..8  u_x, u_y, u_z           9  grad b' . n
//   10  kappa_h (d_x b' n_x + d_y b' n_y) + kappa_v d_z b' n_z                             11  kappa_v n_z
//   12  z                        13  d_z b'
//
// z(q) = sum_m lambda_m z_m over the cell's own vertices.  kappa_h, kappa_v: the caller's tables [6][npiece] at the piece points, a missing
// table contributes 0; with cl.kappa_c > 0 kappa_v grows by the convection closure of mixing_core.h at the point's own d_z b'.
//
// THE FOLD (section_fold).  out[bin][ch] = the terms of the bin's pieces added in ONE order that is a function of the plan alone: 64
// accumulators take the bin's pieces round-robin in piece order, each from 0.0, and are then added pairwise in a fixed tree (stated at
// section_fold); an empty bin gives 14 zeros.
//
// Device piece tables are component-major: lam[12][npiece] (corner j, barycentric m at 4 j + m; all four barycentrics are stored, none
// is recomputed as 1 - the rest), terms [NPG_NSEC][npiece].  T: cell(i), sec(i), lam(k, i), area(i), normal(a, s), coef(which, q, i) /
// has(which), and the engine's G(k, c), u(x, l, c), p(x, m, c), b(x, i, c), z(m, c).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <string>
#include <vector>

#include "cell_view.h"
#include "mixing_core.h"

namespace npg {

constexpr int kNSec = 14;
constexpr int kSecQ = 6;                       // points of the triangle rule
constexpr int kSecMaxSections = 64;
constexpr int64_t kSecMaxBins = (int64_t)1 << 20;
enum { kSecKh = 0, kSecKv, kSecNCoef };
#ifndef NPG_SEC_BLOCK
#define NPG_SEC_BLOCK 256
#endif

// the symmetric degree-4 rule on a triangle, weights normalised to the area
constexpr double kSecWa = 0.223381589678011, kSecWb = 0.109951743655322;
constexpr double kSecA1 = 0.108103018168070, kSecA2 = 0.445948490915965, kSecB1 = 0.816847572980459, kSecB2 = 0.091576213509771;
constexpr double kSecW[kSecQ] = {kSecWa, kSecWa, kSecWa, kSecWb, kSecWb, kSecWb};
constexpr double kSecMu[kSecQ][3] = {{kSecA1, kSecA2, kSecA2}, {kSecA2, kSecA1, kSecA2}, {kSecA2, kSecA2, kSecA1},
                                     {kSecB1, kSecB2, kSecB2}, {kSecB2, kSecB1, kSecB2}, {kSecB2, kSecB2, kSecB1}};

// (x - o) . a in the ONE association the cut rule and the in-plane coordinates use
NPG_HD double sec_dot(const double *x, const double *o, const double *a) {
    return ((x[0] - o[0]) * a[0] + (x[1] - o[1]) * a[1]) + (x[2] - o[2]) * a[2];
}

// ---- the plan -----------------------------------------------------------------------------------------------------------------------
struct SecPlan {
    int nsec = 0;
    int64_t nbin = 0, ncut_cells = 0, max_per_bin = 0;
    std::vector<int64_t> sec_bin0;              // [nsec + 1]: section s owns the bins [sec_bin0[s], sec_bin0[s + 1])
    std::vector<double> normal;                 // [nsec][3]
    std::vector<int32_t> cell, bin;             // [npiece]
    std::vector<uint8_t> sec;                   // [npiece]
    std::vector<double> lam;                    // [npiece][3][4]
    std::vector<double> area;                   // [npiece]
    std::vector<int64_t> bin_ptr;               // [nbin + 1]
    int64_t npiece() const { return (int64_t)cell.size(); }
};

// npg_sections_create's argument checks, for both libraries: "" or what is wrong.  `flat`: the engine is an embedded 2-D one.
inline std::string check_sections_create(bool have_handles, bool flat, int64_t ncell, const double *cell_xyz, int nsec, const double *frames,
                                         const int32_t *n1, const int32_t *n2, const double *edges1, const double *edges2) {
    if (!have_handles) return "npg_sections_create: NULL argument";
    if (flat) return "npg_sections_create: an embedded 2-D engine is refused (a plane cuts its cells in segments, not in polygons)";
    if (nsec < 1 || nsec > kSecMaxSections) return msgf("npg_sections_create: nsec must be 1 .. %d, got %d", kSecMaxSections, nsec);
    if (!(cell_xyz && frames && n1 && n2 && edges1 && edges2)) return "npg_sections_create: NULL table";
    int64_t nbin = 0;
    const double *e[2] = {edges1, edges2};
    for (int s = 0; s < nsec; ++s) {
        const double *f = frames + 12 * s;
        for (int k = 0; k < 12; ++k)
            if (!std::isfinite(f[k])) return msgf("npg_sections_create: section %d: the frame is not finite", s);
        for (int a = 1; a < 4; ++a)
            for (int b = a; b < 4; ++b) {
                const double dot = (f[3 * a] * f[3 * b] + f[3 * a + 1] * f[3 * b + 1]) + f[3 * a + 2] * f[3 * b + 2];
                if (!(std::fabs(dot - (a == b ? 1.0 : 0.0)) <= 1e-12))
                    return msgf("npg_sections_create: section %d: the axes n, e1, e2 are not orthonormal to 1e-12", s);
            }
        const int32_t n[2] = {n1[s], n2[s]};
        for (int ax = 0; ax < 2; ++ax) {
            if (n[ax] < 1) return msgf("npg_sections_create: section %d: axis %d needs at least one bin, got %d", s, ax + 1, n[ax]);
            if ((int64_t)n[ax] > kSecMaxBins) return msgf("npg_sections_create: more than 2^20 bins");
            for (int32_t i = 0; i <= n[ax]; ++i) {
                const double v = e[ax][i];
                const bool ok = std::isfinite(v) || (i == 0 && v == -std::numeric_limits<double>::infinity()) ||
                                (i == n[ax] && v == std::numeric_limits<double>::infinity());
                if (!ok) return msgf("npg_sections_create: section %d: edges%d[%d] is not finite (only the first may be -inf, the last +inf)", s, ax + 1, i);
                if (i > 0 && !(e[ax][i - 1] < v)) return msgf("npg_sections_create: section %d: edges%d is not strictly increasing at %d", s, ax + 1, i);
            }
            e[ax] += n[ax] + 1;
        }
        nbin += (int64_t)n1[s] * n2[s];
        if (nbin > kSecMaxBins) return msgf("npg_sections_create: more than 2^20 bins");
    }
    for (int64_t i = 0; i < ncell * 12; ++i)
        if (!std::isfinite(cell_xyz[i])) return msgf("npg_sections_create: cell %lld: a vertex is not finite", (long long)(i / 12));
    return "";
}

struct SecCorner {
    double lam[4], s1, s2;
};
constexpr int kSecMaxCorners = 12;              // 4 of the cut, at most one more per clipping line (4 lines)

// keep the part of the polygon on the inside of edge E of in-plane coordinate `ax` (0: s1, 1: s2); lower: inside iff s >= E, else s < E
inline int sec_clip(const SecCorner *in, int n, int ax, double E, bool lower, SecCorner *out) {
    int m = 0;
    for (int i = 0; i < n; ++i) {
        const SecCorner &P = in[i], &Q = in[(i + 1) % n];
        const double sp = ax ? P.s2 : P.s1, sq = ax ? Q.s2 : Q.s1;
        const bool pge = sp >= E, qge = sq >= E;
        if (pge == lower) out[m++] = P;
        if (pge != qge) {
            const SecCorner &Lo = pge ? Q : P, &Hi = pge ? P : Q;
            const double sl = pge ? sq : sp, sh = pge ? sp : sq;
            const double t = (E - sl) / (sh - sl);
            SecCorner X;
            for (int k = 0; k < 4; ++k) X.lam[k] = Lo.lam[k] + t * (Hi.lam[k] - Lo.lam[k]);
            if (ax) X.s2 = E, X.s1 = Lo.s1 + t * (Hi.s1 - Lo.s1);
            else X.s1 = E, X.s2 = Lo.s2 + t * (Hi.s2 - Lo.s2);
            out[m++] = X;
        }
    }
    return m;
}

// the bins [lo, hi] of edges[0 .. n] that the interval [smin, smax] reaches under the half-open rule (lo > hi: none)
inline void sec_bin_range(const double *edges, int32_t n, double smin, double smax, int32_t &lo, int32_t &hi) {
    lo = (int32_t)(std::upper_bound(edges, edges + n + 1, smin) - edges) - 1;          // the last edge <= smin
    hi = (int32_t)(std::upper_bound(edges, edges + n + 1, smax) - edges) - 1;
    lo = std::max(lo, 0), hi = std::min(hi, n - 1);
}

inline void sec_physical(const double *X, const double *lam, double *x) {
    for (int a = 0; a < 3; ++a) x[a] = ((lam[0] * X[a] + lam[1] * X[3 + a]) + lam[2] * X[6 + a]) + lam[3] * X[9 + a];
}

// validation and plan of npg_sections_create, for both libraries: "" or what is wrong (nothing has been allocated or launched yet)
inline std::string sec_build_plan(bool have_handles, bool flat, int64_t ncell, const double *cell_xyz, int nsec, const double *frames,
                                  const int32_t *n1, const int32_t *n2, const double *edges1, const double *edges2, const uint8_t *cell_mask,
                                  SecPlan &pl) {
    const std::string bad = check_sections_create(have_handles, flat, ncell, cell_xyz, nsec, frames, n1, n2, edges1, edges2);
    if (!bad.empty()) return bad;
    pl = SecPlan();
    pl.nsec = nsec;
    pl.sec_bin0.assign(1, 0);
    std::vector<int32_t> cell, bin;             // in the order found: (section, cell, bin, index)
    std::vector<double> lam, area;
    std::vector<uint8_t> cut(ncell > 0 ? (size_t)ncell : 0, 0);
    const double *e1s = edges1, *e2s = edges2;
    for (int s = 0; s < nsec; ++s) {
        const double *o = frames + 12 * s, *nrm = o + 3, *e1 = o + 6, *e2 = o + 9;
        for (int a = 0; a < 3; ++a) pl.normal.push_back(nrm[a]);
        const int64_t bin0 = pl.sec_bin0.back();
        for (int64_t c = 0; c < ncell; ++c) {
            if (cell_mask && !cell_mask[c]) continue;
            const double *X = cell_xyz + 12 * c;
            double d[4];
            int below[4], above[4], nb = 0, na = 0;
            for (int k = 0; k < 4; ++k) {
                d[k] = sec_dot(X + 3 * k, o, nrm);
                if (d[k] < 0.0) below[nb++] = k;
                else above[na++] = k;
            }
            if (nb == 0 || nb == 4) continue;
            int ea[4], eb[4], nc;               // the corners' edges (below, above), in order round the polygon
            if (nb == 1) {
                nc = 3;
                for (int i = 0; i < 3; ++i) ea[i] = below[0], eb[i] = above[i];
            } else if (nb == 3) {
                nc = 3;
                for (int i = 0; i < 3; ++i) ea[i] = below[i], eb[i] = above[0];
            } else {
                nc = 4;
                ea[0] = below[0], eb[0] = above[0];
                ea[1] = below[0], eb[1] = above[1];
                ea[2] = below[1], eb[2] = above[1];
                ea[3] = below[1], eb[3] = above[0];
            }
            SecCorner poly[kSecMaxCorners], p1[kSecMaxCorners], p2[kSecMaxCorners], tmp[kSecMaxCorners];
            double s1min = std::numeric_limits<double>::infinity(), s1max = -s1min;
            for (int i = 0; i < nc; ++i) {
                const double t = d[ea[i]] / (d[ea[i]] - d[eb[i]]);
                SecCorner &P = poly[i];
                for (int k = 0; k < 4; ++k) P.lam[k] = 0.0;
                P.lam[ea[i]] = 1.0 - t, P.lam[eb[i]] = t;
                double x[3];
                sec_physical(X, P.lam, x);
                P.s1 = sec_dot(x, o, e1), P.s2 = sec_dot(x, o, e2);
                s1min = std::min(s1min, P.s1), s1max = std::max(s1max, P.s1);
            }
            int32_t ilo, ihi;
            sec_bin_range(e1s, n1[s], s1min, s1max, ilo, ihi);
            bool any = false;
            for (int32_t i = ilo; i <= ihi; ++i) {
                int m1 = nc;
                const SecCorner *q1 = poly;
                if (std::isfinite(e1s[i])) m1 = sec_clip(q1, m1, 0, e1s[i], true, tmp), q1 = tmp;
                if (std::isfinite(e1s[i + 1])) m1 = sec_clip(q1, m1, 0, e1s[i + 1], false, p1), q1 = p1;
                if (m1 < 3) continue;
                if (q1 != p1) std::copy(q1, q1 + m1, p1);
                double s2min = std::numeric_limits<double>::infinity(), s2max = -s2min;
                for (int k = 0; k < m1; ++k) s2min = std::min(s2min, p1[k].s2), s2max = std::max(s2max, p1[k].s2);
                int32_t jlo, jhi;
                sec_bin_range(e2s, n2[s], s2min, s2max, jlo, jhi);
                for (int32_t j = jlo; j <= jhi; ++j) {
                    int m2 = m1;
                    const SecCorner *q2 = p1;
                    if (std::isfinite(e2s[j])) m2 = sec_clip(q2, m2, 1, e2s[j], true, tmp), q2 = tmp;
                    if (std::isfinite(e2s[j + 1])) m2 = sec_clip(q2, m2, 1, e2s[j + 1], false, p2), q2 = p2;
                    if (m2 < 3) continue;
                    double x0[3];
                    sec_physical(X, q2[0].lam, x0);
                    for (int k = 1; k + 1 < m2; ++k) {
                        double xa[3], xb[3];
                        sec_physical(X, q2[k].lam, xa);
                        sec_physical(X, q2[k + 1].lam, xb);
                        const double ax = xa[0] - x0[0], ay = xa[1] - x0[1], az = xa[2] - x0[2];
                        const double bx = xb[0] - x0[0], by = xb[1] - x0[1], bz = xb[2] - x0[2];
                        const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
                        const double ar = 0.5 * std::sqrt((cx * cx + cy * cy) + cz * cz);
                        if (!(ar > 0.0)) continue;
                        if ((int64_t)cell.size() >= (int64_t)INT32_MAX) return "npg_sections_create: more than 2^31 - 1 pieces";
                        cell.push_back((int32_t)c);
                        bin.push_back((int32_t)(bin0 + (int64_t)i * n2[s] + j));
                        pl.sec.push_back((uint8_t)s);
                        area.push_back(ar);
                        lam.insert(lam.end(), q2[0].lam, q2[0].lam + 4);
                        lam.insert(lam.end(), q2[k].lam, q2[k].lam + 4);
                        lam.insert(lam.end(), q2[k + 1].lam, q2[k + 1].lam + 4);
                        any = true;
                    }
                }
            }
            if (any) cut[(size_t)c] = 1;
        }
        pl.sec_bin0.push_back(bin0 + (int64_t)n1[s] * n2[s]);
        e1s += n1[s] + 1, e2s += n2[s] + 1;
    }
    pl.nbin = pl.sec_bin0.back();
    for (int64_t c = 0; c < ncell; ++c) pl.ncut_cells += cut[(size_t)c];
    // a stable counting sort by bin: (bin, cell, index) - the bins of a section are found cell by cell
    const size_t np = cell.size();
    pl.bin_ptr.assign((size_t)pl.nbin + 1, 0);
    for (size_t i = 0; i < np; ++i) ++pl.bin_ptr[(size_t)bin[i] + 1];
    for (int64_t k = 0; k < pl.nbin; ++k) {
        pl.max_per_bin = std::max(pl.max_per_bin, pl.bin_ptr[(size_t)k + 1]);
        pl.bin_ptr[(size_t)k + 1] += pl.bin_ptr[(size_t)k];
    }
    std::vector<int64_t> next(pl.bin_ptr.begin(), pl.bin_ptr.end() - 1);
    std::vector<uint8_t> sec(np);
    pl.cell.resize(np), pl.bin.resize(np), pl.area.resize(np), pl.lam.resize(12 * np);
    for (size_t i = 0; i < np; ++i) {
        const size_t k = (size_t)next[(size_t)bin[i]]++;
        pl.cell[k] = cell[i], pl.bin[k] = bin[i], sec[k] = pl.sec[i], pl.area[k] = area[i];
        std::copy(lam.begin() + 12 * i, lam.begin() + 12 * (i + 1), pl.lam.begin() + 12 * k);
    }
    pl.sec.swap(sec);
    return "";
}

// what npg_sections_set_coeff accepts: "" or what is wrong
inline std::string check_sections_coeff(bool have_handle, int which, const double *table, int64_t npiece) {
    if (!have_handle) return "npg_sections_set_coeff: NULL argument";
    if (which < 0 || which >= kSecNCoef) return msgf("npg_sections_set_coeff: which must be NPG_SEC_KH or NPG_SEC_KV, got %d", which);
    if (table)
        for (int64_t i = 0; i < kSecQ * npiece; ++i)
            if (!std::isfinite(table[i]))
                return msgf("npg_sections_set_coeff: table %d is not finite at point %d of piece %lld", which, (int)(i / npiece), (long long)(i % npiece));
    return "";
}

inline std::string check_sections_closure(bool have_handle, double kappa_c, double N2min, double alpha, double N2c) {
    if (!have_handle) return "npg_sections_set_closure: NULL argument";
    if (!(std::isfinite(kappa_c) && kappa_c >= 0.0 && std::isfinite(N2min) && std::isfinite(alpha) && std::isfinite(N2c)))
        return "npg_sections_set_closure: kappa_c must be finite and >= 0, N2min, alpha and N2c finite";
    if (!(kappa_c == 0.0 || N2min > 0.0)) return msgf("npg_sections_set_closure: kappa_c > 0 needs N2min > 0, got %g", N2min);
    return "";
}

// the sizes npg_sections_compute needs (pieces_n < 0: no per-piece output)
inline std::string check_sections_compute(bool have_handles, int64_t n_inv, int64_t n_b, int64_t x_inv_n, int64_t b_n, int64_t nbin, int64_t npiece,
                                          int64_t out_n, int64_t pieces_n, bool same_ctx) {
    if (!have_handles) return "npg_sections_compute: NULL argument";
    const std::string bad = check_state_vectors("npg_sections_compute", n_inv, n_b, x_inv_n, b_n);
    if (!bad.empty()) return bad;
    if (out_n < nbin * kNSec)
        return msgf("npg_sections_compute: out holds %lld doubles, needs nbin * NPG_NSEC = %lld", (long long)out_n, (long long)(nbin * kNSec));
    if (pieces_n >= 0 && pieces_n < npiece * kNSec)
        return msgf("npg_sections_compute: pieces_out holds %lld doubles, needs NPG_NSEC * npiece = %lld", (long long)pieces_n,
                    (long long)(npiece * kNSec));
    if (!same_ctx) return "npg_sections_compute: arguments of different contexts";
    return "";
}

// ---- the arithmetic -------------------------------------------------------------------------------------------------------------------
// the engine's cell tables with the cells' own z, and the piece tables ([component][piece] in both libraries)
template <class View>
struct SecPieces : CellsYZ<View> {
    int64_t np;
    const int32_t *cell_;
    const uint8_t *sec_;
    const double *lam_, *area_, *normal_;      // [12][np], [np], [nsec][3]
    const double *coef_[kSecNCoef];            // [6][np] or null
    NPG_HD int64_t cell(int64_t i) const { return cell_[i]; }
    NPG_HD int sec(int64_t i) const { return sec_[i]; }
    NPG_HD double lam(int k, int64_t i) const { return lam_[(size_t)k * (size_t)np + i]; }
    NPG_HD double area(int64_t i) const { return area_[i]; }
    NPG_HD double normal(int a, int s) const { return normal_[3 * s + a]; }
    NPG_HD bool has(int w) const { return coef_[w] != nullptr; }
    NPG_HD double coef(int w, int q, int64_t i) const { return coef_[w][(size_t)q * (size_t)np + i]; }
};

template <int NB, class T>
NPG_HD void section_piece(const T &t, const double *xu, const double *xb, int64_t i, const MixClosure &cl, double term[kNSec]) {
    const int64_t c = t.cell(i);
    const int s = t.sec(i);
    double G[12], u[30], p[4], b[NB], z[4], L[12];
NPG_UNROLL
    for (int k = 0; k < 12; ++k) G[k] = t.G(k, c);
NPG_UNROLL
    for (int l = 0; l < 30; ++l) u[l] = t.u(xu, l, c);
NPG_UNROLL
    for (int m = 0; m < 4; ++m) p[m] = t.p(xu, m, c), z[m] = t.z(m, c);
NPG_UNROLL
    for (int k = 0; k < NB; ++k) b[k] = t.b(xb, k, c);
NPG_UNROLL
    for (int k = 0; k < 12; ++k) L[k] = t.lam(k, i);
    const double area = t.area(i), nx = t.normal(0, s), ny = t.normal(1, s), nz = t.normal(2, s);
NPG_UNROLL
    for (int k = 0; k < kNSec; ++k) term[k] = 0.0;
    constexpr int ea[6] = {0, 0, 1, 0, 1, 2}, eb[6] = {1, 2, 2, 3, 3, 3};
    for (int q = 0; q < kSecQ; ++q) {
        const double m0 = kSecMu[q][0], m1 = kSecMu[q][1], m2 = kSecMu[q][2];
        double lam[4], N[10];
NPG_UNROLL
        for (int m = 0; m < 4; ++m) lam[m] = (m0 * L[m] + m1 * L[4 + m]) + m2 * L[8 + m];
NPG_UNROLL
        for (int m = 0; m < 4; ++m) N[m] = lam[m] * (2.0 * lam[m] - 1.0);
NPG_UNROLL
        for (int e = 0; e < 6; ++e) N[4 + e] = 4.0 * lam[ea[e]] * lam[eb[e]];
        double ux = 0.0, uy = 0.0, uz = 0.0;
NPG_UNROLL
        for (int k = 0; k < 10; ++k) ux += N[k] * u[3 * k], uy += N[k] * u[3 * k + 1], uz += N[k] * u[3 * k + 2];
        const double pq = ((lam[0] * p[0] + lam[1] * p[1]) + lam[2] * p[2]) + lam[3] * p[3];
        const double zq = ((lam[0] * z[0] + lam[1] * z[1]) + lam[2] * z[2]) + lam[3] * z[3];
        double bq = 0.0, l[4];
        if constexpr (NB == 10) {
            // d N_m / d lambda_m = 4 lambda_m - 1; d N_e / d lambda_ea = 4 lambda_eb, d N_e / d lambda_eb = 4 lambda_ea
NPG_UNROLL
            for (int k = 0; k < 10; ++k) bq += N[k] * b[k];
NPG_UNROLL
            for (int m = 0; m < 4; ++m) l[m] = (4.0 * lam[m] - 1.0) * b[m];
NPG_UNROLL
            for (int e = 0; e < 6; ++e) l[ea[e]] += (4.0 * lam[eb[e]]) * b[4 + e], l[eb[e]] += (4.0 * lam[ea[e]]) * b[4 + e];
        } else {
            bq = ((lam[0] * b[0] + lam[1] * b[1]) + lam[2] * b[2]) + lam[3] * b[3];
NPG_UNROLL
            for (int m = 0; m < 4; ++m) l[m] = b[m];
        }
        const double gx = ((l[0] * G[0] + l[1] * G[3]) + l[2] * G[6]) + l[3] * G[9];
        const double gy = ((l[0] * G[1] + l[1] * G[4]) + l[2] * G[7]) + l[3] * G[10];
        const double gz = ((l[0] * G[2] + l[1] * G[5]) + l[2] * G[8]) + l[3] * G[11];
        const double un = (ux * nx + uy * ny) + uz * nz;
        const double gh = gx * nx + gy * ny;
        const double kh = t.has(kSecKh) ? t.coef(kSecKh, q, i) : 0.0;
        double kv = t.has(kSecKv) ? t.coef(kSecKv, q, i) : 0.0;
        if (cl.kappa_c > 0.0) kv = kv + closure_kappa(cl, gz);
        const double w = kSecW[q] * area;
        term[0] += w;
        term[1] += w * un;
        term[2] += w * bq;
        term[3] += w * (bq * un);
        term[4] += w * (zq * un);
        term[5] += w * pq;
        term[6] += w * ux, term[7] += w * uy, term[8] += w * uz;
        term[9] += w * (gh + gz * nz);
        term[10] += w * (kh * gh + kv * (gz * nz));
        term[11] += w * (kv * nz);
        term[12] += w * zq;
        term[13] += w * gz;
    }
}

// out[bin][ch] of terms[ch][0 .. np): the order of the fold, for the host library and any restatement - piece k of the bin (k = 0, 1, ...
// in piece order) is added to accumulator k mod 64, each accumulator from 0.0 in ascending k; then v[l] = v[l] + v[l + off] over l < off
// for off = 32, 16, 8, 4, 2, 1; the result is v[0].  (The device's wave does the same: lane l is accumulator l, the tree is wave_sum's
// butterfly, whose lane 0 adds exactly these pairs.)
constexpr int kSecFoldLanes = 64;
inline double section_fold(const int64_t *bin_ptr, const double *terms, int64_t np, int64_t bin, int ch) {
    double v[kSecFoldLanes];
    for (int l = 0; l < kSecFoldLanes; ++l) v[l] = 0.0;
    const double *t = terms + (size_t)ch * (size_t)np;
    const int64_t first = bin_ptr[bin], last = bin_ptr[bin + 1];
    for (int64_t i = first; i < last; ++i) v[(i - first) & (kSecFoldLanes - 1)] += t[i];
    for (int off = kSecFoldLanes / 2; off > 0; off >>= 1)
        for (int l = 0; l < off; ++l) v[l] = v[l] + v[l + off];
    return v[0];
}

}  // namespace npg
