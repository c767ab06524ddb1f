// Point location and point evaluation of the FE state: the arithmetic shared by the device kernels (sample.hip) and the host
// library (csrc_host/nupgcm_host.cpp), so that GPU() and CPU() apply the same bins, the same acceptance rule, the same tie-break
// and the same closed-form shape functions.  nan_eval / plot_slice / plot_profiles of src/plotting.jl:9-90 rest on this.
//
// Geometry of a cell: 12 doubles {x0[3], G1[3], G2[3], G3[3]} at geo[kGeoStride * cell] - x0 the cell's own anchor vertex
// (local vertex 0) and G_i = grad lambda_i, so lambda_i(x) = G_i . (x - x0) for i = 1..3 and lambda_0 = 1 - sum.  The stride is
// 16 doubles = 128 bytes: a candidate costs one cache line.
//
// Bins: a uniform grid of nb[0] x nb[1] x nb[2] boxes over the mesh's bounding box; bin (ix, iy, iz) has the number
// (iz * nb[1] + iy) * nb[0] + ix and lists, cell-ascending, the cells whose (slightly padded) bounding box overlaps it:
// bin_cells[bin_ptr[b] .. bin_ptr[b + 1]).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "cell_view.h"

namespace npg {

constexpr int kGeoStride = 16;
constexpr int kGeoEngine = 12;          // partitioned locators: record slot 12 = the cell's index in the rank's engine, -1 = not owned
constexpr double kInsideTol = -1e-10;   // a point belongs to the mesh when the best candidate's min lambda is >= this

struct BinGrid {
    double lo[3], hi[3];    // bounding box of the mesh
    double inv_h[3];        // bins per unit length
    double pad[3];          // a point this far outside the box is still looked up (rounding of a boundary point)
    int32_t nb[3];
};

NPG_HD int32_t bin_coord(const BinGrid &g, int a, double x) {
    const double t = (x - g.lo[a]) * g.inv_h[a];
    int32_t i = t > 0.0 ? (t < (double)g.nb[a] ? (int32_t)t : g.nb[a] - 1) : 0;     // monotone in x, clamped to the grid
    return i;
}

// The cell of point p: among the candidates of p's bin the one with the largest min lambda, ties to the lowest cell id.
// cell = -1 and lambda = NaN when p lies outside the bounding box or the best min lambda is below kInsideTol.
// PART: the locator of one rank of a partitioned mesh (build_bins_cells).  Its records are the rank's owned cells and their witness
// layer in ascending GLOBAL cell id, so the tie on the record index is the tie on the global id; the election is the same, and the
// winner's record then gives the cell's index in the rank's engine - or -1 when the winner is not owned here ("not mine": another
// rank reports the point), which reads like a point outside the mesh.
template <bool PART = false>
NPG_HD void locate_point(const BinGrid &g, const int32_t *bin_ptr, const int32_t *bin_cells, const double *geo,
                         const double p[3], int32_t *cell, double lam[4]) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    int32_t best = -1;
    double bl0 = nan, bl1 = nan, bl2 = nan, bl3 = nan;
    bool in_box = true;
NPG_UNROLL
    for (int a = 0; a < 3; ++a) in_box = in_box && (p[a] >= g.lo[a] - g.pad[a]) && (p[a] <= g.hi[a] + g.pad[a]);   // NaN: outside
    if (in_box) {
        const int64_t b = ((int64_t)bin_coord(g, 2, p[2]) * g.nb[1] + bin_coord(g, 1, p[1])) * g.nb[0] + bin_coord(g, 0, p[0]);
        const int32_t e0 = bin_ptr[b], e1 = bin_ptr[b + 1];
        double bmin = kInsideTol;
        for (int32_t e = e0; e < e1; ++e) {
            const int32_t c = bin_cells[e];
            const double *q = geo + (size_t)c * kGeoStride;
            const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
            const double l1 = q[3] * dx + q[4] * dy + q[5] * dz;
            const double l2 = q[6] * dx + q[7] * dy + q[8] * dz;
            const double l3 = q[9] * dx + q[10] * dy + q[11] * dz;
            const double l0 = 1.0 - (l1 + l2 + l3);
            const double m = fmin(fmin(l0, l1), fmin(l2, l3));
            // bins list their cells in ascending order, so `>` alone would already keep the lowest id of a tie; the id test makes
            // the rule independent of that order
            if (m >= kInsideTol && (best < 0 || m > bmin || (m == bmin && c < best))) {
                best = c;
                bmin = m;
                bl0 = l0, bl1 = l1, bl2 = l2, bl3 = l3;
            }
        }
    }
    if (PART && best >= 0) {
        best = (int32_t)geo[(size_t)best * kGeoStride + kGeoEngine];
        if (best < 0) bl0 = bl1 = bl2 = bl3 = nan;
    }
    *cell = best;
    lam[0] = bl0, lam[1] = bl1, lam[2] = bl2, lam[3] = bl3;
}

// P2 nodal basis in the local ordering of fe.p2_tables: vertices 0..3, then the edges (0,1) (0,2) (1,2) (0,3) (1,3) (2,3)
NPG_HD void p2_shape(const double l[4], double N[10]) {
NPG_UNROLL
    for (int k = 0; k < 4; ++k) N[k] = l[k] * (2.0 * l[k] - 1.0);
    N[4] = 4.0 * l[0] * l[1];
    N[5] = 4.0 * l[0] * l[2];
    N[6] = 4.0 * l[1] * l[2];
    N[7] = 4.0 * l[0] * l[3];
    N[8] = 4.0 * l[1] * l[3];
    N[9] = 4.0 * l[2] * l[3];
}

// d(sum_i v_i N_i)/d lambda_k of a P2 function with nodal values v
NPG_HD void p2_dlambda(const double l[4], const double v[10], double d[4]) {
    d[0] = (4.0 * l[0] - 1.0) * v[0] + 4.0 * (l[1] * v[4] + l[2] * v[5] + l[3] * v[7]);
    d[1] = (4.0 * l[1] - 1.0) * v[1] + 4.0 * (l[0] * v[4] + l[2] * v[6] + l[3] * v[8]);
    d[2] = (4.0 * l[2] - 1.0) * v[2] + 4.0 * (l[0] * v[5] + l[1] * v[6] + l[3] * v[9]);
    d[3] = (4.0 * l[3] - 1.0) * v[3] + 4.0 * (l[0] * v[7] + l[1] * v[8] + l[2] * v[9]);
}

// Evaluate `field` at one located point.  T gives the tables of the engine: cu(l, c), cp(m, c), cb(i, c) DoF codes, G(k, c)
// component k = 3 vertex + axis of grad lambda, udiri / bdiri value tables, nb buoyancy nodes per cell.  x = the vector the
// field lives in.  The caller has checked 0 <= c < ncell.
template <class T>
NPG_HD void sample_point(const T &t, int field, const double *x, int64_t c, const double l[4], double *out) {
    if (field == NPG_SAMPLE_U) {
        double N[10];
        p2_shape(l, N);
        double u0 = 0.0, u1 = 0.0, u2 = 0.0;
NPG_UNROLL
        for (int i = 0; i < 10; ++i) {
            const int32_t i0 = t.cu(3 * i, c), i1 = t.cu(3 * i + 1, c), i2 = t.cu(3 * i + 2, c);
            u0 += N[i] * (i0 >= 0 ? x[i0] : t.udiri[-1 - i0]);
            u1 += N[i] * (i1 >= 0 ? x[i1] : t.udiri[-1 - i1]);
            u2 += N[i] * (i2 >= 0 ? x[i2] : t.udiri[-1 - i2]);
        }
        out[0] = u0, out[1] = u1, out[2] = u2;
    } else if (field == NPG_SAMPLE_P) {
        double p = 0.0;
NPG_UNROLL
        for (int m = 0; m < 4; ++m) {
            const int32_t im = t.cp(m, c);
            p += l[m] * (im >= 0 ? x[im] : 0.0);      // the pinned vertex of the zero-mean space
        }
        out[0] = p;
    } else {
        const bool grad = field == NPG_SAMPLE_GRAD_B;
        double d[4], val = 0.0;
        if (t.nb == 10) {
            double v[10];
NPG_UNROLL
            for (int i = 0; i < 10; ++i) {
                const int32_t ii = t.cb(i, c);
                v[i] = ii >= 0 ? x[ii] : t.bdiri[-1 - ii];
            }
            if (grad) {
                p2_dlambda(l, v, d);
            } else {
                double N[10];
                p2_shape(l, N);
NPG_UNROLL
                for (int i = 0; i < 10; ++i) val += N[i] * v[i];
            }
        } else {
NPG_UNROLL
            for (int i = 0; i < 4; ++i) {
                const int32_t ii = t.cb(i, c);
                d[i] = ii >= 0 ? x[ii] : t.bdiri[-1 - ii];     // d N_i / d lambda_k = delta_ik
                val += l[i] * d[i];
            }
        }
        if (grad) {
NPG_UNROLL
            for (int a = 0; a < 3; ++a)
                out[a] = d[0] * t.G(a, c) + d[1] * t.G(3 + a, c) + d[2] * t.G(6 + a, c) + d[3] * t.G(9 + a, c);
        } else {
            out[0] = val;
        }
    }
}

NPG_HD int sample_ncomp(int field) { return field == NPG_SAMPLE_U || field == NPG_SAMPLE_GRAD_B ? 3 : 1; }

// ---- integrals over a tensor grid x[nx] (x) y[ny] (x) z[nz] (npg_fe_grid_integrals): what one grid point contributes ----------
// postprocess/utils.py:81-94, streamfunctions.py:14-80, stratification.py:45-62 reduce the sampled grid with trapezoids along z
// (columns) and along x (zonal lines); a point outside the mesh is a zero there, in the mask and in every field.
constexpr int kGridCol = 4;    // col[.][nx][ny]: count, H = int mask dz, int u_x dz, int u_y dz
constexpr int kGridZon = 6;    // zon[.][ny][nz]: count, width = int mask dx, int u_y dx, int u_z dx, int b dx, int max(dz b, 0) dx
constexpr int kGridVal = 6;    // one point: mask, u_x, u_y, u_z, b (full), max(dz b, 0) (full)
constexpr int kGridChunk = 16; // consecutive x indices per partial sum of a zonal line (the device folds the partials in order)

// weight of node i in trapezoid(f, x = a): half the distance between its neighbours, one-sided at the ends
NPG_HD double trapezoid_weight(const double *a, int64_t n, int64_t i) {
    return 0.5 * ((i + 1 < n ? a[i + 1] : a[i]) - (i > 0 ? a[i - 1] : a[i]));
}

// The values of grid point p (located: cell c, lambda l; c < 0 = outside the mesh).  The fields are evaluated one after another
// from the same lambda.  xu = [u; p], xb = b'; the full buoyancy is N2 z + b', its vertical derivative N2 + dz b'.
template <class T>
NPG_HD void grid_point_values(const T &t, const double *xu, const double *xb, double N2, double z, int64_t c, const double l[4],
                              double v[kGridVal]) {
NPG_UNROLL
    for (int a = 0; a < kGridVal; ++a) v[a] = 0.0;
    if (c < 0) return;
    v[0] = 1.0;
    sample_point(t, NPG_SAMPLE_U, xu, c, l, v + 1);
    double bp, g[3];
    sample_point(t, NPG_SAMPLE_B, xb, c, l, &bp);
    v[4] = N2 * z + bp;
    sample_point(t, NPG_SAMPLE_GRAD_B, xb, c, l, g);
    v[5] = fmax(N2 + g[2], 0.0);
}

// the terms a point of vertical weight wz adds to its column's integrals
NPG_HD void grid_col_terms(double wz, const double v[kGridVal], double term[kGridCol]) {
    term[0] = v[0], term[1] = wz * v[0], term[2] = wz * v[1], term[3] = wz * v[2];
}

// a point of zonal weight wx added to the integrals of its zonal line
NPG_HD void grid_zon_add(double wx, const double v[kGridVal], double acc[kGridZon]) {
    acc[0] += v[0], acc[1] += wx * v[0], acc[2] += wx * v[2], acc[3] += wx * v[3], acc[4] += wx * v[4], acc[5] += wx * v[5];
}

// nullptr if a[0..n) is a usable axis: n >= 2, finite, strictly increasing
inline const char *check_axis(const double *a, int64_t n) {
    if (n < 2) return "every axis needs at least 2 points";
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(a[i]) || (i > 0 && !(a[i] > a[i - 1]))) return "the axes must be finite and strictly increasing";
    return nullptr;
}

// ---- set-up on the host (both libraries): cell geometry records, bounding box, bins --------------------------------------
struct BinTables {
    BinGrid grid;
    std::vector<double> geo;            // [ncell][kGeoStride]
    std::vector<int32_t> bin_ptr;       // nbins + 1
    std::vector<int32_t> bin_cells;
    int64_t max_per_bin = 0;
};

// One cell's record q = {x0, G1, G2, G3} from its anchor x0 and the rows g = {G1, G2, G3}, its padded bounding box clo / chi, and
// lo / hi widened by its (unpadded) extent.  Every bounding box in this file comes from here, so a mesh has ONE box whoever asks.
inline const char *cell_record(const double *x0, const double *g, double *q, double *clo, double *chi, double lo[3], double hi[3]) {
    for (int a = 0; a < 3; ++a) q[a] = x0[a];
    for (int k = 0; k < 9; ++k) q[3 + k] = g[k];
    // the edge vectors v_j - x0 are the columns of inverse([G1; G2; G3])
    const double det = g[0] * (g[4] * g[8] - g[5] * g[7]) - g[1] * (g[3] * g[8] - g[5] * g[6]) + g[2] * (g[3] * g[7] - g[4] * g[6]);
    if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) return "npg_locator_create: a cell has singular grad_lambda";
    const double id = 1.0 / det;
    const double E[3][3] = {
        {(g[4] * g[8] - g[5] * g[7]) * id, (g[2] * g[7] - g[1] * g[8]) * id, (g[1] * g[5] - g[2] * g[4]) * id},
        {(g[5] * g[6] - g[3] * g[8]) * id, (g[0] * g[8] - g[2] * g[6]) * id, (g[2] * g[3] - g[0] * g[5]) * id},
        {(g[3] * g[7] - g[4] * g[6]) * id, (g[1] * g[6] - g[0] * g[7]) * id, (g[0] * g[4] - g[1] * g[3]) * id}};
    for (int a = 0; a < 3; ++a) {
        double mn = q[a], mx = q[a];
        for (int j = 0; j < 3; ++j) {
            const double v = q[a] + E[a][j];
            if (!std::isfinite(v)) return "npg_locator_create: non-finite cell geometry";
            mn = std::min(mn, v), mx = std::max(mx, v);
        }
        // a point accepted at min lambda >= -1e-10 lies within 1e-10 cell extents of the cell: 1e-6 covers it and the rounding
        // of the reconstructed vertices
        const double pad = 1e-6 * (mx - mn);
        clo[a] = mn - pad, chi[a] = mx + pad;
        lo[a] = std::min(lo[a], mn), hi[a] = std::max(hi[a], mx);
    }
    return nullptr;
}

// The bins of ncell cells with the padded boxes clo / chi over the bounding box lo .. hi, about `target` bins in all
inline const char *fill_bins(const double lo[3], const double hi[3], const std::vector<double> &clo, const std::vector<double> &chi,
                             int64_t ncell, double target, BinTables &out) {
    BinGrid &gr = out.grid;
    double ext[3], vol = 1.0;
    for (int a = 0; a < 3; ++a) {
        ext[a] = hi[a] - lo[a];
        if (!(ext[a] > 0.0)) return "npg_locator_create: the mesh's bounding box is flat";
        vol *= ext[a];
    }
    const double s = std::cbrt(vol / target);           // cubic bins
    int64_t total = 1;
    for (int a = 0; a < 3; ++a) {
        gr.lo[a] = lo[a], gr.hi[a] = hi[a];
        gr.nb[a] = (int32_t)std::min(1024.0, std::max(1.0, std::ceil(ext[a] / s)));
        gr.inv_h[a] = gr.nb[a] / ext[a];
        gr.pad[a] = 1e-9 * ext[a];
        total *= gr.nb[a];
    }
    // count -> prefix sum -> fill
    std::vector<int64_t> cnt((size_t)total + 1, 0);
    auto range = [&](int64_t c, int a, int32_t &i0, int32_t &i1) {
        i0 = bin_coord(gr, a, clo[(size_t)c * 3 + a]);
        i1 = bin_coord(gr, a, chi[(size_t)c * 3 + a]);
    };
    for (int64_t c = 0; c < ncell; ++c) {
        int32_t x0, x1, y0, y1, z0, z1;
        range(c, 0, x0, x1), range(c, 1, y0, y1), range(c, 2, z0, z1);
        for (int32_t z = z0; z <= z1; ++z)
            for (int32_t y = y0; y <= y1; ++y)
                for (int32_t x = x0; x <= x1; ++x) ++cnt[(size_t)(((int64_t)z * gr.nb[1] + y) * gr.nb[0] + x) + 1];
    }
    out.max_per_bin = 0;
    for (int64_t b = 0; b < total; ++b) {
        out.max_per_bin = std::max(out.max_per_bin, cnt[(size_t)b + 1]);
        cnt[(size_t)b + 1] += cnt[(size_t)b];
    }
    if (cnt[(size_t)total] >= INT32_MAX) return "npg_locator_create: too many bin entries for 32-bit offsets (ask for fewer bins)";
    out.bin_ptr.assign(cnt.begin(), cnt.end());
    out.bin_cells.assign((size_t)cnt[(size_t)total], 0);
    std::vector<int32_t> next(out.bin_ptr.begin(), out.bin_ptr.end() - 1);
    for (int64_t c = 0; c < ncell; ++c) {      // cells in ascending order: every bin's list is ascending
        int32_t x0, x1, y0, y1, z0, z1;
        range(c, 0, x0, x1), range(c, 1, y0, y1), range(c, 2, z0, z1);
        for (int32_t z = z0; z <= z1; ++z)
            for (int32_t y = y0; y <= y1; ++y)
                for (int32_t x = x0; x <= x1; ++x)
                    out.bin_cells[(size_t)next[(size_t)(((int64_t)z * gr.nb[1] + y) * gr.nb[0] + x)]++] = (int32_t)c;
    }
    return nullptr;
}

// G: grad lambda as [ncell][12] (component 3 k + a of cell c at G[12 c + 3 k + a]); anchor: [ncell][3]; nbins_target: 0 = one
// bin per cell.  Returns an error text or nullptr.
inline const char *build_bins(const double *G, const double *anchor, int64_t ncell, int64_t nbins_target, BinTables &out) {
    out.geo.assign((size_t)ncell * kGeoStride, 0.0);
    std::vector<double> clo((size_t)ncell * 3), chi((size_t)ncell * 3);
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t c = 0; c < ncell; ++c) {
        const char *err = cell_record(anchor + (size_t)c * 3, G + (size_t)c * 12 + 3, &out.geo[(size_t)c * kGeoStride],
                                      &clo[(size_t)c * 3], &chi[(size_t)c * 3], lo, hi);
        if (err) return err;
    }
    return fill_bins(lo, hi, clo, chi, ncell, (double)(nbins_target > 0 ? nbins_target : ncell), out);
}

// The bounding box build_bins gives a mesh, {lo[3], hi[3]}, without the bins
inline const char *mesh_box(const double *G, const double *anchor, int64_t ncell, double box[6]) {
    double q[kGeoStride], clo[3], chi[3];
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t c = 0; c < ncell; ++c) {
        const char *err = cell_record(anchor + (size_t)c * 3, G + (size_t)c * 12 + 3, q, clo, chi, lo, hi);
        if (err) return err;
    }
    for (int a = 0; a < 3; ++a) box[a] = lo[a], box[3 + a] = hi[a];
    return nullptr;
}

// The bins of one rank of a partitioned mesh: ncell explicit records geo12 = {x0, G1, G2, G3}, given in ascending global cell id,
// engine[c] = the cell's index in the rank's engine where the rank owns it, -1 otherwise (stored in record slot kGeoEngine), over
// the GLOBAL bounding box `box` (mesh_box of the whole mesh): points are binned as the one-device locator bins them, and bins
// away from the rank's cells stay empty.  nbins_target: 0 = one bin per record.
inline const char *build_bins_cells(const double *geo12, const int32_t *engine, int64_t ncell, const double box[6],
                                    int64_t nbins_target, BinTables &out) {
    out.geo.assign((size_t)ncell * kGeoStride, 0.0);
    std::vector<double> clo((size_t)ncell * 3), chi((size_t)ncell * 3);
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t c = 0; c < ncell; ++c) {
        double *q = &out.geo[(size_t)c * kGeoStride];
        const char *err = cell_record(geo12 + (size_t)c * 12, geo12 + (size_t)c * 12 + 3, q, &clo[(size_t)c * 3], &chi[(size_t)c * 3], lo, hi);
        if (err) return err;
        q[kGeoEngine] = (double)engine[c];
    }
    for (int a = 0; a < 3; ++a)
        if (!(lo[a] >= box[a] && hi[a] <= box[3 + a])) return "npg_locator_create_cells: a cell lies outside the bounding box given";
    return fill_bins(box, box + 3, clo, chi, ncell, (double)(nbins_target > 0 ? nbins_target : ncell), out);
}

}  // namespace npg
