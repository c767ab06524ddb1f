// Maps on buoyancy surfaces (npg_surfaces_*): the arithmetic shared by the device kernel (surfaces.hip) and the host
// library (csrc_host/nupgcm_host.cpp), so that GPU() and CPU() tile a column into the same segments and find the same crossings.
//
// Set-up (host code in both libraries): build_columns tiles every column (x_j, y_j) into the cells the vertical line passes through,
// top to bottom, from the locator's cell records {x0, G1, G2, G3} (sample_core.h).  The result is CSR-like: column j owns the
// segments col_ptr[j] .. col_ptr[j + 1), each (cell, z_top, z_bot), and the z_top of a segment IS the z_bot of the one above.
//
// The scan (column_surfaces, one column = one device thread): along a segment the full buoyancy B = N2 z + b' is the quadratic through
// its values at the top, the midpoint and the bottom of the segment - exact for P2 b', because z is linear in lambda along a
// vertical line; P1 b' is linear and skips the midpoint.  The top value is CARRIED from the segment above: the two cells that share a
// face then agree bit for bit on which side of a level the face lies, and a crossing on the face is counted once.
#pragma once
#include "sample_core.h"

namespace npg {

constexpr int kNSurf = 9;           // out[.][nlev][ncol]: z_up, z_low, ncross, u_x, u_y, u_z, d_x B, d_y B, d_z B
constexpr int kNSurfCol = 4;        // cols[.][ncol]: z_top, z_bot, B_top, B_bot
constexpr double kColumnTol = 1e-12;    // of the box's z extent: shorter intervals are no candidates, closer ends are a tie
constexpr double kVerticalTol = 1e-12;  // |d_z lambda_i| <= this |grad lambda_i|: the constraint does not depend on z

struct ColumnTables {
    std::vector<int64_t> col_ptr;       // ncol + 1
    std::vector<int32_t> seg_cell;
    std::vector<double> seg_ztop, seg_zbot;
    int64_t max_per_col = 0, ndry = 0;
};

// The interval {z : lambda_i(x, y, z) >= 0 for all i} of the cell with record q; false = empty
inline bool column_interval(const double *q, double x, double y, double &lo, double &hi) {
    const double dx = x - q[0], dy = y - q[1];
    double c[4], g[4], n[4];
    c[0] = 1.0, g[0] = 0.0;
    double s[3] = {0.0, 0.0, 0.0};
    for (int i = 1; i < 4; ++i) {
        const double *G = q + 3 * i;
        c[i] = G[0] * dx + G[1] * dy;
        g[i] = G[2];
        n[i] = std::sqrt(G[0] * G[0] + G[1] * G[1] + G[2] * G[2]);
        c[0] -= c[i], g[0] -= g[i];
        for (int a = 0; a < 3; ++a) s[a] += G[a];
    }
    n[0] = std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    lo = -INFINITY, hi = INFINITY;
    for (int i = 0; i < 4; ++i) {
        if (std::fabs(g[i]) <= kVerticalTol * n[i]) {
            if (!(c[i] >= kInsideTol)) return false;
        } else {
            const double z = q[2] - c[i] / g[i];       // lambda_i = c_i + g_i (z - z0) = 0
            if (g[i] > 0.0) lo = std::max(lo, z);
            else hi = std::min(hi, z);
        }
    }
    return hi > lo;
}

// xy[ncol][2]; geo: the locator's records [ncell][kGeoStride]; zlo, zhi: the z extent of the mesh's bounding box.  The columns are
// independent: an OpenMP loop where the translation unit is compiled with it (the host library).  Returns an error text or nullptr.
inline const char *build_columns(const double *geo, int64_t ncell, double zlo, double zhi, const double *xy, int64_t ncol,
                                 ColumnTables &out) {
    const double tol = kColumnTol * (zhi - zlo);
    // cells binned by their (padded) footprint in the x-y plane: about one bin per cell of a horizontal layer
    std::vector<double> clo((size_t)ncell * 3), chi((size_t)ncell * 3);
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    {
        double rec[kGeoStride];
        for (int64_t c = 0; c < ncell; ++c) {
            const double *q = geo + (size_t)c * kGeoStride;
            const char *err = cell_record(q, q + 3, rec, &clo[(size_t)c * 3], &chi[(size_t)c * 3], lo, hi);
            if (err) return "npg_surfaces_create: a cell record of the locator is singular";
        }
    }
    const double ex = hi[0] - lo[0], ey = hi[1] - lo[1];
    if (!(ex > 0.0) || !(ey > 0.0)) return "npg_surfaces_create: the mesh's footprint is flat";
    const double side = std::sqrt(ex * ey) / std::max(1.0, std::cbrt((double)ncell));
    const int64_t nbx = (int64_t)std::min(2048.0, std::max(1.0, std::ceil(ex / side)));
    const int64_t nby = (int64_t)std::min(2048.0, std::max(1.0, std::ceil(ey / side)));
    const double ihx = nbx / ex, ihy = nby / ey;
    auto bx = [&](double x) { const double t = (x - lo[0]) * ihx; return t > 0.0 ? (t < (double)nbx ? (int64_t)t : nbx - 1) : 0; };
    auto by = [&](double y) { const double t = (y - lo[1]) * ihy; return t > 0.0 ? (t < (double)nby ? (int64_t)t : nby - 1) : 0; };
    std::vector<int64_t> ptr((size_t)(nbx * nby) + 1, 0);
    for (int64_t c = 0; c < ncell; ++c)
        for (int64_t j = by(clo[(size_t)c * 3 + 1]); j <= by(chi[(size_t)c * 3 + 1]); ++j)
            for (int64_t i = bx(clo[(size_t)c * 3]); i <= bx(chi[(size_t)c * 3]); ++i) ++ptr[(size_t)(j * nbx + i) + 1];
    for (size_t b = 0; b < (size_t)(nbx * nby); ++b) ptr[b + 1] += ptr[b];
    std::vector<int32_t> cells((size_t)ptr.back());
    {
        std::vector<int64_t> next(ptr.begin(), ptr.end() - 1);
        for (int64_t c = 0; c < ncell; ++c)
            for (int64_t j = by(clo[(size_t)c * 3 + 1]); j <= by(chi[(size_t)c * 3 + 1]); ++j)
                for (int64_t i = bx(clo[(size_t)c * 3]); i <= bx(chi[(size_t)c * 3]); ++i) cells[(size_t)next[(size_t)(j * nbx + i)]++] = (int32_t)c;
    }
    struct Seg {
        int32_t cell;
        double top, bot;
    };
    std::vector<std::vector<Seg>> per((size_t)ncol);
    const double padx = 1e-9 * ex, pady = 1e-9 * ey;
#if defined(_OPENMP)
#pragma omp parallel for schedule(dynamic, 64)
#endif
    for (int64_t j = 0; j < ncol; ++j) {
        const double x = xy[2 * j], y = xy[2 * j + 1];
        if (!(x >= lo[0] - padx && x <= hi[0] + padx && y >= lo[1] - pady && y <= hi[1] + pady)) continue;      // NaN: dry
        struct Cand {
            double lo, hi;
            int32_t cell;
        };
        std::vector<Cand> cand;
        const size_t b = (size_t)(by(y) * nbx + bx(x));
        double z_cur = -INFINITY;
        for (int64_t e = ptr[b]; e < ptr[b + 1]; ++e) {
            const int32_t c = cells[(size_t)e];
            double l, h;
            if (column_interval(geo + (size_t)c * kGeoStride, x, y, l, h) && h - l > tol) {
                cand.push_back({l, h, c});
                z_cur = std::max(z_cur, h);
            }
        }
        std::vector<Seg> &segs = per[(size_t)j];
        while (!cand.empty()) {
            const double probe = z_cur - tol;          // the point just below z_cur
            double deepest = INFINITY;
            for (const Cand &k : cand)
                if (k.hi >= probe && k.lo < probe) deepest = std::min(deepest, k.lo);
            if (!(deepest < INFINITY)) break;          // a gap (or the bottom): the column is its uppermost connected piece
            int32_t best = INT32_MAX;
            double blo = deepest;
            for (const Cand &k : cand)
                if (k.hi >= probe && k.lo < probe && k.lo <= deepest + tol && k.cell < best) best = k.cell, blo = k.lo;
            segs.push_back({best, z_cur, blo});
            z_cur = blo;                               // carried: the next segment starts where this one ends, bit for bit
        }
    }
    out.col_ptr.assign((size_t)ncol + 1, 0);
    out.max_per_col = 0, out.ndry = 0;
    for (int64_t j = 0; j < ncol; ++j) {
        const int64_t n = (int64_t)per[(size_t)j].size();
        out.col_ptr[(size_t)j + 1] = out.col_ptr[(size_t)j] + n;
        out.max_per_col = std::max(out.max_per_col, n);
        out.ndry += n == 0;
    }
    const size_t nseg = (size_t)out.col_ptr[(size_t)ncol];
    if (nseg >= (size_t)INT32_MAX) return "npg_surfaces_create: too many segments for 32-bit offsets (ask for fewer columns)";
    out.seg_cell.resize(nseg), out.seg_ztop.resize(nseg), out.seg_zbot.resize(nseg);
    for (int64_t j = 0; j < ncol; ++j) {
        size_t s = (size_t)out.col_ptr[(size_t)j];
        for (const Seg &g : per[(size_t)j]) out.seg_cell[s] = g.cell, out.seg_ztop[s] = g.top, out.seg_zbot[s] = g.bot, ++s;
    }
    return nullptr;
}

// nullptr if levels[0..nlev) and N2 are usable
inline const char *check_levels(const double *levels, int nlev, double N2) {
    if (nlev < 1) return "nlev must be >= 1";
    if (!levels) return "NULL levels";
    if (!std::isfinite(N2)) return "N2 is not finite";
    for (int k = 0; k < nlev; ++k)
        if (!std::isfinite(levels[k]) || (k > 0 && !(levels[k] > levels[k - 1]))) return "the levels must be finite and strictly increasing";
    return nullptr;
}

// ---- the scan -------------------------------------------------------------------------------------------------------------------
struct SurfaceColumns {             // the handle's tables as the scan reads them
    const int64_t *col_ptr;
    const int32_t *seg_cell;
    const double *seg_ztop, *seg_zbot;
    const double *xy;               // [ncol][2]
    const double *geo;              // the locator's records
    int64_t ncol;
};

NPG_HD void column_lambda(const double *q, double x, double y, double z, double l[4]) {
    const double dx = x - q[0], dy = y - q[1], dz = z - q[2];
    l[1] = q[3] * dx + q[4] * dy + q[5] * dz;
    l[2] = q[6] * dx + q[7] * dy + q[8] * dz;
    l[3] = q[9] * dx + q[10] * dy + q[11] * dz;
    l[0] = 1.0 - (l[1] + l[2] + l[3]);
}

// b' of the cell with nodal values v at lambda
template <int NB>
NPG_HD double column_b(const double v[NB], const double l[4]) {
    double val = 0.0;
    if constexpr (NB == 10) {
        double N[10];
        p2_shape(l, N);
NPG_UNROLL
        for (int i = 0; i < 10; ++i) val += N[i] * v[i];
    } else {
NPG_UNROLL
        for (int i = 0; i < 4; ++i) val += l[i] * v[i];
    }
    return val;
}

// The root in [0, 1] of a0 + a1 s + a2 s^2 at which the sign changes, given that the signs at s = 0 and s = 1 differ (above0: the
// value at 0 is >= 0).  Stable quadratic formula; of two roots in range - one of them an end where the value is exactly 0 - the one
// at which "above" flips.
NPG_HD double root_between(double a0, double a1, double a2, bool above0) {
    double s;
    if (a2 == 0.0) {
        s = -a0 / a1;
    } else {
        const double disc = fmax(a1 * a1 - 4.0 * a2 * a0, 0.0);
        const double qq = -0.5 * (a1 + copysign(sqrt(disc), a1));
        const double r1 = qq / a2, r2 = qq != 0.0 ? a0 / qq : r1;
        const double d1 = r1 < 0.0 ? -r1 : (r1 > 1.0 ? r1 - 1.0 : 0.0), d2 = r2 < 0.0 ? -r2 : (r2 > 1.0 ? r2 - 1.0 : 0.0);
        if (d1 == 0.0 && d2 == 0.0) s = above0 ? fmax(r1, r2) : fmin(r1, r2);
        else s = d1 <= d2 ? r1 : r2;                   // (a NaN distance compares false: the other root)
    }
    return s > 0.0 ? (s < 1.0 ? s : 1.0) : 0.0;         // NaN -> 0
}

// One column.  T: the engine's tables as sample_point reads them.  xb = b'.  Writes channels 0 .. 2 of out[.][k][j] for every level
// k (NaN / 0 in the others), cross_cell[k][j] = the cell of the uppermost crossing (-1: none) and cols[.][j]: straight to memory, no
// per-level state in registers (a run-time index into a register array would spill).
template <int NB, class T>
NPG_HD void column_surfaces(const SurfaceColumns &S, const T &t, const double *xb, double N2, const double *levels, int nlev, int64_t j,
                            double *out, int32_t *cross_cell, double *cols) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const size_t plane = (size_t)nlev * (size_t)S.ncol;
    for (int k = 0; k < nlev; ++k) {
        const size_t o = (size_t)k * (size_t)S.ncol + (size_t)j;
NPG_UNROLL
        for (int ch = 0; ch < kNSurf; ++ch) out[ch * plane + o] = ch == 2 ? 0.0 : nan;
        cross_cell[o] = -1;
    }
    const int64_t s0 = S.col_ptr[j], s1 = S.col_ptr[j + 1];
    if (s1 == s0) {
NPG_UNROLL
        for (int ch = 0; ch < kNSurfCol; ++ch) cols[(size_t)ch * S.ncol + j] = nan;
        return;
    }
    const double x = S.xy[2 * j], y = S.xy[2 * j + 1];
    double F0 = 0.0, Btop = 0.0;
    for (int64_t s = s0; s < s1; ++s) {
        const int64_t c = S.seg_cell[s];
        const double zt = S.seg_ztop[s], zb = S.seg_zbot[s];
        const double *q = S.geo + (size_t)c * kGeoStride;
        double v[NB], l[4];
NPG_UNROLL
        for (int i = 0; i < NB; ++i) {
            const int32_t ii = t.cb(i, c);
            v[i] = ii >= 0 ? xb[ii] : t.bdiri[-1 - ii];
        }
        if (s == s0) {                                 // only the first segment evaluates its top: below, F0 is the F1 of the one above
            column_lambda(q, x, y, zt, l);
            F0 = N2 * zt + column_b<NB>(v, l);
            Btop = F0;
        }
        column_lambda(q, x, y, zb, l);
        const double F1 = N2 * zb + column_b<NB>(v, l);
        double a1 = F1 - F0, a2 = 0.0;
        if (NB == 10) {
            const double zm = 0.5 * (zt + zb);
            column_lambda(q, x, y, zm, l);
            const double Fm = N2 * zm + column_b<NB>(v, l);
            a1 = -3.0 * F0 + 4.0 * Fm - F1;
            a2 = 2.0 * (F0 - 2.0 * Fm + F1);
        }
        // the range of the quadratic on [0, 1]: levels outside it are not looked at
        double qmin = fmin(F0, F1), qmax = fmax(F0, F1), sv = -1.0;
        if (a2 != 0.0) {
            sv = -a1 / (2.0 * a2);
            if (sv > 0.0 && sv < 1.0) {
                const double Fv = F0 - a1 * a1 / (4.0 * a2);
                qmin = fmin(qmin, Fv), qmax = fmax(qmax, Fv);
            } else {
                sv = -1.0;
            }
        }
        int k = 0;
        for (int hi = nlev; k < hi;) {                 // the first level >= qmin
            const int mid = (k + hi) >> 1;
            if (levels[mid] < qmin) k = mid + 1;
            else hi = mid;
        }
        for (; k < nlev; ++k) {
            const double Bk = levels[k];
            if (Bk > qmax) break;
            const double a0 = F0 - Bk;
            const bool above0 = a0 >= 0.0, above1 = F1 - Bk >= 0.0;
            double sa, sb;                             // the crossings of this segment, sa <= sb
            int nc;
            if (above0 != above1) {
                sa = sb = root_between(a0, a1, a2, above0);
                nc = 1;
            } else {
                if (sv < 0.0) continue;
                const double av = a0 - a1 * a1 / (4.0 * a2);           // the quadratic at its vertex, less B_k
                if ((av >= 0.0) == above0) continue;
                const double disc = fmax(a1 * a1 - 4.0 * a2 * a0, 0.0);
                const double qq = -0.5 * (a1 + copysign(sqrt(disc), a1));
                const double r1 = qq / a2, r2 = qq != 0.0 ? a0 / qq : r1;
                sa = fmin(r1, r2), sb = fmax(r1, r2);
                sa = sa > 0.0 ? (sa < 1.0 ? sa : 1.0) : 0.0;
                sb = sb > 0.0 ? (sb < 1.0 ? sb : 1.0) : 0.0;
                nc = 2;
            }
            const size_t o = (size_t)k * (size_t)S.ncol + (size_t)j;
            const double seen = out[2 * plane + o];
            out[2 * plane + o] = seen + (double)nc;
            out[1 * plane + o] = zt + sb * (zb - zt);
            if (seen == 0.0) {                         // the sweep runs top to bottom: the first crossing met is the uppermost
                out[o] = zt + sa * (zb - zt);
                cross_cell[o] = (int32_t)c;
            }
        }
        F0 = F1;
        if (s == s1 - 1) {
            cols[j] = S.seg_ztop[s0], cols[(size_t)S.ncol + j] = zb;
            cols[2 * (size_t)S.ncol + j] = Btop, cols[3 * (size_t)S.ncol + j] = F1;
        }
    }
}

// The flow on the surfaces: entry o = k ncol + j of the level-column table.  Where the scan found a crossing, u and grad B at
// (x_j, y_j, z_up) in the cell the scan met it in, through sample_point; N2 is added to the z gradient.  xu = [u; p].
template <class T>
NPG_HD void surface_fields(const SurfaceColumns &S, const T &t, const double *xu, const double *xb, double N2, int nlev, int64_t o,
                           const int32_t *cross_cell, double *out) {
    const int64_t c = cross_cell[o];
    if (c < 0) return;                                 // the scan wrote NaN
    const size_t plane = (size_t)nlev * (size_t)S.ncol;
    const int64_t j = o % S.ncol;
    double l[4], u[3], gB[3];
    column_lambda(S.geo + (size_t)c * kGeoStride, S.xy[2 * j], S.xy[2 * j + 1], out[o], l);
    sample_point(t, NPG_SAMPLE_U, xu, c, l, u);
    sample_point(t, NPG_SAMPLE_GRAD_B, xb, c, l, gB);
    out[3 * plane + o] = u[0], out[4 * plane + o] = u[1], out[5 * plane + o] = u[2];
    out[6 * plane + o] = gB[0], out[7 * plane + o] = gB[1], out[8 * plane + o] = gB[2] + N2;
}

}  // namespace npg
