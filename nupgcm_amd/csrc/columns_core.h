// Column integrals (npg_columns_*): the arithmetic shared by the device kernels (columns.hip) and the host library
// (csrc_host/nupgcm_host.cpp), so that GPU() and CPU() integrate a column to the same bits.
//
// The columns and their tiling are those of the buoyancy surfaces (surfaces_core.h: build_columns, column_lambda, the locator's
// records), unchanged.  Along a segment (cell, z_top, z_bot) of a vertical line z is linear in the barycentrics, so u and b' (P2) are
// quadratics in z, p (P1) is linear, and every integrand below is a polynomial in z of degree <= 5: the 3-point Gauss-Legendre rule
// integrates it exactly.
//
// A segment (segment_terms).  dz = z_top - z_bot.  The points are z_g = z_bot + s_g dz with s = {1/2 (1 - sqrt(3/5)), 1/2,
// 1/2 (1 + sqrt(3/5))} (bottom to top) and the weights W = {5/18, 8/18, 5/18}; the term of an integrand f is
//     ((W_0 f(z_0) + W_1 f(z_1)) + W_2 f(z_2)) dz
// (gauss_term).  The integrands that are constant on the segment are taken as the constant times dz: channel 0 (1) and channels 7, 8
// (grad_h p of a P1 pressure).  The fields are evaluated as sample_point evaluates them - the same shape functions, the same order
// of the sums, DoF codes through field_val and the Dirichlet tables, p = 0 at the pinned vertex - one field after another: u, b', p.
//
// A column (the fold).  Per channel the terms of a column's segments are added TOP TO BOTTOM, starting from 0.0:
//     a = 0.0;  for s = col_ptr[j] .. col_ptr[j + 1) - 1:  a = a + term[s]
// in both libraries.  The end values (column_ends) are taken in the last segment's cell at its z_bot and in the first segment's cell
// at its z_top.  A dry column has NaN in every channel.
#pragma once
#include "surfaces_core.h"

namespace npg {

constexpr int kNColI = 17;     // integrals: 1; u_x u_y u_z; b'; z b'; p; d_x p, d_y p; d_x b', d_y b'; z d_x b', z d_y b'; (u_x^2 + u_y^2)/2; u b'
constexpr int kNColE = 14;     // ends: bottom p, b', d_z b', d_x p, d_y p, d_z p, d_x z_bot, d_y z_bot; top p, b', u_x, u_y, d_x z_top, d_y z_top

NPG_HD double gauss_term(double f0, double f1, double f2, double dz) {
    return ((5.0 / 18.0 * f0 + 8.0 / 18.0 * f1) + 5.0 / 18.0 * f2) * dz;
}

// The kNColI terms of the segment (c, zt, zb) of the column (x, y) -> term[ch * stride].  q: the locator's record of cell c; xu =
// [u; p], xb = b'.
template <int NB, class T>
NPG_HD void segment_terms(const T &t, const double *q, const double *xu, const double *xb, int64_t c, double x, double y, double zt,
                          double zb, double *term, size_t stride) {
    const double dz = zt - zb;
    const double s[3] = {0.5 * (1.0 - 0.7745966692414834), 0.5, 0.5 * (1.0 + 0.7745966692414834)};
    double z[3], l[3][4], N[3][10];
NPG_UNROLL
    for (int g = 0; g < 3; ++g) {
        z[g] = zb + s[g] * dz;
        column_lambda(q, x, y, z[g], l[g]);
        p2_shape(l[g], N[g]);
    }
    term[0] = dz;
    // u
    double u[3][3];
NPG_UNROLL
    for (int g = 0; g < 3; ++g) u[g][0] = u[g][1] = u[g][2] = 0.0;
NPG_UNROLL
    for (int i = 0; i < 10; ++i) {
        const double v0 = t.u(xu, 3 * i, c), v1 = t.u(xu, 3 * i + 1, c), v2 = t.u(xu, 3 * i + 2, c);
NPG_UNROLL
        for (int g = 0; g < 3; ++g) u[g][0] += N[g][i] * v0, u[g][1] += N[g][i] * v1, u[g][2] += N[g][i] * v2;
    }
    term[1 * stride] = gauss_term(u[0][0], u[1][0], u[2][0], dz);
    term[2 * stride] = gauss_term(u[0][1], u[1][1], u[2][1], dz);
    term[3 * stride] = gauss_term(u[0][2], u[1][2], u[2][2], dz);
    term[13 * stride] = gauss_term(0.5 * (u[0][0] * u[0][0] + u[0][1] * u[0][1]), 0.5 * (u[1][0] * u[1][0] + u[1][1] * u[1][1]),
                                   0.5 * (u[2][0] * u[2][0] + u[2][1] * u[2][1]), dz);
    // grad_h lambda of the cell: the engine's table, as sample_point reads it
    double gx[4], gy[4];
NPG_UNROLL
    for (int k = 0; k < 4; ++k) gx[k] = t.G(3 * k, c), gy[k] = t.G(3 * k + 1, c);
    // b'
    {
        double v[NB], bv[3], bx[3], by[3];
NPG_UNROLL
        for (int i = 0; i < NB; ++i) v[i] = t.b(xb, i, c);
NPG_UNROLL
        for (int g = 0; g < 3; ++g) {
            double d[4], val = 0.0;
            if constexpr (NB == 10) {
NPG_UNROLL
                for (int i = 0; i < 10; ++i) val += N[g][i] * v[i];
                p2_dlambda(l[g], v, d);
            } else {
NPG_UNROLL
                for (int i = 0; i < 4; ++i) val += l[g][i] * v[i], d[i] = v[i];
            }
            bv[g] = val;
            bx[g] = d[0] * gx[0] + d[1] * gx[1] + d[2] * gx[2] + d[3] * gx[3];
            by[g] = d[0] * gy[0] + d[1] * gy[1] + d[2] * gy[2] + d[3] * gy[3];
        }
        term[4 * stride] = gauss_term(bv[0], bv[1], bv[2], dz);
        term[5 * stride] = gauss_term(z[0] * bv[0], z[1] * bv[1], z[2] * bv[2], dz);
        term[9 * stride] = gauss_term(bx[0], bx[1], bx[2], dz);
        term[10 * stride] = gauss_term(by[0], by[1], by[2], dz);
        term[11 * stride] = gauss_term(z[0] * bx[0], z[1] * bx[1], z[2] * bx[2], dz);
        term[12 * stride] = gauss_term(z[0] * by[0], z[1] * by[1], z[2] * by[2], dz);
        term[14 * stride] = gauss_term(u[0][0] * bv[0], u[1][0] * bv[1], u[2][0] * bv[2], dz);
        term[15 * stride] = gauss_term(u[0][1] * bv[0], u[1][1] * bv[1], u[2][1] * bv[2], dz);
        term[16 * stride] = gauss_term(u[0][2] * bv[0], u[1][2] * bv[1], u[2][2] * bv[2], dz);
    }
    // p
    {
        double pm[4], pv[3];
NPG_UNROLL
        for (int m = 0; m < 4; ++m) pm[m] = t.p(xu, m, c);
NPG_UNROLL
        for (int g = 0; g < 3; ++g) {
            double val = 0.0;
NPG_UNROLL
            for (int m = 0; m < 4; ++m) val += l[g][m] * pm[m];
            pv[g] = val;
        }
        term[6 * stride] = gauss_term(pv[0], pv[1], pv[2], dz);
        term[7 * stride] = (pm[0] * gx[0] + pm[1] * gx[1] + pm[2] * gx[2] + pm[3] * gx[3]) * dz;
        term[8 * stride] = (pm[0] * gy[0] + pm[1] * gy[1] + pm[2] * gy[2] + pm[3] * gy[3]) * dz;
    }
}

// d_x z, d_y z of the end of the column's interval in the cell with record q: the constraint lambda_i = 0 that bounds the interval
// from below (bottom) or from above, found as column_interval finds lo and hi - the same c_i, g_i and z_i = z0 - c_i / g_i, a
// constraint that does not depend on z left out - and, at a tie, the lowest i.  z_i(x, y) has the slope - G_ix / G_iz.
NPG_HD void column_end_slope(const double *q, double x, double y, bool bottom, double sl[2]) {
    const double dx = x - q[0], dy = y - q[1];
    double c0 = 1.0, g0x = 0.0, g0y = 0.0, g0z = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
    double best = bottom ? -INFINITY : INFINITY;
    sl[0] = sl[1] = std::numeric_limits<double>::quiet_NaN();
    double ci[4], G[4][3];
NPG_UNROLL
    for (int i = 1; i < 4; ++i) {
        G[i][0] = q[3 * i], G[i][1] = q[3 * i + 1], G[i][2] = q[3 * i + 2];
        ci[i] = G[i][0] * dx + G[i][1] * dy;
        c0 -= ci[i], g0x -= G[i][0], g0y -= G[i][1], g0z -= G[i][2];
        sx += G[i][0], sy += G[i][1], sz += G[i][2];
    }
    ci[0] = c0, G[0][0] = g0x, G[0][1] = g0y, G[0][2] = g0z;
NPG_UNROLL
    for (int i = 0; i < 4; ++i) {
        const double n = i == 0 ? sqrt(sx * sx + sy * sy + sz * sz) : sqrt(G[i][0] * G[i][0] + G[i][1] * G[i][1] + G[i][2] * G[i][2]);
        const double g = G[i][2];
        if (fabs(g) <= kVerticalTol * n) continue;
        const double zi = q[2] - ci[i] / g;
        const bool take = bottom ? (g > 0.0 && zi > best) : (g < 0.0 && zi < best);
        if (take) best = zi, sl[0] = -G[i][0] / g, sl[1] = -G[i][1] / g;
    }
}

// The kNColE end values of the column (x, y) whose first segment is (c_top, zt, .) and whose last is (c_bot, ., zb) -> e[k * stride]
template <int NB, class T>
NPG_HD void column_ends(const T &t, const double *geo, const double *xu, const double *xb, double x, double y, int64_t c_top, double zt,
                        int64_t c_bot, double zb, double *e, size_t stride) {
    double l[4], pm[4], gb[3], sl[2];
    {   // the bottom end
        const double *q = geo + (size_t)c_bot * kGeoStride;
        column_lambda(q, x, y, zb, l);
        double p = 0.0;
NPG_UNROLL
        for (int m = 0; m < 4; ++m) pm[m] = t.p(xu, m, c_bot), p += l[m] * pm[m];
        e[0] = p;
        sample_point(t, NPG_SAMPLE_B, xb, c_bot, l, e + stride);
        sample_point(t, NPG_SAMPLE_GRAD_B, xb, c_bot, l, gb);
        e[2 * stride] = gb[2];
NPG_UNROLL
        for (int a = 0; a < 3; ++a)
            e[(3 + a) * stride] = pm[0] * t.G(a, c_bot) + pm[1] * t.G(3 + a, c_bot) + pm[2] * t.G(6 + a, c_bot) + pm[3] * t.G(9 + a, c_bot);
        column_end_slope(q, x, y, true, sl);
        e[6 * stride] = sl[0], e[7 * stride] = sl[1];
    }
    {   // the top end
        const double *q = geo + (size_t)c_top * kGeoStride;
        column_lambda(q, x, y, zt, l);
        double p = 0.0, u[3];
NPG_UNROLL
        for (int m = 0; m < 4; ++m) p += l[m] * t.p(xu, m, c_top);
        e[8 * stride] = p;
        sample_point(t, NPG_SAMPLE_B, xb, c_top, l, e + 9 * stride);
        sample_point(t, NPG_SAMPLE_U, xu, c_top, l, u);
        e[10 * stride] = u[0], e[11 * stride] = u[1];
        column_end_slope(q, x, y, false, sl);
        e[12 * stride] = sl[0], e[13 * stride] = sl[1];
    }
}

// ---- the argument checks both libraries share: the message, empty = fine --------------------------------------------------------------
inline std::string check_columns_create(bool null_arg, int64_t ncol, bool one_ctx, bool partitioned, int64_t loc_ncell, int64_t fe_ncell) {
    if (null_arg) return "npg_columns_create: NULL argument";
    if (ncol < 1 || ncol > ((int64_t)1 << 30)) return msgf("npg_columns_create: 1 .. 2^30 columns, got %lld", (long long)ncol);
    if (!one_ctx) return "npg_columns_create: arguments of different contexts";
    if (partitioned)
        return "npg_columns_create: a partitioned locator (npg_locator_create_cells) is refused - a column runs through the cells of "
               "several ranks, and stitching its pieces together is not implemented";
    if (loc_ncell != fe_ncell)
        return "npg_columns_create: the locator was built for another mesh (an embedded 2-D engine has no locator: column integrals "
               "need a tetrahedral mesh)";
    return "";
}

// seg_n: the length of segments_out, -1 = not given
inline std::string check_columns_compute(bool null_arg, bool one_ctx, int64_t n_inv, int64_t n_b, int64_t x_inv_n, int64_t b_n,
                                         int64_t out_n, int64_t seg_n, int64_t ncol, int64_t nseg) {
    if (null_arg) return "npg_columns_compute: NULL argument";
    if (!one_ctx) return "npg_columns_compute: arguments of different contexts";
    const std::string m = check_state_vectors("npg_columns_compute", n_inv, n_b, x_inv_n, b_n);
    if (!m.empty()) return m;
    if (out_n != (int64_t)(kNColI + kNColE) * ncol)
        return msgf("npg_columns_compute: out must hold %d ncol = %lld entries, got %lld", kNColI + kNColE,
                    (long long)(kNColI + kNColE) * ncol, (long long)out_n);
    if (seg_n >= 0 && seg_n != (int64_t)kNColI * nseg)
        return msgf("npg_columns_compute: segments_out must hold %d nseg = %lld entries, got %lld", kNColI, (long long)kNColI * nseg,
                    (long long)seg_n);
    return "";
}

}  // namespace npg
