// The adjoint of the tangent load (npg_fe_tangent_adjoint): what ONE cell adds to the transpose of tangent_core.h's
//     T_i = int ( u_base . grad db + du . grad b_base + du_z N2 ) phi_i
// at the same base state.  With lam_h = sum_i lam_i phi_i (lam reads 0 on a Dirichlet DoF, as pert_val does)
//     g_b[j]      = int lam_h u_base . grad phi_j                         (u_base with its Dirichlet values)
//     g_x[(j, a)] = int lam_h (d_a b_base + N2 delta_az) phi^u_j          (b_base with its Dirichlet values; pressure rows are 0)
// so that <lam, T(db, dx)> = <g_b, db> + <g_x, dx> for all lam, db, dx.  Both are load vectors with lam_h as a weight.
// The arithmetic shared by the device kernel (tangent_adjoint.hip) and the host library (csrc_host/nupgcm_host.cpp), with the argument
// checks of the entry point.  Always fp64.
//
// THE ORDER OF THE SUMS is part of this header.  Per cell, with wl_q = (qw[q] wdet) lam_q, lam_q and the other nodal sums over local
// nodes ascending from 0:
//     g_b   acc_j += dn_j0 t_0 + dn_j1 t_1 + dn_j2 t_2 + dn_j3 t_3,   t_k = G[3k] f_0 + G[3k+1] f_1 + G[3k+2] f_2,   f_a = wl_q u_q,a
//           over all q, ascending
//     g_x   acc_(3i+a) += c_a N2shape_i(q),   c_a = wl_q g_a (a = 0, 1),   c_2 = wl_q (g_2 + N2),   g = grad b_base at q as tangent_core.h
//           forms it, over all q, ascending
// One output after the other: the velocity (30 values) is live beside lam[NB] and acc[NB] for g_b; b_base[NB] beside lam[NB] and
// acc[30] for g_x.  A row is then the sum of its local entries in cell-ascending order (the engine's inverted indices).
//
// S: the shape tables - qw[q], N2[10 q + i], Nb[NB q + i], dNb[4 (NB q + i) + k].  T: the cell tables (cell_view.h); local entry j of
// g_b goes to loc_b[t.at(j, NB, c)], local entry l < 30 of g_x to loc_x[t.at(l, 34, c)] - the layout the inverted index of the
// inversion rows addresses; its four pressure entries (l = 30..33) are never written here: they stay the zeros they were set to.
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <string>

#include "cell_view.h"
#include "tangent_core.h"

namespace npg {

// lam_h at quadrature point q times the point's weight
template <int NB, class S>
NPG_HD double adjoint_weight(const S &s, double wdet, int q, const double *lam) {
    double lq = 0;
NPG_UNROLL
    for (int i = 0; i < NB; ++i) lq += s.Nb[q * NB + i] * lam[i];
    return (s.qw[q] * wdet) * lq;
}

// g_b of cell c
template <int NB, class S, class T>
NPG_HD void cell_adjoint_b(const S &s, const T &t, int nq, const double *G, double wdet, const double *x_base, const double *lam, int64_t c,
                           double *loc_b) {
    double v[30], acc[NB];
NPG_UNROLL
    for (int l = 0; l < 30; ++l) v[l] = t.u(x_base, l, c);
NPG_UNROLL
    for (int j = 0; j < NB; ++j) acc[j] = 0.0;
    for (int q = 0; q < nq; ++q) {
        const double wl = adjoint_weight<NB>(s, wdet, q, lam);
        double ux = 0, uy = 0, uz = 0;
NPG_UNROLL
        for (int i = 0; i < 10; ++i) {
            const double n = s.N2[q * 10 + i];
            ux += n * v[3 * i];
            uy += n * v[3 * i + 1];
            uz += n * v[3 * i + 2];
        }
        const double f0 = wl * ux, f1 = wl * uy, f2 = wl * uz;
        const double t0 = G[0] * f0 + G[1] * f1 + G[2] * f2;
        const double t1 = G[3] * f0 + G[4] * f1 + G[5] * f2;
        const double t2 = G[6] * f0 + G[7] * f1 + G[8] * f2;
        const double t3 = G[9] * f0 + G[10] * f1 + G[11] * f2;
NPG_UNROLL
        for (int j = 0; j < NB; ++j) {
            const double *dn = &s.dNb[(q * NB + j) * 4];
            acc[j] += dn[0] * t0 + dn[1] * t1 + dn[2] * t2 + dn[3] * t3;
        }
    }
NPG_UNROLL
    for (int j = 0; j < NB; ++j) loc_b[t.at(j, NB, c)] = acc[j];
}

// the 30 velocity entries of g_x of cell c
template <int NB, class S, class T>
NPG_HD void cell_adjoint_x(const S &s, const T &t, int nq, double N2, const double *G, double wdet, const double *b_base, const double *lam,
                           int64_t c, double *loc_x) {
    double sc[NB], acc[30];
NPG_UNROLL
    for (int i = 0; i < NB; ++i) sc[i] = t.b(b_base, i, c);
NPG_UNROLL
    for (int l = 0; l < 30; ++l) acc[l] = 0.0;
    for (int q = 0; q < nq; ++q) {
        const double wl = adjoint_weight<NB>(s, wdet, q, lam);
        double gl0 = 0, gl1 = 0, gl2 = 0, gl3 = 0;
NPG_UNROLL
        for (int i = 0; i < NB; ++i) {
            const double *dn = &s.dNb[(q * NB + i) * 4];
            gl0 += dn[0] * sc[i];
            gl1 += dn[1] * sc[i];
            gl2 += dn[2] * sc[i];
            gl3 += dn[3] * sc[i];
        }
        const double gx = gl0 * G[0] + gl1 * G[3] + gl2 * G[6] + gl3 * G[9];
        const double gy = gl0 * G[1] + gl1 * G[4] + gl2 * G[7] + gl3 * G[10];
        const double gz = gl0 * G[2] + gl1 * G[5] + gl2 * G[8] + gl3 * G[11];
        const double c0 = wl * gx, c1 = wl * gy, c2 = wl * (gz + N2);
NPG_UNROLL
        for (int i = 0; i < 10; ++i) {
            const double n = s.N2[q * 10 + i];
            acc[3 * i] += c0 * n;
            acc[3 * i + 1] += c1 * n;
            acc[3 * i + 2] += c2 * n;
        }
    }
NPG_UNROLL
    for (int l = 0; l < 30; ++l) loc_x[t.at(l, 34, c)] = acc[l];
}

// pass 1: both local vectors of cell c, one after the other
template <int NB, class S, class T>
NPG_HD void cell_tangent_adjoint(const S &s, const T &t, int nq, double N2, const double *b_base, const double *x_base, const double *lam_vec,
                                 int64_t c, double *loc_b, double *loc_x) {
    double G[12], lam[NB];
NPG_UNROLL
    for (int k = 0; k < 12; ++k) G[k] = t.G(k, c);
    const double wdet = t.wdet(c);
NPG_UNROLL
    for (int i = 0; i < NB; ++i) lam[i] = pert_val(lam_vec, t.cb(i, c));
    cell_adjoint_b<NB>(s, t, nq, G, wdet, x_base, lam, c, loc_b);
    cell_adjoint_x<NB>(s, t, nq, N2, G, wdet, b_base, lam, c, loc_x);
}

// an output that is one of the three inputs or the other output (handles compared: every output against every input)
inline bool adjoint_outputs_alias(const void *b_base, const void *x_base, const void *lam, const void *out_b, const void *out_x) {
    for (const void *o : {out_b, out_x})
        for (const void *in : {b_base, x_base, lam})
            if (o == in) return true;
    return out_b == out_x;
}

// npg_fe_tangent_adjoint's arguments, for both libraries ("" = fine; nothing has been launched or allocated yet)
inline std::string check_tangent_adjoint(bool any_null, bool aliased, double N2, int64_t n_inv, int64_t n_b, int64_t b_base_n, int64_t x_base_n,
                                         int64_t lam_n, int64_t out_b_n, int64_t out_x_n, bool one_ctx) {
    if (any_null) return "npg_fe_tangent_adjoint: NULL argument";
    if (!(N2 == N2) || N2 - N2 != 0.0) return "npg_fe_tangent_adjoint: N2 must be finite";
    std::string m = check_state_vectors("npg_fe_tangent_adjoint (base state)", n_inv, n_b, x_base_n, b_base_n);
    if (!m.empty()) return m;
    if (lam_n != n_b) return msgf("npg_fe_tangent_adjoint: the multiplier has %lld entries, expected %lld", (long long)lam_n, (long long)n_b);
    m = check_state_vectors("npg_fe_tangent_adjoint (output)", n_inv, n_b, out_x_n, out_b_n);
    if (!m.empty()) return m;
    if (aliased) return "npg_fe_tangent_adjoint: an output must not be an input or the other output";
    if (!one_ctx) return "npg_fe_tangent_adjoint: arguments of different contexts";
    return "";
}

}  // namespace npg
