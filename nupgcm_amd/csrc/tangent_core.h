// The tangent of the advection load (npg_fe_tangent_rhs): what ONE cell adds to the directional derivative of
//     adv(x, b)_i = int ( u . grad b + w N2 ) phi_i
// at a base state (b_base, x_base) along a perturbation (db, dx):
//     T_i = int ( u_base . grad db + du . grad b_base + du_z N2 ) phi_i .
// The arithmetic shared by the device kernel (linearized.hip) and the host library (csrc_host/nupgcm_host.cpp), with the argument
// checks of the entry point: GPU() and CPU() evaluate the same expressions in the same order, cell by cell.  Always fp64.
//
// The base state reads the engine's Dirichlet tables, as npg_fe_advection_rhs reads b / x_inv.  A perturbation has no Dirichlet
// values: a negative DoF code reads 0.
//
// THE ORDER OF THE SUMS is part of this header.  Per cell, from acc = 0:
//     first   acc_i += (wq (u_base_q . grad db_q)) phi_i(q)                     over all q, ascending
//     then    acc_i += (wq (du_q . grad b_base_q + du_z,q N2)) phi_i(q)         over all q, ascending
// with wq = qw[q] wdet and the inner sums over local nodes ascending from 0.  Two loops, not one: one velocity (30 values) and one
// scalar (NB values) are live at a time beside G[12] and acc[NB], against 80 nodal values if the four fields were loaded up front.
//
// S: the shape tables - qw[q], N2[10 q + i], Nb[NB q + i], dNb[4 (NB q + i) + k].  T: the cell tables (cell_view.h); local entry i
// of cell c goes to loc[t.at(i, NB, c)].
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "cell_view.h"

namespace npg {

// a perturbation's value at DoF code idx: Dirichlet nodes carry none
NPG_HD double pert_val(const double *x, int32_t idx) { return idx >= 0 ? x[idx] : 0.0; }

// acc_i += sum_q wq (v_q . grad s_q [+ vz_q N2]) phi_i(q) for the nodal velocity v[30] and the nodal scalar sc[NB]
template <int NB, bool WITH_N2, class S>
NPG_HD void tangent_term(const S &s, const double *G, double wdet, int nq, double N2, const double *v, const double *sc, double *acc) {
    for (int q = 0; q < nq; ++q) {
        double gl0 = 0, gl1 = 0, gl2 = 0, gl3 = 0;
NPG_UNROLL
        for (int i = 0; i < NB; ++i) {
            const double *dn = &s.dNb[(q * NB + i) * 4];
            gl0 += dn[0] * sc[i];
            gl1 += dn[1] * sc[i];
            gl2 += dn[2] * sc[i];
            gl3 += dn[3] * sc[i];
        }
        double ux = 0, uy = 0, uz = 0;
NPG_UNROLL
        for (int i = 0; i < 10; ++i) {
            const double n = s.N2[q * 10 + i];
            ux += n * v[3 * i];
            uy += n * v[3 * i + 1];
            uz += n * v[3 * i + 2];
        }
        const double gx = gl0 * G[0] + gl1 * G[3] + gl2 * G[6] + gl3 * G[9];
        const double gy = gl0 * G[1] + gl1 * G[4] + gl2 * G[7] + gl3 * G[10];
        const double gz = gl0 * G[2] + gl1 * G[5] + gl2 * G[8] + gl3 * G[11];
        const double integrand = WITH_N2 ? ux * gx + uy * gy + uz * gz + uz * N2 : ux * gx + uy * gy + uz * gz;
        const double wq = s.qw[q] * wdet * integrand;
NPG_UNROLL
        for (int i = 0; i < NB; ++i) acc[i] += wq * s.Nb[q * NB + i];
    }
}

// pass 1: the local vector of cell c
template <int NB, class S, class T>
NPG_HD void cell_tangent(const S &s, const T &t, int nq, double N2, const double *b_base, const double *x_base, const double *db,
                         const double *dx, int64_t c, double *loc) {
    double G[12];
NPG_UNROLL
    for (int k = 0; k < 12; ++k) G[k] = t.G(k, c);
    const double wdet = t.wdet(c);
    double acc[NB];
NPG_UNROLL
    for (int i = 0; i < NB; ++i) acc[i] = 0.0;
    {   // u_base . grad db: the perturbation feels no N2
        double v[30], sc[NB];
NPG_UNROLL
        for (int l = 0; l < 30; ++l) v[l] = t.u(x_base, l, c);
NPG_UNROLL
        for (int i = 0; i < NB; ++i) sc[i] = pert_val(db, t.cb(i, c));
        tangent_term<NB, false>(s, G, wdet, nq, 0.0, v, sc, acc);
    }
    {   // du . grad b_base + du_z N2
        double v[30], sc[NB];
NPG_UNROLL
        for (int l = 0; l < 30; ++l) v[l] = pert_val(dx, t.cu(l, c));
NPG_UNROLL
        for (int i = 0; i < NB; ++i) sc[i] = t.b(b_base, i, c);
        tangent_term<NB, true>(s, G, wdet, nq, N2, v, sc, acc);
    }
NPG_UNROLL
    for (int i = 0; i < NB; ++i) loc[t.at(i, NB, c)] = acc[i];
}

// npg_fe_tangent_rhs's arguments, for both libraries ("" = fine; nothing has been launched yet)
inline std::string check_tangent(bool any_null, double N2, int64_t n_inv, int64_t n_b, int64_t b_base_n, int64_t x_base_n, int64_t db_n,
                                 int64_t dx_n, int64_t out_n, bool one_ctx) {
    if (any_null) return "npg_fe_tangent_rhs: NULL argument";
    if (!(N2 == N2) || N2 - N2 != 0.0) return "npg_fe_tangent_rhs: N2 must be finite";
    std::string m = check_state_vectors("npg_fe_tangent_rhs (base state)", n_inv, n_b, x_base_n, b_base_n);
    if (!m.empty()) return m;
    m = check_state_vectors("npg_fe_tangent_rhs (perturbation)", n_inv, n_b, dx_n, db_n);
    if (!m.empty()) return m;
    if (out_n != n_b) return msgf("npg_fe_tangent_rhs: the output vector has %lld entries, expected %lld", (long long)out_n, (long long)n_b);
    if (!one_ctx) return "npg_fe_tangent_rhs: arguments of different contexts";
    return "";
}

}  // namespace npg
