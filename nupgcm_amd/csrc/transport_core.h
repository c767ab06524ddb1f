// The tracers' transport operator as a matrix (npg_tracers_transport_*): equilibria and implicit-advection steps of the
// passive tracers with a frozen flow.  The arithmetic shared by the device kernels (tracers.hip) and the host library
// (csrc_host/nupgcm_host.cpp), as redi_core.h is for the rotated tensor: both evaluate the same expressions, point by point.  The
// reference has no counterpart.
//
//    C_ij  = sum_{cells, q} W phi_i(q) ( u(q) . grad phi_j(q) ),      W = w_q |J|,  u(q) = scale sum_a N2[q][a] u_a
//    g_k,i = int ( S_k - u_z Gamma_k - u . grad c_D,k - lambda_k c_D,k ) phi_i
//            - kappa^ int ( kappa_h grad_h c_D,k . grad_h phi_i + kappa_v d_z c_D,k d_z phi_i )  + kappa^ Gamma_k rhs_diff1_i + flux_k,i
//
// cell_transport_velocity   the three tables ux, uy, uz of ONE cell at its quadrature points (from the cell's 30 velocity values)
// transport_entry           what one quadrature point adds to entry (i, j) of C: (w phi_i)(ux g_jx + uy g_jy + uz g_jz) - u = 0 gives
//                           exact zeros
// cell_transport_load       what ONE cell adds to the local load vectors of K tracers: the velocity tables are read once per cell, then a
//                           loop over the tracers reloads only the tracer's Dirichlet values; the last two terms of g ride on
//                           tracer_row (tracers_core.h) with theta = kappa^ and dt = 1
// check_transport           every argument check of the entry points, for both libraries
//
// Everything here is fp64 whatever npg_fe_set_precision says: an equilibrium solve amplifies the operator's rounding by its condition.
//
// S: the shape tables - qw[q], N2[10 q + a], Nb[NB q + i], dNb[4 (NB q + i) + k].  T: the cell tables (cell_view.h) and the three
// velocity tables (TransportCells).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "cell_view.h"
#include "tracers_core.h"

namespace npg {

enum { kTransportOff = 0, kTransportUpdated = 1 };      // the state npg_tracers_transport_info reports

// the tracers' view of the cell tables with the velocity tables ([nq] per cell in the view's layout)
template <class View>
struct TransportCells : View {
    const double *ux_, *uy_, *uz_;
    NPG_HD size_t loc(int i, int64_t c) const { return this->at(i, this->nb, c); }
    NPG_HD double ux(int q, int64_t c) const { return ux_[this->at(q, this->nq, c)]; }
    NPG_HD double uy(int q, int64_t c) const { return uy_[this->at(q, this->nq, c)]; }
    NPG_HD double uz(int q, int64_t c) const { return uz_[this->at(q, this->nq, c)]; }
};

template <class S, class T>
NPG_HD void cell_transport_velocity(const S &s, const T &t, int nq, double scale, const double *xi, int64_t c, double *ux, double *uy,
                                    double *uz) {
    double un[30];
NPG_UNROLL
    for (int l = 0; l < 30; ++l) un[l] = t.u(xi, l, c);
    for (int q = 0; q < nq; ++q) {
        double ax = 0, ay = 0, az = 0;
NPG_UNROLL
        for (int i = 0; i < 10; ++i) {
            const double n = s.N2[q * 10 + i];
            ax += n * un[3 * i];
            ay += n * un[3 * i + 1];
            az += n * un[3 * i + 2];
        }
        const size_t o = t.at(q, nq, c);
        ux[o] = scale * ax, uy[o] = scale * ay, uz[o] = scale * az;
    }
}

// w = qw wdet; phi_i: the row's basis function at the point; gj: the physical gradient of the column's
NPG_HD double transport_entry(double w, double phi_i, double ux, double uy, double uz, double gjx, double gjy, double gjz) {
    return (w * phi_i) * (ux * gjx + uy * gjy + uz * gjz);
}

// decay: [ntracer] or null (= 0).  ts.c / ts.c_prev are not read.  U: the storage of the cell's nq x 3 velocities across the loop over
// the tracers, as in cell_tracers (uq(3 q + a): on the device a per-lane column of LDS, on the host a local array).
template <int NB, class S, class T, class U>
NPG_HD void cell_transport_load(const S &s, const T &t, U &uq, int nq, double kappa_hat, const double *decay, const TracerSet &ts, int64_t c) {
    double G[12];
NPG_UNROLL
    for (int k = 0; k < 12; ++k) G[k] = t.G(k, c);
    const double wdet = t.wdet(c);
    for (int q = 0; q < nq; ++q) uq(3 * q) = t.ux(q, c), uq(3 * q + 1) = t.uy(q, c), uq(3 * q + 2) = t.uz(q, c);      // once per cell
    for (int k = 0; k < ts.ntracer; ++k) {
        const double *dk = ts.diri + (size_t)k * ts.n_diri;
        const double gam = ts.gamma[k], src = ts.source[k], lam = decay ? decay[k] : 0.0;
        double cd[NB], acc[NB];
        bool lift = false;
NPG_UNROLL
        for (int i = 0; i < NB; ++i) {
            const int32_t idx = t.cb(i, c);
            cd[i] = idx < 0 ? dk[-1 - idx] : 0.0;
            lift = lift || cd[i] != 0.0;
            acc[i] = 0.0;
        }
        for (int q = 0; q < nq; ++q) {
            const double w = s.qw[q] * wdet;
            const double ux = uq(3 * q), uy = uq(3 * q + 1), uz = uq(3 * q + 2);
            double integrand = src - uz * gam;
            if (lift) {
                double cq = 0, gl0 = 0, gl1 = 0, gl2 = 0, gl3 = 0;
NPG_UNROLL
                for (int i = 0; i < NB; ++i) {
                    cq += s.Nb[q * NB + i] * cd[i];
                    const double *dn = &s.dNb[(q * NB + i) * 4];
                    gl0 += dn[0] * cd[i];
                    gl1 += dn[1] * cd[i];
                    gl2 += dn[2] * cd[i];
                    gl3 += dn[3] * cd[i];
                }
                const double gx = gl0 * G[0] + gl1 * G[3] + gl2 * G[6] + gl3 * G[9];
                const double gy = gl0 * G[1] + gl1 * G[4] + gl2 * G[7] + gl3 * G[10];
                const double gz = gl0 * G[2] + gl1 * G[5] + gl2 * G[8] + gl3 * G[11];
                integrand -= (ux * gx + uy * gy + uz * gz) + lam * cq;
                const double kh = kappa_hat * t.kh(q, c), kv = kappa_hat * t.kv(q, c);
                const double ax = kh * gx, ay = kh * gy, az = kv * gz;
NPG_UNROLL
                for (int i = 0; i < NB; ++i) {
                    const double *dn = &s.dNb[(q * NB + i) * 4];
                    const double px = dn[0] * G[0] + dn[1] * G[3] + dn[2] * G[6] + dn[3] * G[9];
                    const double py = dn[0] * G[1] + dn[1] * G[4] + dn[2] * G[7] + dn[3] * G[10];
                    const double pz = dn[0] * G[2] + dn[1] * G[5] + dn[2] * G[8] + dn[3] * G[11];
                    acc[i] -= w * (ax * px + ay * py + az * pz);
                }
            }
            const double wq = w * integrand;
NPG_UNROLL
            for (int i = 0; i < NB; ++i) acc[i] += wq * s.Nb[q * NB + i];
        }
        double *lk = ts.loc + (size_t)k * ts.loc_stride;
NPG_UNROLL
        for (int i = 0; i < NB; ++i) lk[t.loc(i, c)] = acc[i];
    }
}

// ---- the argument checks of npg_tracers_transport_update / _matrix / _load / _tables ("" = fine) ----------------------------------------
struct TransportCheck {
    const char *who;
    bool same_ctx = true;            // every handle of the call lives in the tracers' context
    // update: the scale, the flow vector, whether the engine is an embedded 2-D one
    bool update = false;
    double scale = 1.0;
    int64_t n_inv = 0, vec_n = -1;
    bool flat = false;
    // matrix / load / tables: the state the call needs and the one the handle is in
    int need = kTransportOff, state = kTransportOff;
    // matrix: its shape and whether it is a plain CSR matrix
    int64_t n_b = 0, mat_m = -1, mat_n = -1;
    bool mat_plain = true;
    // load: kappa^, the decay rates (or null), the sizes of the vectors (-1: absent), which tables the tracers need
    bool load = false;
    double kappa_hat = 0.0;
    const double *decay = nullptr;
    int ntracer = 0;
    int64_t diff1_n = -1, flux_n = -1, out_n = -1;
    bool need_diff1 = false, need_coeff = false;
};

inline std::string check_transport(const TransportCheck &a) {
    if (!a.same_ctx) return msgf("%s: arguments of different contexts", a.who);
    if (a.update) {
        if (a.flat) return msgf("%s: an embedded 2-D engine is refused (the operator is written for tetrahedra)", a.who);
        if (!std::isfinite(a.scale)) return msgf("%s: scale must be finite, got %g", a.who, a.scale);
        if (a.vec_n != a.n_inv) return msgf("%s: the flow vector has %lld entries, expected %lld", a.who, (long long)a.vec_n, (long long)a.n_inv);
        return "";
    }
    if (a.load) {
        if (!std::isfinite(a.kappa_hat) || a.kappa_hat < 0.0) return msgf("%s: kappa_hat must be finite and >= 0, got %g", a.who, a.kappa_hat);
        if (a.decay)
            for (int k = 0; k < a.ntracer; ++k)
                if (!std::isfinite(a.decay[k]) || a.decay[k] < 0.0)
                    return msgf("%s: a decay rate must be finite and >= 0, tracer %d has %g", a.who, k, a.decay[k]);
    }
    if (a.need == kTransportUpdated && a.state != kTransportUpdated)
        return msgf("%s: the velocity tables have not been built (call npg_tracers_transport_update first)", a.who);
    if (a.mat_m >= 0) {
        if (!a.mat_plain) return msgf("%s: the matrix is not a plain CSR matrix on the buoyancy pattern", a.who);
        if (a.mat_m != a.n_b || a.mat_n != a.n_b)
            return msgf("%s: the matrix is %lld x %lld, not the buoyancy pattern (n_b = %lld)", a.who, (long long)a.mat_m, (long long)a.mat_n,
                        (long long)a.n_b);
    }
    if (a.load) {
        const long long want = (long long)a.ntracer * a.n_b;
        if (a.out_n != want) return msgf("%s: the output vector must have ntracer * n_b = %lld entries, got %lld", a.who, want, (long long)a.out_n);
        if (a.flux_n >= 0 && a.flux_n != want) return msgf("%s: flux must have ntracer * n_b = %lld entries", a.who, want);
        if (a.diff1_n >= 0 && a.diff1_n != a.n_b) return msgf("%s: rhs_diff1 must have n_b = %lld entries", a.who, (long long)a.n_b);
        if (a.need_diff1 && a.diff1_n < 0) return msgf("%s: a tracer has a background gradient but rhs_diff1 is NULL", a.who);
        if (a.need_coeff) return msgf("%s: a tracer has non-zero Dirichlet values but the coefficients kappa_h / kappa_v have not been set", a.who);
    }
    return "";
}

}  // namespace npg
