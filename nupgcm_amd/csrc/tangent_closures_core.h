// The derivatives of the convection and eddy closures (npg_fe_tangent_diffusion, npg_fe_tangent_eddy, npg_fe_tangent_eddy_adjoint,
// DESIGN.md 35): what ONE cell adds to three load vectors of the linearised model when kappa_v and nu depend on the base buoyancy.
// With s = alpha (N2 + d_z b_base) at a quadrature point (b_base with its Dirichlet values; `abz` of the engine's closure kernel):
//     convection   kappa_v(s) = kappa_v0 + kappa_c (1 + tanh(-s / m)) / 2,        m = N2min
//                  kappa_eff  = kappa_v(s) + s kappa_v'(s),   kappa_v'(s) = -kappa_c (1 - tanh^2(s / m)) / (2 m)
//                  (D_v db)_i = int kappa_eff d_z db d_z phi_i                    (db reads 0 on a Dirichlet DoF)
//     eddy         nu(s) = LSE_beta(nu_min, nu_e),   nu_e = f^2 / sqrt(n^2 + s^2),   n = N2min,   beta = smoothing
//                  nu'(s) = w (-nu_e s / (n^2 + s^2)),   w = e^(beta nu_e) / (e^(beta nu_min) + e^(beta nu_e))
//                  r_x[(i, a)] = -a2e2 int dnu ( grad u_a . grad phi_i  [+ sum_c d_a u_c d_c phi_i  if full_stress] ),
//                                dnu = nu'(s) alpha d_z db                        (u = x_base with its Dirichlet values)
//                  g[j]        = -a2e2 int nu'(s) alpha d_z phi^b_j E,   E = sum_{a,c} d_c mu_a (d_c u_a [+ d_a u_c])
//                                                                                 (mu reads 0 on a Dirichlet DoF)
// so that <mu, r_x(db)> = <g(mu), db> and <lam, D_v db> = <D_v lam, db>.  The arithmetic shared by the device kernels
// (tangent_closures.hip) and the host library (csrc_host/nupgcm_host.cpp), with the argument checks of the entry points.  Always fp64.
//
// tanh and exp are NOT the libraries': two implementations of them differ in the last bits, and the two libraries must agree in every
// bit.  closure_exp below is built from +, -, *, the conversion to an integer and an exponent written into the bits - the same result
// wherever IEEE arithmetic runs without contraction - and the closures use it through
//     E = closure_exp(-2 |s| / m):   (1 + tanh(-s / m)) / 2 = (s >= 0 ? E : 1) / (1 + E),   1 - tanh^2(s / m) = 4 E / (1 + E)^2
//     E = closure_exp(-|d|), d = beta nu_e - beta nu_min:   w = (d >= 0 ? 1 : E) / (1 + E)
// (the max-shift of the engine's LogSumExp: the larger exponent is 0).  sqrt and / are correctly rounded on both sides.
//
// THE ORDER OF THE SUMS is part of this header.  Per cell, gz_i(q) = dn_i0 Gz0 + dn_i1 Gz1 + dn_i2 Gz2 + dn_i3 Gz3 (Gz_k = G[3k + 2]),
// nodal sums over local nodes ascending from 0, wq = qw[q] wdet:
//     s        = alpha (N2 + sum_i b_i gz_i)                                      (the expression of the engine's closure kernel)
//     D_v      acc_i += (wq (kappa_eff (sum_j db_j gz_j))) gz_i                   over all q, ascending
//     r_x      J[a][c] = sum_j u_(3j+a) g_jc,  g_j = grad of velocity shape j as fe.hip's grad_u forms it;
//              M[a][c] = full_stress ? J[a][c] + J[c][a] : J[a][c];   wd = -(a2e2 (wq (nu'(s) (alpha (sum_j db_j gz_j)))));
//              acc_(3i+a) += wd (M[a][0] g_i0 + M[a][1] g_i1 + M[a][2] g_i2)      over all q, ascending
//     g        Jm[a][c] = sum_j mu_(3j+a) g_jc;   E = sum_a (Jm[a][0] M[a][0] + Jm[a][1] M[a][1] + Jm[a][2] M[a][2]), a ascending;
//              acc_j += (-(a2e2 (wq ((nu'(s) alpha) E)))) gz_j                    over all q, ascending
// A row is then the sum of its local entries in cell-ascending order (the engine's inverted indices).
//
// S: the shape tables - qw[q], dN2[4 (10 q + i) + k], dNb[4 (NB q + i) + k].  T: the cell tables (cell_view.h).  kv0 / f: the
// background kappa_v and the Coriolis table at the quadrature points, in the view's layout (t.at(q, nq, c)).  Local entry i of a
// buoyancy load goes to loc[t.at(i, NB, c)], local entry l < 30 of r_x to loc_x[t.at(l, 34, c)]; the four pressure entries of loc_x
// are never written: they stay the zeros they were set to.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <string>

#include "cell_view.h"
#include "tangent_core.h"

namespace npg {

// e^x for x <= 0 (0 below -708; x > 0 is treated as 0): k = round(x / ln 2), r = x - k ln 2 in two pieces (|r| <= 0.35; ln2_hi =
// 0x3FE62E42FEE00000 has 32 significant bits, |k| < 1024 needs 10 more: k ln2_hi is exact), a Taylor
// polynomial of degree 13 by Horner (remainder < 3e-18 relative), scaled by 2^k through the exponent bits.  About 1 ulp; what matters
// is that every operation is an IEEE one, so the device and the host return the same bits.
NPG_HD double closure_exp(double x) {
    if (!(x < 0.0)) return 1.0;
    if (x < -708.0) return 0.0;
    const double kf = (double)(int64_t)(x * 1.4426950408889634 - 0.5);      // truncation toward zero of a negative number: round half up
    const double r = (x - kf * 0.693147180369123816490) - kf * 1.90821492927058770002e-10;
    double p = 1.0 / 6227020800.0;
    p = p * r + 1.0 / 479001600.0;
    p = p * r + 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    p = p * r + 0.5;
    p = p * r + 1.0;
    p = p * r + 1.0;
    const uint64_t bits = (uint64_t)((int64_t)kf + 1023) << 52;             // 2^k, k in [-1022, 0]
    double scale;
    __builtin_memcpy(&scale, &bits, sizeof scale);
    return p * scale;
}

struct ConvClosure {
    double kappa_c, N2min;
};
struct EddyClosure {
    double N2min, smoothing, nu_min;
};

// kappa_eff = kappa_v(s) + s kappa_v'(s); kappa_c = 0: the background alone, whatever s is
NPG_HD double conv_kappa_eff(const ConvClosure &cl, double kv0, double s) {
    if (cl.kappa_c == 0.0) return kv0;
    const double a = s < 0.0 ? -s : s;
    const double E = closure_exp(-2.0 * a / cl.N2min);
    const double d = 1.0 + E;
    const double h = (s >= 0.0 ? E : 1.0) / d;               // (1 + tanh(-s / m)) / 2
    const double sech2 = 4.0 * E / (d * d);                  // 1 - tanh^2(s / m)
    const double dk = -cl.kappa_c * sech2 / (2.0 * cl.N2min);
    return (kv0 + cl.kappa_c * h) + s * dk;
}

// nu'(s)
NPG_HD double eddy_nu_prime(const EddyClosure &cl, double f, double s) {
    const double r2 = cl.N2min * cl.N2min + s * s;
    const double nue = f * (f / sqrt(r2));                   // the engine's expression
    const double d = cl.smoothing * nue - cl.smoothing * cl.nu_min;
    const double E = closure_exp(d < 0.0 ? d : -d);
    const double w = (d >= 0.0 ? 1.0 : E) / (1.0 + E);
    return w * (-(nue * s) / r2);
}

// gz_i(q), i < NB: d_z of the buoyancy shape functions
template <int NB, class S>
NPG_HD void closure_gz(const S &s, const double *Gz, int q, double *gz) {
NPG_UNROLL
    for (int i = 0; i < NB; ++i) {
        const double *dn = &s.dNb[(q * NB + i) * 4];
        gz[i] = dn[0] * Gz[0] + dn[1] * Gz[1] + dn[2] * Gz[2] + dn[3] * Gz[3];
    }
}

// pass 1 of npg_fe_tangent_diffusion
template <int NB, class S, class T>
NPG_HD void cell_tangent_diffusion(const S &s, const T &t, int nq, const ConvClosure &cl, double alpha, double N2, const double *kv0,
                                   const double *b_base, const double *db, int64_t c, double *loc) {
    double Gz[4], bn[NB], dn[NB], acc[NB];
NPG_UNROLL
    for (int k = 0; k < 4; ++k) Gz[k] = t.G(3 * k + 2, c);
    const double wdet = t.wdet(c);
NPG_UNROLL
    for (int i = 0; i < NB; ++i) {
        const int32_t code = t.cb(i, c);
        bn[i] = field_val(b_base, t.bdiri, code);
        dn[i] = pert_val(db, code);
        acc[i] = 0.0;
    }
    for (int q = 0; q < nq; ++q) {
        double gz[NB];
        closure_gz<NB>(s, Gz, q, gz);
        double bz = 0.0, dz = 0.0;
NPG_UNROLL
        for (int i = 0; i < NB; ++i) {
            bz += bn[i] * gz[i];
            dz += dn[i] * gz[i];
        }
        const double sv = alpha * (N2 + bz);
        const double w = (s.qw[q] * wdet) * (conv_kappa_eff(cl, kv0[t.at(q, nq, c)], sv) * dz);
NPG_UNROLL
        for (int i = 0; i < NB; ++i) acc[i] += w * gz[i];
    }
NPG_UNROLL
    for (int i = 0; i < NB; ++i) loc[t.at(i, NB, c)] = acc[i];
}

// J[a][c] = sum_j v_(3j+a) g_jc at quadrature point q: the gradient of a nodal velocity
template <class S>
NPG_HD void closure_grad_u(const S &s, const double *G, int q, const double *v, double J[3][3]) {
NPG_UNROLL
    for (int a = 0; a < 3; ++a) J[a][0] = J[a][1] = J[a][2] = 0.0;
NPG_UNROLL
    for (int j = 0; j < 10; ++j) {
        const double *dn = &s.dN2[(q * 10 + j) * 4];
        const double g0 = dn[0] * G[0] + dn[1] * G[3] + dn[2] * G[6] + dn[3] * G[9];
        const double g1 = dn[0] * G[1] + dn[1] * G[4] + dn[2] * G[7] + dn[3] * G[10];
        const double g2 = dn[0] * G[2] + dn[1] * G[5] + dn[2] * G[8] + dn[3] * G[11];
NPG_UNROLL
        for (int a = 0; a < 3; ++a) {
            J[a][0] += v[3 * j + a] * g0;
            J[a][1] += v[3 * j + a] * g1;
            J[a][2] += v[3 * j + a] * g2;
        }
    }
}

// M = J (+ J' if full_stress): what the viscous form contracts a test gradient with
NPG_HD void closure_stress(int full_stress, const double J[3][3], double M[3][3]) {
NPG_UNROLL
    for (int a = 0; a < 3; ++a)
NPG_UNROLL
        for (int c = 0; c < 3; ++c) M[a][c] = full_stress ? J[a][c] + J[c][a] : J[a][c];
}

// pass 1 of npg_fe_tangent_eddy: the 30 velocity entries of r_x of cell c
template <int NB, class S, class T>
NPG_HD void cell_tangent_eddy(const S &s, const T &t, int nq, double a2e2, int full_stress, const EddyClosure &cl, double alpha, double N2,
                              const double *f, const double *b_base, const double *x_base, const double *db, int64_t c, double *loc_x) {
    double G[12], Gz[4], bn[NB], dn[NB], v[30], acc[30];
NPG_UNROLL
    for (int k = 0; k < 12; ++k) G[k] = t.G(k, c);
NPG_UNROLL
    for (int k = 0; k < 4; ++k) Gz[k] = G[3 * k + 2];
    const double wdet = t.wdet(c);
NPG_UNROLL
    for (int i = 0; i < NB; ++i) {
        const int32_t code = t.cb(i, c);
        bn[i] = field_val(b_base, t.bdiri, code);
        dn[i] = pert_val(db, code);
    }
NPG_UNROLL
    for (int l = 0; l < 30; ++l) {
        v[l] = t.u(x_base, l, c);
        acc[l] = 0.0;
    }
    for (int q = 0; q < nq; ++q) {
        double gz[NB];
        closure_gz<NB>(s, Gz, q, gz);
        double bz = 0.0, dz = 0.0;
NPG_UNROLL
        for (int i = 0; i < NB; ++i) {
            bz += bn[i] * gz[i];
            dz += dn[i] * gz[i];
        }
        const double nup = eddy_nu_prime(cl, f[t.at(q, nq, c)], alpha * (N2 + bz));
        const double wd = -(a2e2 * ((s.qw[q] * wdet) * (nup * (alpha * dz))));
        double J[3][3], M[3][3];
        closure_grad_u(s, G, q, v, J);
        closure_stress(full_stress, J, M);
NPG_UNROLL
        for (int i = 0; i < 10; ++i) {
            const double *d4 = &s.dN2[(q * 10 + i) * 4];
            const double g0 = d4[0] * G[0] + d4[1] * G[3] + d4[2] * G[6] + d4[3] * G[9];
            const double g1 = d4[0] * G[1] + d4[1] * G[4] + d4[2] * G[7] + d4[3] * G[10];
            const double g2 = d4[0] * G[2] + d4[1] * G[5] + d4[2] * G[8] + d4[3] * G[11];
NPG_UNROLL
            for (int a = 0; a < 3; ++a) acc[3 * i + a] += wd * (M[a][0] * g0 + M[a][1] * g1 + M[a][2] * g2);
        }
    }
NPG_UNROLL
    for (int l = 0; l < 30; ++l) loc_x[t.at(l, 34, c)] = acc[l];
}

// pass 1 of npg_fe_tangent_eddy_adjoint
template <int NB, class S, class T>
NPG_HD void cell_tangent_eddy_adjoint(const S &s, const T &t, int nq, double a2e2, int full_stress, const EddyClosure &cl, double alpha,
                                      double N2, const double *f, const double *b_base, const double *x_base, const double *mu, int64_t c,
                                      double *loc) {
    double G[12], Gz[4], bn[NB], acc[NB], v[30], m[30];
NPG_UNROLL
    for (int k = 0; k < 12; ++k) G[k] = t.G(k, c);
NPG_UNROLL
    for (int k = 0; k < 4; ++k) Gz[k] = G[3 * k + 2];
    const double wdet = t.wdet(c);
NPG_UNROLL
    for (int i = 0; i < NB; ++i) {
        bn[i] = t.b(b_base, i, c);
        acc[i] = 0.0;
    }
NPG_UNROLL
    for (int l = 0; l < 30; ++l) {
        const int32_t code = t.cu(l, c);
        v[l] = field_val(x_base, t.udiri, code);
        m[l] = pert_val(mu, code);
    }
    for (int q = 0; q < nq; ++q) {
        double gz[NB];
        closure_gz<NB>(s, Gz, q, gz);
        double bz = 0.0;
NPG_UNROLL
        for (int i = 0; i < NB; ++i) bz += bn[i] * gz[i];
        const double nup = eddy_nu_prime(cl, f[t.at(q, nq, c)], alpha * (N2 + bz));
        double J[3][3], M[3][3], Jm[3][3];
        closure_grad_u(s, G, q, v, J);
        closure_stress(full_stress, J, M);
        closure_grad_u(s, G, q, m, Jm);
        double E = 0.0;
NPG_UNROLL
        for (int a = 0; a < 3; ++a) E += Jm[a][0] * M[a][0] + Jm[a][1] * M[a][1] + Jm[a][2] * M[a][2];
        const double w = -(a2e2 * ((s.qw[q] * wdet) * ((nup * alpha) * E)));
NPG_UNROLL
        for (int i = 0; i < NB; ++i) acc[i] += w * gz[i];
    }
NPG_UNROLL
    for (int i = 0; i < NB; ++i) loc[t.at(i, NB, c)] = acc[i];
}

inline bool closure_finite(double x) { return x == x && x - x == 0.0; }

// what the three entry points share ("" = fine): the base buoyancy, the input and the output of the sizes given, no aliasing, one context
inline std::string check_closure_common(const char *who, bool any_null, bool aliased, double N2min, double alpha, double N2, int64_t n_b,
                                        int64_t b_base_n, bool one_ctx) {
    if (any_null) return msgf("%s: NULL argument", who);
    if (!closure_finite(N2min) || !closure_finite(alpha) || !closure_finite(N2)) return msgf("%s: N2min, alpha and N2 must be finite", who);
    if (!(N2min > 0.0)) return msgf("%s: N2min must be positive, got %g", who, N2min);
    if (b_base_n != n_b) return msgf("%s: the base buoyancy vector has %lld entries, expected %lld", who, (long long)b_base_n, (long long)n_b);
    if (aliased) return msgf("%s: the output must not be an input", who);
    if (!one_ctx) return msgf("%s: arguments of different contexts", who);
    return "";
}

// npg_fe_tangent_diffusion's arguments, for both libraries (nothing has been launched yet)
inline std::string check_tangent_diffusion(bool any_null, bool aliased, bool have_kv0, double kappa_c, double N2min, double alpha, double N2,
                                           int64_t n_b, int64_t b_base_n, int64_t db_n, int64_t out_n, bool one_ctx) {
    const char *who = "npg_fe_tangent_diffusion";
    std::string m = check_closure_common(who, any_null, aliased, N2min, alpha, N2, n_b, b_base_n, one_ctx);
    if (!m.empty()) return m;
    if (!closure_finite(kappa_c)) return msgf("%s: kappa_c must be finite", who);
    if (db_n != n_b) return msgf("%s: the perturbation has %lld entries, expected %lld", who, (long long)db_n, (long long)n_b);
    if (out_n != n_b) return msgf("%s: the output vector has %lld entries, expected %lld", who, (long long)out_n, (long long)n_b);
    if (!have_kv0) return msgf("%s: background kappa_v has not been set", who);
    return "";
}

// npg_fe_tangent_eddy's (adjoint = false: in = db, n_b entries, out = r_x, n_inv entries) and npg_fe_tangent_eddy_adjoint's (adjoint =
// true: in = mu, n_inv entries, out = g, n_b entries) arguments, for both libraries (nothing has been launched or allocated yet)
inline std::string check_tangent_eddy(bool adjoint, bool any_null, bool aliased, bool have_f, double a2e2, int full_stress, double N2min,
                                      double alpha, double N2, double smoothing, double nu_min, int64_t n_inv, int64_t n_b, int64_t b_base_n,
                                      int64_t x_base_n, int64_t in_n, int64_t out_n, bool one_ctx) {
    const char *who = adjoint ? "npg_fe_tangent_eddy_adjoint" : "npg_fe_tangent_eddy";
    std::string m = check_closure_common(who, any_null, aliased, N2min, alpha, N2, n_b, b_base_n, one_ctx);
    if (!m.empty()) return m;
    if (!closure_finite(a2e2) || !closure_finite(smoothing) || !closure_finite(nu_min))
        return msgf("%s: a2e2, smoothing and nu_min must be finite", who);
    if (!(smoothing > 0.0)) return msgf("%s: smoothing must be positive, got %g", who, smoothing);
    if (full_stress != 0 && full_stress != 1) return msgf("%s: full_stress must be 0 or 1, got %d", who, full_stress);
    if (x_base_n != n_inv) return msgf("%s: the base flow vector has %lld entries, expected %lld", who, (long long)x_base_n, (long long)n_inv);
    const int64_t want_in = adjoint ? n_inv : n_b, want_out = adjoint ? n_b : n_inv;
    if (in_n != want_in)
        return msgf("%s: the %s has %lld entries, expected %lld", who, adjoint ? "multiplier" : "perturbation", (long long)in_n, (long long)want_in);
    if (out_n != want_out) return msgf("%s: the output vector has %lld entries, expected %lld", who, (long long)out_n, (long long)want_out);
    if (!have_f) return msgf("%s: coefficient f has not been set", who);
    return "";
}

// npg_fe_get_coeff's arguments
inline std::string check_get_coeff(bool any_null, int index, const char *name, bool is_set) {
    if (any_null) return "npg_fe_get_coeff: NULL argument";
    if (index < 0) return msgf("npg_fe_get_coeff: unknown coefficient '%s'", name);
    if (!is_set) return msgf("npg_fe_get_coeff: coefficient '%s' has not been set", name);
    return "";
}

}  // namespace npg
