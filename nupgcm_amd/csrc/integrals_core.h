// Quadrature integrals of the finite-element fields over the mesh (npg_integrals_compute): what ONE cell adds to the NPG_NINT
// channels.  The arithmetic shared by the device kernel (integrals.hip) and the host library (csrc_host/nupgcm_host.cpp), as
// sample_core.h is for the point samples: GPU() and CPU() evaluate the same expressions in the same order, cell by cell.
//
// Always fp64: npg_fe_set_precision (the fp32 element-local mode of the assembly kernels) does NOT apply here - these numbers are
// compared with matrix identities (x' A x, b' M b, ...) to rounding, and there is no fp32 instance.
//
// Raw integrals only: the prefactors of the model (alpha^2 eps^2, 1 / alpha, N2) are applied by the caller.  acc[k] grows by
// qw[q] * wdet * integrand_k(q) for every point q of the ENGINE's rule (tetrahedra: Keast's 11 points; the embedded 2-D meshes: the
// 3 x 3 collapsed rule on the face lambda_4 = 0 with wdet = the triangle's Jacobian - nothing here assumes wdet / 6):
//
//    0  1                                        volume (area on the embedded 2-D meshes)
//    1  b'                                       2  b'^2
//    3  (u_x^2 + u_y^2) / 2                      4  u_z^2 / 2
//    5  u_z b'                                   buoyancy production before the 1 / alpha
//    6  nu grad u : grad u                       Laplacian form of the dissipation; 0 without a nu table
//    7  2 nu sigma : sigma, sigma = (grad u + grad u') / 2     full-stress form, formed only when asked (else 0)
//    8  z b'                                     z(q) = sum_i lambda_i(q) z_i over the cell's OWN vertices
//    9  u . grad b'                              advective tendency
//   10  u_z
//   11  kappa_h (d_x b'^2 + d_y b'^2) + kappa_v d_z b'^2       variance destruction; a missing table contributes 0
//   12  kappa_v d_z b'                           13  kappa_v
//   14  (div u)^2
//
// S: the shape tables - qw[q], N2[10 q + i], dN2[4 (10 q + i) + k], Nb[NB q + i], dNb[4 (NB q + i) + k], N1[4 q + m] (= lambda_m
// at point q).  T: the cell tables - G(k, c) (component 3 vertex + axis of grad lambda), wdet(c), z(i, c), u(x, l, c) / b(x, i, c)
// (nodal values, Dirichlet nodes included), nu / kh / kv (q, c) behind has_nu / has_kh / has_kv.
#pragma once
#include <cmath>
#include <cstdint>

#include "cell_view.h"

namespace npg {

constexpr int kNInt = 15;
constexpr int kIntChunk = 256;     // cells per partial row of the host library (a constant: the sums do not depend on the thread count)

template <int NB, class S, class T>
NPG_HD void cell_integrals(const S &s, const T &t, int nq, const double *xu, const double *xb, int64_t c, bool full_stress,
                           double acc[kNInt]) {
    double G[12], z[4], u[30], b[NB];
NPG_UNROLL
    for (int k = 0; k < 12; ++k) G[k] = t.G(k, c);
NPG_UNROLL
    for (int i = 0; i < 4; ++i) z[i] = t.z(i, c);
NPG_UNROLL
    for (int l = 0; l < 30; ++l) u[l] = t.u(xu, l, c);
NPG_UNROLL
    for (int i = 0; i < NB; ++i) b[i] = t.b(xb, i, c);
    const double wdet = t.wdet(c);
    for (int q = 0; q < nq; ++q) {
        const double w = s.qw[q] * wdet;
        // the fields one group after another from the same nodal registers: u, grad u, then b', grad b', then the coefficients
        double ux = 0.0, uy = 0.0, uz = 0.0;
NPG_UNROLL
        for (int i = 0; i < 10; ++i) {
            const double n = s.N2[q * 10 + i];
            ux += n * u[3 * i], uy += n * u[3 * i + 1], uz += n * u[3 * i + 2];
        }
        acc[0] += w;
        acc[3] += w * (0.5 * (ux * ux + uy * uy));
        acc[4] += w * (0.5 * (uz * uz));
        acc[10] += w * uz;
        double gu[9];                       // gu[3 a + j] = d_j u_a
NPG_UNROLL
        for (int a = 0; a < 3; ++a) {
            double l0 = 0.0, l1 = 0.0, l2 = 0.0, l3 = 0.0;
NPG_UNROLL
            for (int i = 0; i < 10; ++i) {
                const double *dn = &s.dN2[(q * 10 + i) * 4];
                const double v = u[3 * i + a];
                l0 += dn[0] * v, l1 += dn[1] * v, l2 += dn[2] * v, l3 += dn[3] * v;
            }
NPG_UNROLL
            for (int j = 0; j < 3; ++j) gu[3 * a + j] = l0 * G[j] + l1 * G[3 + j] + l2 * G[6 + j] + l3 * G[9 + j];
        }
        const double div = gu[0] + gu[4] + gu[8];
        acc[14] += w * (div * div);
        const double nu = t.has_nu() ? t.nu(q, c) : 0.0;
        double gg = 0.0;
NPG_UNROLL
        for (int k = 0; k < 9; ++k) gg += gu[k] * gu[k];
        acc[6] += w * (nu * gg);
        if (full_stress) {
            const double sxy = 0.5 * (gu[1] + gu[3]), sxz = 0.5 * (gu[2] + gu[6]), syz = 0.5 * (gu[5] + gu[7]);
            const double ss = (gu[0] * gu[0] + gu[4] * gu[4] + gu[8] * gu[8]) + 2.0 * (sxy * sxy + sxz * sxz + syz * syz);
            acc[7] += w * (2.0 * nu * ss);
        }
        double bq = 0.0, l0 = 0.0, l1 = 0.0, l2 = 0.0, l3 = 0.0;
NPG_UNROLL
        for (int i = 0; i < NB; ++i) {
            const double *dn = &s.dNb[(q * NB + i) * 4];
            bq += s.Nb[q * NB + i] * b[i];
            l0 += dn[0] * b[i], l1 += dn[1] * b[i], l2 += dn[2] * b[i], l3 += dn[3] * b[i];
        }
        const double gx = l0 * G[0] + l1 * G[3] + l2 * G[6] + l3 * G[9];
        const double gy = l0 * G[1] + l1 * G[4] + l2 * G[7] + l3 * G[10];
        const double gz = l0 * G[2] + l1 * G[5] + l2 * G[8] + l3 * G[11];
        const double *lam = &s.N1[q * 4];
        const double zq = lam[0] * z[0] + lam[1] * z[1] + lam[2] * z[2] + lam[3] * z[3];
        acc[1] += w * bq;
        acc[2] += w * (bq * bq);
        acc[5] += w * (uz * bq);
        acc[8] += w * (zq * bq);
        acc[9] += w * (ux * gx + uy * gy + uz * gz);
        const double kh = t.has_kh() ? t.kh(q, c) : 0.0, kv = t.has_kv() ? t.kv(q, c) : 0.0;
        acc[11] += w * (kh * (gx * gx + gy * gy) + kv * (gz * gz));
        acc[12] += w * (kv * gz);
        acc[13] += w * kv;
    }
}

// The argument checks of the entry points, for both libraries (the message, empty: fine).  handles = "fe and out are not NULL".
inline std::string check_integrals_create(bool handles, const double *cell_z, int64_t ncell) {
    if (!handles) return "npg_integrals_create: NULL argument";
    if (!cell_z) return "npg_integrals_create: cell_z is NULL";
    for (int64_t k = 0; k < ncell * 4; ++k)
        if (!std::isfinite(cell_z[k])) return msgf("npg_integrals_create: cell_z[%lld][%d] is not finite", (long long)(k / 4), (int)(k % 4));
    return "";
}

// I: the handle (its engine fe with n_inv, n_b, ctx); the vectors carry n and ctx
template <class H, class V>
std::string check_integrals_compute(const H *I, const V *x_inv, const V *b, int full_stress, const V *out) {
    if (!(I && x_inv && b && out)) return "npg_integrals_compute: NULL argument";
    const auto *fe = I->fe;
    const std::string err = check_state_vectors("npg_integrals_compute", fe->n_inv, fe->n_b, x_inv->n, b->n);
    if (!err.empty()) return err;
    if (out->n < kNInt) return msgf("npg_integrals_compute: out holds %lld doubles, needs NPG_NINT = %d", (long long)out->n, kNInt);
    if (full_stress != 0 && full_stress != 1) return msgf("npg_integrals_compute: full_stress must be 0 or 1, got %d", full_stress);
    if (!(x_inv->ctx == fe->ctx && b->ctx == fe->ctx && out->ctx == fe->ctx)) return "npg_integrals_compute: arguments of different contexts";
    return "";
}

}  // namespace npg
