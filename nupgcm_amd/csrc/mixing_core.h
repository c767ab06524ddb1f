// Water-mass transformation by mixing (npg_classes_mixing): what ONE sample of ONE cell adds to the NPG_NMIX diffusivity-weighted
// channels of its (latitude band, buoyancy class) bin.  The arithmetic shared by the device kernels (classes.hip: k_mixing_scan /
// k_mixing_bin) and the host library (csrc_host/nupgcm_host.cpp), as classes_core.h is for the census: the sample rule, the measure,
// the edges, the bin search and the expressions for y, z, B and grad B are class_sample's, in its order - without the velocity.
//
// At a sample (lam, measure w = wq wdet):
//     B = N2 z + b',     grad B = grad b' + N2 e_z          (N2: the BINNING argument; 0 bins the perturbation)
//     kappa_h = the caller's value at the sample
//     kappa_v = kappa_v0 + kappa_c (1 + tanh(-a / N2min)) / 2,     a = alpha (N2c + d_z b')
// kappa_v0 is the BACKGROUND diffusivity at the sample, the second term the convection closure (the formula of k_coeff_from_bz mode 0,
// fe.hip) evaluated from the sample's own d_z b'; N2c and alpha are the closure's arguments, separate from the binning N2.
// kappa_c = 0: closure off - tanh is not called and kappa_v = kappa_v0, so the closure-off bits cannot depend on it.
//
// term[k] = measure * integrand_k (raw integrals):
//     0  1 (the census again)                        4  kappa_v
//     1  kappa_h (d_x B^2 + d_y B^2)                 5  kappa_h
//     2  kappa_v (d_z B)^2                           6  |grad B|^2
//     3  kappa_v d_z B                               7  kappa_v - kappa_v0 (the closure's part; 0 when off)
// Channels 1 + 2 are the dissipation D whose derivative in B is the diffusive buoyancy flux through a buoyancy surface.  Always fp64.
//
// T: the cell tables - G(k, c), wdet(c), y(i, c), z(i, c), b(x, i, c), as class_cell_load reads them.
#pragma once
#include "classes_core.h"

namespace npg {

constexpr int kNMix = 8;
static_assert(kNMix == kNCls, "the mixing table reuses the partial rows, the scales and the integer table of the classes");

// the convection closure's arguments; kappa_c = 0: off
struct MixClosure {
    double kappa_c, N2min, alpha, N2c;
};

// the closure's part of kappa_v where d_z b' = bz (called with cl.kappa_c > 0 only); boundary_core.h evaluates the same expression
NPG_HD double closure_kappa(const MixClosure &cl, double bz) {
    const double a = cl.alpha * (cl.N2c + bz);
    return cl.kappa_c * (1.0 + tanh(-a / cl.N2min)) / 2.0;
}

// the nodal values of one cell: ClassCell without the velocity
template <int NB>
struct MixCell {
    double G[12], y[4], z[4], b[NB], wdet;
};

template <int NB, class T>
NPG_HD void mix_cell_load(const T &t, const double *xb, int64_t c, MixCell<NB> &n) {
NPG_UNROLL
    for (int k = 0; k < 12; ++k) n.G[k] = t.G(k, c);
NPG_UNROLL
    for (int i = 0; i < 4; ++i) n.y[i] = t.y(i, c), n.z[i] = t.z(i, c);
NPG_UNROLL
    for (int i = 0; i < NB; ++i) n.b[i] = t.b(xb, i, c);
    n.wdet = t.wdet(c);
}

// Sample (lam, wq = w[s] * qsum) of the cell n with the diffusivities kh, kv0 of this sample: false when B or y is not finite (nothing
// else is written then); otherwise the terms and - BIN - the band and the class.
template <int NB, bool BIN>
NPG_HD bool mix_sample(const MixCell<NB> &n, const double lam[4], double wq, double N2, double kh, double kv0, const MixClosure &cl,
                       const double *y_edges, int64_t ny, const double *b_edges, int64_t nb, int64_t *band, int64_t *cls,
                       double term[kNMix]) {
    const double y = lam[0] * n.y[0] + lam[1] * n.y[1] + lam[2] * n.y[2] + lam[3] * n.y[3];
    const double z = lam[0] * n.z[0] + lam[1] * n.z[1] + lam[2] * n.z[2] + lam[3] * n.z[3];
    double bp = 0.0, d[4];
    if constexpr (NB == 10) {
        double N[10];
        p2_shape(lam, N);
NPG_UNROLL
        for (int i = 0; i < 10; ++i) bp += N[i] * n.b[i];
        p2_dlambda(lam, n.b, d);
    } else {
NPG_UNROLL
        for (int i = 0; i < 4; ++i) d[i] = n.b[i], bp += lam[i] * n.b[i];        // d N_i / d lambda_k = delta_ik
    }
    const double B = N2 * z + bp;
    if (!(B - B == 0.0) || !(y - y == 0.0)) return false;                         // NaN or infinite
    const double gx = d[0] * n.G[0] + d[1] * n.G[3] + d[2] * n.G[6] + d[3] * n.G[9];
    const double gy = d[0] * n.G[1] + d[1] * n.G[4] + d[2] * n.G[7] + d[3] * n.G[10];
    const double bz = d[0] * n.G[2] + d[1] * n.G[5] + d[2] * n.G[8] + d[3] * n.G[11];      // d_z b'
    const double gz = bz + N2;
    double kc = 0.0, kv = kv0;
    if (cl.kappa_c > 0.0) {
        kc = closure_kappa(cl, bz);
        kv = kv0 + kc;
    }
    const double gh2 = gx * gx + gy * gy;
    const double w = wq * n.wdet;
    term[0] = w;
    term[1] = w * (kh * gh2);
    term[2] = w * (kv * (gz * gz));
    term[3] = w * (kv * gz);
    term[4] = w * kv;
    term[5] = w * kh;
    term[6] = w * (gh2 + gz * gz);
    term[7] = w * kc;
    if (BIN) {
        *band = edge_count_le(y_edges, ny, y);
        *cls = edge_count_le(b_edges, nb, B);
    }
    return true;
}

// nullptr if v is usable as a diffusivity: finite and >= 0
inline const char *check_diffusivity(double v) { return std::isfinite(v) && v >= 0.0 ? nullptr : "must be finite and >= 0"; }

}  // namespace npg
