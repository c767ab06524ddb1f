// Water-mass transformation by mixing (npg_classes_mixing): what ONE sample of ONE cell adds to the NPG_NMIX diffusivity-weighted
// channels of its (latitude band, buoyancy class) bin.  The arithmetic shared by the device kernels (classes.hip: k_class_scan /
// k_class_bin with the MixSampler below) and the host library (csrc_host/nupgcm_host.cpp), as classes_core.h is for the census: the sample rule, the measure,
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

// The mixing SAMPLER (classes_core.h: CensusSampler): the buoyancy, the binning N2, the diffusivities of the samples - tables kh / kv0
// of ns values per cell in the layout of the cell tables (t.at(s, ns, c), cell_view.h), or, where a table is null, the scalar - and the
// closure.
struct MixSampler {
    const double *kh, *kv0;
    double kh_s, kv0_s;
    MixClosure cl;
    const double *xb;
    double N2;
    template <int NB>
    using Cell = MixCell<NB>;
    template <int NB, class T>
    NPG_HD void load(const T &t, int64_t c, MixCell<NB> &n) const {
        mix_cell_load<NB>(t, xb, c, n);
    }
    template <int NB, bool QUANT, class T>
    NPG_HD bool sample(const T &t, const MixCell<NB> &n, const ClsRule &r, int s, int64_t c, int64_t *band, int64_t *cls,
                       double term[kNMix]) const {
        const size_t i = t.at(s, r.ns, c);
        const double h = kh ? kh[i] : kh_s, v0 = kv0 ? kv0[i] : kv0_s;
        return mix_sample<NB, QUANT>(n, r.lam + 4 * s, r.wq[s], N2, h, v0, cl, r.y_edges, r.ny, r.b_edges, r.nb, band, cls, term);
    }
};

// nullptr if v is usable as a diffusivity: finite and >= 0
inline const char *check_diffusivity(double v) { return std::isfinite(v) && v >= 0.0 ? nullptr : "must be finite and >= 0"; }

// The argument checks of the entry points, for both libraries (the message, empty: fine).  n = ncell ns, the entries of a table.
inline std::string check_classes_set_diffusivity(bool handle, int64_t n, int ns, const double *kappa_h, double kappa_h_scalar,
                                                 const double *kappa_v0, double kappa_v0_scalar) {
    if (!handle) return "npg_classes_set_diffusivity: NULL argument";
    const char *err = kappa_h ? nullptr : check_diffusivity(kappa_h_scalar);
    if (err) return msgf("npg_classes_set_diffusivity: the scalar kappa_h %s, got %.17g", err, kappa_h_scalar);
    err = kappa_v0 ? nullptr : check_diffusivity(kappa_v0_scalar);
    if (err) return msgf("npg_classes_set_diffusivity: the scalar kappa_v0 %s, got %.17g", err, kappa_v0_scalar);
    const double *src[2] = {kappa_h, kappa_v0};
    for (int t = 0; t < 2; ++t)
        for (int64_t i = 0; src[t] && i < n; ++i)
            if (check_diffusivity(src[t][i]))
                return msgf("npg_classes_set_diffusivity: %s[%lld][%d] must be finite and >= 0, got %.17g", t ? "kappa_v0" : "kappa_h",
                            (long long)(i / ns), (int)(i % ns), src[t][i]);
    return "";
}

// K: the handle (kap_set, nbins, its engine fe with n_b, ctx); the vectors carry n and ctx
template <class H, class V>
std::string check_classes_mixing(const H *K, const V *b, double N2, const MixClosure &cl, const V *table, const V *info) {
    if (!(K && b && table && info)) return "npg_classes_mixing: NULL argument";
    if (!K->kap_set) return "npg_classes_mixing: no diffusivities: call npg_classes_set_diffusivity first";
    const auto *fe = K->fe;
    const std::string err = check_state_vectors("npg_classes_mixing", fe->n_inv, fe->n_b, fe->n_inv, b->n);       // no flow vector
    if (!err.empty()) return err;
    if (table->n < K->nbins * kNMix)
        return msgf("npg_classes_mixing: table holds %lld doubles, needs (ny + 1)(nb + 1) NPG_NMIX = %lld", (long long)table->n,
                    (long long)(K->nbins * kNMix));
    if (info->n < 1 + kNMix) return msgf("npg_classes_mixing: info holds %lld doubles, needs 1 + NPG_NMIX = %d", (long long)info->n, 1 + kNMix);
    if (check_diffusivity(N2)) return msgf("npg_classes_mixing: N2 must be finite and >= 0, got %.17g", N2);
    if (check_diffusivity(cl.kappa_c)) return msgf("npg_classes_mixing: kappa_c must be finite and >= 0, got %.17g", cl.kappa_c);
    if (check_diffusivity(cl.alpha)) return msgf("npg_classes_mixing: alpha must be finite and >= 0, got %.17g", cl.alpha);
    if (check_diffusivity(cl.N2c)) return msgf("npg_classes_mixing: N2c must be finite and >= 0, got %.17g", cl.N2c);
    if (cl.kappa_c > 0.0 && !(cl.N2min > 0.0)) return msgf("npg_classes_mixing: kappa_c > 0 needs N2min > 0, got %.17g", cl.N2min);
    if (!(b->ctx == fe->ctx && table->ctx == fe->ctx && info->ctx == fe->ctx)) return "npg_classes_mixing: arguments of different contexts";
    return "";
}

}  // namespace npg
