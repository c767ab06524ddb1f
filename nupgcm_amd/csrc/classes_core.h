// The flow binned into (latitude band, buoyancy class) (npg_classes_compute): what ONE sample of ONE cell adds to the NPG_NCLS
// channels of its bin, and the edge search that names the bin.  The arithmetic shared by the device kernels (classes.hip) and the
// host library (csrc_host/nupgcm_host.cpp), as integrals_core.h is for the mesh integrals: GPU() and CPU() evaluate the same
// expressions in the same order and bin with the same comparisons.
//
// Sample rule - NOT the engine's quadrature (Keast's 11-point rule has a negative weight; a census must not put negative volume
// into a class): ns barycentric points lam[ns][4] with weights w[ns] > 0, sum w = 1 (the caller's; Python builds the centroids of
// the 8^level equal sub-tetrahedra of `level` red refinements).  Sample s of cell c carries the measure
//     w[s] * wdet(c) * qsum,        qsum = sum_q qw[q] of the ENGINE's table, formed once on the host
// (1 / 6 on tetrahedra, 1 / 2 on the embedded 2-D meshes - nothing here assumes either).  Exact for functions linear in the cell; a
// positive Riemann sum otherwise.
//
// Values at a sample, all from ONE lambda with the closed-form shape functions of sample_core.h (p2_shape, p2_dlambda) and the
// nodal values (Dirichlet nodes included):  y = sum lambda_i y_i,  z = sum lambda_i z_i  over the cell's OWN vertices,
//     B = N2 z + b',     u,     grad B = grad b' + N2 e_z.
// Class of a sample = the number of b_edges <= B (searchsorted(edges, B, side = "right"), 0 .. nb); band = the same of y_edges and y.
// A sample whose B or y is not finite goes to no bin (the caller counts it as dropped).
//
// term[k] = measure * integrand_k:   0  1     1  u_x     2  u_y     3  u_z     4  z     5  B     6  d_z B     7  u . grad B
// Raw integrals: prefactors are the caller's.  Always fp64.
//
// T: the cell tables - G(k, c) (component 3 vertex + axis of grad lambda), wdet(c), y(i, c), z(i, c), u(x, l, c) / b(x, i, c).
#pragma once
#include <cmath>
#include <cstdint>

#include "sample_core.h"

namespace npg {

constexpr int kNCls = 8;
constexpr int kClsInfo = 1 + kNCls;       // pass 1 sums per lane: |term| of the kNCls channels, then the dropped samples
constexpr int kClsChunk = 256;            // cells per partial row of the host library's pass 1 (as kIntChunk)
constexpr int kClsMaxSamples = 4096;
constexpr int64_t kClsMaxBins = (int64_t)1 << 22;

// the number of edges[0 .. n) that are <= v: edges strictly increasing, v finite
NPG_HD int64_t edge_count_le(const double *edges, int64_t n, double v) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (edges[mid] <= v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the fixed-point scale of a channel whose |term| sum to S: 2^(61 - e) with frexp(S) = (m, e), so that S scale < 2^61 and the
// rounded terms of a channel sum to less than 2^62 in magnitude; 1 for S = 0; 0 (the channel comes back NaN) when S is not finite
NPG_HD double class_scale(double S) {
    if (!(S == S) || S - S != 0.0) return 0.0;
    if (S == 0.0) return 1.0;
    int e;
    (void)frexp(S, &e);
    const int p = 61 - e;
    return ldexp(1.0, p < 1023 ? p : 1023);
}

// the nodal values of one cell, loaded once and used by all its samples
template <int NB>
struct ClassCell {
    double G[12], y[4], z[4], u[30], b[NB], wdet;
};

template <int NB, class T>
NPG_HD void class_cell_load(const T &t, const double *xu, const double *xb, int64_t c, ClassCell<NB> &n) {
NPG_UNROLL
    for (int k = 0; k < 12; ++k) n.G[k] = t.G(k, c);
NPG_UNROLL
    for (int i = 0; i < 4; ++i) n.y[i] = t.y(i, c), n.z[i] = t.z(i, c);
NPG_UNROLL
    for (int l = 0; l < 30; ++l) n.u[l] = t.u(xu, l, c);
NPG_UNROLL
    for (int i = 0; i < NB; ++i) n.b[i] = t.b(xb, i, c);
    n.wdet = t.wdet(c);
}

// Sample (lam, wq = w[s] * qsum) of the cell n: false when B or y is not finite (nothing else is written then); otherwise the
// terms and - BIN - the band and the class.
template <int NB, bool BIN>
NPG_HD bool class_sample(const ClassCell<NB> &n, const double lam[4], double wq, double N2, const double *y_edges, int64_t ny,
                         const double *b_edges, int64_t nb, int64_t *band, int64_t *cls, double term[kNCls]) {
    const double y = lam[0] * n.y[0] + lam[1] * n.y[1] + lam[2] * n.y[2] + lam[3] * n.y[3];
    const double z = lam[0] * n.z[0] + lam[1] * n.z[1] + lam[2] * n.z[2] + lam[3] * n.z[3];
    double N[10];
    p2_shape(lam, N);
    double ux = 0.0, uy = 0.0, uz = 0.0;
NPG_UNROLL
    for (int i = 0; i < 10; ++i) ux += N[i] * n.u[3 * i], uy += N[i] * n.u[3 * i + 1], uz += N[i] * n.u[3 * i + 2];
    double bp = 0.0, d[4];
    if constexpr (NB == 10) {
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
    const double gz = (d[0] * n.G[2] + d[1] * n.G[5] + d[2] * n.G[8] + d[3] * n.G[11]) + N2;
    const double w = wq * n.wdet;
    term[0] = w;
    term[1] = w * ux;
    term[2] = w * uy;
    term[3] = w * uz;
    term[4] = w * z;
    term[5] = w * B;
    term[6] = w * gz;
    term[7] = w * (ux * gx + uy * gy + uz * gz);
    if (BIN) {
        *band = edge_count_le(y_edges, ny, y);
        *cls = edge_count_le(b_edges, nb, B);
    }
    return true;
}

// a term in units of 1 / scale, rounded to nearest (ties to even, the default mode); scale = 0 (class_scale of a non-finite sum): 0
NPG_HD int64_t class_quantise(double term, double scale) { return scale != 0.0 ? (int64_t)llrint(term * scale) : 0; }

// the rule and the edges: lam[ns][4], wq[ns] = w[s] qsum, y_edges[ny], b_edges[nb]
struct ClsRule {
    const double *lam, *wq, *y_edges, *b_edges;
    int ns;
    int64_t ny, nb;
};

// A SAMPLER is what the two passes of a class table (classes.hip: k_class_scan / k_class_bin; the host library: class_cell) are
// written over: the nodal values Cell<NB> of one cell, load() that fills them from the cell tables t, and sample<NB, QUANT>() that
// gives the terms of sample s of cell c and - QUANT - its band and class, or false (dropped).  It carries its own inputs.
// The census: the flow, the buoyancy and the binning N2.
struct CensusSampler {
    const double *xu, *xb;
    double N2;
    template <int NB>
    using Cell = ClassCell<NB>;
    template <int NB, class T>
    NPG_HD void load(const T &t, int64_t c, ClassCell<NB> &n) const {
        class_cell_load<NB>(t, xu, xb, c, n);
    }
    template <int NB, bool QUANT, class T>
    NPG_HD bool sample(const T &, const ClassCell<NB> &n, const ClsRule &r, int s, int64_t, int64_t *band, int64_t *cls,
                       double term[kNCls]) const {
        return class_sample<NB, QUANT>(n, r.lam + 4 * s, r.wq[s], N2, r.y_edges, r.ny, r.b_edges, r.nb, band, cls, term);
    }
};

// nullptr if e[0 .. n) is usable as bin edges: finite and strictly increasing (n = 0 is: one open bin)
inline const char *check_edges(const double *e, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(e[i]) || (i > 0 && !(e[i] > e[i - 1]))) return "must be finite and strictly increasing";
    return nullptr;
}

// The argument checks of the entry points, for both libraries (the message, empty: fine).  handles = "fe and out are not NULL".
inline std::string check_classes_create(bool handles, int64_t ncell, const double *cell_y, const double *cell_z, const double *rule_lam,
                                        const double *rule_w, int ns, const double *y_edges, int64_t ny, const double *b_edges, int64_t nb) {
    if (!handles) return "npg_classes_create: NULL argument";
    if (!(cell_y && cell_z)) return "npg_classes_create: cell_y or cell_z is NULL";
    if (!(ns >= 1 && ns <= kClsMaxSamples)) return msgf("npg_classes_create: 1 .. %d samples per cell, got %d", kClsMaxSamples, ns);
    if (!(rule_lam && rule_w)) return "npg_classes_create: rule_lam or rule_w is NULL";
    if (!(ny >= 0 && nb >= 0 && (ny == 0 || y_edges) && (nb == 0 || b_edges))) return "npg_classes_create: edges missing or a negative count";
    if (!(ny < kClsMaxBins && nb < kClsMaxBins && (ny + 1) * (nb + 1) <= kClsMaxBins))
        return msgf("npg_classes_create: ny = %lld and nb = %lld give more than 2^22 bins (ny + 1)(nb + 1)", (long long)ny, (long long)nb);
    const char *err = check_edges(y_edges, ny);
    if (err) return msgf("npg_classes_create: y_edges %s", err);
    err = check_edges(b_edges, nb);
    if (err) return msgf("npg_classes_create: b_edges %s", err);
    double wsum = 0.0;
    for (int s = 0; s < ns; ++s) {
        if (!(rule_w[s] > 0.0 && std::isfinite(rule_w[s]))) return msgf("npg_classes_create: weight %d of the rule is not > 0", s);
        wsum += rule_w[s];
        const double *l = rule_lam + 4 * s;
        if (!(std::fabs((l[0] + l[1]) + (l[2] + l[3]) - 1.0) <= 1e-12)) return msgf("npg_classes_create: lam row %d of the rule does not sum to 1", s);
    }
    if (!(std::fabs(wsum - 1.0) <= 1e-12)) return msgf("npg_classes_create: the weights of the rule sum to %.17g, not 1", wsum);
    for (int64_t k = 0; k < ncell * 4; ++k) {
        if (!std::isfinite(cell_y[k])) return msgf("npg_classes_create: cell_y[%lld][%d] is not finite", (long long)(k / 4), (int)(k % 4));
        if (!std::isfinite(cell_z[k])) return msgf("npg_classes_create: cell_z[%lld][%d] is not finite", (long long)(k / 4), (int)(k % 4));
    }
    return "";
}

// K: the handle (nbins, its engine fe with n_inv, n_b, ctx); the vectors carry n and ctx
template <class H, class V>
std::string check_classes_compute(const H *K, const V *x_inv, const V *b, double N2, const V *table, const V *info) {
    if (!(K && x_inv && b && table && info)) return "npg_classes_compute: NULL argument";
    const auto *fe = K->fe;
    const std::string err = check_state_vectors("npg_classes_compute", fe->n_inv, fe->n_b, x_inv->n, b->n);
    if (!err.empty()) return err;
    if (table->n < K->nbins * kNCls)
        return msgf("npg_classes_compute: table holds %lld doubles, needs (ny + 1)(nb + 1) NPG_NCLS = %lld", (long long)table->n,
                    (long long)(K->nbins * kNCls));
    if (info->n < 1 + kNCls) return msgf("npg_classes_compute: info holds %lld doubles, needs 1 + NPG_NCLS = %d", (long long)info->n, 1 + kNCls);
    if (!std::isfinite(N2)) return "npg_classes_compute: N2 is not finite";
    if (!(x_inv->ctx == fe->ctx && b->ctx == fe->ctx && table->ctx == fe->ctx && info->ctx == fe->ctx))
        return "npg_classes_compute: arguments of different contexts";
    return "";
}

}  // namespace npg
