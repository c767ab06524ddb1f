// Time means and co-moments of the running state (npg_tavg_*): the arithmetic shared by the device kernels (tavg.hip)
// and the host library (csrc_host/nupgcm_host.cpp), with the argument checks of the entry points: GPU() and CPU() evaluate the same
// expressions in the same order.  Always fp64; add, subtract and multiply only, no division, no contraction (-ffp-contract=off).
//
// The weighted running mean and co-moments of West / Welford.  For a sample of weight w > 0 the HOST forms, in fp64,
//   W' = W + w,   r = w / W',   q = w (W / W')
// and one call does, with the OLD means,
//   delta_a = a - mu_a                               every free DoF of [u; p] and of b
//   C_ab    = C_ab + (q delta_a) delta_b             ten pairs per node: uu uv uw vv vw ww ub vb wb bb
//   mu_a    = mu_a + r delta_a
// The first sample has r = 1, q = 0: mu takes the sample's bits and C stays 0.
//
// The co-moments live on mesh nodes.  The node table pairs the differently numbered fields: iu[c][node] the position of velocity
// component c in x_inv, ib[0..1][node] two positions in b - equal for a P2 node or a vertex; the two vertices of the edge for a
// mid-node of a P1 buoyancy, which takes delta_b = 0.5 (delta_b(v0) + delta_b(v1)).  A position < 0 is a Dirichlet DoF: constant
// in time, delta = 0, no value table needed, and every co-moment it enters stays exactly 0.
// Tables and co-moments are component-major, [c][node] and [pair][node]: unit stride across the lanes of a wave.
//   pass 1 (tavg_node)   one node: gathers up to five values and their old means, updates its ten co-moments
//   pass 2 (tavg_mean)   one entry of [x_inv | b]: its mean.  Second, because with a P1 buoyancy several mid-nodes read one mu_b.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

#include "cell_view.h"

namespace npg {

constexpr int kTavgPairs = 10;      // uu uv uw vv vw ww ub vb wb bb
#ifndef NPG_TAVG_BLOCK
#define NPG_TAVG_BLOCK 256
#endif

struct TavgTable {
    int64_t nnode;
    const int32_t *iu;              // [3][nnode]
    const int32_t *ib;              // [2][nnode]
};

NPG_HD double tavg_delta(const double *a, const double *mu, int32_t i) { return i >= 0 ? a[i] - mu[i] : 0.0; }

// the ten co-moments of table node j
NPG_HD void tavg_node(const TavgTable &t, int64_t j, double q, const double *x, const double *b, const double *mean_x, const double *mean_b,
                      double *comom) {
    const size_t n = (size_t)t.nnode;
    const double du = tavg_delta(x, mean_x, t.iu[j]), dv = tavg_delta(x, mean_x, t.iu[n + j]), dw = tavg_delta(x, mean_x, t.iu[2 * n + j]);
    const int32_t b0 = t.ib[j], b1 = t.ib[n + j];
    const double db = b0 == b1 ? tavg_delta(b, mean_b, b0) : 0.5 * (tavg_delta(b, mean_b, b0) + tavg_delta(b, mean_b, b1));
    const double qu = q * du, qv = q * dv, qw = q * dw;
    double *c = comom + j, v[kTavgPairs];
    NPG_UNROLL
    for (int p = 0; p < kTavgPairs; ++p) v[p] = c[(size_t)p * n];       // all ten loads in flight before the first store
    v[0] = v[0] + qu * du;
    v[1] = v[1] + qu * dv;
    v[2] = v[2] + qu * dw;
    v[3] = v[3] + qv * dv;
    v[4] = v[4] + qv * dw;
    v[5] = v[5] + qw * dw;
    v[6] = v[6] + qu * db;
    v[7] = v[7] + qv * db;
    v[8] = v[8] + qw * db;
    v[9] = v[9] + (q * db) * db;
    NPG_UNROLL
    for (int p = 0; p < kTavgPairs; ++p) c[(size_t)p * n] = v[p];
}

// the mean of entry i of [x_inv | b]
NPG_HD void tavg_mean(int64_t i, int64_t n_inv, double r, const double *x, const double *b, double *mean_x, double *mean_b) {
    const bool inv = i < n_inv;
    const double a = inv ? x[i] : b[i - n_inv];
    double *mu = inv ? mean_x + i : mean_b + (i - n_inv);
    *mu = *mu + r * (a - *mu);
}

// npg_tavg_create's arguments, for both libraries
inline std::string tavg_check_create(int64_t n_inv, int64_t n_b, int64_t nnode, const int32_t *iu, const int32_t *ib) {
    if (n_inv < 0 || n_b < 0 || nnode < 0) return "npg_tavg_create: negative size";
    if (n_inv > INT32_MAX || n_b > INT32_MAX || nnode > INT32_MAX) return "npg_tavg_create: sizes must fit 32-bit positions";
    if (nnode > 0 && (!iu || !ib)) return "npg_tavg_create: NULL node table";
    for (int64_t k = 0; k < 3 * nnode; ++k)
        if (iu[k] < -1 || iu[k] >= n_inv)
            return msgf("npg_tavg_create: velocity position %d of node %lld, component %d is outside [-1, %lld)", iu[k], (long long)(k % nnode),
                        (int)(k / nnode), (long long)n_inv);
    for (int64_t k = 0; k < 2 * nnode; ++k)
        if (ib[k] < -1 || ib[k] >= n_b)
            return msgf("npg_tavg_create: buoyancy position %d of node %lld is outside [-1, %lld)", ib[k], (long long)(k % nnode), (long long)n_b);
    return "";
}

// npg_tavg_accumulate's arguments, for both libraries.  comom_n < 0: no co-moments (means only)
inline std::string tavg_check_accumulate(double r, double q, int64_t n_inv, int64_t n_b, int64_t nnode, bool have_all, int64_t x_n, int64_t b_n,
                                         int64_t mean_x_n, int64_t mean_b_n, int64_t comom_n, bool aliased, bool one_ctx) {
    if (!have_all) return "npg_tavg_accumulate: NULL argument";
    if (!(std::isfinite(r) && r > 0.0 && r <= 1.0)) return msgf("npg_tavg_accumulate: r must be in (0, 1], got %g", r);
    if (!(std::isfinite(q) && q >= 0.0)) return msgf("npg_tavg_accumulate: q must be finite and >= 0, got %g", q);
    const std::string m = check_state_vectors("npg_tavg_accumulate", n_inv, n_b, x_n, b_n);
    if (!m.empty()) return m;
    if (mean_x_n != n_inv || mean_b_n != n_b)
        return msgf("npg_tavg_accumulate: the means have %lld and %lld entries, expected %lld and %lld", (long long)mean_x_n, (long long)mean_b_n,
                    (long long)n_inv, (long long)n_b);
    if (comom_n >= 0 && comom_n != kTavgPairs * nnode)
        return msgf("npg_tavg_accumulate: the co-moments have %lld entries, expected %d x %lld", (long long)comom_n, kTavgPairs, (long long)nnode);
    if (aliased) return "npg_tavg_accumulate: the accumulators must not be the state vectors or one another";
    if (!one_ctx) return "npg_tavg_accumulate: arguments of different contexts";
    return "";
}

}  // namespace npg
