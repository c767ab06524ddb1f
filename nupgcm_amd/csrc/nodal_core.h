// Gradients of the finite-element fields recovered at the mesh's P2 nodes (npg_nodal_*): the arithmetic shared by the
// device kernels (nodal.hip) and the host library (csrc_host/nupgcm_host.cpp), with the argument checks of the entry points.  GPU() and
// CPU() evaluate the same expressions in the same order: add, subtract, multiply and ONE division per value, no contraction
// (-ffp-contract=off).  Always fp64.
//
// A P2 node n has incidences (c, i): cell c holds it as local node i = 0..9 (vertices 0..3, then the edges (0,1) (0,2) (1,2) (0,3) (1,3)
// (2,3) of fe.p2_tables), listed in ascending c.  Per cell and field the gradient at the cell's four VERTICES is
//     d = p2_dlambda(e_k, v)  (a P1 field: d_i = v_i),    g_a = d0 G(a) + d1 G(3 + a) + d2 G(6 + a) + d3 G(9 + a)
// exactly as sample_point forms it; at the mid-node of the edge (a, b)  g = 0.5 (g_a + g_b)  - the gradient of a P2 function is affine in
// lambda, so this IS the gradient at the midpoint.  The cells carry their own G: a periodic seam needs nothing special.  Per node
//     S = sum_c w_c g_{c,i},   W = sum_c w_c     both from 0.0 in incidence order,      result = S / W
// with w_c = wdet(c) (kNodalVolume) or 1.0 (kNodalCount).  A boundary node's average is one-sided: it has cells on one side only.
//
//   pass 1 (nodal_cell)   one cell: its vertex gradients into its own record rec[nslot] of the scratch (unweighted; plain stores)
//   pass 2 (nodal_node)   one selected node: walks its incidences, reads one record entry per channel for a vertex and two for a mid-node
// The scratch is cell-major, [ncell][nslot]: the node pass gathers, and the 12 (or 15) values it wants of a vertex are then neighbours.
// A record holds the groups the call asked for: u 4 x 9 (vertex k, d_j u_a at 9 k + 3 a + j), b' 4 x 3 (P2) or 3 (P1: one gradient per
// cell), p 3.  Output channels per selected node, compact over the groups asked for: d_j u_a (9), grad b' (3), grad p (3), W, the valence.
#pragma once
#include <cstdint>
#include <string>

#include "sample_core.h"

namespace npg {

enum { kNodalU = 1, kNodalB = 2, kNodalP = 4, kNodalAll = 7 };
enum { kNodalVolume = 0, kNodalCount = 1 };
constexpr int kNodalMaxCh = 17;
constexpr int64_t kNodalMaxCells = (int64_t)1 << 27;      // an incidence is packed as 16 cell + local in 32 bits
#ifndef NPG_NODAL_BLOCK
#define NPG_NODAL_BLOCK 256
#endif

// where the groups of one call live in a cell's record and in the output
struct NodalPlan {
    int mask, nslot, nch;
    int off_u, off_b, off_p;        // record offsets
    int bstride;                    // 3: b' has a gradient per vertex (P2); 0: one per cell (P1)
    int ch_b, ch_p, ch_w;           // first output channel of grad b', grad p, and of W (the valence follows)
};

NPG_HD NodalPlan nodal_plan(int mask, int nb) {
    NodalPlan pl{};
    pl.mask = mask;
    pl.bstride = nb == 10 ? 3 : 0;
    int s = 0, ch = 0;
    pl.off_u = s;
    if (mask & kNodalU) s += 36, ch += 9;
    pl.off_b = s, pl.ch_b = ch;
    if (mask & kNodalB) s += nb == 10 ? 12 : 3, ch += 3;
    pl.off_p = s, pl.ch_p = ch;
    if (mask & kNodalP) s += 3, ch += 3;
    pl.nslot = s, pl.ch_w = ch, pl.nch = ch + 2;
    return pl;
}

// g[3 k + a]: the gradient at vertex k of the P2 function with nodal values v
NPG_HD void nodal_p2_vertex_gradients(const double G[12], const double v[10], double *g, int kstride) {
NPG_UNROLL
    for (int k = 0; k < 4; ++k) {
        const double l[4] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0, k == 3 ? 1.0 : 0.0};
        double d[4];
        p2_dlambda(l, v, d);
NPG_UNROLL
        for (int a = 0; a < 3; ++a) g[k * kstride + a] = d[0] * G[a] + d[1] * G[3 + a] + d[2] * G[6 + a] + d[3] * G[9 + a];
    }
}

// pass 1: the record of cell c.  One field at a time: ten nodal values, d[4] and the cell's G are what is live
template <class View, int NB>
NPG_HD void nodal_cell(const View &t, const NodalPlan &pl, const double *xu, const double *xb, int64_t c, double *rec) {
    double G[12];
NPG_UNROLL
    for (int k = 0; k < 12; ++k) G[k] = t.G(k, c);
    if (pl.mask & kNodalU) {
NPG_UNROLL
        for (int a = 0; a < 3; ++a) {
            double v[10];
NPG_UNROLL
            for (int i = 0; i < 10; ++i) v[i] = t.u(xu, 3 * i + a, c);
            nodal_p2_vertex_gradients(G, v, rec + pl.off_u + 3 * a, 9);
        }
    }
    if (pl.mask & kNodalB) {
        if (NB == 10) {
            double v[10];
NPG_UNROLL
            for (int i = 0; i < 10; ++i) v[i] = t.b(xb, i, c);
            nodal_p2_vertex_gradients(G, v, rec + pl.off_b, 3);
        } else {
            double d[4];
NPG_UNROLL
            for (int i = 0; i < 4; ++i) d[i] = t.b(xb, i, c);                 // d N_i / d lambda_k = delta_ik
NPG_UNROLL
            for (int a = 0; a < 3; ++a) rec[pl.off_b + a] = d[0] * G[a] + d[1] * G[3 + a] + d[2] * G[6 + a] + d[3] * G[9 + a];
        }
    }
    if (pl.mask & kNodalP) {
        double d[4];
NPG_UNROLL
        for (int m = 0; m < 4; ++m) d[m] = t.p(xu, m, c);
NPG_UNROLL
        for (int a = 0; a < 3; ++a) rec[pl.off_p + a] = d[0] * G[a] + d[1] * G[3 + a] + d[2] * G[6 + a] + d[3] * G[9 + a];
    }
}

// the cell's gradient at its local node i from the per-vertex entries r[k * stride]: a vertex's own, half the sum of an edge's two
NPG_HD double nodal_at(const double *r, int stride, int i) {
    if (i < 4) return r[i * stride];
    const int e = i - 4;
    const int a = e == 2 ? 1 : (e == 4 ? 1 : (e == 5 ? 2 : 0));               // edges (0,1) (0,2) (1,2) (0,3) (1,3) (2,3)
    const int b = e == 0 ? 1 : (e < 3 ? 2 : 3);
    return 0.5 * (r[a * stride] + r[b * stride]);
}

struct NodalTable {
    int64_t nsel;
    const int64_t *ptr;             // [nsel + 1]
    const int32_t *inc;             // 16 cell + local, ascending within a node
    const double *wdet;             // the engine's [ncell]
    int weight_mode;
};

// pass 2: selected node j; out[ch][nsel]
NPG_HD void nodal_node(const NodalTable &t, const NodalPlan &pl, const double *scr, int64_t j, double *out) {
    double Su[9], Sb[3], Sp[3], W = 0.0;
NPG_UNROLL
    for (int k = 0; k < 9; ++k) Su[k] = 0.0;
NPG_UNROLL
    for (int k = 0; k < 3; ++k) Sb[k] = 0.0, Sp[k] = 0.0;
    const int64_t e0 = t.ptr[j], e1 = t.ptr[j + 1];
    for (int64_t e = e0; e < e1; ++e) {
        const int32_t code = t.inc[e];
        const int64_t c = code >> 4;
        const int i = code & 15;
        const double w = t.weight_mode == kNodalVolume ? t.wdet[c] : 1.0;
        const double *rec = scr + (size_t)c * (size_t)pl.nslot;
        W += w;
        if (pl.mask & kNodalU) {
NPG_UNROLL
            for (int k = 0; k < 9; ++k) Su[k] += w * nodal_at(rec + pl.off_u + k, 9, i);
        }
        if (pl.mask & kNodalB) {
NPG_UNROLL
            for (int k = 0; k < 3; ++k) Sb[k] += w * nodal_at(rec + pl.off_b + k, pl.bstride, i);
        }
        if (pl.mask & kNodalP) {
NPG_UNROLL
            for (int k = 0; k < 3; ++k) Sp[k] += w * nodal_at(rec + pl.off_p + k, 0, i);
        }
    }
    const size_t n = (size_t)t.nsel;
    if (pl.mask & kNodalU) {
NPG_UNROLL
        for (int k = 0; k < 9; ++k) out[(size_t)k * n + j] = Su[k] / W;
    }
    if (pl.mask & kNodalB) {
NPG_UNROLL
        for (int k = 0; k < 3; ++k) out[(size_t)(pl.ch_b + k) * n + j] = Sb[k] / W;
    }
    if (pl.mask & kNodalP) {
NPG_UNROLL
        for (int k = 0; k < 3; ++k) out[(size_t)(pl.ch_p + k) * n + j] = Sp[k] / W;
    }
    out[(size_t)pl.ch_w * n + j] = W;
    out[(size_t)(pl.ch_w + 1) * n + j] = (double)(e1 - e0);
}

// npg_nodal_create's arguments, for both libraries ("" = fine; nothing has been allocated or launched yet)
inline std::string check_nodal_create(int64_t ncell, int64_t nsel, const int64_t *ptr, const int32_t *inc, int weight_mode, int64_t *max_valence) {
    if (weight_mode != kNodalVolume && weight_mode != kNodalCount)
        return msgf("npg_nodal_create: weight_mode must be 0 (cell volume) or 1 (count), got %d", weight_mode);
    if (ncell >= kNodalMaxCells) return msgf("npg_nodal_create: %lld cells, an incidence 16 cell + local needs fewer than 2^27", (long long)ncell);
    if (nsel < 0 || nsel > INT32_MAX) return "npg_nodal_create: nsel must be 0 .. 2^31 - 1";
    if (!ptr) return "npg_nodal_create: NULL inc_ptr";
    if (ptr[0] != 0) return msgf("npg_nodal_create: inc_ptr must start at 0, got %lld", (long long)ptr[0]);
    int64_t vmax = 0;
    for (int64_t j = 0; j < nsel; ++j) {
        if (ptr[j + 1] < ptr[j]) return msgf("npg_nodal_create: inc_ptr decreases at node %lld", (long long)j);
        if (ptr[j + 1] == ptr[j]) return msgf("npg_nodal_create: node %lld has no incidence (a selected node needs at least one cell)", (long long)j);
        vmax = ptr[j + 1] - ptr[j] > vmax ? ptr[j + 1] - ptr[j] : vmax;
    }
    if (nsel > 0 && !inc) return "npg_nodal_create: NULL incidence table";
    for (int64_t j = 0; j < nsel; ++j)
        for (int64_t e = ptr[j]; e < ptr[j + 1]; ++e) {
            if (inc[e] < 0 || (inc[e] >> 4) >= ncell)
                return msgf("npg_nodal_create: node %lld: incidence cell %lld is outside [0, %lld)", (long long)j, (long long)(inc[e] >> 4), (long long)ncell);
            if ((inc[e] & 15) >= 10) return msgf("npg_nodal_create: node %lld: incidence local node %d must be 0 .. 9", (long long)j, inc[e] & 15);
            if (e > ptr[j] && (inc[e] >> 4) <= (inc[e - 1] >> 4))
                return msgf("npg_nodal_create: node %lld: its incidences must come in ascending cell order", (long long)j);
        }
    if (max_valence) *max_valence = vmax;
    return "";
}

// npg_nodal_compute's arguments, for both libraries
inline std::string check_nodal_compute(int64_t n_inv, int64_t n_b, int nb, int64_t nsel, int64_t x_n, int64_t b_n, int fields_mask, int64_t out_n,
                                       bool one_ctx) {
    if (fields_mask < 1 || fields_mask > kNodalAll)
        return msgf("npg_nodal_compute: fields_mask must be a combination of 1 (u), 2 (b), 4 (p), got %d", fields_mask);
    const std::string m = check_state_vectors("npg_nodal_compute", n_inv, n_b, x_n, b_n);
    if (!m.empty()) return m;
    const int64_t need = (int64_t)nodal_plan(fields_mask, nb).nch * nsel;
    if (out_n < need) return msgf("npg_nodal_compute: out holds %lld doubles, needs channels x nsel = %lld", (long long)out_n, (long long)need);
    if (!one_ctx) return "npg_nodal_compute: arguments of different contexts";
    return "";
}

}  // namespace npg
