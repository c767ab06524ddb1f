// Time means and co-moments of the running state on the device (npg_tavg_*): one call per time step folds the state into
// a weighted running mean of [u; p] and b and into the ten co-moments of (u, v, w, b) on the mesh nodes.  The arithmetic and the
// argument checks are tavg_core.h's, shared with the host library.  The handle owns the node table only; the accumulators are the
// caller's vectors.
//   k_tavg_comoments   one lane per table node: gathers up to five state values and their OLD means through the table, forms the four
//                      deltas, updates the ten co-moments [pair][node] (unit stride across the wave).  Launched first
//   k_tavg_means       one lane per entry of [x_inv | b]: mu += r (a - mu).  Launched second on the same stream; alone for means only
// No atomics, no LDS, add / subtract / multiply in one association: the same bits as the host library and as a numpy restatement.
#include <cmath>

#include "common.h"
#include "tavg_core.h"

namespace npg {

constexpr int kTavgBlock = NPG_TAVG_BLOCK;
static_assert(kTavgBlock % kWave == 0 && kTavgBlock <= 1024, "whole waves");

__global__ void __launch_bounds__(kTavgBlock) k_tavg_comoments(TavgTable t, double q, const double *__restrict__ x, const double *__restrict__ b,
                                                               const double *__restrict__ mean_x, const double *__restrict__ mean_b,
                                                               double *__restrict__ comom) {
    const int64_t j = (int64_t)blockIdx.x * kTavgBlock + threadIdx.x;
    if (j < t.nnode) tavg_node(t, j, q, x, b, mean_x, mean_b, comom);
}

__global__ void __launch_bounds__(kTavgBlock) k_tavg_means(int64_t n, int64_t n_inv, double r, const double *__restrict__ x,
                                                           const double *__restrict__ b, double *__restrict__ mean_x,
                                                           double *__restrict__ mean_b) {
    const int64_t i = (int64_t)blockIdx.x * kTavgBlock + threadIdx.x;
    if (i < n) tavg_mean(i, n_inv, r, x, b, mean_x, mean_b);
}

}  // namespace npg

using namespace npg;

struct npg_tavg {
    npg_ctx *ctx = nullptr;
    int64_t n_inv = 0, n_b = 0, nnode = 0;
    DevBuf<int32_t> iu, ib;
};

NPG_API int npg_tavg_create(npg_ctx *ctx, int64_t n_inv, int64_t n_b, int64_t nnode, const int32_t *iu, const int32_t *ib, npg_tavg **out) {
    NPG_REQUIRE(ctx && out, "npg_tavg_create: NULL argument");
    NPG_REQUIRE_OK(tavg_check_create(n_inv, n_b, nnode, iu, ib));
    NPG_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<npg_tavg> T(new npg_tavg());
    T->ctx = ctx;
    T->n_inv = n_inv, T->n_b = n_b, T->nnode = nnode;
    NPG_HIP(T->iu.upload(iu, 3 * (size_t)nnode));
    NPG_HIP(T->ib.upload(ib, 2 * (size_t)nnode));
    *out = T.release();
    return NPG_OK;
}

NPG_API int npg_tavg_destroy(npg_tavg *T) {
    if (!T) return NPG_OK;
    hipStreamSynchronize(T->ctx->stream);
    delete T;
    return NPG_OK;
}

NPG_API int npg_tavg_info(const npg_tavg *T, int64_t *nnode, int64_t *n_inv, int64_t *n_b) {
    NPG_REQUIRE(T, "npg_tavg_info: NULL argument");
    if (nnode) *nnode = T->nnode;
    if (n_inv) *n_inv = T->n_inv;
    if (n_b) *n_b = T->n_b;
    return NPG_OK;
}

NPG_API int npg_tavg_accumulate(npg_tavg *T, double r, double q, const npg_vec *x_inv, const npg_vec *b, npg_vec *mean_x, npg_vec *mean_b,
                                npg_vec *comom) {
    NPG_REQUIRE(T, "npg_tavg_accumulate: NULL argument");
    const bool all = x_inv && b && mean_x && mean_b;
    const bool aliased = all && (mean_x->d == x_inv->d || mean_b->d == b->d || mean_x->d == mean_b->d ||
                                 (comom && (comom->d == x_inv->d || comom->d == b->d || comom->d == mean_x->d || comom->d == mean_b->d)));
    const bool one_ctx = all && x_inv->ctx == T->ctx && b->ctx == T->ctx && mean_x->ctx == T->ctx && mean_b->ctx == T->ctx &&
                         (!comom || comom->ctx == T->ctx);
    NPG_REQUIRE_OK(tavg_check_accumulate(r, q, T->n_inv, T->n_b, T->nnode, all, all ? x_inv->n : 0, all ? b->n : 0, all ? mean_x->n : 0,
                                         all ? mean_b->n : 0, comom ? comom->n : -1, aliased, one_ctx));
    NPG_HIP(hipSetDevice(T->ctx->device));
    hipStream_t st = T->ctx->stream;
    if (comom && T->nnode > 0) {
        const TavgTable t{T->nnode, T->iu.p, T->ib.p};
        hipLaunchKernelGGL(k_tavg_comoments, dim3((unsigned)((T->nnode + kTavgBlock - 1) / kTavgBlock)), dim3(kTavgBlock), 0, st, t, q, x_inv->d,
                           b->d, mean_x->d, mean_b->d, comom->d);
        NPG_HIP(hipGetLastError());
    }
    const int64_t n = T->n_inv + T->n_b;
    if (n > 0) {
        hipLaunchKernelGGL(k_tavg_means, dim3((unsigned)((n + kTavgBlock - 1) / kTavgBlock)), dim3(kTavgBlock), 0, st, n, T->n_inv, r, x_inv->d,
                           b->d, mean_x->d, mean_b->d);
        NPG_HIP(hipGetLastError());
    }
    return NPG_OK;
}
