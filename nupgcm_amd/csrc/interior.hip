// Interior buoyancy forcing on the device (npg_interior_*): the volume load of a source Q(x, t) and of a sponge
// gamma (b* - b), recomputed from keyframe tables for the time level being solved, the gamma-weighted mass matrix R of the sponge and
// the three integrals of its budget.  The reference has no interior forcing.  The arithmetic, the plan and the checks are
// interior_core.h's, shared with the host library.
//   k_interior_local<NB>    one lane per kept cell: blend the two keyframes of Q and b* at the cell's quadrature points, form
//                           Q + gamma (b* - b_D), weigh, contract with the cell's shape values; loc[k][kept cell].  Tables and loc are
//                           [..][kept cell]: unit stride across a wave; the shape values come from LDS
//   k_interior_gather       one lane per buoyancy row: its slots of loc added in (kept cell, local node) order; rows without slots get 0
//   k_interior_matrix<NB>   one lane per matrix entry that some kept cell touches: its slots (kept cell, i, j) added in order
//   k_interior_budget<NB>   one lane per kept cell, grid-stride; wave_sum, the 4 waves added in order: one partial row per workgroup,
//   k_interior_fold         folded by one workgroup in the fixed order of reduce_partials (as integrals.hip does)
// No atomics, one order of every sum: the same bits on every call.  Always fp64.
#include <cmath>

#include "common.h"
#include "device_utils.h"
#include "fe_dev.h"
#include "interior_core.h"

static_assert(NPG_ITR_NSERIES == npg::kItrNSeries, "NPG_ITR_NSERIES of the header and kItrNSeries of interior_core.h must agree");
static_assert(NPG_ITR_NBUDGET == npg::kItrNBudget, "NPG_ITR_NBUDGET of the header and kItrNBudget of interior_core.h must agree");
static_assert(npg::kItrNBudget <= npg::kPartStride, "a partial row holds the integrals");

namespace npg {

constexpr int kItrBlock = NPG_ITR_BLOCK;
static_assert(kItrBlock == kBlock, "the partial rows are those of a kBlock workgroup");
constexpr int kItrSlices = kItrBlock / kPartStride;    // reduce_partials: rows slice, slice + kItrSlices, ...
constexpr int kItrMaxBlocks = 1024;                    // partial rows of the budget at most

// the two shape tables these kernels read, in LDS
struct ItrShape {
    double qw[kMaxQ];
    double Nb[kMaxQ * 10];
};
__device__ __forceinline__ void stage_shape(const FeDev &d, ItrShape &s) {
    for (int i = threadIdx.x; i < d.nq; i += blockDim.x) s.qw[i] = d.qw[i];
    for (int i = threadIdx.x; i < d.nq * d.nb; i += blockDim.x) s.Nb[i] = d.Nb[i];
    __syncthreads();
}

template <int NB>
__global__ void __launch_bounds__(kItrBlock) k_interior_local(FeDev d, ItrCells t, double *__restrict__ loc) {
    __shared__ ItrShape s;
    stage_shape(d, s);
    const int64_t kc = (int64_t)blockIdx.x * kItrBlock + threadIdx.x;
    if (kc < t.nkept) itr_cell_load<NB>(s, cell_view(d), t, kc, loc);
}

__global__ void __launch_bounds__(kItrBlock) k_interior_gather(int64_t nrow, const int32_t *__restrict__ ptr, const int32_t *__restrict__ slot,
                                                               const double *__restrict__ loc, double *__restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * kItrBlock + threadIdx.x;
    if (r < nrow) itr_gather_row(r, ptr, slot, loc, out);
}

template <int NB>
__global__ void __launch_bounds__(kItrBlock) k_interior_matrix(FeDev d, ItrCells t, int64_t nent, const int32_t *__restrict__ eptr,
                                                               const int32_t *__restrict__ ecell, const uint8_t *__restrict__ ecode,
                                                               const int64_t *__restrict__ epos, double *__restrict__ val) {
    __shared__ ItrShape s;
    stage_shape(d, s);
    const int64_t e = (int64_t)blockIdx.x * kItrBlock + threadIdx.x;
    if (e < nent) val[epos[e]] = itr_matrix_entry<NB>(s, cell_view(d), t, eptr, ecell, ecode, e);
}

// part[blockIdx.x][kPartStride]: the workgroup's sums of the three integrals over its kept cells
template <int NB>
__global__ void __launch_bounds__(kItrBlock) k_interior_budget(FeDev d, ItrCells t, const double *__restrict__ xb, double *__restrict__ part) {
    __shared__ ItrShape s;
    __shared__ double sh[(kItrBlock / kWave) * kPartStride];
    stage_shape(d, s);
    const DevCells cells = cell_view(d);
    double acc[kItrNBudget];
#pragma unroll
    for (int k = 0; k < kItrNBudget; ++k) acc[k] = 0.0;
    for (int64_t kc = (int64_t)blockIdx.x * kItrBlock + threadIdx.x; kc < t.nkept; kc += (int64_t)gridDim.x * kItrBlock)
        itr_cell_budget<NB>(s, cells, t, xb, kc, acc);
    block_store_partials<kItrNBudget, kItrBlock / kWave>(acc, kItrNBudget, sh, part);
}

__global__ void __launch_bounds__(kItrBlock) k_interior_fold(const double *__restrict__ part, int nblocks, double *__restrict__ out) {
    __shared__ double tmp[kItrSlices * kPartStride], tot[kPartStride];
    reduce_partials<kItrSlices, kItrMaxBlocks / kItrSlices>(part, nblocks, kItrNBudget, tmp, tot);
    if (threadIdx.x < kItrNBudget) out[threadIdx.x] = tot[threadIdx.x];
}

}  // namespace npg

using namespace npg;

struct npg_interior {
    npg_ctx *ctx = nullptr;
    npg_fe *fe = nullptr;
    int64_t nkept = 0;
    ItrPlan plan;                               // host
    int32_t nkey[kItrNSeries] = {0, 0};
    DevBuf<int32_t> cell;
    DevBuf<double> ser[kItrNSeries], gamma, loc, part;
    DevBuf<int32_t> gptr, gslot, eptr, ecell;
    DevBuf<uint8_t> ecode;
    DevBuf<int64_t> epos;
    int nblocks = 0;
};

static ItrCells itr_cells(const npg_interior *F) {
    ItrCells t{};
    t.nkept = F->nkept;
    t.nq = F->fe->d.nq;
    t.cell = F->cell;
    for (int c = 0; c < kItrNSeries; ++c) t.ser[c] = F->ser[c], t.nkey[c] = F->nkey[c];
    t.gamma = F->gamma;
    return t;
}

static void itr_set_keys(const npg_interior *F, const int32_t *key, const double *w, ItrCells &t) {
    for (int c = 0; c < kItrNSeries; ++c) t.key[c] = F->nkey[c] ? key[c] : 0, t.w[c] = F->nkey[c] ? w[c] : 0.0;
}

NPG_API int npg_interior_destroy(npg_interior *F) {
    if (!F) return NPG_OK;
    hipStreamSynchronize(F->ctx->stream);
    delete F;
    return NPG_OK;
}

NPG_API int npg_interior_create(npg_fe *fe, int64_t nkept, const int32_t *cells, const npg_csr *pattern, npg_interior **out) {
    NPG_REQUIRE(fe && out, "npg_interior_create: NULL argument");
    NPG_REQUIRE(!pattern || (pattern->ctx == fe->ctx && pattern->nnode() == 0 && !pattern->uperm),
                "npg_interior_create: the pattern must be a plain-CSR matrix of the engine's context");
    NPG_HIP(hipSetDevice(fe->ctx->device));
    NPG_HIP(hipStreamSynchronize(fe->ctx->stream));
    const FeDev &d = fe->d;
    // the engine's buoyancy DoF codes and the pattern on the host: the plan is host work, done once
    std::vector<int32_t> cb((size_t)d.ncell * d.nb), col;
    NPG_HIP(hipMemcpy(cb.data(), d.cb, cb.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (pattern) {
        NPG_REQUIRE((int64_t)pattern->h_rowptr.size() == pattern->m + 1, "npg_interior_create: the pattern has no host row offsets");
        col.resize((size_t)pattern->nnz);
        NPG_HIP(hipMemcpy(col.data(), pattern->col, col.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    DevCells hv{};
    hv.cb_ = cb.data(), hv.ncell = d.ncell, hv.nb = d.nb;
    std::unique_ptr<npg_interior> F(new npg_interior());
    NPG_REQUIRE_OK(itr_build_plan(hv, fe->n_b, nkept, cells, pattern ? pattern->m : 0, pattern ? pattern->h_rowptr.data() : nullptr,
                                  pattern ? col.data() : nullptr, F->plan));
    F->ctx = fe->ctx;
    F->fe = fe;
    F->nkept = nkept;
    F->nblocks = (int)std::min<int64_t>((nkept + kItrBlock - 1) / kItrBlock, kItrMaxBlocks);
    const ItrPlan &pl = F->plan;
    NPG_HIP(F->cell.upload(cells, (size_t)nkept));
    NPG_HIP(F->loc.alloc((size_t)d.nb * (size_t)nkept));                   // (pass 1 writes every entry pass 2 reads)
    NPG_HIP(F->part.alloc((size_t)F->nblocks * kPartStride));
    NPG_HIP(F->gptr.upload(pl.gptr));
    NPG_HIP(F->gslot.upload(pl.gslot));
    NPG_HIP(F->eptr.upload(pl.eptr));
    NPG_HIP(F->ecell.upload(pl.ecell));
    NPG_HIP(F->ecode.upload(pl.ecode));
    NPG_HIP(F->epos.upload(pl.epos));
    *out = F.release();
    return NPG_OK;
}

NPG_API int npg_interior_set_series(npg_interior *F, int which, int nkey, const double *tables) {
    NPG_REQUIRE_OK(check_interior_set_series(F != nullptr, which, nkey, tables, F ? F->fe->d.nq : 0, F ? F->nkept : 0));
    NPG_HIP(hipSetDevice(F->ctx->device));
    NPG_HIP(hipStreamSynchronize(F->ctx->stream));          // an apply still in flight reads the table this call replaces
    // (nkept = 0: no storage, but the series counts as set - one double keeps the pointer non-null)
    const size_t n = tables ? std::max<size_t>(1, (size_t)nkey * F->fe->d.nq * (size_t)F->nkept) : 0;
    NPG_HIP(F->ser[which].zeros(n));
    if (tables && F->nkept > 0) NPG_HIP(hipMemcpy(F->ser[which].p, tables, n * sizeof(double), hipMemcpyHostToDevice));
    F->nkey[which] = tables ? nkey : 0;
    return NPG_OK;
}

NPG_API int npg_interior_set_gamma(npg_interior *F, const double *table) {
    NPG_REQUIRE_OK(check_interior_set_gamma(F != nullptr, table, F ? F->fe->d.nq : 0, F ? F->nkept : 0));
    NPG_HIP(hipSetDevice(F->ctx->device));
    NPG_HIP(hipStreamSynchronize(F->ctx->stream));
    const size_t n = table ? std::max<size_t>(1, (size_t)F->fe->d.nq * (size_t)F->nkept) : 0;
    NPG_HIP(F->gamma.zeros(n));
    if (table && F->nkept > 0) NPG_HIP(hipMemcpy(F->gamma.p, table, n * sizeof(double), hipMemcpyHostToDevice));
    return NPG_OK;
}

NPG_API int npg_interior_apply(npg_interior *F, const int32_t *key, const double *w, npg_vec *rhs_src_out) {
    const bool all = F && rhs_src_out;
    NPG_REQUIRE_OK(check_interior_apply(all, key, w, all ? F->nkey : nullptr, all ? F->fe->n_b : 0, all ? rhs_src_out->n : 0,
                                        all && rhs_src_out->ctx == F->ctx));
    NPG_HIP(hipSetDevice(F->ctx->device));
    hipStream_t st = F->ctx->stream;
    const FeDev &d = F->fe->d;
    ItrCells t = itr_cells(F);
    itr_set_keys(F, key, w, t);
    if (F->nkept > 0) {
        const dim3 grid((unsigned)((F->nkept + kItrBlock - 1) / kItrBlock)), block(kItrBlock);
        if (d.nb == 10) hipLaunchKernelGGL(k_interior_local<10>, grid, block, 0, st, d, t, F->loc.p);
        else hipLaunchKernelGGL(k_interior_local<4>, grid, block, 0, st, d, t, F->loc.p);
        NPG_HIP(hipGetLastError());
    }
    const int64_t nrow = F->fe->n_b;
    if (nrow > 0) {
        hipLaunchKernelGGL(k_interior_gather, dim3((unsigned)((nrow + kItrBlock - 1) / kItrBlock)), dim3(kItrBlock), 0, st, nrow, F->gptr.p,
                           F->gslot.p, F->loc.p, rhs_src_out->d);
        NPG_HIP(hipGetLastError());
    }
    return NPG_OK;
}

NPG_API int npg_interior_matrix(npg_interior *F, npg_csr *R) {
    const bool all = F && R;
    NPG_REQUIRE_OK(check_interior_matrix(all, all && F->plan.has_pattern, all && F->gamma.p != nullptr,
                                         all && R->ctx == F->ctx && R->nnode() == 0 && !R->uperm && !R->packed && R->m == F->plan.pat_m &&
                                             R->nnz == F->plan.pat_nnz));
    NPG_HIP(hipSetDevice(F->ctx->device));
    hipStream_t st = F->ctx->stream;
    NPG_HIP(hipMemsetAsync(R->val, 0, (size_t)R->nnz * sizeof(double), st));
    const int64_t nent = (int64_t)F->plan.epos.size();
    if (nent > 0) {
        const FeDev &d = F->fe->d;
        const ItrCells t = itr_cells(F);
        const dim3 grid((unsigned)((nent + kItrBlock - 1) / kItrBlock)), block(kItrBlock);
        if (d.nb == 10)
            hipLaunchKernelGGL(k_interior_matrix<10>, grid, block, 0, st, d, t, nent, F->eptr.p, F->ecell.p, F->ecode.p, F->epos.p, R->val.p);
        else
            hipLaunchKernelGGL(k_interior_matrix<4>, grid, block, 0, st, d, t, nent, F->eptr.p, F->ecell.p, F->ecode.p, F->epos.p, R->val.p);
        NPG_HIP(hipGetLastError());
    }
    return NPG_OK;
}

NPG_API int npg_interior_budget(npg_interior *F, const int32_t *key, const double *w, const npg_vec *b, npg_vec *out) {
    const bool all = F && b && out;
    NPG_REQUIRE_OK(check_interior_budget(all, key, w, all ? F->nkey : nullptr, all ? F->fe->n_b : 0, all ? b->n : 0, all ? out->n : 0,
                                         all && b->ctx == F->ctx && out->ctx == F->ctx));
    NPG_HIP(hipSetDevice(F->ctx->device));
    hipStream_t st = F->ctx->stream;
    const FeDev &d = F->fe->d;
    ItrCells t = itr_cells(F);
    itr_set_keys(F, key, w, t);
    const dim3 block(kItrBlock);
    if (F->nblocks > 0) {
        const dim3 grid((unsigned)F->nblocks);
        if (d.nb == 10) hipLaunchKernelGGL(k_interior_budget<10>, grid, block, 0, st, d, t, b->d, F->part.p);
        else hipLaunchKernelGGL(k_interior_budget<4>, grid, block, 0, st, d, t, b->d, F->part.p);
        NPG_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_interior_fold, dim3(1), block, 0, st, F->part.p, F->nblocks, out->d);       // (no partial rows: zeros)
    NPG_HIP(hipGetLastError());
    return NPG_OK;
}

NPG_API int npg_interior_info(const npg_interior *F, int64_t *nkept, int64_t *load_slots, int64_t *matrix_entries, int64_t *matrix_slots) {
    NPG_REQUIRE(F, "npg_interior_info: NULL argument");
    if (nkept) *nkept = F->nkept;
    if (load_slots) *load_slots = (int64_t)F->plan.gslot.size();
    if (matrix_entries) *matrix_entries = (int64_t)F->plan.epos.size();
    if (matrix_slots) *matrix_slots = (int64_t)F->plan.ecell.size();
    return NPG_OK;
}
