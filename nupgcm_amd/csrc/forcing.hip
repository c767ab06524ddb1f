// Time-dependent surface forcing on the device (npg_forcing_*): the wind part of the inversion's right-hand side and the
// flux vector of the evolution, recomputed from keyframe tables for the time level being solved, and the surface mass matrix of a
// restoring condition.  The reference evaluates its surface integrals once, on the host.  The arithmetic, the plan and the checks are
// forcing_core.h's, shared with the host library.
//   k_forcing_local<KB>           one lane per face: blend the two keyframes of every channel at the nine face points, weigh, contract
//                                 with the face functions; loc[load][k][face].  Tables and loc are [..][face]: unit stride across a wave
//   k_forcing_gather              one lane per destination row of [inversion rows | buoyancy rows]: its slots of loc added in (face, k)
//                                 order, out = base + alpha sum / alpha sum; rows without slots get the base / 0
//   k_forcing_surface_matrix<KB>  one lane per matrix entry that some face touches: its slots (face, i, j) added in order
// No atomics, no LDS, one order of every sum: the same bits on every call.
#include <cmath>

#include "common.h"
#include "device_utils.h"
#include "fe_dev.h"
#include "forcing_core.h"

static_assert(NPG_FRC_NSERIES == npg::kFrcNSeries, "NPG_FRC_NSERIES of the header and kFrcNSeries of forcing_core.h must agree");

namespace npg {

constexpr int kFrcBlock = NPG_FRC_BLOCK;
static_assert(kFrcBlock % kWave == 0 && kFrcBlock <= 1024, "whole waves");

template <int KB>
__global__ void __launch_bounds__(kFrcBlock) k_forcing_local(FrcFaces t, double *__restrict__ loc) {
    const int64_t f = (int64_t)blockIdx.x * kFrcBlock + threadIdx.x;
    if (f < t.nface) frc_face_loads<KB>(t, f, loc);
}

__global__ void __launch_bounds__(kFrcBlock) k_forcing_gather(int64_t nrow, int64_t n_inv, const int32_t *__restrict__ ptr,
                                                              const int32_t *__restrict__ slot, const double *__restrict__ loc, double alpha,
                                                              const double *__restrict__ base, double *__restrict__ inv_out,
                                                              double *__restrict__ flux_out) {
    const int64_t r = (int64_t)blockIdx.x * kFrcBlock + threadIdx.x;
    if (r < nrow) frc_gather_row(r, n_inv, ptr, slot, loc, alpha, base, inv_out, flux_out);
}

template <int KB>
__global__ void __launch_bounds__(kFrcBlock) k_forcing_surface_matrix(FrcFaces t, int64_t nent, const int32_t *__restrict__ eptr,
                                                                      const int32_t *__restrict__ eface, const uint8_t *__restrict__ ecode,
                                                                      const int64_t *__restrict__ epos, double scale, double *__restrict__ val) {
    const int64_t e = (int64_t)blockIdx.x * kFrcBlock + threadIdx.x;
    if (e < nent) val[epos[e]] = scale * frc_matrix_entry<KB>(t, eptr, eface, ecode, e);
}

}  // namespace npg

using namespace npg;

struct npg_forcing {
    npg_ctx *ctx = nullptr;
    npg_fe *fe = nullptr;
    int64_t nface = 0;
    FrcPlan plan;                               // host
    int32_t nkey[kFrcNSeries] = {0, 0, 0, 0};
    DevBuf<double> area2, ser[kFrcNSeries], gamma, loc;
    DevBuf<int32_t> gptr, gslot, eptr, eface;
    DevBuf<uint8_t> ecode;
    DevBuf<int64_t> epos;
};

static FrcFaces frc_faces(const npg_forcing *F) {
    FrcFaces t{};
    t.nface = F->nface;
    t.area2 = F->area2;
    for (int c = 0; c < kFrcNSeries; ++c) t.ser[c] = F->ser[c], t.nkey[c] = F->nkey[c];
    t.gamma = F->gamma;
    return t;
}

NPG_API int npg_forcing_destroy(npg_forcing *F) {
    if (!F) return NPG_OK;
    hipStreamSynchronize(F->ctx->stream);
    delete F;
    return NPG_OK;
}

NPG_API int npg_forcing_create(npg_fe *fe, int64_t nface, const int32_t *face_cell, const uint8_t *face_local, const double *face_area2,
                               const npg_csr *pattern, npg_forcing **out) {
    NPG_REQUIRE(fe && out, "npg_forcing_create: NULL argument");
    NPG_REQUIRE(!pattern || (pattern->ctx == fe->ctx && pattern->nnode() == 0 && !pattern->uperm),
                "npg_forcing_create: the pattern must be a plain-CSR matrix of the engine's context");
    NPG_HIP(hipSetDevice(fe->ctx->device));
    NPG_HIP(hipStreamSynchronize(fe->ctx->stream));
    const FeDev &d = fe->d;
    {   // an embedded 2-D engine keeps every quadrature point on the face lambda_4 = 0 of its padded tetrahedra: it has no boundary faces
        std::vector<double> n1((size_t)d.nq * 4);
        NPG_HIP(hipMemcpy(n1.data(), d.N1, n1.size() * sizeof(double), hipMemcpyDeviceToHost));
        bool flat = true;
        for (int q = 0; q < d.nq; ++q) flat = flat && n1[(size_t)q * 4 + 3] == 0.0;
        NPG_REQUIRE(!flat, "npg_forcing_create: an embedded 2-D engine is refused (its boundary is made of segments, not of faces)");
    }
    // the engine's DoF codes and the pattern on the host: the plan is host work, done once
    std::vector<int32_t> cu((size_t)d.ncell * 30), cb((size_t)d.ncell * d.nb), col;
    NPG_HIP(hipMemcpy(cu.data(), d.cu, cu.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    NPG_HIP(hipMemcpy(cb.data(), d.cb, cb.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (pattern) {
        NPG_REQUIRE((int64_t)pattern->h_rowptr.size() == pattern->m + 1, "npg_forcing_create: the pattern has no host row offsets");
        col.resize((size_t)pattern->nnz);
        NPG_HIP(hipMemcpy(col.data(), pattern->col, col.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    DevCells hv{};
    hv.cu_ = cu.data(), hv.cb_ = cb.data(), hv.ncell = d.ncell, hv.nb = d.nb;
    std::unique_ptr<npg_forcing> F(new npg_forcing());
    NPG_REQUIRE_OK(frc_build_plan(hv, fe->n_inv, fe->n_b, nface, face_cell, face_local, face_area2, pattern ? pattern->m : 0,
                                  pattern ? pattern->h_rowptr.data() : nullptr, pattern ? col.data() : nullptr, F->plan));
    F->ctx = fe->ctx;
    F->fe = fe;
    F->nface = nface;
    const FrcPlan &pl = F->plan;
    NPG_HIP(F->area2.upload(face_area2, (size_t)nface));
    NPG_HIP(F->loc.alloc((size_t)kFrcNLoad * kFrcK * (size_t)nface));      // (pass 1 writes every entry pass 2 reads)
    NPG_HIP(F->gptr.upload(pl.gptr));
    NPG_HIP(F->gslot.upload(pl.gslot));
    NPG_HIP(F->eptr.upload(pl.eptr));
    NPG_HIP(F->eface.upload(pl.eface));
    NPG_HIP(F->ecode.upload(pl.ecode));
    NPG_HIP(F->epos.upload(pl.epos));
    *out = F.release();
    return NPG_OK;
}

NPG_API int npg_forcing_set_series(npg_forcing *F, int which, int nkey, const double *tables) {
    NPG_REQUIRE(F, "npg_forcing_set_series: NULL argument");
    NPG_REQUIRE(which >= 0 && which < kFrcNSeries, "npg_forcing_set_series: which must be NPG_FRC_TAUX .. NPG_FRC_TARGET, got %d", which);
    NPG_REQUIRE(!tables || nkey >= 1, "npg_forcing_set_series: nkey must be >= 1, got %d", nkey);
    if (tables) NPG_REQUIRE_OK(frc_check_table("npg_forcing_set_series", tables, nkey, F->nface, false));
    NPG_HIP(hipSetDevice(F->ctx->device));
    NPG_HIP(hipStreamSynchronize(F->ctx->stream));          // an apply still in flight reads the table this call replaces
    // (nface = 0: no storage, but the series counts as set - one double keeps the pointer non-null)
    const size_t n = tables ? std::max<size_t>(1, (size_t)nkey * kBndQ * (size_t)F->nface) : 0;
    NPG_HIP(F->ser[which].zeros(n));
    if (tables && F->nface > 0) NPG_HIP(hipMemcpy(F->ser[which].p, tables, n * sizeof(double), hipMemcpyHostToDevice));
    F->nkey[which] = tables ? nkey : 0;
    return NPG_OK;
}

NPG_API int npg_forcing_set_gamma(npg_forcing *F, const double *table) {
    NPG_REQUIRE(F, "npg_forcing_set_gamma: NULL argument");
    if (table) NPG_REQUIRE_OK(frc_check_table("npg_forcing_set_gamma", table, 1, F->nface, true));
    NPG_HIP(hipSetDevice(F->ctx->device));
    NPG_HIP(hipStreamSynchronize(F->ctx->stream));
    const size_t n = table ? std::max<size_t>(1, kBndQ * (size_t)F->nface) : 0;
    NPG_HIP(F->gamma.zeros(n));
    if (table && F->nface > 0) NPG_HIP(hipMemcpy(F->gamma.p, table, n * sizeof(double), hipMemcpyHostToDevice));
    return NPG_OK;
}

NPG_API int npg_forcing_apply(npg_forcing *F, const int32_t *key, const double *w, double alpha, const npg_vec *b_inv_base, npg_vec *b_inv_out,
                              npg_vec *rhs_flux_out) {
    NPG_REQUIRE(F, "npg_forcing_apply: NULL argument");
    const bool all = b_inv_base && b_inv_out && rhs_flux_out;
    NPG_REQUIRE_OK(frc_check_apply(key, w, alpha, F->nkey, F->fe->n_inv, F->fe->n_b, all, all ? b_inv_base->n : 0, all ? b_inv_out->n : 0,
                                   all ? rhs_flux_out->n : 0, all && b_inv_base->d == b_inv_out->d,
                                   all && b_inv_base->ctx == F->ctx && b_inv_out->ctx == F->ctx && rhs_flux_out->ctx == F->ctx));
    NPG_HIP(hipSetDevice(F->ctx->device));
    hipStream_t st = F->ctx->stream;
    FrcFaces t = frc_faces(F);
    for (int c = 0; c < kFrcNSeries; ++c) t.key[c] = F->nkey[c] ? key[c] : 0, t.w[c] = F->nkey[c] ? w[c] : 0.0;
    if (F->nface > 0) {
        const dim3 grid((unsigned)((F->nface + kFrcBlock - 1) / kFrcBlock)), block(kFrcBlock);
        if (F->plan.kb == 6) hipLaunchKernelGGL(k_forcing_local<6>, grid, block, 0, st, t, F->loc.p);
        else hipLaunchKernelGGL(k_forcing_local<3>, grid, block, 0, st, t, F->loc.p);
        NPG_HIP(hipGetLastError());
    }
    const int64_t nrow = F->fe->n_inv + F->fe->n_b;
    if (nrow > 0) {
        hipLaunchKernelGGL(k_forcing_gather, dim3((unsigned)((nrow + kFrcBlock - 1) / kFrcBlock)), dim3(kFrcBlock), 0, st, nrow, F->fe->n_inv,
                           F->gptr.p, F->gslot.p, F->loc.p, alpha, b_inv_base->d, b_inv_out->d, rhs_flux_out->d);
        NPG_HIP(hipGetLastError());
    }
    return NPG_OK;
}

NPG_API int npg_forcing_surface_matrix(npg_forcing *F, double scale, npg_csr *S) {
    NPG_REQUIRE(F && S, "npg_forcing_surface_matrix: NULL argument");
    NPG_REQUIRE(std::isfinite(scale), "npg_forcing_surface_matrix: scale is not finite");
    NPG_REQUIRE(F->plan.has_pattern, "npg_forcing_surface_matrix: the handle was created without a pattern");
    NPG_REQUIRE(F->gamma.p, "npg_forcing_surface_matrix: no gamma table (npg_forcing_set_gamma)");
    NPG_REQUIRE(S->ctx == F->ctx && S->nnode() == 0 && !S->uperm && !S->packed && S->m == F->plan.pat_m && S->nnz == F->plan.pat_nnz,
                "npg_forcing_surface_matrix: S must be a plain-CSR matrix with the pattern given at create");
    NPG_HIP(hipSetDevice(F->ctx->device));
    hipStream_t st = F->ctx->stream;
    NPG_HIP(hipMemsetAsync(S->val, 0, (size_t)S->nnz * sizeof(double), st));
    const int64_t nent = (int64_t)F->plan.epos.size();
    if (nent > 0) {
        const FrcFaces t = frc_faces(F);
        const dim3 grid((unsigned)((nent + kFrcBlock - 1) / kFrcBlock)), block(kFrcBlock);
        if (F->plan.kb == 6)
            hipLaunchKernelGGL(k_forcing_surface_matrix<6>, grid, block, 0, st, t, nent, F->eptr.p, F->eface.p, F->ecode.p, F->epos.p, scale, S->val);
        else
            hipLaunchKernelGGL(k_forcing_surface_matrix<3>, grid, block, 0, st, t, nent, F->eptr.p, F->eface.p, F->ecode.p, F->epos.p, scale, S->val);
        NPG_HIP(hipGetLastError());
    }
    return NPG_OK;
}

NPG_API int npg_forcing_info(const npg_forcing *F, int64_t *nface, int64_t *wind_slots, int64_t *flux_slots, int64_t *matrix_entries,
                             int64_t *matrix_slots) {
    NPG_REQUIRE(F, "npg_forcing_info: NULL argument");
    if (nface) *nface = F->nface;
    if (wind_slots) *wind_slots = F->plan.wind_slots;
    if (flux_slots) *flux_slots = F->plan.flux_slots;
    if (matrix_entries) *matrix_entries = (int64_t)F->plan.epos.size();
    if (matrix_slots) *matrix_slots = (int64_t)F->plan.eface.size();
    return NPG_OK;
}
