// Transports of the device-resident state through sections (npg_sections_*): area, volume and buoyancy transport, the
// diffusive flux and the means of b', p, u, z, d_z b' over the bins of planes that cut the mesh - the NPG_NSEC channels of
// sections_core.h.  The plan (which cells a plane cuts, the polygons clipped at the bin edges, the pieces sorted by bin), the per-piece
// arithmetic, the fold order and the argument checks are sections_core.h's, shared with the host library.  Two launches:
//   k_section_pieces<NB>  one lane per piece, the grid a function of npiece alone: unit-stride reads of the component-major piece tables
//                         (lam[12][npiece], all four barycentrics of the three corners stored), the cell's 44 DoF codes and values gathered
//                         through the engine's [component][cell] tables, the six points of the triangle rule with the P2 basis formed on
//                         the fly; the piece's 14 terms go to terms[ch][piece] with plain stores - the handle's scratch, or the caller's
//                         pieces_out, which then IS the scratch
//   k_section_fold        one wave per (bin, channel): lane l adds the bin's pieces l, l + 64, ... in order from 0.0, then the lanes are
//                         added in wave_sum's fixed tree - the order sections_core.h states; an empty bin stores 0.0
// Deterministic: every sum has one order that is a function of the plan alone, no atomics, no LDS - the bits of the host library on
// every call (the closure's tanh apart).
#include "common.h"
#include "device_utils.h"
#include "fe_dev.h"
#include "sections_core.h"

static_assert(NPG_NSEC == npg::kNSec, "NPG_NSEC of the header and kNSec of sections_core.h must agree");
static_assert(NPG_SEC_KH == npg::kSecKh && NPG_SEC_KV == npg::kSecKv, "the coefficient codes of the header and of sections_core.h must agree");

namespace npg {

constexpr int kSecBlock = NPG_SEC_BLOCK;
static_assert(kSecBlock % kWave == 0 && kSecBlock <= 1024, "whole waves");

using DevPieces = SecPieces<DevCells>;

template <int NB>
__global__ void __launch_bounds__(kSecBlock) k_section_pieces(DevPieces t, const double *__restrict__ xu, const double *__restrict__ xb,
                                                              MixClosure cl, double *__restrict__ terms) {
    const int64_t i = (int64_t)blockIdx.x * kSecBlock + threadIdx.x;
    if (i >= t.np) return;
    double term[kNSec];
    section_piece<NB>(t, xu, xb, i, cl, term);
#pragma unroll
    for (int k = 0; k < kNSec; ++k) terms[(size_t)k * (size_t)t.np + i] = term[k];
}

// one wave per (bin, channel): lane l adds the bin's pieces l, l + 64, ... in ascending order from 0.0 (unit stride across the wave),
// wave_sum's butterfly adds the 64 lanes - the order section_fold states, so lane 0 holds the host library's bits
__global__ void __launch_bounds__(kSecBlock) k_section_fold(const int64_t *__restrict__ bin_ptr, const double *__restrict__ terms, int64_t np,
                                                            int64_t nbin, double *__restrict__ out) {
    static_assert(kSecFoldLanes == kWave, "one accumulator per lane");
    const int64_t j = (int64_t)blockIdx.x * (kSecBlock / kWave) + (threadIdx.x >> 6);      // uniform over the wave
    if (j >= nbin * kNSec) return;
    const int64_t bin = j / kNSec;
    const double *t = terms + (size_t)(j % kNSec) * (size_t)np;
    const int64_t last = bin_ptr[bin + 1];
    double sum = 0.0;
#pragma unroll 8                                        // (eight loads in flight; the additions keep their order)
    for (int64_t i = bin_ptr[bin] + (threadIdx.x & 63); i < last; i += kWave) sum += t[i];
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0) out[j] = sum;
}

}  // namespace npg

using namespace npg;

struct npg_sections {
    npg_ctx *ctx = nullptr;
    npg_fe *fe = nullptr;
    SecPlan plan;                       // host: what npg_sections_pieces hands back
    int64_t np = 0;
    MixClosure cl{0.0, 0.0, 0.0, 0.0};
    DevBuf<double> cz;                  // [4][ncell]: z of the cells' own vertices
    DevBuf<int32_t> cell;               // [np]
    DevBuf<uint8_t> sec;                // [np]
    DevBuf<double> lam, area, normal;   // [12][np], [np], [nsec][3]
    DevBuf<int64_t> bin_ptr;            // [nbin + 1]
    DevBuf<double> coef[kSecNCoef];     // [6][np] or null
    DevBuf<double> terms;               // [NPG_NSEC][np]: the scratch of a compute without pieces_out
};

NPG_API int npg_sections_destroy(npg_sections *S) {
    if (!S) return NPG_OK;
    hipStreamSynchronize(S->ctx->stream);
    delete S;
    return NPG_OK;
}

NPG_API int npg_sections_create(npg_fe *fe, const double *cell_xyz, int nsec, const double *frames, const int32_t *n1, const int32_t *n2,
                                const double *edges1, const double *edges2, const uint8_t *cell_mask, npg_sections **out) {
    NPG_REQUIRE(fe && out, "npg_sections_create: NULL argument");
    NPG_HIP(hipSetDevice(fe->ctx->device));
    bool flat = true;                   // an embedded 2-D engine keeps every quadrature point on the face lambda_4 = 0 of its padded tetrahedra
    {
        std::vector<double> q1((size_t)fe->d.nq * 4);
        NPG_HIP(hipMemcpy(q1.data(), fe->d.N1, q1.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (int q = 0; q < fe->d.nq; ++q) flat = flat && q1[(size_t)q * 4 + 3] == 0.0;
    }
    std::unique_ptr<npg_sections> S(new npg_sections());
    const int64_t nc = fe->d.ncell;
    NPG_REQUIRE_OK(sec_build_plan(true, flat, nc, cell_xyz, nsec, frames, n1, n2, edges1, edges2, cell_mask, S->plan));
    S->ctx = fe->ctx;
    S->fe = fe;
    const SecPlan &pl = S->plan;
    const size_t np = (size_t)pl.npiece();
    S->np = (int64_t)np;
    std::vector<double> cz((size_t)nc * 4), lam(12 * np);
    for (int64_t c = 0; c < nc; ++c)
        for (int k = 0; k < 4; ++k) cz[(size_t)k * nc + c] = cell_xyz[(size_t)c * 12 + 3 * k + 2];
    for (size_t i = 0; i < np; ++i)
        for (int k = 0; k < 12; ++k) lam[(size_t)k * np + i] = pl.lam[12 * i + k];
    NPG_HIP(S->cz.upload(cz));
    NPG_HIP(S->cell.upload(pl.cell));
    NPG_HIP(S->sec.upload(pl.sec));
    NPG_HIP(S->lam.upload(lam));
    NPG_HIP(S->area.upload(pl.area));
    NPG_HIP(S->normal.upload(pl.normal));
    NPG_HIP(S->bin_ptr.upload(pl.bin_ptr));
    NPG_HIP(S->terms.alloc((size_t)kNSec * np));
    *out = S.release();
    return NPG_OK;
}

NPG_API int npg_sections_info(const npg_sections *S, int64_t *npiece, int64_t *nbin, int64_t *ncut_cells, int64_t *max_per_bin) {
    NPG_REQUIRE(S, "npg_sections_info: NULL argument");
    if (npiece) *npiece = S->np;
    if (nbin) *nbin = S->plan.nbin;
    if (ncut_cells) *ncut_cells = S->plan.ncut_cells;
    if (max_per_bin) *max_per_bin = S->plan.max_per_bin;
    return NPG_OK;
}

NPG_API int npg_sections_pieces(const npg_sections *S, int32_t *cell, int32_t *bin, double *lam, double *area) {
    NPG_REQUIRE(S, "npg_sections_pieces: NULL argument");
    const SecPlan &pl = S->plan;
    if (cell) std::copy(pl.cell.begin(), pl.cell.end(), cell);
    if (bin) std::copy(pl.bin.begin(), pl.bin.end(), bin);
    if (lam) std::copy(pl.lam.begin(), pl.lam.end(), lam);
    if (area) std::copy(pl.area.begin(), pl.area.end(), area);
    return NPG_OK;
}

NPG_API int npg_sections_set_coeff(npg_sections *S, int which, const double *table) {
    NPG_REQUIRE_OK(check_sections_coeff(S != nullptr, which, table, S ? S->np : 0));
    NPG_HIP(hipSetDevice(S->ctx->device));
    DevBuf<double> t;                   // uploaded beside the table in use: a failure leaves the handle as it was
    if (table) NPG_HIP(t.upload(table, (size_t)kSecQ * (size_t)S->np));
    NPG_HIP(hipStreamSynchronize(S->ctx->stream));          // a compute still in flight reads the table this call replaces
    S->coef[which].swap(t);
    return NPG_OK;
}

NPG_API int npg_sections_set_closure(npg_sections *S, double kappa_c, double N2min, double alpha, double N2c) {
    NPG_REQUIRE_OK(check_sections_closure(S != nullptr, kappa_c, N2min, alpha, N2c));
    S->cl = MixClosure{kappa_c, N2min, alpha, N2c};
    return NPG_OK;
}

NPG_API int npg_sections_compute(npg_sections *S, const npg_vec *x_inv, const npg_vec *b, npg_vec *out, npg_vec *pieces_out) {
    NPG_REQUIRE(S && x_inv && b && out, "npg_sections_compute: NULL argument");
    npg_fe *fe = S->fe;
    NPG_REQUIRE_OK(check_sections_compute(true, fe->n_inv, fe->n_b, x_inv->n, b->n, S->plan.nbin, S->np, out->n, pieces_out ? pieces_out->n : -1,
                                          x_inv->ctx == fe->ctx && b->ctx == fe->ctx && out->ctx == fe->ctx &&
                                              (!pieces_out || pieces_out->ctx == fe->ctx)));
    NPG_HIP(hipSetDevice(fe->ctx->device));
    hipStream_t st = fe->ctx->stream;
    double *terms = pieces_out ? pieces_out->d : S->terms.p;
    if (S->np > 0) {
        DevPieces t{{cell_view(fe->d), nullptr, S->cz.p}, S->np, S->cell.p, S->sec.p, S->lam.p, S->area.p, S->normal.p, {}};
        for (int w = 0; w < kSecNCoef; ++w) t.coef_[w] = S->coef[w].p;
        const dim3 grid((unsigned)((S->np + kSecBlock - 1) / kSecBlock)), block(kSecBlock);
        if (fe->d.nb == 10) hipLaunchKernelGGL(k_section_pieces<10>, grid, block, 0, st, t, x_inv->d, b->d, S->cl, terms);
        else hipLaunchKernelGGL(k_section_pieces<4>, grid, block, 0, st, t, x_inv->d, b->d, S->cl, terms);
        NPG_HIP(hipGetLastError());
    }
    const int64_t nout = S->plan.nbin * kNSec;
    constexpr int kPerBlock = kSecBlock / kWave;        // (bin, channel) sums per workgroup
    hipLaunchKernelGGL(k_section_fold, dim3((unsigned)((nout + kPerBlock - 1) / kPerBlock)), dim3(kSecBlock), 0, st, S->bin_ptr.p, terms, S->np,
                       S->plan.nbin, out->d);
    NPG_HIP(hipGetLastError());
    return NPG_OK;
}
