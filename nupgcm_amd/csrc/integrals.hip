// Quadrature integrals of the device-resident state over the mesh (npg_integrals_compute): volume, mean and variance of b', kinetic
// energy, buoyancy production, dissipation, potential energy, advective tendency, variance destruction, diffusive flux, (div u)^2 -
// the NPG_NINT channels of integrals_core.h.  The reference has no counterpart (its run log prints maxima, its post-processing
// stops at streamfunctions); the discrete identities x' A x, x_u' (B b + lift), b' M b, b' (Kh + Kv) b pin the numbers.
//   k_cell_integrals<NB>  one lane per cell, grid-stride; the [component][cell] tables are read with unit stride, the shape tables
//                         come from LDS (stage_tables); a lane keeps its NPG_NINT accumulators in registers across its cells; at the
//                         end wave_sum, lane 0 of each wave -> LDS, the 4 waves added in order: one partial row per workgroup
//   k_integrals_fold      one workgroup adds the partial rows in the fixed order of reduce_partials
// Deterministic: the grid is a function of ncell alone (not of the device, not of the environment), every sum has one order, no
// atomics - two calls on the same state give the same bits.  Always fp64 (npg_fe_set_precision does not apply).
#include <cmath>

#include "common.h"
#include "device_utils.h"
#include "fe_dev.h"
#include "integrals_core.h"

static_assert(NPG_NINT == npg::kNInt, "NPG_NINT of the header and kNInt of integrals_core.h must agree");
static_assert(npg::kNInt <= npg::kPartStride, "a partial row holds the channels");

namespace npg {

constexpr int kIntSlices = kBlock / kPartStride;       // reduce_partials: rows slice, slice + kIntSlices, ... per 32-lane slice
constexpr int kIntMaxBlocks = 1024;                    // partial rows at most: 4 per CU, and kIntSlices x 128 rows in the fold

// part[blockIdx.x][kPartStride]: the workgroup's sums of the NPG_NINT channels over its cells (mask: null = every cell counts)
template <int NB>
__global__ void __launch_bounds__(kBlock) k_cell_integrals(FeDev d, const double *__restrict__ cz, const uint8_t *__restrict__ mask,
                                                           const double *__restrict__ xu, const double *__restrict__ xb,
                                                           int full_stress, double *__restrict__ part) {
    __shared__ FeTables t;
    __shared__ double sh[(kBlock / kWave) * kPartStride];
    stage_tables(d, t);
    const CellsYZ<DevCells> cells{cell_view(d), nullptr, cz};        // cz = z of the cell's own vertices, [4][ncell]
    double acc[kNInt];
#pragma unroll
    for (int k = 0; k < kNInt; ++k) acc[k] = 0.0;
    for (int64_t c = blockIdx.x * (int64_t)kBlock + threadIdx.x; c < d.ncell; c += (int64_t)gridDim.x * kBlock)
        if (!mask || mask[c]) cell_integrals<NB>(t, cells, d.nq, xu, xb, c, full_stress != 0, acc);
    block_store_partials<kNInt, kBlock / kWave>(acc, kNInt, sh, part);
}

__global__ void __launch_bounds__(kBlock) k_integrals_fold(const double *__restrict__ part, int nblocks, double *__restrict__ out) {
    __shared__ double tmp[kIntSlices * kPartStride], tot[kPartStride];
    reduce_partials<kIntSlices, kIntMaxBlocks / kIntSlices>(part, nblocks, kNInt, tmp, tot);
    if (threadIdx.x < kNInt) out[threadIdx.x] = tot[threadIdx.x];
}

}  // namespace npg

using namespace npg;

struct npg_integrals {
    npg_ctx *ctx = nullptr;
    npg_fe *fe = nullptr;
    DevBuf<double> cz;           // [4][ncell]
    DevBuf<uint8_t> mask;        // [ncell] or null
    DevBuf<double> part;         // [nblocks][kPartStride]
    int nblocks = 0;
};

NPG_API int npg_integrals_destroy(npg_integrals *I) {
    if (!I) return NPG_OK;
    hipStreamSynchronize(I->ctx->stream);
    delete I;
    return NPG_OK;
}

NPG_API int npg_integrals_create(npg_fe *fe, const double *cell_z, const uint8_t *cell_mask, npg_integrals **out) {
    NPG_REQUIRE_OK(check_integrals_create(fe && out, cell_z, fe ? fe->d.ncell : 0));
    const int64_t nc = fe->d.ncell;
    std::vector<double> zt((size_t)nc * 4);
    for (int64_t c = 0; c < nc; ++c)
        for (int i = 0; i < 4; ++i) zt[(size_t)i * nc + c] = cell_z[(size_t)c * 4 + i];
    NPG_HIP(hipSetDevice(fe->ctx->device));
    std::unique_ptr<npg_integrals> I(new npg_integrals());
    I->ctx = fe->ctx;
    I->fe = fe;
    I->nblocks = (int)std::min<int64_t>((nc + kBlock - 1) / kBlock, kIntMaxBlocks);
    NPG_HIP(I->cz.upload(zt));
    if (cell_mask) NPG_HIP(I->mask.upload(cell_mask, (size_t)nc));
    NPG_HIP(I->part.alloc((size_t)I->nblocks * kPartStride));
    *out = I.release();
    return NPG_OK;
}

NPG_API int npg_integrals_compute(npg_integrals *I, const npg_vec *x_inv, const npg_vec *b, int full_stress, npg_vec *out) {
    NPG_REQUIRE_OK(check_integrals_compute(I, x_inv, b, full_stress, out));
    npg_fe *fe = I->fe;
    NPG_HIP(hipSetDevice(fe->ctx->device));
    hipStream_t st = fe->ctx->stream;
    const FeDev &d = fe->d;
    const dim3 grid((unsigned)I->nblocks), block(kBlock);
    if (d.nb == 10)
        hipLaunchKernelGGL(k_cell_integrals<10>, grid, block, 0, st, d, I->cz.p, I->mask.p, x_inv->d, b->d, full_stress, I->part.p);
    else
        hipLaunchKernelGGL(k_cell_integrals<4>, grid, block, 0, st, d, I->cz.p, I->mask.p, x_inv->d, b->d, full_stress, I->part.p);
    NPG_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_integrals_fold, dim3(1), block, 0, st, I->part.p, I->nblocks, out->d);
    NPG_HIP(hipGetLastError());
    return NPG_OK;
}
