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

// the engine's cell tables as cell_integrals reads them ([component][cell]); cz = z of the cell's own vertices, [4][ncell]
struct IntCells {
    FeDev d;
    const double *cz;
    bool has_nu, has_kh, has_kv;
    __device__ __forceinline__ double G(int k, int64_t c) const { return d.G[(size_t)k * d.ncell + c]; }
    __device__ __forceinline__ double wdet(int64_t c) const { return d.wdet[c]; }
    __device__ __forceinline__ double z(int i, int64_t c) const { return cz[(size_t)i * d.ncell + c]; }
    __device__ __forceinline__ double u(const double *x, int l, int64_t c) const {
        return field_val(x, d.u_diri, d.cu[(size_t)l * d.ncell + c]);
    }
    __device__ __forceinline__ double b(const double *x, int i, int64_t c) const {
        return field_val(x, d.b_diri, d.cb[(size_t)i * d.ncell + c]);
    }
    __device__ __forceinline__ double nu(int q, int64_t c) const { return d.nu[(size_t)q * d.ncell + c]; }
    __device__ __forceinline__ double kh(int q, int64_t c) const { return d.kh[(size_t)q * d.ncell + c]; }
    __device__ __forceinline__ double kv(int q, int64_t c) const { return d.kv[(size_t)q * d.ncell + c]; }
};

// part[blockIdx.x][kPartStride]: the workgroup's sums of the NPG_NINT channels over its cells (mask: null = every cell counts)
template <int NB>
__global__ void __launch_bounds__(kBlock) k_cell_integrals(FeDev d, const double *__restrict__ cz, const uint8_t *__restrict__ mask,
                                                           const double *__restrict__ xu, const double *__restrict__ xb,
                                                           int full_stress, double *__restrict__ part) {
    __shared__ FeTables t;
    __shared__ double sh[(kBlock / kWave) * kPartStride];
    stage_tables(d, t);
    const IntCells cells{d, cz, d.nu != nullptr, d.kh != nullptr, d.kv != nullptr};
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
    double *cz = nullptr;        // [4][ncell]
    uint8_t *mask = nullptr;     // [ncell] or null
    double *part = nullptr;      // [nblocks][kPartStride]
    int nblocks = 0;
};

NPG_API int npg_integrals_destroy(npg_integrals *I) {
    if (!I) return NPG_OK;
    hipStreamSynchronize(I->ctx->stream);
    hipFree(I->cz);
    hipFree(I->mask);
    hipFree(I->part);
    delete I;
    return NPG_OK;
}

NPG_API int npg_integrals_create(npg_fe *fe, const double *cell_z, const uint8_t *cell_mask, npg_integrals **out) {
    NPG_REQUIRE(fe && out, "npg_integrals_create: NULL argument");
    NPG_REQUIRE(cell_z, "npg_integrals_create: cell_z is NULL");
    const int64_t nc = fe->d.ncell;
    std::vector<double> zt((size_t)nc * 4);
    for (int64_t c = 0; c < nc; ++c)
        for (int i = 0; i < 4; ++i) {
            const double z = cell_z[(size_t)c * 4 + i];
            NPG_REQUIRE(std::isfinite(z), "npg_integrals_create: cell_z[%lld][%d] is not finite", (long long)c, i);
            zt[(size_t)i * nc + c] = z;
        }
    NPG_HIP(hipSetDevice(fe->ctx->device));
    npg_integrals *I = new npg_integrals();
    I->ctx = fe->ctx;
    I->fe = fe;
    I->nblocks = (int)std::min<int64_t>((nc + kBlock - 1) / kBlock, kIntMaxBlocks);
    hipError_t e = hipMalloc((void **)&I->cz, zt.size() * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(I->cz, zt.data(), zt.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess && cell_mask) {
        e = hipMalloc((void **)&I->mask, (size_t)nc);
        if (e == hipSuccess) e = hipMemcpy(I->mask, cell_mask, (size_t)nc, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipMalloc((void **)&I->part, (size_t)I->nblocks * kPartStride * sizeof(double));
    if (e != hipSuccess) {
        npg_integrals_destroy(I);
        NPG_HIP(e);
    }
    *out = I;
    return NPG_OK;
}

NPG_API int npg_integrals_compute(npg_integrals *I, const npg_vec *x_inv, const npg_vec *b, int full_stress, npg_vec *out) {
    NPG_REQUIRE(I && x_inv && b && out, "npg_integrals_compute: NULL argument");
    npg_fe *fe = I->fe;
    NPG_REQUIRE(x_inv->n == fe->n_inv, "npg_integrals_compute: the flow vector has %lld entries, expected %lld", (long long)x_inv->n,
                (long long)fe->n_inv);
    NPG_REQUIRE(b->n == fe->n_b, "npg_integrals_compute: the buoyancy vector has %lld entries, expected %lld", (long long)b->n,
                (long long)fe->n_b);
    NPG_REQUIRE(out->n >= NPG_NINT, "npg_integrals_compute: out holds %lld doubles, needs NPG_NINT = %d", (long long)out->n, NPG_NINT);
    NPG_REQUIRE(full_stress == 0 || full_stress == 1, "npg_integrals_compute: full_stress must be 0 or 1, got %d", full_stress);
    NPG_REQUIRE(x_inv->ctx == fe->ctx && b->ctx == fe->ctx && out->ctx == fe->ctx, "npg_integrals_compute: arguments of different contexts");
    NPG_HIP(hipSetDevice(fe->ctx->device));
    hipStream_t st = fe->ctx->stream;
    const FeDev &d = fe->d;
    const dim3 grid((unsigned)I->nblocks), block(kBlock);
    if (d.nb == 10)
        hipLaunchKernelGGL(k_cell_integrals<10>, grid, block, 0, st, d, I->cz, I->mask, x_inv->d, b->d, full_stress, I->part);
    else
        hipLaunchKernelGGL(k_cell_integrals<4>, grid, block, 0, st, d, I->cz, I->mask, x_inv->d, b->d, full_stress, I->part);
    NPG_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_integrals_fold, dim3(1), block, 0, st, I->part, I->nblocks, out->d);
    NPG_HIP(hipGetLastError());
    return NPG_OK;
}
