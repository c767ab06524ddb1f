// The device-resident state binned into (latitude band, buoyancy class) (npg_classes_compute): volume census, transports by class
// (the residual overturning), mean depth / buoyancy / stratification and the advective tendency of every class - the NPG_NCLS
// channels of classes_core.h.  The reference overlays isopycnals on a z-coordinate streamfunction and stops there.
//
// The destination of a term depends on the data, so there is no fixed summation order per output as in integrals.hip.  The same
// bits on every call come from ORDER-INDEPENDENT arithmetic instead: the terms are added as 64-bit integers.
//   k_class_scan<NB, S>  pass 1, one lane per cell, grid-stride: S_c = sum |term_c| per channel over the counted samples and the
//                        number of dropped samples, in fp64, reduced exactly as k_cell_integrals does (block_store_partials; the
//                        grid is a function of ncell alone) - one partial row per workgroup
//   k_classes_fold       one workgroup adds the partial rows in the fixed order of reduce_partials, writes the info vector
//                        {dropped, S_c} and the channels' scales 2^(61 - e), frexp(S_c) = (m, e) (class_scale)
//   k_class_bin<NB, S>   pass 2, the same loop: every term -> llrint(term scale_c) -> added as int64 to its bin's slot with a relaxed
//                        device-scope atomic on global memory.  A lane adds up a RUN of samples that share a bin in registers
//                        (the samples of a cell, and the lane's next cells, almost always do) and touches memory only when the bin
//                        changes; zeros are not sent.  Integer addition is associative: any arrival order gives the same table.
//   k_classes_convert    pass 3, integer table -> doubles (value / scale_c)
// sum |round(term scale)| < 2^61 + half a unit per sample: inside int64 for any mesh.  Quantisation: at most half a unit per
// sample, n_bin 2^-61 S_c per bin.  Always fp64 (npg_fe_set_precision does not apply).
//
// S is the SAMPLER (classes_core.h): CensusSampler for npg_classes_compute; MixSampler for the water-mass transformation by mixing
// (npg_classes_mixing, mixing_core.h) - the same passes over the same grid with the NPG_NMIX diffusivity-weighted channels, no velocity
// gathered, the diffusivities of a sample from tables [ns][ncell] (coalesced across the lanes of a wave) or, where a table is null,
// from the scalar.  The partial rows, the scales and the integer table are shared (NPG_NMIX == NPG_NCLS).
#include <cmath>

#include "common.h"
#include "device_utils.h"
#include "fe_dev.h"
#include "classes_core.h"
#include "mixing_core.h"

static_assert(NPG_NMIX == npg::kNMix, "NPG_NMIX of the header and kNMix of mixing_core.h must agree");
static_assert(NPG_NCLS == npg::kNCls, "NPG_NCLS of the header and kNCls of classes_core.h must agree");
static_assert(npg::kClsInfo <= npg::kPartStride, "a partial row holds the channels and the dropped count");

namespace npg {

constexpr int kClsSlices = kBlock / kPartStride;
constexpr int kClsMaxBlocks = 1024;                    // partial rows at most, as kIntMaxBlocks

// part[blockIdx.x][kPartStride]: the workgroup's sums of |term| of the channels, then its dropped samples; cy / cz = y / z of the
// cells' own vertices, [4][ncell]
template <int NB, class Sampler>
__global__ void __launch_bounds__(kBlock) k_class_scan(FeDev d, const double *__restrict__ cy, const double *__restrict__ cz,
                                                       const uint8_t *__restrict__ mask, ClsRule r, Sampler sm, double *__restrict__ part) {
    __shared__ double sh[(kBlock / kWave) * kPartStride];
    const CellsYZ<DevCells> cells{cell_view(d), cy, cz};
    double acc[kClsInfo];
#pragma unroll
    for (int k = 0; k < kClsInfo; ++k) acc[k] = 0.0;
    for (int64_t c = blockIdx.x * (int64_t)kBlock + threadIdx.x; c < d.ncell; c += (int64_t)gridDim.x * kBlock) {
        if (mask && !mask[c]) continue;
        typename Sampler::template Cell<NB> n;
        sm.template load<NB>(cells, c, n);
        for (int s = 0; s < r.ns; ++s) {
            double term[kNCls];
            int64_t band, cls;
            if (sm.template sample<NB, false>(cells, n, r, s, c, &band, &cls, term)) {
#pragma unroll
                for (int k = 0; k < kNCls; ++k) acc[k] += fabs(term[k]);
            } else {
                acc[kNCls] += 1.0;
            }
        }
    }
    block_store_partials<kClsInfo, kBlock / kWave>(acc, kClsInfo, sh, part);
}

// info[0] = dropped, info[1 + k] = S_k; scale[k] = class_scale(S_k)
__global__ void __launch_bounds__(kBlock) k_classes_fold(const double *__restrict__ part, int nblocks, double *__restrict__ info,
                                                         double *__restrict__ scale) {
    __shared__ double tmp[kClsSlices * kPartStride], tot[kPartStride];
    reduce_partials<kClsSlices, kClsMaxBlocks / kClsSlices>(part, nblocks, kClsInfo, tmp, tot);
    if (threadIdx.x < kNCls) {
        info[1 + threadIdx.x] = tot[threadIdx.x];
        scale[threadIdx.x] = class_scale(tot[threadIdx.x]);
    }
    if (threadIdx.x == kNCls) info[0] = tot[kNCls];
}

// the lane's run of samples in one bin -> the bin's slots (nothing for a zero)
__device__ __forceinline__ void classes_flush(long long *__restrict__ itab, int64_t bin, const int64_t (&run)[kNCls]) {
#pragma unroll
    for (int k = 0; k < kNCls; ++k)
        if (run[k] != 0)
            __hip_atomic_fetch_add(&itab[bin * kNCls + k], (long long)run[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// itab[(band (nb + 1) + class) NPG_NCLS + k] += llrint(term_k scale_k), zeroed before the launch
template <int NB, class Sampler>
__global__ void __launch_bounds__(kBlock) k_class_bin(FeDev d, const double *__restrict__ cy, const double *__restrict__ cz,
                                                      const uint8_t *__restrict__ mask, ClsRule r, Sampler sm,
                                                      const double *__restrict__ scale, long long *__restrict__ itab) {
    const CellsYZ<DevCells> cells{cell_view(d), cy, cz};
    double sc[kNCls];
#pragma unroll
    for (int k = 0; k < kNCls; ++k) sc[k] = scale[k];
    int64_t run[kNCls], cur = -1;
#pragma unroll
    for (int k = 0; k < kNCls; ++k) run[k] = 0;
    for (int64_t c = blockIdx.x * (int64_t)kBlock + threadIdx.x; c < d.ncell; c += (int64_t)gridDim.x * kBlock) {
        if (mask && !mask[c]) continue;
        typename Sampler::template Cell<NB> n;
        sm.template load<NB>(cells, c, n);
        for (int s = 0; s < r.ns; ++s) {
            double term[kNCls];
            int64_t band, cls;
            if (!sm.template sample<NB, true>(cells, n, r, s, c, &band, &cls, term)) continue;
            const int64_t bin = band * (r.nb + 1) + cls;             // band <= ny, cls <= nb: inside the table
            if (bin != cur) {
                if (cur >= 0) classes_flush(itab, cur, run);
                cur = bin;
#pragma unroll
                for (int k = 0; k < kNCls; ++k) run[k] = 0;
            }
#pragma unroll
            for (int k = 0; k < kNCls; ++k) run[k] += class_quantise(term[k], sc[k]);
        }
    }
    if (cur >= 0) classes_flush(itab, cur, run);
}

__global__ void __launch_bounds__(kBlock) k_classes_convert(const long long *__restrict__ itab, int64_t n, const double *__restrict__ scale,
                                                            double *__restrict__ out) {
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
        out[i] = (double)itab[i] / scale[i & (kNCls - 1)];
}

}  // namespace npg

using namespace npg;

struct npg_classes {
    npg_ctx *ctx = nullptr;
    npg_fe *fe = nullptr;
    DevBuf<double> cyz;          // [2][4][ncell]: y then z of the cells' own vertices
    DevBuf<uint8_t> mask;        // [ncell] or null
    DevBuf<double> rule;         // lam[ns][4], wq[ns], y_edges[ny], b_edges[nb], scale[NPG_NCLS]
    DevBuf<double> part;         // [nblocks][kPartStride]
    DevBuf<long long> itab;      // [(ny + 1)(nb + 1)][NPG_NCLS]
    int ns = 0, nblocks = 0;
    int64_t ny = 0, nb = 0, nbins = 0;
    // the diffusivities of npg_classes_mixing (npg_classes_set_diffusivity)
    DevBuf<double> kap;          // [2][ns][ncell]: kappa_h then kappa_v0 at the samples (a half is unused where the scalar holds)
    bool kap_set = false, kh_table = false, kv0_table = false;
    double kh_s = 0.0, kv0_s = 0.0;
};

NPG_API int npg_classes_destroy(npg_classes *K) {
    if (!K) return NPG_OK;
    hipStreamSynchronize(K->ctx->stream);
    delete K;
    return NPG_OK;
}

NPG_API int npg_classes_create(npg_fe *fe, const double *cell_y, const double *cell_z, const uint8_t *cell_mask, const double *rule_lam,
                               const double *rule_w, int ns, const double *y_edges, int64_t ny, const double *b_edges, int64_t nb,
                               npg_classes **out) {
    NPG_REQUIRE_OK(check_classes_create(fe && out, fe ? fe->d.ncell : 0, cell_y, cell_z, rule_lam, rule_w, ns, y_edges, ny, b_edges, nb));
    const int64_t nc = fe->d.ncell;
    std::vector<double> yz((size_t)nc * 8);
    for (int64_t c = 0; c < nc; ++c)
        for (int i = 0; i < 4; ++i) {
            yz[(size_t)i * nc + c] = cell_y[(size_t)c * 4 + i];
            yz[(size_t)(4 + i) * nc + c] = cell_z[(size_t)c * 4 + i];
        }
    NPG_HIP(hipSetDevice(fe->ctx->device));
    // the measure of a sample is w[s] wdet qsum, qsum from the engine's own weights
    std::vector<double> qw((size_t)fe->d.nq);
    NPG_HIP(hipMemcpy(qw.data(), fe->d.qw, qw.size() * sizeof(double), hipMemcpyDeviceToHost));
    double qsum = 0.0;
    for (double w : qw) qsum += w;
    std::vector<double> rule((size_t)ns * 5 + (size_t)ny + (size_t)nb + kNCls, 1.0);
    for (int s = 0; s < ns; ++s) {
        for (int i = 0; i < 4; ++i) rule[(size_t)4 * s + i] = rule_lam[4 * s + i];
        rule[(size_t)4 * ns + s] = rule_w[s] * qsum;
    }
    for (int64_t j = 0; j < ny; ++j) rule[(size_t)5 * ns + j] = y_edges[j];
    for (int64_t k = 0; k < nb; ++k) rule[(size_t)5 * ns + ny + k] = b_edges[k];
    std::unique_ptr<npg_classes> K(new npg_classes());
    K->ctx = fe->ctx;
    K->fe = fe;
    K->ns = ns, K->ny = ny, K->nb = nb, K->nbins = (ny + 1) * (nb + 1);
    K->nblocks = (int)std::min<int64_t>((nc + kBlock - 1) / kBlock, kClsMaxBlocks);
    NPG_HIP(K->cyz.upload(yz));
    if (cell_mask) NPG_HIP(K->mask.upload(cell_mask, (size_t)nc));
    NPG_HIP(K->rule.upload(rule));
    NPG_HIP(K->part.alloc((size_t)K->nblocks * kPartStride));
    NPG_HIP(K->itab.alloc((size_t)K->nbins * kNCls));
    *out = K.release();
    return NPG_OK;
}

// the two passes of a class table with the sampler sm: memset, scan, fold, bin, convert on the context's stream
template <class Sampler>
static int class_passes(npg_classes *K, const Sampler &sm, npg_vec *table, npg_vec *info) {
    npg_fe *fe = K->fe;
    NPG_HIP(hipSetDevice(fe->ctx->device));
    hipStream_t st = fe->ctx->stream;
    const FeDev &d = fe->d;
    const double *lam = K->rule, *wq = lam + (size_t)4 * K->ns, *ye = wq + K->ns, *be = ye + K->ny;
    double *scale = K->rule + (size_t)5 * K->ns + K->ny + K->nb;
    const ClsRule r{lam, wq, ye, be, K->ns, K->ny, K->nb};
    const double *cy = K->cyz, *cz = K->cyz + (size_t)4 * d.ncell;
    const int64_t nent = K->nbins * kNCls;
    const dim3 grid((unsigned)K->nblocks), block(kBlock);
    NPG_HIP(hipMemsetAsync(K->itab, 0, (size_t)nent * sizeof(long long), st));
    if (d.nb == 10) hipLaunchKernelGGL((k_class_scan<10, Sampler>), grid, block, 0, st, d, cy, cz, K->mask.p, r, sm, K->part.p);
    else hipLaunchKernelGGL((k_class_scan<4, Sampler>), grid, block, 0, st, d, cy, cz, K->mask.p, r, sm, K->part.p);
    NPG_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_classes_fold, dim3(1), block, 0, st, K->part.p, K->nblocks, info->d, scale);
    NPG_HIP(hipGetLastError());
    if (d.nb == 10) hipLaunchKernelGGL((k_class_bin<10, Sampler>), grid, block, 0, st, d, cy, cz, K->mask.p, r, sm, scale, K->itab.p);
    else hipLaunchKernelGGL((k_class_bin<4, Sampler>), grid, block, 0, st, d, cy, cz, K->mask.p, r, sm, scale, K->itab.p);
    NPG_HIP(hipGetLastError());
    const unsigned cgrid = (unsigned)std::min<int64_t>((nent + kBlock - 1) / kBlock, 4 * kNumCU);
    hipLaunchKernelGGL(k_classes_convert, dim3(cgrid), block, 0, st, K->itab.p, nent, scale, table->d);
    NPG_HIP(hipGetLastError());
    return NPG_OK;
}

NPG_API int npg_classes_compute(npg_classes *K, const npg_vec *x_inv, const npg_vec *b, double N2, npg_vec *table, npg_vec *info) {
    NPG_REQUIRE_OK(check_classes_compute(K, x_inv, b, N2, (const npg_vec *)table, (const npg_vec *)info));
    return class_passes(K, CensusSampler{x_inv->d, b->d, N2}, table, info);
}

NPG_API int npg_classes_set_diffusivity(npg_classes *K, const double *kappa_h, double kappa_h_scalar, const double *kappa_v0,
                                        double kappa_v0_scalar) {
    NPG_REQUIRE_OK(check_classes_set_diffusivity(K != nullptr, K ? K->fe->d.ncell * K->ns : 0, K ? K->ns : 1, kappa_h, kappa_h_scalar, kappa_v0,
                                                 kappa_v0_scalar));
    const int64_t nc = K->fe->d.ncell;
    const int ns = K->ns;
    NPG_HIP(hipSetDevice(K->ctx->device));
    NPG_HIP(hipStreamSynchronize(K->ctx->stream));               // a mixing call in flight still reads the tables it was given
    if ((kappa_h || kappa_v0) && !K->kap) NPG_HIP(K->kap.alloc((size_t)2 * ns * nc));
    const double *src[2] = {kappa_h, kappa_v0};
    std::vector<double> tr;
    for (int t = 0; t < 2; ++t) {
        if (!src[t]) continue;
        tr.resize((size_t)ns * nc);                              // [ncell][ns] -> [ns][ncell]
        for (int64_t c = 0; c < nc; ++c)
            for (int s = 0; s < ns; ++s) tr[(size_t)s * nc + c] = src[t][(size_t)c * ns + s];
        NPG_HIP(hipMemcpy(K->kap + (size_t)t * ns * nc, tr.data(), tr.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    K->kh_table = kappa_h != nullptr, K->kv0_table = kappa_v0 != nullptr;
    K->kh_s = kappa_h_scalar, K->kv0_s = kappa_v0_scalar;
    K->kap_set = true;
    return NPG_OK;
}

NPG_API int npg_classes_mixing(npg_classes *K, const npg_vec *b, double N2, double kappa_c, double N2min, double alpha, double N2c,
                               npg_vec *table, npg_vec *info) {
    const MixClosure cl{kappa_c, N2min, alpha, N2c};
    NPG_REQUIRE_OK(check_classes_mixing(K, b, N2, cl, (const npg_vec *)table, (const npg_vec *)info));
    const MixSampler sm{K->kh_table ? K->kap.p : nullptr, K->kv0_table ? K->kap + (size_t)K->ns * K->fe->d.ncell : nullptr, K->kh_s, K->kv0_s,
                        cl, b->d, N2};
    return class_passes(K, sm, table, info);
}
