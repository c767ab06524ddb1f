// The device-resident state binned into (latitude band, buoyancy class) (npg_classes_compute): volume census, transports by class
// (the residual overturning), mean depth / buoyancy / stratification and the advective tendency of every class - the NPG_NCLS
// channels of classes_core.h.  The reference overlays isopycnals on a z-coordinate streamfunction and stops there.
//
// The destination of a term depends on the data, so there is no fixed summation order per output as in integrals.hip.  The same
// bits on every call come from ORDER-INDEPENDENT arithmetic instead: the terms are added as 64-bit integers.
//   k_classes_scan<NB>   pass 1, one lane per cell, grid-stride: S_c = sum |term_c| per channel over the counted samples and the
//                        number of dropped samples, in fp64, reduced exactly as k_cell_integrals does (block_store_partials; the
//                        grid is a function of ncell alone) - one partial row per workgroup
//   k_classes_fold       one workgroup adds the partial rows in the fixed order of reduce_partials, writes the info vector
//                        {dropped, S_c} and the channels' scales 2^(61 - e), frexp(S_c) = (m, e) (class_scale)
//   k_classes_bin<NB>    pass 2, the same loop: every term -> llrint(term scale_c) -> added as int64 to its bin's slot with a relaxed
//                        device-scope atomic on global memory.  A lane adds up a RUN of samples that share a bin in registers
//                        (the samples of a cell, and the lane's next cells, almost always do) and touches memory only when the bin
//                        changes; zeros are not sent.  Integer addition is associative: any arrival order gives the same table.
//   k_classes_convert    pass 3, integer table -> doubles (value / scale_c)
// sum |round(term scale)| < 2^61 + half a unit per sample: inside int64 for any mesh.  Quantisation: at most half a unit per
// sample, n_bin 2^-61 S_c per bin.  Always fp64 (npg_fe_set_precision does not apply).
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

// the engine's cell tables as class_cell_load reads them ([component][cell]); cy / cz = y / z of the cell's own vertices, [4][ncell]
struct ClsCells {
    FeDev d;
    const double *cy, *cz;
    __device__ __forceinline__ double G(int k, int64_t c) const { return d.G[(size_t)k * d.ncell + c]; }
    __device__ __forceinline__ double wdet(int64_t c) const { return d.wdet[c]; }
    __device__ __forceinline__ double y(int i, int64_t c) const { return cy[(size_t)i * d.ncell + c]; }
    __device__ __forceinline__ double z(int i, int64_t c) const { return cz[(size_t)i * d.ncell + c]; }
    __device__ __forceinline__ double u(const double *x, int l, int64_t c) const {
        return field_val(x, d.u_diri, d.cu[(size_t)l * d.ncell + c]);
    }
    __device__ __forceinline__ double b(const double *x, int i, int64_t c) const {
        return field_val(x, d.b_diri, d.cb[(size_t)i * d.ncell + c]);
    }
};

// the rule and the edges: lam[ns][4], wq[ns] = w[s] qsum, y_edges[ny], b_edges[nb]
struct ClsRule {
    const double *lam, *wq, *y_edges, *b_edges;
    int ns;
    int64_t ny, nb;
};

// part[blockIdx.x][kPartStride]: the workgroup's sums of |term| of the NPG_NCLS channels, then its dropped samples
template <int NB>
__global__ void __launch_bounds__(kBlock) k_classes_scan(FeDev d, const double *__restrict__ cy, const double *__restrict__ cz,
                                                         const uint8_t *__restrict__ mask, ClsRule r, const double *__restrict__ xu,
                                                         const double *__restrict__ xb, double N2, double *__restrict__ part) {
    __shared__ double sh[(kBlock / kWave) * kPartStride];
    const ClsCells cells{d, cy, cz};
    double acc[kClsInfo];
#pragma unroll
    for (int k = 0; k < kClsInfo; ++k) acc[k] = 0.0;
    for (int64_t c = blockIdx.x * (int64_t)kBlock + threadIdx.x; c < d.ncell; c += (int64_t)gridDim.x * kBlock) {
        if (mask && !mask[c]) continue;
        ClassCell<NB> n;
        class_cell_load<NB>(cells, xu, xb, c, n);
        for (int s = 0; s < r.ns; ++s) {
            double term[kNCls];
            int64_t band, cls;
            if (class_sample<NB, false>(n, r.lam + 4 * s, r.wq[s], N2, r.y_edges, r.ny, r.b_edges, r.nb, &band, &cls, term)) {
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
template <int NB>
__global__ void __launch_bounds__(kBlock) k_classes_bin(FeDev d, const double *__restrict__ cy, const double *__restrict__ cz,
                                                        const uint8_t *__restrict__ mask, ClsRule r, const double *__restrict__ xu,
                                                        const double *__restrict__ xb, double N2, const double *__restrict__ scale,
                                                        long long *__restrict__ itab) {
    const ClsCells cells{d, cy, cz};
    double sc[kNCls];
#pragma unroll
    for (int k = 0; k < kNCls; ++k) sc[k] = scale[k];
    int64_t run[kNCls], cur = -1;
#pragma unroll
    for (int k = 0; k < kNCls; ++k) run[k] = 0;
    for (int64_t c = blockIdx.x * (int64_t)kBlock + threadIdx.x; c < d.ncell; c += (int64_t)gridDim.x * kBlock) {
        if (mask && !mask[c]) continue;
        ClassCell<NB> n;
        class_cell_load<NB>(cells, xu, xb, c, n);
        for (int s = 0; s < r.ns; ++s) {
            double term[kNCls];
            int64_t band, cls;
            if (!class_sample<NB, true>(n, r.lam + 4 * s, r.wq[s], N2, r.y_edges, r.ny, r.b_edges, r.nb, &band, &cls, term)) continue;
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

// ---- water-mass transformation by mixing (npg_classes_mixing, mixing_core.h): the same two passes over the same grid with the
// NPG_NMIX diffusivity-weighted channels.  No velocity is gathered; the diffusivities of a sample come from the tables
// kap_h / kap_v0 [ns][ncell] (coalesced across the lanes of a wave) or, where a table is null, from the scalar.  k_classes_fold,
// k_classes_convert, the partial rows, the scales and the integer table are the census's (NPG_NMIX == NPG_NCLS). --------------------
struct MixCoef {
    const double *kh, *kv0;      // [ns][ncell] or null: the scalar holds everywhere
    double kh_s, kv0_s;
    MixClosure cl;
    __device__ __forceinline__ double h(int s, int64_t c, int64_t ncell) const { return kh ? kh[(size_t)s * ncell + c] : kh_s; }
    __device__ __forceinline__ double v0(int s, int64_t c, int64_t ncell) const { return kv0 ? kv0[(size_t)s * ncell + c] : kv0_s; }
};

template <int NB>
__global__ void __launch_bounds__(kBlock) k_mixing_scan(FeDev d, const double *__restrict__ cy, const double *__restrict__ cz,
                                                        const uint8_t *__restrict__ mask, ClsRule r, MixCoef k,
                                                        const double *__restrict__ xb, double N2, double *__restrict__ part) {
    __shared__ double sh[(kBlock / kWave) * kPartStride];
    const ClsCells cells{d, cy, cz};
    double acc[kClsInfo];
#pragma unroll
    for (int a = 0; a < kClsInfo; ++a) acc[a] = 0.0;
    for (int64_t c = blockIdx.x * (int64_t)kBlock + threadIdx.x; c < d.ncell; c += (int64_t)gridDim.x * kBlock) {
        if (mask && !mask[c]) continue;
        MixCell<NB> n;
        mix_cell_load<NB>(cells, xb, c, n);
        for (int s = 0; s < r.ns; ++s) {
            double term[kNMix];
            int64_t band, cls;
            if (mix_sample<NB, false>(n, r.lam + 4 * s, r.wq[s], N2, k.h(s, c, d.ncell), k.v0(s, c, d.ncell), k.cl, r.y_edges, r.ny,
                                      r.b_edges, r.nb, &band, &cls, term)) {
#pragma unroll
                for (int a = 0; a < kNMix; ++a) acc[a] += fabs(term[a]);
            } else {
                acc[kNMix] += 1.0;
            }
        }
    }
    block_store_partials<kClsInfo, kBlock / kWave>(acc, kClsInfo, sh, part);
}

template <int NB>
__global__ void __launch_bounds__(kBlock) k_mixing_bin(FeDev d, const double *__restrict__ cy, const double *__restrict__ cz,
                                                       const uint8_t *__restrict__ mask, ClsRule r, MixCoef k,
                                                       const double *__restrict__ xb, double N2, const double *__restrict__ scale,
                                                       long long *__restrict__ itab) {
    const ClsCells cells{d, cy, cz};
    double sc[kNMix];
#pragma unroll
    for (int a = 0; a < kNMix; ++a) sc[a] = scale[a];
    int64_t run[kNMix], cur = -1;
#pragma unroll
    for (int a = 0; a < kNMix; ++a) run[a] = 0;
    for (int64_t c = blockIdx.x * (int64_t)kBlock + threadIdx.x; c < d.ncell; c += (int64_t)gridDim.x * kBlock) {
        if (mask && !mask[c]) continue;
        MixCell<NB> n;
        mix_cell_load<NB>(cells, xb, c, n);
        for (int s = 0; s < r.ns; ++s) {
            double term[kNMix];
            int64_t band, cls;
            if (!mix_sample<NB, true>(n, r.lam + 4 * s, r.wq[s], N2, k.h(s, c, d.ncell), k.v0(s, c, d.ncell), k.cl, r.y_edges, r.ny,
                                      r.b_edges, r.nb, &band, &cls, term))
                continue;
            const int64_t bin = band * (r.nb + 1) + cls;             // band <= ny, cls <= nb: inside the table
            if (bin != cur) {
                if (cur >= 0) classes_flush(itab, cur, run);
                cur = bin;
#pragma unroll
                for (int a = 0; a < kNMix; ++a) run[a] = 0;
            }
#pragma unroll
            for (int a = 0; a < kNMix; ++a) run[a] += class_quantise(term[a], sc[a]);
        }
    }
    if (cur >= 0) classes_flush(itab, cur, run);
}

}  // namespace npg

using namespace npg;

struct npg_classes {
    npg_ctx *ctx = nullptr;
    npg_fe *fe = nullptr;
    double *cyz = nullptr;       // [2][4][ncell]: y then z of the cells' own vertices
    uint8_t *mask = nullptr;     // [ncell] or null
    double *rule = nullptr;      // lam[ns][4], wq[ns], y_edges[ny], b_edges[nb], scale[NPG_NCLS]
    double *part = nullptr;      // [nblocks][kPartStride]
    long long *itab = nullptr;   // [(ny + 1)(nb + 1)][NPG_NCLS]
    int ns = 0, nblocks = 0;
    int64_t ny = 0, nb = 0, nbins = 0;
    // the diffusivities of npg_classes_mixing (npg_classes_set_diffusivity)
    double *kap = nullptr;       // [2][ns][ncell]: kappa_h then kappa_v0 at the samples (a half is unused where the scalar holds)
    bool kap_set = false, kh_table = false, kv0_table = false;
    double kh_s = 0.0, kv0_s = 0.0;
};

NPG_API int npg_classes_destroy(npg_classes *K) {
    if (!K) return NPG_OK;
    hipStreamSynchronize(K->ctx->stream);
    hipFree(K->cyz);
    hipFree(K->mask);
    hipFree(K->rule);
    hipFree(K->part);
    hipFree(K->itab);
    hipFree(K->kap);
    delete K;
    return NPG_OK;
}

NPG_API int npg_classes_create(npg_fe *fe, const double *cell_y, const double *cell_z, const uint8_t *cell_mask, const double *rule_lam,
                               const double *rule_w, int ns, const double *y_edges, int64_t ny, const double *b_edges, int64_t nb,
                               npg_classes **out) {
    NPG_REQUIRE(fe && out, "npg_classes_create: NULL argument");
    NPG_REQUIRE(cell_y && cell_z, "npg_classes_create: cell_y or cell_z is NULL");
    NPG_REQUIRE(ns >= 1 && ns <= kClsMaxSamples, "npg_classes_create: 1 .. %d samples per cell, got %d", kClsMaxSamples, ns);
    NPG_REQUIRE(rule_lam && rule_w, "npg_classes_create: rule_lam or rule_w is NULL");
    NPG_REQUIRE(ny >= 0 && nb >= 0 && (ny == 0 || y_edges) && (nb == 0 || b_edges), "npg_classes_create: edges missing or a negative count");
    NPG_REQUIRE(ny < kClsMaxBins && nb < kClsMaxBins && (ny + 1) * (nb + 1) <= kClsMaxBins,
                "npg_classes_create: ny = %lld and nb = %lld give more than 2^22 bins (ny + 1)(nb + 1)", (long long)ny, (long long)nb);
    const char *err = check_edges(y_edges, ny);
    NPG_REQUIRE(!err, "npg_classes_create: y_edges %s", err);
    err = check_edges(b_edges, nb);
    NPG_REQUIRE(!err, "npg_classes_create: b_edges %s", err);
    double wsum = 0.0;
    for (int s = 0; s < ns; ++s) {
        NPG_REQUIRE(rule_w[s] > 0.0 && std::isfinite(rule_w[s]), "npg_classes_create: weight %d of the rule is not > 0", s);
        wsum += rule_w[s];
        const double *l = rule_lam + 4 * s;
        NPG_REQUIRE(std::fabs((l[0] + l[1]) + (l[2] + l[3]) - 1.0) <= 1e-12, "npg_classes_create: lam row %d of the rule does not sum to 1", s);
    }
    NPG_REQUIRE(std::fabs(wsum - 1.0) <= 1e-12, "npg_classes_create: the weights of the rule sum to %.17g, not 1", wsum);
    const int64_t nc = fe->d.ncell;
    std::vector<double> yz((size_t)nc * 8);
    for (int64_t c = 0; c < nc; ++c)
        for (int i = 0; i < 4; ++i) {
            const double y = cell_y[(size_t)c * 4 + i], z = cell_z[(size_t)c * 4 + i];
            NPG_REQUIRE(std::isfinite(y), "npg_classes_create: cell_y[%lld][%d] is not finite", (long long)c, i);
            NPG_REQUIRE(std::isfinite(z), "npg_classes_create: cell_z[%lld][%d] is not finite", (long long)c, i);
            yz[(size_t)i * nc + c] = y;
            yz[(size_t)(4 + i) * nc + c] = z;
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
    npg_classes *K = new npg_classes();
    K->ctx = fe->ctx;
    K->fe = fe;
    K->ns = ns, K->ny = ny, K->nb = nb, K->nbins = (ny + 1) * (nb + 1);
    K->nblocks = (int)std::min<int64_t>((nc + kBlock - 1) / kBlock, kClsMaxBlocks);
    hipError_t e = hipMalloc((void **)&K->cyz, yz.size() * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(K->cyz, yz.data(), yz.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess && cell_mask) {
        e = hipMalloc((void **)&K->mask, (size_t)nc);
        if (e == hipSuccess) e = hipMemcpy(K->mask, cell_mask, (size_t)nc, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipMalloc((void **)&K->rule, rule.size() * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(K->rule, rule.data(), rule.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void **)&K->part, (size_t)K->nblocks * kPartStride * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&K->itab, (size_t)K->nbins * kNCls * sizeof(long long));
    if (e != hipSuccess) {
        npg_classes_destroy(K);
        NPG_HIP(e);
    }
    *out = K;
    return NPG_OK;
}

NPG_API int npg_classes_compute(npg_classes *K, const npg_vec *x_inv, const npg_vec *b, double N2, npg_vec *table, npg_vec *info) {
    NPG_REQUIRE(K && x_inv && b && table && info, "npg_classes_compute: NULL argument");
    npg_fe *fe = K->fe;
    NPG_REQUIRE(x_inv->n == fe->n_inv, "npg_classes_compute: the flow vector has %lld entries, expected %lld", (long long)x_inv->n,
                (long long)fe->n_inv);
    NPG_REQUIRE(b->n == fe->n_b, "npg_classes_compute: the buoyancy vector has %lld entries, expected %lld", (long long)b->n,
                (long long)fe->n_b);
    NPG_REQUIRE(table->n >= K->nbins * NPG_NCLS, "npg_classes_compute: table holds %lld doubles, needs (ny + 1)(nb + 1) NPG_NCLS = %lld",
                (long long)table->n, (long long)(K->nbins * NPG_NCLS));
    NPG_REQUIRE(info->n >= 1 + NPG_NCLS, "npg_classes_compute: info holds %lld doubles, needs 1 + NPG_NCLS = %d", (long long)info->n,
                1 + NPG_NCLS);
    NPG_REQUIRE(std::isfinite(N2), "npg_classes_compute: N2 is not finite");
    NPG_REQUIRE(x_inv->ctx == fe->ctx && b->ctx == fe->ctx && table->ctx == fe->ctx && info->ctx == fe->ctx,
                "npg_classes_compute: arguments of different contexts");
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
    if (d.nb == 10)
        hipLaunchKernelGGL(k_classes_scan<10>, grid, block, 0, st, d, cy, cz, K->mask, r, x_inv->d, b->d, N2, K->part);
    else
        hipLaunchKernelGGL(k_classes_scan<4>, grid, block, 0, st, d, cy, cz, K->mask, r, x_inv->d, b->d, N2, K->part);
    NPG_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_classes_fold, dim3(1), block, 0, st, K->part, K->nblocks, info->d, scale);
    NPG_HIP(hipGetLastError());
    if (d.nb == 10)
        hipLaunchKernelGGL(k_classes_bin<10>, grid, block, 0, st, d, cy, cz, K->mask, r, x_inv->d, b->d, N2, scale, K->itab);
    else
        hipLaunchKernelGGL(k_classes_bin<4>, grid, block, 0, st, d, cy, cz, K->mask, r, x_inv->d, b->d, N2, scale, K->itab);
    NPG_HIP(hipGetLastError());
    const unsigned cgrid = (unsigned)std::min<int64_t>((nent + kBlock - 1) / kBlock, 4 * kNumCU);
    hipLaunchKernelGGL(k_classes_convert, dim3(cgrid), block, 0, st, K->itab, nent, scale, table->d);
    NPG_HIP(hipGetLastError());
    return NPG_OK;
}

NPG_API int npg_classes_set_diffusivity(npg_classes *K, const double *kappa_h, double kappa_h_scalar, const double *kappa_v0,
                                        double kappa_v0_scalar) {
    NPG_REQUIRE(K, "npg_classes_set_diffusivity: NULL argument");
    const int64_t nc = K->fe->d.ncell;
    const int ns = K->ns;
    const char *err = kappa_h ? nullptr : check_diffusivity(kappa_h_scalar);
    NPG_REQUIRE(!err, "npg_classes_set_diffusivity: the scalar kappa_h %s, got %.17g", err, kappa_h_scalar);
    err = kappa_v0 ? nullptr : check_diffusivity(kappa_v0_scalar);
    NPG_REQUIRE(!err, "npg_classes_set_diffusivity: the scalar kappa_v0 %s, got %.17g", err, kappa_v0_scalar);
    const double *src[2] = {kappa_h, kappa_v0};
    for (int t = 0; t < 2; ++t)
        for (int64_t i = 0; src[t] && i < nc * ns; ++i)
            NPG_REQUIRE(!check_diffusivity(src[t][i]), "npg_classes_set_diffusivity: %s[%lld][%d] must be finite and >= 0, got %.17g",
                        t ? "kappa_v0" : "kappa_h", (long long)(i / ns), (int)(i % ns), src[t][i]);
    NPG_HIP(hipSetDevice(K->ctx->device));
    NPG_HIP(hipStreamSynchronize(K->ctx->stream));               // a mixing call in flight still reads the tables it was given
    if ((kappa_h || kappa_v0) && !K->kap) NPG_HIP(hipMalloc((void **)&K->kap, (size_t)2 * ns * nc * sizeof(double)));
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
    NPG_REQUIRE(K && b && table && info, "npg_classes_mixing: NULL argument");
    NPG_REQUIRE(K->kap_set, "npg_classes_mixing: no diffusivities: call npg_classes_set_diffusivity first");
    npg_fe *fe = K->fe;
    NPG_REQUIRE(b->n == fe->n_b, "npg_classes_mixing: the buoyancy vector has %lld entries, expected %lld", (long long)b->n,
                (long long)fe->n_b);
    NPG_REQUIRE(table->n >= K->nbins * NPG_NMIX, "npg_classes_mixing: table holds %lld doubles, needs (ny + 1)(nb + 1) NPG_NMIX = %lld",
                (long long)table->n, (long long)(K->nbins * NPG_NMIX));
    NPG_REQUIRE(info->n >= 1 + NPG_NMIX, "npg_classes_mixing: info holds %lld doubles, needs 1 + NPG_NMIX = %d", (long long)info->n,
                1 + NPG_NMIX);
    NPG_REQUIRE(!check_diffusivity(N2), "npg_classes_mixing: N2 must be finite and >= 0, got %.17g", N2);
    NPG_REQUIRE(!check_diffusivity(kappa_c), "npg_classes_mixing: kappa_c must be finite and >= 0, got %.17g", kappa_c);
    NPG_REQUIRE(!check_diffusivity(alpha), "npg_classes_mixing: alpha must be finite and >= 0, got %.17g", alpha);
    NPG_REQUIRE(!check_diffusivity(N2c), "npg_classes_mixing: N2c must be finite and >= 0, got %.17g", N2c);
    NPG_REQUIRE(!(kappa_c > 0.0) || N2min > 0.0, "npg_classes_mixing: kappa_c > 0 needs N2min > 0, got %.17g", N2min);
    NPG_REQUIRE(b->ctx == fe->ctx && table->ctx == fe->ctx && info->ctx == fe->ctx, "npg_classes_mixing: arguments of different contexts");
    NPG_HIP(hipSetDevice(fe->ctx->device));
    hipStream_t st = fe->ctx->stream;
    const FeDev &d = fe->d;
    const double *lam = K->rule, *wq = lam + (size_t)4 * K->ns, *ye = wq + K->ns, *be = ye + K->ny;
    double *scale = K->rule + (size_t)5 * K->ns + K->ny + K->nb;
    const ClsRule r{lam, wq, ye, be, K->ns, K->ny, K->nb};
    const MixCoef k{K->kh_table ? K->kap : nullptr, K->kv0_table ? K->kap + (size_t)K->ns * d.ncell : nullptr, K->kh_s, K->kv0_s,
                    MixClosure{kappa_c, N2min, alpha, N2c}};
    const double *cy = K->cyz, *cz = K->cyz + (size_t)4 * d.ncell;
    const int64_t nent = K->nbins * kNMix;
    const dim3 grid((unsigned)K->nblocks), block(kBlock);
    NPG_HIP(hipMemsetAsync(K->itab, 0, (size_t)nent * sizeof(long long), st));
    if (d.nb == 10) hipLaunchKernelGGL(k_mixing_scan<10>, grid, block, 0, st, d, cy, cz, K->mask, r, k, b->d, N2, K->part);
    else hipLaunchKernelGGL(k_mixing_scan<4>, grid, block, 0, st, d, cy, cz, K->mask, r, k, b->d, N2, K->part);
    NPG_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_classes_fold, dim3(1), block, 0, st, K->part, K->nblocks, info->d, scale);
    NPG_HIP(hipGetLastError());
    if (d.nb == 10) hipLaunchKernelGGL(k_mixing_bin<10>, grid, block, 0, st, d, cy, cz, K->mask, r, k, b->d, N2, scale, K->itab);
    else hipLaunchKernelGGL(k_mixing_bin<4>, grid, block, 0, st, d, cy, cz, K->mask, r, k, b->d, N2, scale, K->itab);
    NPG_HIP(hipGetLastError());
    const unsigned cgrid = (unsigned)std::min<int64_t>((nent + kBlock - 1) / kBlock, 4 * kNumCU);
    hipLaunchKernelGGL(k_classes_convert, dim3(cgrid), block, 0, st, K->itab, nent, scale, table->d);
    NPG_HIP(hipGetLastError());
    return NPG_OK;
}
