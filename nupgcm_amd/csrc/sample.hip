// Point sampling of the device-resident state: nan_eval / plot_slice / plot_profiles of src/plotting.jl:9-90 and the 256^3
// resampling the reference's post-processing starts from (postprocess/utils.py:48-83).  Two kernels, one lane per point:
//   k_locate   bin of the point -> loop over the bin's candidate cells -> the cell with the largest min lambda (sample_core.h)
//   k_sample   closed-form P2 / P1 shape functions at the point's lambda, nodal values gathered through the DoF tables
// The points of a wave of a structured grid fall into the same or neighbouring bins, so the candidate records (one 128-byte
// line each, kGeoStride) are shared by most lanes and come from L2 / the vector cache; the DoF tables keep the engine's
// [component][cell] layout (a point's 10 - 30 indices are a gather either way).  No LDS, no scratch.
// The bins are built on the host when the locator is created (set-up cost; build_bins in sample_core.h, shared with the host
// library so that CPU() and GPU() locate identically).
#include "common.h"
#include "fe_dev.h"
#include "sample_core.h"

namespace npg {

__global__ void __launch_bounds__(kBlock) k_locate(BinGrid g, const int32_t *__restrict__ bin_ptr,
                                                   const int32_t *__restrict__ bin_cells, const double *__restrict__ geo,
                                                   const double *__restrict__ pts, int64_t n, int32_t *__restrict__ cell,
                                                   double *__restrict__ lam) {
    const int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    if (i >= n) return;
    const double p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    int32_t c;
    double l[4];
    locate_point(g, bin_ptr, bin_cells, geo, p, &c, l);
    cell[i] = c;
    lam[4 * i] = l[0], lam[4 * i + 1] = l[1], lam[4 * i + 2] = l[2], lam[4 * i + 3] = l[3];
}

// the engine's tables as sample_point reads them ([component][cell])
struct DevTables {
    const int32_t *cu_, *cp_, *cb_;
    const double *G_, *udiri, *bdiri;
    int64_t ncell;
    int nb;
    __device__ __forceinline__ int32_t cu(int l, int64_t c) const { return cu_[(size_t)l * ncell + c]; }
    __device__ __forceinline__ int32_t cp(int m, int64_t c) const { return cp_[(size_t)m * ncell + c]; }
    __device__ __forceinline__ int32_t cb(int i, int64_t c) const { return cb_[(size_t)i * ncell + c]; }
    __device__ __forceinline__ double G(int k, int64_t c) const { return G_[(size_t)k * ncell + c]; }
};

template <int FIELD, int NB>
__global__ void __launch_bounds__(kBlock) k_sample(DevTables t, const double *__restrict__ x, const int32_t *__restrict__ cell,
                                                   const double *__restrict__ lam, int64_t n, double *__restrict__ out) {
    constexpr int NC = FIELD == NPG_SAMPLE_U || FIELD == NPG_SAMPLE_GRAD_B ? 3 : 1;
    const int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    if (i >= n) return;
    const int32_t c = cell[i];
    double v[NC];
    if (c >= 0 && c < t.ncell) {             // cell ids may come from the caller (npg_located_upload)
        const double l[4] = {lam[4 * i], lam[4 * i + 1], lam[4 * i + 2], lam[4 * i + 3]};
        DevTables tn = t;
        tn.nb = NB;                          // a compile-time constant: the P2 / P1 branch folds away
        sample_point(tn, FIELD, x, c, l, v);
    } else {
#pragma unroll
        for (int a = 0; a < NC; ++a) v[a] = __builtin_nan("");
    }
#pragma unroll
    for (int a = 0; a < NC; ++a) out[NC * i + a] = v[a];
}

}  // namespace npg

using namespace npg;

struct npg_locator {
    npg_ctx *ctx = nullptr;
    int64_t ncell = 0;
    BinGrid grid{};
    int32_t *bin_ptr = nullptr, *bin_cells = nullptr;
    double *geo = nullptr;
    int64_t nentries = 0, max_per_bin = 0;
};

struct npg_located {
    npg_ctx *ctx = nullptr;
    int64_t n = 0;
    int32_t *cell = nullptr;     // [n]
    double *lam = nullptr;       // [n][4]
};

NPG_API int npg_locator_destroy(npg_locator *loc) {
    if (!loc) return NPG_OK;
    hipStreamSynchronize(loc->ctx->stream);
    hipFree(loc->bin_ptr);
    hipFree(loc->bin_cells);
    hipFree(loc->geo);
    delete loc;
    return NPG_OK;
}

NPG_API int npg_locator_create(npg_fe *fe, const double *anchor, int64_t nbins, npg_locator **out) {
    NPG_REQUIRE(fe && anchor && out, "npg_locator_create: NULL argument");
    NPG_REQUIRE(nbins >= 0 && nbins <= ((int64_t)1 << 26), "npg_locator_create: nbins must be 0 (automatic) .. 2^26");
    const int64_t nc = fe->d.ncell;
    NPG_HIP(hipSetDevice(fe->ctx->device));
    // grad_lambda back from the engine ([12][ncell]) -> [ncell][12]
    std::vector<double> Gt((size_t)nc * 12), G((size_t)nc * 12);
    NPG_HIP(hipStreamSynchronize(fe->ctx->stream));
    NPG_HIP(hipMemcpy(Gt.data(), fe->d.G, Gt.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int64_t c = 0; c < nc; ++c)
        for (int k = 0; k < 12; ++k) G[(size_t)c * 12 + k] = Gt[(size_t)k * nc + c];
    BinTables bt;
    const char *err = build_bins(G.data(), anchor, nc, nbins, bt);
    NPG_REQUIRE(!err, "%s", err);
    npg_locator *loc = new npg_locator();
    loc->ctx = fe->ctx;
    loc->ncell = nc;
    loc->grid = bt.grid;
    loc->nentries = (int64_t)bt.bin_cells.size();
    loc->max_per_bin = bt.max_per_bin;
    auto up = [&](void **dst, const void *src, size_t bytes) -> hipError_t {
        hipError_t e = hipMalloc(dst, std::max<size_t>(bytes, 8));
        if (e == hipSuccess && bytes) e = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
        return e;
    };
    hipError_t e = up((void **)&loc->bin_ptr, bt.bin_ptr.data(), bt.bin_ptr.size() * sizeof(int32_t));
    if (e == hipSuccess) e = up((void **)&loc->bin_cells, bt.bin_cells.data(), bt.bin_cells.size() * sizeof(int32_t));
    if (e == hipSuccess) e = up((void **)&loc->geo, bt.geo.data(), bt.geo.size() * sizeof(double));
    if (e != hipSuccess) {
        npg_locator_destroy(loc);
        NPG_HIP(e);
    }
    *out = loc;
    return NPG_OK;
}

NPG_API int npg_locator_info(const npg_locator *loc, int64_t *dims, double *box, int64_t *nentries, int64_t *max_per_bin) {
    NPG_REQUIRE(loc, "npg_locator_info: NULL handle");
    for (int a = 0; a < 3; ++a) {
        if (dims) dims[a] = loc->grid.nb[a];
        if (box) box[a] = loc->grid.lo[a], box[3 + a] = loc->grid.hi[a];
    }
    if (nentries) *nentries = loc->nentries;
    if (max_per_bin) *max_per_bin = loc->max_per_bin;
    return NPG_OK;
}

NPG_API int npg_located_destroy(npg_located *p) {
    if (!p) return NPG_OK;
    hipStreamSynchronize(p->ctx->stream);
    hipFree(p->cell);
    hipFree(p->lam);
    delete p;
    return NPG_OK;
}

NPG_API int npg_located_create(npg_ctx *ctx, int64_t n, npg_located **out) {
    NPG_REQUIRE(ctx && out && n >= 0, "npg_located_create: bad argument");
    NPG_REQUIRE(n <= ((int64_t)1 << 32), "npg_located_create: too many points for one launch (sample in chunks)");
    NPG_HIP(hipSetDevice(ctx->device));
    npg_located *p = new npg_located();
    p->ctx = ctx;
    p->n = n;
    hipError_t e = hipMalloc((void **)&p->cell, std::max<size_t>(1, (size_t)n) * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&p->lam, std::max<size_t>(1, (size_t)n) * 4 * sizeof(double));
    if (e != hipSuccess) {
        npg_located_destroy(p);
        NPG_HIP(e);
    }
    *out = p;
    return NPG_OK;
}

NPG_API int npg_located_upload(npg_located *p, const int32_t *cell, const double *lambda) {
    NPG_REQUIRE(p && (p->n == 0 || (cell && lambda)), "npg_located_upload: NULL argument");
    NPG_HIP(hipStreamSynchronize(p->ctx->stream));
    NPG_HIP(hipMemcpy(p->cell, cell, (size_t)p->n * sizeof(int32_t), hipMemcpyHostToDevice));
    NPG_HIP(hipMemcpy(p->lam, lambda, (size_t)p->n * 4 * sizeof(double), hipMemcpyHostToDevice));
    return NPG_OK;
}

NPG_API int npg_located_download(const npg_located *p, int32_t *cell, double *lambda) {
    NPG_REQUIRE(p, "npg_located_download: NULL handle");
    NPG_HIP(hipStreamSynchronize(p->ctx->stream));
    if (cell) NPG_HIP(hipMemcpy(cell, p->cell, (size_t)p->n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (lambda) NPG_HIP(hipMemcpy(lambda, p->lam, (size_t)p->n * 4 * sizeof(double), hipMemcpyDeviceToHost));
    return NPG_OK;
}

NPG_API int npg_locator_find(npg_locator *loc, const npg_vec *points, int64_t n, npg_located *out) {
    NPG_REQUIRE(loc && points && out, "npg_locator_find: NULL argument");
    NPG_REQUIRE(n >= 0 && points->n == 3 * n && out->n == n, "npg_locator_find: points must hold 3 n doubles and out n points");
    NPG_REQUIRE(points->ctx == loc->ctx && out->ctx == loc->ctx, "npg_locator_find: arguments of different contexts");
    if (n == 0) return NPG_OK;
    const int64_t grid = (n + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_locate, dim3((unsigned)grid), dim3(kBlock), 0, loc->ctx->stream, loc->grid, loc->bin_ptr,
                       loc->bin_cells, loc->geo, points->d, n, out->cell, out->lam);
    NPG_HIP(hipGetLastError());
    return NPG_OK;
}

NPG_API int npg_fe_sample(npg_fe *fe, int field, const npg_vec *vec, const npg_located *pts, npg_vec *out) {
    NPG_REQUIRE(fe && vec && pts && out, "npg_fe_sample: NULL argument");
    NPG_REQUIRE(field >= NPG_SAMPLE_U && field <= NPG_SAMPLE_GRAD_B, "npg_fe_sample: unknown field %d", field);
    const bool flow = field == NPG_SAMPLE_U || field == NPG_SAMPLE_P;
    NPG_REQUIRE(vec->n == (flow ? fe->n_inv : fe->n_b), "npg_fe_sample: the field's vector has %lld entries, expected %lld",
                (long long)vec->n, (long long)(flow ? fe->n_inv : fe->n_b));
    const int64_t n = pts->n;
    NPG_REQUIRE(out->n == n * sample_ncomp(field), "npg_fe_sample: out must hold %d values per point", sample_ncomp(field));
    NPG_REQUIRE(vec->ctx == fe->ctx && pts->ctx == fe->ctx && out->ctx == fe->ctx, "npg_fe_sample: arguments of different contexts");
    if (n == 0) return NPG_OK;
    const FeDev &d = fe->d;
    const DevTables t{d.cu, d.cp, d.cb, d.G, d.u_diri, d.b_diri, d.ncell, d.nb};
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
    hipStream_t st = fe->ctx->stream;
#define NPG_SAMPLE_LAUNCH(F, NB) \
    hipLaunchKernelGGL((k_sample<F, NB>), grid, block, 0, st, t, vec->d, pts->cell, pts->lam, n, out->d)
    if (field == NPG_SAMPLE_U) NPG_SAMPLE_LAUNCH(NPG_SAMPLE_U, 10);
    else if (field == NPG_SAMPLE_P) NPG_SAMPLE_LAUNCH(NPG_SAMPLE_P, 10);
    else if (field == NPG_SAMPLE_B && d.nb == 10) NPG_SAMPLE_LAUNCH(NPG_SAMPLE_B, 10);
    else if (field == NPG_SAMPLE_B) NPG_SAMPLE_LAUNCH(NPG_SAMPLE_B, 4);
    else if (d.nb == 10) NPG_SAMPLE_LAUNCH(NPG_SAMPLE_GRAD_B, 10);
    else NPG_SAMPLE_LAUNCH(NPG_SAMPLE_GRAD_B, 4);
#undef NPG_SAMPLE_LAUNCH
    NPG_HIP(hipGetLastError());
    return NPG_OK;
}
