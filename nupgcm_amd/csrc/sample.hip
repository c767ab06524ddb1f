// Point sampling of the device-resident state: nan_eval / plot_slice / plot_profiles of src/plotting.jl:9-90 and the 256^3
// resampling the reference's post-processing starts from (postprocess/utils.py:48-83).  Two kernels, one lane per point:
//   k_locate   bin of the point -> loop over the bin's candidate cells -> the cell with the largest min lambda (sample_core.h)
//   k_sample   closed-form P2 / P1 shape functions at the point's lambda, nodal values gathered through the DoF tables
// The points of a wave of a structured grid fall into the same or neighbouring bins, so the candidate records (one 128-byte
// line each, kGeoStride) are shared by most lanes and come from L2 / the vector cache; the DoF tables keep the engine's
// [component][cell] layout (a point's 10 - 30 indices are a gather either way).  No LDS, no scratch.
// The bins are built on the host when the locator is created (set-up cost; build_bins in sample_core.h, shared with the host
// library so that CPU() and GPU() locate identically).
//
// Integrals over a tensor grid (npg_fe_grid_integrals: the reductions postprocess/streamfunctions.py and stratification.py apply to
// the 256^3 grid) without the grid ever existing in memory:
//   k_grid_integrals   a workgroup owns one y index and kGridChunk consecutive x indices; its lanes run along z.  Per point:
//                      locate, evaluate u, b, dz b one after another, add to the lane's zonal accumulators (registers, over the
//                      x chunk) and to the column sums (wave_sum over z, then the 4 waves and the z tiles in a fixed order)
//   k_grid_fold        zonal line = the sum of its chunks' partials, in chunk order
// No atomics: every output element has one owner and one summation order.
#include "common.h"
#include "device_utils.h"
#include "fe_dev.h"
#include "sample_core.h"
#include "sample_dev.h"

namespace npg {

template <bool PART>
__global__ void __launch_bounds__(kBlock) k_locate(BinGrid g, const int32_t *__restrict__ bin_ptr,
                                                   const int32_t *__restrict__ bin_cells, const double *__restrict__ geo,
                                                   const double *__restrict__ pts, int64_t n, int32_t *__restrict__ cell,
                                                   double *__restrict__ lam) {
    const int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    if (i >= n) return;
    const double p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    int32_t c;
    double l[4];
    locate_point<PART>(g, bin_ptr, bin_cells, geo, p, &c, l);
    cell[i] = c;
    lam[4 * i] = l[0], lam[4 * i + 1] = l[1], lam[4 * i + 2] = l[2], lam[4 * i + 3] = l[3];
}

template <int FIELD, int NB>
__global__ void __launch_bounds__(kBlock) k_sample(DevCells t, const double *__restrict__ x, const int32_t *__restrict__ cell,
                                                   const double *__restrict__ lam, int64_t n, double *__restrict__ out) {
    constexpr int NC = FIELD == NPG_SAMPLE_U || FIELD == NPG_SAMPLE_GRAD_B ? 3 : 1;
    const int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    if (i >= n) return;
    const int32_t c = cell[i];
    double v[NC];
    if (c >= 0 && c < t.ncell) {             // cell ids may come from the caller (npg_located_upload)
        const double l[4] = {lam[4 * i], lam[4 * i + 1], lam[4 * i + 2], lam[4 * i + 3]};
        DevCells tn = t;
        tn.nb = NB;                          // a compile-time constant: the P2 / P1 branch folds away
        sample_point(tn, FIELD, x, c, l, v);
    } else {
#pragma unroll
        for (int a = 0; a < NC; ++a) v[a] = __builtin_nan("");
    }
#pragma unroll
    for (int a = 0; a < NC; ++a) out[NC * i + a] = v[a];
}

// One workgroup: y index j = blockIdx.x / nchunk, x indices [kGridChunk * cx, ...) with cx = blockIdx.x % nchunk; thread t works
// on z indices t, t + kBlock, ...  part[cx][channel][ny][nz], col[channel][nx][ny].
// PART: the locator of one rank of a partitioned mesh - a point whose winner another rank owns counts as outside here.
template <int NB, bool PART>
__global__ void __launch_bounds__(kBlock) k_grid_integrals(BinGrid g, const int32_t *__restrict__ bin_ptr,
                                                           const int32_t *__restrict__ bin_cells, const double *__restrict__ geo,
                                                           DevCells t, const double *__restrict__ xu, const double *__restrict__ xb,
                                                           double N2, const double *__restrict__ axes, int nx, int ny, int nz,
                                                           int nchunk, double *__restrict__ col, double *__restrict__ part) {
    constexpr int NW = kBlock / 64;
    __shared__ double sh[kGridChunk][NW][kGridCol];
    const int j = blockIdx.x / nchunk, cx = blockIdx.x % nchunk;
    const int i0 = cx * kGridChunk, i1 = min(nx, i0 + kGridChunk);
    const double *ax = axes, *az = axes + nx + ny;
    const double y = axes[nx + j];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ci = threadIdx.x / kGridCol, cch = threadIdx.x % kGridCol;      // the column sum this thread keeps across the z tiles
    const bool col_owner = ci < i1 - i0;
    double colacc = 0.0;
    t.nb = NB;                               // a compile-time constant: the P2 / P1 branch folds away
    for (int k0 = 0; k0 < nz; k0 += kBlock) {
        const int k = k0 + (int)threadIdx.x;
        const bool in = k < nz;
        const double z = in ? az[k] : 0.0;
        const double wz = in ? trapezoid_weight(az, nz, k) : 0.0;
        double acc[kGridZon];
#pragma unroll
        for (int a = 0; a < kGridZon; ++a) acc[a] = 0.0;
        for (int i = i0; i < i1; ++i) {
            const double p[3] = {ax[i], y, z};
            int32_t c = -1;
            double l[4] = {0.0, 0.0, 0.0, 0.0};
            if (in) locate_point<PART>(g, bin_ptr, bin_cells, geo, p, &c, l);
            double v[kGridVal], term[kGridCol];
            grid_point_values(t, xu, xb, N2, z, c, l, v);
            grid_zon_add(trapezoid_weight(ax, nx, i), v, acc);
            grid_col_terms(wz, v, term);
#pragma unroll
            for (int a = 0; a < kGridCol; ++a) {
                const double s = wave_sum(term[a]);
                if (lane == 0) sh[i - i0][wave][a] = s;
            }
        }
        if (in) {
#pragma unroll
            for (int a = 0; a < kGridZon; ++a) part[(((size_t)cx * kGridZon + a) * ny + j) * nz + k] = acc[a];
        }
        __syncthreads();
        if (col_owner) colacc += (sh[ci][0][cch] + sh[ci][1][cch]) + (sh[ci][2][cch] + sh[ci][3][cch]);
        __syncthreads();
    }
    if (col_owner) col[((size_t)cch * nx + i0 + ci) * ny + j] = colacc;
}

// Merging the ranks' point samples (npg_sample_mask / npg_sample_unmask): buf = [n][nc] values, then n counts.  Before the sum over
// ranks a point this rank does not report holds zeros and count 0; after it a point no rank reported (count 0) is NaN.
__global__ void __launch_bounds__(kBlock) k_sample_mask(const int32_t *__restrict__ cell, int64_t n, int nc, double *__restrict__ buf) {
    const int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    if (i >= n) return;
    const bool mine = cell[i] >= 0;
    if (!mine)
        for (int a = 0; a < nc; ++a) buf[nc * i + a] = 0.0;
    buf[(size_t)nc * n + i] = mine ? 1.0 : 0.0;
}

__global__ void __launch_bounds__(kBlock) k_sample_unmask(int64_t n, int nc, double *__restrict__ buf) {
    const int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    if (i >= n) return;
    if (buf[(size_t)nc * n + i] == 0.0)
        for (int a = 0; a < nc; ++a) buf[nc * i + a] = __builtin_nan("");
}

__global__ void __launch_bounds__(kBlock) k_grid_fold(const double *__restrict__ part, int nchunk, int64_t n, double *__restrict__ zon) {
    const int64_t e = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    if (e >= n) return;
    double s = 0.0;
    for (int cx = 0; cx < nchunk; ++cx) s += part[(size_t)cx * n + e];
    zon[e] = s;
}

}  // namespace npg

using namespace npg;

NPG_API int npg_locator_destroy(npg_locator *loc) {
    if (!loc) return NPG_OK;
    hipStreamSynchronize(loc->ctx->stream);
    hipFree(loc->bin_ptr);
    hipFree(loc->bin_cells);
    hipFree(loc->geo);
    hipFree(loc->grid_part);
    delete loc;
    return NPG_OK;
}

static int locator_upload(npg_locator *loc, const BinTables &bt, npg_locator **out);

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
    loc->ncell = loc->nrec = loc->nowned = nc;
    return locator_upload(loc, bt, out);
}

NPG_API int npg_locator_box(const double *grad_lambda, const double *anchor, int64_t ncell, double *box) {
    NPG_REQUIRE(grad_lambda && anchor && box && ncell >= 1, "npg_locator_box: bad argument");
    const char *err = mesh_box(grad_lambda, anchor, ncell, box);
    NPG_REQUIRE(!err, "%s", err);
    return NPG_OK;
}

NPG_API int npg_locator_create_cells(npg_ctx *ctx, const double *geo12, const int32_t *engine_cell, const int64_t *gid,
                                     const uint8_t *owned, int64_t ncell_loc, const double *box6, int64_t nbins, npg_locator **out) {
    NPG_REQUIRE(ctx && geo12 && engine_cell && gid && owned && box6 && out, "npg_locator_create_cells: NULL argument");
    NPG_REQUIRE(ncell_loc >= 1 && ncell_loc < INT32_MAX, "npg_locator_create_cells: 1 .. 2^31 - 2 cells");
    NPG_REQUIRE(nbins >= 0 && nbins <= ((int64_t)1 << 26), "npg_locator_create_cells: nbins must be 0 (automatic) .. 2^26");
    // records in ascending global id: the kernel's tie on the record index is then the tie on the global cell id
    std::vector<int64_t> order((size_t)ncell_loc);
    for (int64_t c = 0; c < ncell_loc; ++c) order[(size_t)c] = c;
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return gid[a] < gid[b]; });
    std::vector<double> geo((size_t)ncell_loc * 12);
    std::vector<int32_t> eng((size_t)ncell_loc);
    int64_t emax = -1, nowned = 0;
    for (int64_t k = 0; k < ncell_loc; ++k) {
        const int64_t c = order[(size_t)k];
        NPG_REQUIRE(k == 0 || gid[c] > gid[order[(size_t)k - 1]], "npg_locator_create_cells: global cell id %lld given twice", (long long)gid[c]);
        NPG_REQUIRE(engine_cell[c] >= -1, "npg_locator_create_cells: engine_cell must be an index or -1");
        NPG_REQUIRE(!owned[c] || engine_cell[c] >= 0, "npg_locator_create_cells: an owned cell needs its index in the engine");
        for (int j = 0; j < 12; ++j) geo[(size_t)k * 12 + j] = geo12[(size_t)c * 12 + j];
        eng[(size_t)k] = owned[c] ? engine_cell[c] : -1;      // `owned` folded into the sign: the kernels read one number
        if (owned[c]) emax = std::max<int64_t>(emax, engine_cell[c]), ++nowned;
    }
    NPG_HIP(hipSetDevice(ctx->device));
    BinTables bt;
    const char *err = build_bins_cells(geo.data(), eng.data(), ncell_loc, box6, nbins, bt);
    NPG_REQUIRE(!err, "%s", err);
    npg_locator *loc = new npg_locator();
    loc->ctx = ctx;
    loc->part = true;
    loc->ncell = emax + 1, loc->nrec = ncell_loc, loc->nowned = nowned;
    return locator_upload(loc, bt, out);
}

static int locator_upload(npg_locator *loc, const BinTables &bt, npg_locator **out) {
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
    if (loc->part)
        hipLaunchKernelGGL(k_locate<true>, dim3((unsigned)grid), dim3(kBlock), 0, loc->ctx->stream, loc->grid, loc->bin_ptr,
                           loc->bin_cells, loc->geo, points->d, n, out->cell, out->lam);
    else
        hipLaunchKernelGGL(k_locate<false>, dim3((unsigned)grid), dim3(kBlock), 0, loc->ctx->stream, loc->grid, loc->bin_ptr,
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
    const DevCells t = cell_view(d);
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

NPG_API int npg_fe_grid_integrals(npg_fe *fe, npg_locator *loc, const npg_vec *x_inv, const npg_vec *b, double N2, const npg_vec *axes,
                                  int64_t nx, int64_t ny, int64_t nz, npg_vec *col, npg_vec *zon) {
    NPG_REQUIRE(fe && loc && x_inv && b && axes && col && zon, "npg_fe_grid_integrals: NULL argument");
    NPG_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, "npg_fe_grid_integrals: every axis needs at least 2 points");
    NPG_REQUIRE(nx <= 65536 && ny <= 65536 && nz <= 65536, "npg_fe_grid_integrals: at most 65536 points per axis");
    NPG_REQUIRE(loc->ctx == fe->ctx && x_inv->ctx == fe->ctx && b->ctx == fe->ctx && axes->ctx == fe->ctx && col->ctx == fe->ctx &&
                    zon->ctx == fe->ctx, "npg_fe_grid_integrals: arguments of different contexts");
    NPG_REQUIRE(loc->part ? loc->ncell <= fe->d.ncell : loc->ncell == fe->d.ncell,
                "npg_fe_grid_integrals: the locator was built for another mesh");
    NPG_REQUIRE_OK(check_state_vectors("npg_fe_grid_integrals", fe->n_inv, fe->n_b, x_inv->n, b->n));
    NPG_REQUIRE(axes->n == nx + ny + nz, "npg_fe_grid_integrals: axes must hold nx + ny + nz doubles");
    NPG_REQUIRE(col->n == kGridCol * nx * ny && zon->n == kGridZon * ny * nz,
                "npg_fe_grid_integrals: col must hold %d nx ny and zon %d ny nz doubles", kGridCol, kGridZon);
    NPG_HIP(hipSetDevice(fe->ctx->device));
    hipStream_t st = fe->ctx->stream;
    // the axes are a few hundred doubles: checked on the host before anything is launched
    std::vector<double> h((size_t)(nx + ny + nz));
    NPG_HIP(hipMemcpyAsync(h.data(), axes->d, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    NPG_HIP(hipStreamSynchronize(st));
    const int64_t len[3] = {nx, ny, nz};
    const double *a = h.data();
    for (int d = 0; d < 3; a += len[d], ++d) {
        const char *err = check_axis(a, len[d]);
        NPG_REQUIRE(!err, "npg_fe_grid_integrals: %s (axis %c)", err, "xyz"[d]);
    }
    const int64_t nchunk = (nx + kGridChunk - 1) / kGridChunk, nzon = kGridZon * ny * nz;
    NPG_REQUIRE(ny * nchunk < ((int64_t)1 << 31), "npg_fe_grid_integrals: too many workgroups for one launch");
    const size_t need = (size_t)nchunk * (size_t)nzon;
    if (need > loc->grid_part_n) {
        NPG_HIP(hipFree(loc->grid_part));
        loc->grid_part = nullptr, loc->grid_part_n = 0;
        NPG_HIP(hipMalloc((void **)&loc->grid_part, need * sizeof(double)));
        loc->grid_part_n = need;
    }
    const FeDev &d = fe->d;
    const DevCells t = cell_view(d);
    const dim3 grid((unsigned)(ny * nchunk)), block(kBlock);
#define NPG_GRID_LAUNCH(NB, PART)                                                                                                \
    hipLaunchKernelGGL((k_grid_integrals<NB, PART>), grid, block, 0, st, loc->grid, loc->bin_ptr, loc->bin_cells, loc->geo, t,    \
                       x_inv->d, b->d, N2, axes->d, (int)nx, (int)ny, (int)nz, (int)nchunk, col->d, loc->grid_part)
    if (d.nb == 10 && !loc->part) NPG_GRID_LAUNCH(10, false);
    else if (!loc->part) NPG_GRID_LAUNCH(4, false);
    else if (d.nb == 10) NPG_GRID_LAUNCH(10, true);
    else NPG_GRID_LAUNCH(4, true);
#undef NPG_GRID_LAUNCH
    NPG_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_grid_fold, dim3((unsigned)((nzon + kBlock - 1) / kBlock)), block, 0, st, loc->grid_part, (int)nchunk, nzon,
                       zon->d);
    NPG_HIP(hipGetLastError());
    return NPG_OK;
}

NPG_API int npg_locator_cells(const npg_locator *loc, int64_t *nrecords, int64_t *nowned, int64_t *bytes) {
    NPG_REQUIRE(loc, "npg_locator_cells: NULL handle");
    if (nrecords) *nrecords = loc->nrec;
    if (nowned) *nowned = loc->nowned;
    if (bytes) {
        int64_t nbin = (int64_t)loc->grid.nb[0] * loc->grid.nb[1] * loc->grid.nb[2];
        *bytes = loc->nrec * kGeoStride * (int64_t)sizeof(double) + (nbin + 1 + loc->nentries) * (int64_t)sizeof(int32_t);
    }
    return NPG_OK;
}

NPG_API int npg_sample_mask(const npg_located *pts, int ncomp, npg_vec *buf) {
    NPG_REQUIRE(pts && buf && ncomp >= 0 && ncomp <= 3, "npg_sample_mask: bad argument");
    NPG_REQUIRE(buf->n == pts->n * (ncomp + 1) && buf->ctx == pts->ctx, "npg_sample_mask: buf must hold (ncomp + 1) n doubles");
    if (pts->n == 0) return NPG_OK;
    hipLaunchKernelGGL(k_sample_mask, dim3((unsigned)((pts->n + kBlock - 1) / kBlock)), dim3(kBlock), 0, pts->ctx->stream,
                       (const int32_t *)pts->cell, pts->n, ncomp, buf->d);
    NPG_HIP(hipGetLastError());
    return NPG_OK;
}

NPG_API int npg_sample_unmask(int64_t n, int ncomp, npg_vec *buf) {
    NPG_REQUIRE(buf && n >= 0 && n <= ((int64_t)1 << 32) && ncomp >= 0 && ncomp <= 3 && buf->n == n * (ncomp + 1),
                "npg_sample_unmask: buf must hold (ncomp + 1) n doubles");
    if (n == 0 || ncomp == 0) return NPG_OK;
    hipLaunchKernelGGL(k_sample_unmask, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, buf->ctx->stream, n, ncomp, buf->d);
    NPG_HIP(hipGetLastError());
    return NPG_OK;
}
