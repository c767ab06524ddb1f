// Maps on buoyancy surfaces (npg_surfaces_compute): where the surfaces B = B_k lie over fixed columns, how thick the
// layers between them are and what the flow is on them, answered while the state is still in HBM.
//   k_surfaces_scan<NB>   one lane per column (surfaces_core.h: column_surfaces).  The lane walks its column's segments top to bottom,
//                         loads a cell's NB buoyancy values once, carries the value at the shared face into the next segment and
//                         writes every crossing straight to out[9][nlev][ncol] - column-fastest, so the stores of a wave coalesce.
//                         NB = 10 (P2: a quadratic per segment) or 4 (P1: linear, no midpoint).  It reads b' alone.
//   k_surfaces_fields     one lane per (level, column): where the scan met a crossing, u and grad B at the uppermost one, in the cell the
//                         scan met it in (kept in cross_cell[nlev][ncol]).  The 40 gathers of a velocity and a gradient stay out of
//                         the scan's loop, and run nlev times as wide.
// No LDS, no atomics, no per-level state in registers: a column is one lane's own, so the result does not depend on the order or the
// number of columns.  Always fp64 (npg_fe_set_precision does not apply).
#include <cmath>
#include <cstring>

#include "common.h"
#include "fe_dev.h"
#include "sample_dev.h"
#include "surfaces_core.h"

static_assert(NPG_NSURF == npg::kNSurf, "NPG_NSURF of the header and kNSurf of surfaces_core.h must agree");

namespace npg {

template <int NB>
__global__ void __launch_bounds__(kBlock) k_surfaces_scan(SurfaceColumns S, DevCells t, const double *__restrict__ xb, double N2,
                                                          const double *__restrict__ levels, int nlev, double *out,
                                                          int32_t *__restrict__ cross_cell, double *__restrict__ cols) {
    const int64_t j = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    if (j >= S.ncol) return;
    column_surfaces<NB>(S, t, xb, N2, levels, nlev, j, out, cross_cell, cols);
}

__global__ void __launch_bounds__(kBlock) k_surfaces_fields(SurfaceColumns S, DevCells t, const double *__restrict__ xu,
                                                            const double *__restrict__ xb, double N2, int nlev,
                                                            const int32_t *__restrict__ cross_cell, double *out) {
    const int64_t o = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    if (o >= (int64_t)nlev * S.ncol) return;
    surface_fields(S, t, xu, xb, N2, nlev, o, cross_cell, out);
}

}  // namespace npg

using namespace npg;

struct npg_surfaces {
    npg_ctx *ctx = nullptr;
    npg_fe *fe = nullptr;
    int64_t ncol = 0, nseg = 0, max_per_col = 0, ndry = 0;
    std::vector<int64_t> h_col_ptr;      // kept for npg_surfaces_columns
    std::vector<double> h_ztop, h_zbot;  // per column, NaN where dry
    DevBuf<int64_t> col_ptr;
    DevBuf<int32_t> seg_cell;
    DevBuf<double> seg_ztop, seg_zbot, xy;
    const double *geo = nullptr;         // the locator's records (not owned: the locator outlives the handle)
    DevBuf<double> levels;               // the levels of the last call, uploaded again only when they change
    DevBuf<int32_t> cross_cell;          // [nlev][ncol] the cell of the uppermost crossing, grown on demand
    size_t cross_n = 0;
    std::vector<double> h_levels;
};

NPG_API int npg_surfaces_destroy(npg_surfaces *S) {
    if (!S) return NPG_OK;
    hipStreamSynchronize(S->ctx->stream);
    delete S;
    return NPG_OK;
}

NPG_API int npg_surfaces_create(npg_fe *fe, npg_locator *loc, const double *xy, int64_t ncol, npg_surfaces **out) {
    NPG_REQUIRE(fe && loc && out && (xy || ncol == 0), "npg_surfaces_create: NULL argument");
    NPG_REQUIRE(ncol >= 0 && ncol <= ((int64_t)1 << 30), "npg_surfaces_create: 0 .. 2^30 columns, got %lld", (long long)ncol);
    NPG_REQUIRE(loc->ctx == fe->ctx, "npg_surfaces_create: arguments of different contexts");
    NPG_REQUIRE(!loc->part, "npg_surfaces_create: a partitioned locator (npg_locator_create_cells) is refused - a column runs through "
                "the cells of several ranks, and stitching its pieces together is not implemented");
    NPG_REQUIRE(loc->ncell == fe->d.ncell, "npg_surfaces_create: the locator was built for another mesh (an embedded 2-D engine has no "
                "locator: buoyancy surfaces need a tetrahedral mesh)");
    NPG_HIP(hipSetDevice(fe->ctx->device));
    NPG_HIP(hipStreamSynchronize(fe->ctx->stream));
    const int64_t ncell = loc->ncell;
    std::vector<double> geo((size_t)ncell * kGeoStride);
    NPG_HIP(hipMemcpy(geo.data(), loc->geo, geo.size() * sizeof(double), hipMemcpyDeviceToHost));
    ColumnTables ct;
    const char *err = build_columns(geo.data(), ncell, loc->grid.lo[2], loc->grid.hi[2], xy, ncol, ct);
    NPG_REQUIRE(!err, "%s", err);
    std::unique_ptr<npg_surfaces> S(new npg_surfaces());
    S->ctx = fe->ctx, S->fe = fe, S->geo = loc->geo;
    S->ncol = ncol, S->nseg = ct.col_ptr[(size_t)ncol], S->max_per_col = ct.max_per_col, S->ndry = ct.ndry;
    S->h_col_ptr = ct.col_ptr;
    S->h_ztop.assign((size_t)ncol, NAN), S->h_zbot.assign((size_t)ncol, NAN);
    for (int64_t j = 0; j < ncol; ++j)
        if (ct.col_ptr[(size_t)j + 1] > ct.col_ptr[(size_t)j])
            S->h_ztop[(size_t)j] = ct.seg_ztop[(size_t)ct.col_ptr[(size_t)j]], S->h_zbot[(size_t)j] = ct.seg_zbot[(size_t)ct.col_ptr[(size_t)j + 1] - 1];
    const size_t ns = std::max<size_t>(1, (size_t)S->nseg), nc = std::max<size_t>(1, (size_t)ncol);
    NPG_HIP(S->col_ptr.upload(ct.col_ptr));
    NPG_HIP(S->seg_cell.alloc(ns));                  // at least one entry each: never a null table in a kernel's arguments
    NPG_HIP(S->seg_ztop.alloc(ns));
    NPG_HIP(S->seg_zbot.alloc(ns));
    NPG_HIP(S->xy.alloc(nc * 2));
    if (S->nseg) {
        NPG_HIP(hipMemcpy(S->seg_cell, ct.seg_cell.data(), (size_t)S->nseg * sizeof(int32_t), hipMemcpyHostToDevice));
        NPG_HIP(hipMemcpy(S->seg_ztop, ct.seg_ztop.data(), (size_t)S->nseg * sizeof(double), hipMemcpyHostToDevice));
        NPG_HIP(hipMemcpy(S->seg_zbot, ct.seg_zbot.data(), (size_t)S->nseg * sizeof(double), hipMemcpyHostToDevice));
    }
    if (ncol) NPG_HIP(hipMemcpy(S->xy, xy, (size_t)ncol * 2 * sizeof(double), hipMemcpyHostToDevice));
    *out = S.release();
    return NPG_OK;
}

NPG_API int npg_surfaces_info(const npg_surfaces *S, int64_t *nseg, int64_t *max_per_col, int64_t *ndry) {
    NPG_REQUIRE(S, "npg_surfaces_info: NULL handle");
    if (nseg) *nseg = S->nseg;
    if (max_per_col) *max_per_col = S->max_per_col;
    if (ndry) *ndry = S->ndry;
    return NPG_OK;
}

NPG_API int npg_surfaces_columns(const npg_surfaces *S, double *z_top, double *z_bot, int32_t *nseg) {
    NPG_REQUIRE(S, "npg_surfaces_columns: NULL handle");
    for (int64_t j = 0; j < S->ncol; ++j) {
        if (z_top) z_top[j] = S->h_ztop[(size_t)j];
        if (z_bot) z_bot[j] = S->h_zbot[(size_t)j];
        if (nseg) nseg[j] = (int32_t)(S->h_col_ptr[(size_t)j + 1] - S->h_col_ptr[(size_t)j]);
    }
    return NPG_OK;
}

NPG_API int npg_surfaces_segments(const npg_surfaces *S, int32_t *cell, double *z_top, double *z_bot) {
    NPG_REQUIRE(S, "npg_surfaces_segments: NULL handle");
    if (S->nseg == 0) return NPG_OK;
    NPG_HIP(hipSetDevice(S->ctx->device));
    const size_t n = (size_t)S->nseg;
    if (cell) NPG_HIP(hipMemcpy(cell, S->seg_cell, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (z_top) NPG_HIP(hipMemcpy(z_top, S->seg_ztop, n * sizeof(double), hipMemcpyDeviceToHost));
    if (z_bot) NPG_HIP(hipMemcpy(z_bot, S->seg_zbot, n * sizeof(double), hipMemcpyDeviceToHost));
    return NPG_OK;
}

NPG_API int npg_surfaces_compute(npg_surfaces *S, const npg_vec *x_inv, const npg_vec *b, double N2, const double *levels, int nlev,
                                 npg_vec *out, npg_vec *cols) {
    NPG_REQUIRE(S && x_inv && b && out && cols, "npg_surfaces_compute: NULL argument");
    const char *err = check_levels(levels, nlev, N2);
    NPG_REQUIRE(!err, "npg_surfaces_compute: %s", err);
    NPG_REQUIRE(x_inv->ctx == S->ctx && b->ctx == S->ctx && out->ctx == S->ctx && cols->ctx == S->ctx,
                "npg_surfaces_compute: arguments of different contexts");
    const npg_fe *fe = S->fe;
    NPG_REQUIRE_OK(check_state_vectors("npg_surfaces_compute", fe->n_inv, fe->n_b, x_inv->n, b->n));
    NPG_REQUIRE(out->n == (int64_t)kNSurf * nlev * S->ncol && cols->n == (int64_t)kNSurfCol * S->ncol,
                "npg_surfaces_compute: out must hold %d nlev ncol = %lld and cols %d ncol = %lld entries, got %lld and %lld", kNSurf,
                (long long)kNSurf * nlev * S->ncol, kNSurfCol, (long long)kNSurfCol * S->ncol, (long long)out->n, (long long)cols->n);
    if (S->ncol == 0) return NPG_OK;
    NPG_HIP(hipSetDevice(S->ctx->device));
    hipStream_t st = S->ctx->stream;
    if ((int)S->h_levels.size() != nlev || std::memcmp(S->h_levels.data(), levels, (size_t)nlev * sizeof(double)) != 0) {
        NPG_HIP(hipStreamSynchronize(st));           // an earlier scan may still read the old levels
        if ((int)S->h_levels.size() != nlev) {
            S->h_levels.clear();
            NPG_HIP(S->levels.alloc((size_t)nlev));
        }
        NPG_HIP(hipMemcpy(S->levels, levels, (size_t)nlev * sizeof(double), hipMemcpyHostToDevice));
        S->h_levels.assign(levels, levels + nlev);
    }
    const size_t ntab = (size_t)nlev * (size_t)S->ncol;
    if (S->cross_n < ntab) {
        NPG_HIP(hipStreamSynchronize(st));
        S->cross_n = 0;
        NPG_HIP(S->cross_cell.alloc(ntab));
        S->cross_n = ntab;
    }
    const FeDev &d = fe->d;
    const DevCells t = cell_view(d);
    const SurfaceColumns sc{S->col_ptr, S->seg_cell, S->seg_ztop, S->seg_zbot, S->xy, S->geo, S->ncol};
    const dim3 grid((unsigned)((S->ncol + kBlock - 1) / kBlock)), block(kBlock);
    if (d.nb == 10)
        hipLaunchKernelGGL(k_surfaces_scan<10>, grid, block, 0, st, sc, t, b->d, N2, S->levels.p, nlev, out->d, S->cross_cell.p, cols->d);
    else
        hipLaunchKernelGGL(k_surfaces_scan<4>, grid, block, 0, st, sc, t, b->d, N2, S->levels.p, nlev, out->d, S->cross_cell.p, cols->d);
    NPG_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_surfaces_fields, dim3((unsigned)((ntab + kBlock - 1) / kBlock)), block, 0, st, sc, t, x_inv->d, b->d, N2, nlev,
                       S->cross_cell.p, out->d);
    NPG_HIP(hipGetLastError());
    return NPG_OK;
}
