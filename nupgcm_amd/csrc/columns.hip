// Column integrals (npg_columns_compute): the exact vertical integrals of the state over fixed columns - transports,
// the baroclinic potential energy, the depth-integrated pressure gradient - and the state at the columns' ends, answered while the
// state is still in HBM.
//   k_column_segments<NB>  one lane per SEGMENT (columns_core.h: segment_terms).  A column is tens of cells walked in a serial gather
//                          chain, and there are fewer wet columns than lanes on the device; the segments are the parallel axis.  The lane
//                          gathers its cell's DoF codes and values through DevCells ([component][cell]), forms the P2 basis at the three
//                          Gauss points once and evaluates u, then b', then p, so the 44 nodal values are never all live.  The 17 terms
//                          go to terms[ch][seg] with plain stores.  NB = 10 (P2 b') or 4 (P1).
//   k_column_fold<NB>      one lane per (column, channel), column-fastest: it adds the column's run of terms[ch][.] top to bottom from 0.0
//                          - the order of columns_core.h, the host library's too - and writes out[ch][col] once.  The lanes of one more
//                          "channel" evaluate the 14 end values of their column (column_ends).
// No LDS, no atomics: every output has one writer and one order of summation, so the bits do not depend on the launch.  Always fp64.
#include <cmath>

#include "common.h"
#include "fe_dev.h"
#include "sample_dev.h"
#include "columns_core.h"

static_assert(NPG_NCOLI == npg::kNColI && NPG_NCOLE == npg::kNColE, "NPG_NCOLI / NPG_NCOLE of the header and columns_core.h must agree");

namespace npg {

struct ColumnSegments {             // the handle's tables as the kernels read them
    const int64_t *col_ptr;         // [ncol + 1]
    const int32_t *seg_cell, *seg_col;
    const double *seg_ztop, *seg_zbot;
    const double *xy;               // [ncol][2]
    const double *geo;              // the locator's records
    int64_t ncol, nseg;
};

template <int NB>
__global__ void __launch_bounds__(kBlock) k_column_segments(ColumnSegments S, DevCells t, const double *__restrict__ xu,
                                                            const double *__restrict__ xb, double *__restrict__ terms) {
    const int64_t s = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    if (s >= S.nseg) return;
    const int64_t c = S.seg_cell[s], j = S.seg_col[s];
    segment_terms<NB>(t, S.geo + (size_t)c * kGeoStride, xu, xb, c, S.xy[2 * j], S.xy[2 * j + 1], S.seg_ztop[s], S.seg_zbot[s], terms + s,
                      (size_t)S.nseg);
}

template <int NB>
__global__ void __launch_bounds__(kBlock) k_column_fold(ColumnSegments S, DevCells t, const double *__restrict__ xu,
                                                        const double *__restrict__ xb, const double *__restrict__ terms,
                                                        double *__restrict__ out) {
    const int64_t o = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    if (o >= (int64_t)(kNColI + 1) * S.ncol) return;
    const int64_t ch = o / S.ncol, j = o - ch * S.ncol;
    const int64_t s0 = S.col_ptr[j], s1 = S.col_ptr[j + 1];
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (ch < kNColI) {
        const double *run = terms + (size_t)ch * (size_t)S.nseg;
        double a = 0.0;
        for (int64_t s = s0; s < s1; ++s) a += run[s];
        out[o] = s1 > s0 ? a : nan;
    } else {
        double *e = out + (size_t)kNColI * (size_t)S.ncol + j;
        if (s1 > s0) {
            column_ends<NB>(t, S.geo, xu, xb, S.xy[2 * j], S.xy[2 * j + 1], S.seg_cell[s0], S.seg_ztop[s0], S.seg_cell[s1 - 1],
                            S.seg_zbot[s1 - 1], e, (size_t)S.ncol);
        } else {
NPG_UNROLL
            for (int k = 0; k < kNColE; ++k) e[(size_t)k * S.ncol] = nan;
        }
    }
}

}  // namespace npg

using namespace npg;

struct npg_columns {
    npg_ctx *ctx = nullptr;
    npg_fe *fe = nullptr;
    int64_t ncol = 0, nseg = 0, max_per_col = 0, ndry = 0;
    std::vector<int64_t> h_col_ptr;      // kept for npg_columns_columns
    std::vector<double> h_ztop, h_zbot;  // per column, NaN where dry
    DevBuf<int64_t> col_ptr;
    DevBuf<int32_t> seg_cell, seg_col;
    DevBuf<double> seg_ztop, seg_zbot, xy;
    DevBuf<double> terms;                // [NPG_NCOLI][nseg], written by every call that is given no segments_out
    const double *geo = nullptr;         // the locator's records (not owned: the locator outlives the handle)
};

NPG_API int npg_columns_destroy(npg_columns *C) {
    if (!C) return NPG_OK;
    hipStreamSynchronize(C->ctx->stream);
    delete C;
    return NPG_OK;
}

NPG_API int npg_columns_create(npg_fe *fe, npg_locator *loc, const double *xy, int64_t ncol, npg_columns **out) {
    const bool null_arg = !(fe && loc && xy && out);
    NPG_REQUIRE_OK(check_columns_create(null_arg, ncol, null_arg || loc->ctx == fe->ctx, !null_arg && loc->part, null_arg ? 0 : loc->ncell,
                                        null_arg ? 0 : fe->d.ncell));
    NPG_HIP(hipSetDevice(fe->ctx->device));
    NPG_HIP(hipStreamSynchronize(fe->ctx->stream));
    const int64_t ncell = loc->ncell;
    std::vector<double> geo((size_t)ncell * kGeoStride);
    NPG_HIP(hipMemcpy(geo.data(), loc->geo, geo.size() * sizeof(double), hipMemcpyDeviceToHost));
    ColumnTables ct;
    const char *err = build_columns(geo.data(), ncell, loc->grid.lo[2], loc->grid.hi[2], xy, ncol, ct);
    NPG_REQUIRE(!err, "npg_columns_create: %s", err);      // (nseg >= 2^31 among them)
    std::unique_ptr<npg_columns> C(new npg_columns());
    C->ctx = fe->ctx, C->fe = fe, C->geo = loc->geo;
    C->ncol = ncol, C->nseg = ct.col_ptr[(size_t)ncol], C->max_per_col = ct.max_per_col, C->ndry = ct.ndry;
    C->h_col_ptr = ct.col_ptr;
    C->h_ztop.assign((size_t)ncol, NAN), C->h_zbot.assign((size_t)ncol, NAN);
    std::vector<int32_t> seg_col((size_t)C->nseg);
    for (int64_t j = 0; j < ncol; ++j) {
        const int64_t s0 = ct.col_ptr[(size_t)j], s1 = ct.col_ptr[(size_t)j + 1];
        if (s1 > s0) C->h_ztop[(size_t)j] = ct.seg_ztop[(size_t)s0], C->h_zbot[(size_t)j] = ct.seg_zbot[(size_t)s1 - 1];
        for (int64_t s = s0; s < s1; ++s) seg_col[(size_t)s] = (int32_t)j;
    }
    const size_t ns = std::max<size_t>(1, (size_t)C->nseg);
    NPG_HIP(C->col_ptr.upload(ct.col_ptr));
    NPG_HIP(C->seg_cell.alloc(ns));                  // at least one entry each: never a null table in a kernel's arguments
    NPG_HIP(C->seg_col.alloc(ns));
    NPG_HIP(C->seg_ztop.alloc(ns));
    NPG_HIP(C->seg_zbot.alloc(ns));
    NPG_HIP(C->terms.alloc(ns * kNColI));
    NPG_HIP(C->xy.upload(xy, (size_t)ncol * 2));
    if (C->nseg) {
        NPG_HIP(hipMemcpy(C->seg_cell, ct.seg_cell.data(), (size_t)C->nseg * sizeof(int32_t), hipMemcpyHostToDevice));
        NPG_HIP(hipMemcpy(C->seg_col, seg_col.data(), (size_t)C->nseg * sizeof(int32_t), hipMemcpyHostToDevice));
        NPG_HIP(hipMemcpy(C->seg_ztop, ct.seg_ztop.data(), (size_t)C->nseg * sizeof(double), hipMemcpyHostToDevice));
        NPG_HIP(hipMemcpy(C->seg_zbot, ct.seg_zbot.data(), (size_t)C->nseg * sizeof(double), hipMemcpyHostToDevice));
    }
    *out = C.release();
    return NPG_OK;
}

NPG_API int npg_columns_info(const npg_columns *C, int64_t *nseg, int64_t *max_per_col, int64_t *ndry) {
    NPG_REQUIRE(C, "npg_columns_info: NULL handle");
    if (nseg) *nseg = C->nseg;
    if (max_per_col) *max_per_col = C->max_per_col;
    if (ndry) *ndry = C->ndry;
    return NPG_OK;
}

NPG_API int npg_columns_columns(const npg_columns *C, double *z_top, double *z_bot, int32_t *nseg) {
    NPG_REQUIRE(C, "npg_columns_columns: NULL handle");
    for (int64_t j = 0; j < C->ncol; ++j) {
        if (z_top) z_top[j] = C->h_ztop[(size_t)j];
        if (z_bot) z_bot[j] = C->h_zbot[(size_t)j];
        if (nseg) nseg[j] = (int32_t)(C->h_col_ptr[(size_t)j + 1] - C->h_col_ptr[(size_t)j]);
    }
    return NPG_OK;
}

NPG_API int npg_columns_segments(const npg_columns *C, int32_t *cell, double *z_top, double *z_bot) {
    NPG_REQUIRE(C, "npg_columns_segments: NULL handle");
    if (C->nseg == 0) return NPG_OK;
    NPG_HIP(hipSetDevice(C->ctx->device));
    const size_t n = (size_t)C->nseg;
    if (cell) NPG_HIP(hipMemcpy(cell, C->seg_cell, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (z_top) NPG_HIP(hipMemcpy(z_top, C->seg_ztop, n * sizeof(double), hipMemcpyDeviceToHost));
    if (z_bot) NPG_HIP(hipMemcpy(z_bot, C->seg_zbot, n * sizeof(double), hipMemcpyDeviceToHost));
    return NPG_OK;
}

NPG_API int npg_columns_compute(npg_columns *C, const npg_vec *x_inv, const npg_vec *b, npg_vec *out, npg_vec *segments_out) {
    const bool null_arg = !(C && x_inv && b && out);
    NPG_REQUIRE_OK(check_columns_compute(
        null_arg, null_arg || (x_inv->ctx == C->ctx && b->ctx == C->ctx && out->ctx == C->ctx && (!segments_out || segments_out->ctx == C->ctx)),
        null_arg ? 0 : C->fe->n_inv, null_arg ? 0 : C->fe->n_b, null_arg ? 0 : x_inv->n, null_arg ? 0 : b->n, null_arg ? 0 : out->n,
        segments_out ? segments_out->n : -1, null_arg ? 0 : C->ncol, null_arg ? 0 : C->nseg));
    NPG_HIP(hipSetDevice(C->ctx->device));
    hipStream_t st = C->ctx->stream;
    const FeDev &d = C->fe->d;
    const DevCells t = cell_view(d);
    const ColumnSegments cs{C->col_ptr, C->seg_cell, C->seg_col, C->seg_ztop, C->seg_zbot, C->xy, C->geo, C->ncol, C->nseg};
    double *terms = segments_out && C->nseg ? segments_out->d : C->terms.p;
    const dim3 block(kBlock);
    if (C->nseg) {
        const dim3 grid((unsigned)((C->nseg + kBlock - 1) / kBlock));
        if (d.nb == 10) hipLaunchKernelGGL(k_column_segments<10>, grid, block, 0, st, cs, t, x_inv->d, b->d, terms);
        else hipLaunchKernelGGL(k_column_segments<4>, grid, block, 0, st, cs, t, x_inv->d, b->d, terms);
        NPG_HIP(hipGetLastError());
    }
    const dim3 grid((unsigned)(((int64_t)(kNColI + 1) * C->ncol + kBlock - 1) / kBlock));
    if (d.nb == 10) hipLaunchKernelGGL(k_column_fold<10>, grid, block, 0, st, cs, t, x_inv->d, b->d, terms, out->d);
    else hipLaunchKernelGGL(k_column_fold<4>, grid, block, 0, st, cs, t, x_inv->d, b->d, terms, out->d);
    NPG_HIP(hipGetLastError());
    return NPG_OK;
}
