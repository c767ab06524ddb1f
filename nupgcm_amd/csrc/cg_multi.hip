// Preconditioned CG for several right-hand sides against ONE matrix: cg.hip's algorithm column by column, with one
// snapshot per column, in launches that stream the matrix once for up to eight columns.
//
// Contract: every column has the BITS of npg_cg_solve on that column.  The build does not contract a*b+c, so this holds when each
// column keeps the single solver's order of operations:
//   - products and row sums: spmv_tile_multi (spmv_multi.h) = spmv_tile's plain-CSR path per column, on the matrix's own tiles;
//   - partial sums: the same grids G1 / G2, the same thread-to-row mapping in the init, product and update kernels, the same
//     block_store_partials / reduce_partials with the column as the value index (kPartStride = 32 values: the column cap).
// Internal vectors p, r, z, Ap are STACKED like the caller's x and y (column k at k n).  The row-major layout (row i's K values
// adjacent) is kept behind NPG_CGM_LAYOUT=rows: it measured slower - a column's gathers then touch a cache line per lane instead of
// sharing lines between neighbouring lanes, and the lines do not survive in L1 until the next column.
// A column whose snapshot says done is frozen: masked out of every kernel, its x / r / z / p / history are not written again.
// Columns are served in blocks of C = 1, 2, 4 or 8 (template: the per-column accumulators stay in registers), one launch per block.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>

#include "common.h"
#include "spmv_multi.h"

namespace npg {

struct MSnap {      // = cg.hip's CSnap
    double gamma, eps, rnorm0, rnorm;
    int iter, done, first, pad;
};

struct MParams {
    double atol, rtol;
    long long itmax;
};

struct MDev {
    CsrDev A;
    const TileDesc *tile_ptr;
    int ntiles, n;
    int K;                // columns of this solve
    int64_t rs, ks;       // p, r, z, Ap: entry (row, column k) at row * rs + k * ks - row-major (K, 1) or stacked (1, n)
    int smax;             // snapshots per slot (the workspace's ncol_max)
    int pkind;
    double pscalar;
    const double *pdiag;
    const double *b;      // stacked
    double *x;            // stacked
    double *r, *z, *p, *Ap;
    double *Pg, *Pp;
    int G1, G2;
    MSnap *S;             // [2][smax]
    int *brk;             // [smax]: cg.hip's brk per column
    double *hist;         // [smax][hist_cap]
    int hist_cap;
    const MParams *prm;
};

constexpr int kMB = 1024;                 // as cg.hip
constexpr int kMW = kMB / 64;
constexpr int kMNS = kMB / kPartStride;
constexpr int kMMaxG = 256;
constexpr int kMMaxI = kMMaxG / kMNS;
constexpr int kMCols = NPG_CG_MULTI_MAX;
constexpr int kMBlockDefault = 8;          // columns per launch and internal layout: chosen by measurement
constexpr bool kMStackedDefault = true;
static_assert(kMCols <= kPartStride, "a partial row carries one value per column");

struct MShared {
    double tmp[kMNS * kPartStride];
    double red[kPartStride];
    double wsum[kMW * kPartStride];
    double beta[kMCols];
    int done[kMCols];
    int first[kMCols];
};

__device__ __forceinline__ double cgm_precond(const MDev &d, int64_t row) {
    return d.pkind == NPG_PRECOND_SCALAR ? d.pscalar : (d.pkind == NPG_PRECOND_DIAG ? d.pdiag[row] : 1.0);
}

// bit j: column cb + j exists and is not done in slot `slot`
template <int C>
__device__ __forceinline__ unsigned cgm_active(const MDev &d, int slot, int cb) {
    unsigned m = 0;
#pragma unroll
    for (int j = 0; j < C; ++j)
        if (cb + j < d.K && d.S[slot * d.smax + cb + j].done == 0) m |= 1u << j;
    return m;
}

// r = b - A x ; z = P r ; partial r'z         columns [cb, cb + C)
template <int L, int C>
__global__ void __launch_bounds__(kMB) k_cgm_init(MDev d, int cb) {
    __shared__ double sh[kMW * kPartStride];
    __shared__ TileLds tl;
    __shared__ double sw[kTileRows];
    double acc[C];
#pragma unroll
    for (int j = 0; j < C; ++j) acc[j] = 0.0;
    const unsigned active = cb + C <= d.K ? (1u << C) - 1u : (1u << (d.K - cb)) - 1u;
    TileDesc nd = d.tile_ptr[blockIdx.x < (unsigned)d.ntiles ? blockIdx.x : 0];
    for (int t = blockIdx.x; t < d.ntiles; t += gridDim.x) {
        const TileDesc td = nd;
        if (t + (int)gridDim.x < d.ntiles) nd = d.tile_ptr[t + gridDim.x];      // in flight during this tile
        spmv_tile_multi<kMB, L, C>(d.A, d.x + (int64_t)cb * d.n, 1, d.n, active, td, tl, sw, [&](int j) {
            if ((int)threadIdx.x < td.nrows) {
                const int row = td.r0 + threadIdx.x;
                const int64_t i = row * d.rs + (cb + j) * d.ks;
                const double r = d.b[(int64_t)(cb + j) * d.n + row] - sw[threadIdx.x];
                const double z = cgm_precond(d, row) * r;
                d.r[i] = r;
                d.z[i] = z;
                acc[j] += r * z;
            }
        });
    }
    block_store_partials<C, kMW>(acc, C, sh, d.Pg + cb);
}

// CS: Ap = A p, partial p'Ap                  columns [cb, cb + C)
template <int L, int C>
__global__ void __launch_bounds__(kMB) k_cgm_spmv(MDev d, int slot, int cb) {
    __shared__ double sh[kMW * kPartStride];
    __shared__ TileLds tl;
    __shared__ double sw[kTileRows];
    const unsigned active = cgm_active<C>(d, slot, cb);
    if (active == 0) return;
    double acc[C];
#pragma unroll
    for (int j = 0; j < C; ++j) acc[j] = 0.0;
    TileDesc nd = d.tile_ptr[blockIdx.x < (unsigned)d.ntiles ? blockIdx.x : 0];
    for (int t = blockIdx.x; t < d.ntiles; t += gridDim.x) {
        const TileDesc td = nd;
        if (t + (int)gridDim.x < d.ntiles) nd = d.tile_ptr[t + gridDim.x];      // in flight during this tile
        spmv_tile_multi<kMB, L, C>(d.A, d.p + cb * d.ks, d.rs, d.ks, active, td, tl, sw, [&](int j) {
            if ((int)threadIdx.x < td.nrows) {
                const int64_t i = (td.r0 + threadIdx.x) * d.rs + (cb + j) * d.ks;
                const double ap = sw[threadIdx.x];
                d.Ap[i] = ap;
                acc[j] += d.p[i] * ap;
            }
        });
    }
    block_store_partials<C, kMW>(acc, C, sh, d.Pp + cb);
}

// CU: alpha = gamma / p'Ap ; x += alpha p ; r -= alpha Ap ; z = P r ; partial r'z          columns [cb, cb + C)
template <int C>
__global__ void __launch_bounds__(kMB) k_cgm_update(MDev d, int slot, int cb) {
    __shared__ MShared sh;
    reduce_partials<kMNS, kMMaxI>(d.Pp, d.G1, d.K, sh.tmp, sh.red);
    unsigned active = cgm_active<C>(d, slot, cb);
    if (active == 0) return;
    double alpha[C], acc[C];
#pragma unroll
    for (int j = 0; j < C; ++j) {
        acc[j] = 0.0;
        alpha[j] = 0.0;
        if ((active >> j) & 1u) {
            const double pAp = sh.red[cb + j];
            const bool refuse = !(pAp > 0.0);       // as k_cg_update: no step for this column, a flag for k_cgm_direction
            if (blockIdx.x == 0 && threadIdx.x == 0) d.brk[cb + j] = refuse ? 1 : 0;
            if (refuse)
                active &= ~(1u << j);
            else
                alpha[j] = d.S[slot * d.smax + cb + j].gamma / pAp;
        }
    }
    for (int64_t row = blockIdx.x * (int64_t)kMB + threadIdx.x; row < d.n; row += (int64_t)gridDim.x * kMB) {
        const double pc = cgm_precond(d, row);
#pragma unroll
        for (int j = 0; j < C; ++j) {
            if (!((active >> j) & 1u)) continue;
            const int64_t i = row * d.rs + (cb + j) * d.ks;
            const double pv = d.p[i];
            d.x[(int64_t)(cb + j) * d.n + row] += alpha[j] * pv;
            const double r = d.r[i] - alpha[j] * d.Ap[i];
            const double z = pc * r;
            d.r[i] = r;
            d.z[i] = z;
            acc[j] += r * z;
        }
    }
    block_store_partials<C, kMW>(acc, C, sh.wsum, d.Pg + cb);
}

// CP for all columns: thread k < K does column k's scalar work (cg.hip's k_cg_direction, thread 0); p = z + beta p is element-wise,
// so any thread-to-entry mapping serves.  Reads slot `src`, writes slot `dst`.
__global__ void __launch_bounds__(kMB) k_cgm_direction(MDev d, int src, int dst, int ng) {
    __shared__ MShared sh;
    reduce_partials<kMNS, kMMaxI>(d.Pg, ng, d.K, sh.tmp, sh.red);
    if ((int)threadIdx.x < d.K) {
        const int k = threadIdx.x;
        const MSnap prev = d.S[src * d.smax + k];
        MSnap s = prev;
        double beta = 0.0;
        if (s.done == 0) {
            const double g = sh.red[k];
            const bool refused = !s.first && d.brk[k] != 0;
            double *hist = d.hist + (size_t)k * d.hist_cap;
            if (s.first) {
                s.rnorm0 = sqrt(g);
                s.rnorm = s.rnorm0;
                s.eps = d.prm->atol + d.prm->rtol * s.rnorm0;
                s.first = 0;
                s.iter = 0;
                s.done = !isfinite(g) ? 3 : ((g == 0.0) ? 4 : (s.rnorm0 <= s.eps ? 1 : 0));
                s.pad = 1;   // first step: p = z
                if (blockIdx.x == 0) hist[0] = s.rnorm0;
            } else if (refused) {
                s.done = 3;  // no step was taken: iter, rnorm, gamma and the history stay at the last completed iteration
            } else {
                s.rnorm = sqrt(g);
                s.iter += 1;
                if (blockIdx.x == 0 && s.iter < d.hist_cap) hist[s.iter] = s.rnorm;
                const bool solved = (s.rnorm <= s.eps) || (s.rnorm + 1.0 <= 1.0);
                s.done = solved ? 1 : ((long long)s.iter >= d.prm->itmax ? 2 : (g != g ? 3 : 0));
                s.pad = 0;
            }
            beta = s.pad ? 0.0 : g / prev.gamma;
            if (!refused) s.gamma = g;
            if (blockIdx.x == 0) d.S[dst * d.smax + k] = s;
        } else if (blockIdx.x == 0 && d.S[dst * d.smax + k].done == 0) {
            d.S[dst * d.smax + k] = s;      // a finished column's state reaches the other slot once, then stays
        }
        sh.beta[k] = beta;
        sh.done[k] = s.done;
        sh.first[k] = s.pad;
    }
    __syncthreads();
    if (d.ks != 1) {        // stacked: column by column
        for (int k = 0; k < d.K; ++k) {
            if (sh.done[k] != 0) continue;
            const double beta = sh.beta[k];
            double *__restrict__ p = d.p + (int64_t)k * d.n;
            const double *__restrict__ z = d.z + (int64_t)k * d.n;
            if (sh.first[k]) {      // first step: the old p is not read (cg.hip)
                for (int64_t row = blockIdx.x * (int64_t)kMB + threadIdx.x; row < d.n; row += (int64_t)gridDim.x * kMB) p[row] = z[row];
                continue;
            }
            for (int64_t row = blockIdx.x * (int64_t)kMB + threadIdx.x; row < d.n; row += (int64_t)gridDim.x * kMB) p[row] = z[row] + beta * p[row];
        }
        return;
    }
    const int64_t nk = (int64_t)d.n * d.K;
    int k = (int)((blockIdx.x * (int64_t)kMB + threadIdx.x) % d.K);
    const int dk = (int)(((int64_t)gridDim.x * kMB) % d.K);
    for (int64_t i = blockIdx.x * (int64_t)kMB + threadIdx.x; i < nk; i += (int64_t)gridDim.x * kMB) {
        if (sh.done[k] == 0) d.p[i] = sh.first[k] ? d.z[i] : d.z[i] + sh.beta[k] * d.p[i];
        k += dk;
        if (k >= d.K) k -= d.K;
    }
}

}  // namespace npg

using namespace npg;

struct npg_cg_multi {
    npg_ctx *ctx = nullptr;
    int64_t n = 0;
    int ncol_max = 0;
    double *r = nullptr, *z = nullptr, *p = nullptr, *Ap = nullptr, *Pg = nullptr, *Pp = nullptr;
    MSnap *S = nullptr;
    int *brk = nullptr;
    MParams *prm = nullptr;
    double *hist = nullptr;
    int hist_cap = 0;
    MSnap *h_S = nullptr;            // pinned: ncol_max snapshots read back + ncol_max initial ones
    MParams *h_prm = nullptr;
    int last_ncol = 0;
    int64_t hist_len[NPG_CG_MULTI_MAX] = {};
};

NPG_API int npg_cg_multi_create(npg_ctx *ctx, int64_t n, int ncol_max, npg_cg_multi **out) {
    NPG_REQUIRE(ctx && out && n > 0 && n < INT32_MAX, "npg_cg_multi_create: bad argument");
    NPG_REQUIRE(ncol_max >= 1 && ncol_max <= NPG_CG_MULTI_MAX, "npg_cg_multi_create: ncol_max = %d, need 1 <= ncol_max <= %d", ncol_max,
                NPG_CG_MULTI_MAX);
    npg_cg_multi *ws = new npg_cg_multi();
    ws->ctx = ctx;
    ws->n = n;
    ws->ncol_max = ncol_max;
    NPG_HIP(hipSetDevice(ctx->device));
    const size_t vb = (size_t)n * (size_t)ncol_max * sizeof(double);
    NPG_HIP(hipMalloc((void **)&ws->r, vb));
    NPG_HIP(hipMalloc((void **)&ws->z, vb));
    NPG_HIP(hipMalloc((void **)&ws->p, vb));
    NPG_HIP(hipMalloc((void **)&ws->Ap, vb));
    const size_t pb = (size_t)kMMaxG * kPartStride * sizeof(double);
    NPG_HIP(hipMalloc((void **)&ws->Pg, pb));
    NPG_HIP(hipMalloc((void **)&ws->Pp, pb));
    NPG_HIP(hipMalloc((void **)&ws->S, 2 * (size_t)ncol_max * sizeof(MSnap)));
    NPG_HIP(hipMalloc((void **)&ws->brk, (size_t)ncol_max * sizeof(int)));
    NPG_HIP(hipMalloc((void **)&ws->prm, sizeof(MParams)));
    ws->hist_cap = (int)std::min<int64_t>(2 * n + 2, 1 << 22);
    NPG_HIP(hipMalloc((void **)&ws->hist, sizeof(double) * (size_t)ws->hist_cap * (size_t)ncol_max));
    NPG_HIP(hipHostMalloc((void **)&ws->h_S, 2 * (size_t)ncol_max * sizeof(MSnap), hipHostMallocDefault));
    NPG_HIP(hipHostMalloc((void **)&ws->h_prm, sizeof(MParams), hipHostMallocDefault));
    NPG_HIP(hipMemsetAsync(ws->Pg, 0, pb, ctx->stream));
    NPG_HIP(hipMemsetAsync(ws->Pp, 0, pb, ctx->stream));
    NPG_HIP(hipStreamSynchronize(ctx->stream));
    *out = ws;
    return NPG_OK;
}

NPG_API int npg_cg_multi_destroy(npg_cg_multi *ws) {
    if (!ws) return NPG_OK;
    hipStreamSynchronize(ws->ctx->stream);
    void *ptrs[] = {ws->r, ws->z, ws->p, ws->Ap, ws->Pg, ws->Pp, ws->S, ws->brk, ws->prm, ws->hist};
    for (void *p : ptrs)
        if (p) hipFree(p);
    if (ws->h_S) hipHostFree(ws->h_S);
    if (ws->h_prm) hipHostFree(ws->h_prm);
    delete ws;
    return NPG_OK;
}

namespace {

// tuning overrides (as NPG_SPMV_LANES): NPG_CGM_BLOCK = 1, 2, 4 or 8 columns per launch at most; NPG_CGM_LAYOUT = stacked | rows
inline int block_cap() {
    static const int cap = [] {
        const char *e = getenv("NPG_CGM_BLOCK");
        const int v = e ? atoi(e) : kMBlockDefault;
        return (v == 1 || v == 2 || v == 4 || v == 8) ? v : kMBlockDefault;
    }();
    return cap;
}
inline bool layout_stacked() {
    static const bool st = [] {
        const char *e = getenv("NPG_CGM_LAYOUT");
        return e ? strcmp(e, "stacked") == 0 : kMStackedDefault;
    }();
    return st;
}
// the column blocks of a solve: block_cap() at a time, the tail in the smallest instance that holds it
inline int block_width(int rem) {
    const int cap = block_cap();
    return rem >= cap ? cap : rem > 4 ? 8 : rem > 2 ? 4 : rem;
}

template <int L, int C>
void cgm_launch_tiles(bool init, const MDev &d, int slot, int cb, hipStream_t st) {
    if (init)
        hipLaunchKernelGGL((k_cgm_init<L, C>), dim3(d.G1), dim3(kMB), 0, st, d, cb);
    else
        hipLaunchKernelGGL((k_cgm_spmv<L, C>), dim3(d.G1), dim3(kMB), 0, st, d, slot, cb);
}

template <int L>
void cgm_tiles(bool init, const MDev &d, int slot, hipStream_t st) {
    for (int cb = 0; cb < d.K; cb += block_cap()) {
        switch (block_width(d.K - cb)) {
            case 1: cgm_launch_tiles<L, 1>(init, d, slot, cb, st); break;
            case 2: cgm_launch_tiles<L, 2>(init, d, slot, cb, st); break;
            case 4: cgm_launch_tiles<L, 4>(init, d, slot, cb, st); break;
            default: cgm_launch_tiles<L, 8>(init, d, slot, cb, st); break;
        }
    }
}

void cgm_update(const MDev &d, int slot, hipStream_t st) {
    for (int cb = 0; cb < d.K; cb += block_cap()) {
        switch (block_width(d.K - cb)) {
            case 1: hipLaunchKernelGGL(k_cgm_update<1>, dim3(d.G2), dim3(kMB), 0, st, d, slot, cb); break;
            case 2: hipLaunchKernelGGL(k_cgm_update<2>, dim3(d.G2), dim3(kMB), 0, st, d, slot, cb); break;
            case 4: hipLaunchKernelGGL(k_cgm_update<4>, dim3(d.G2), dim3(kMB), 0, st, d, slot, cb); break;
            default: hipLaunchKernelGGL(k_cgm_update<8>, dim3(d.G2), dim3(kMB), 0, st, d, slot, cb); break;
        }
    }
}

template <int L>
int cgm_run(npg_cg_multi *ws, const MDev &d, int64_t itmax) {
    hipStream_t st = ws->ctx->stream;
    cgm_tiles<L>(true, d, 0, st);
    hipLaunchKernelGGL(k_cgm_direction, dim3(d.G2), dim3(kMB), 0, st, d, 0, 1, d.G1);
    int cur = 1;
    const int chunk = 4;
    int64_t it = 0;
    while (true) {
        NPG_HIP(hipMemcpyAsync(ws->h_S, ws->S + (size_t)cur * ws->ncol_max, (size_t)d.K * sizeof(MSnap), hipMemcpyDeviceToHost, st));
        NPG_HIP(hipStreamSynchronize(st));
        bool all = true;
        for (int k = 0; k < d.K; ++k) all = all && ws->h_S[k].done != 0;
        if (all || it >= itmax) break;
        for (int c = 0; c < chunk; ++c, ++it) {
            cgm_tiles<L>(false, d, cur, st);
            cgm_update(d, cur, st);
            hipLaunchKernelGGL(k_cgm_direction, dim3(d.G2), dim3(kMB), 0, st, d, cur, cur ^ 1, d.G2);
            cur ^= 1;
        }
        NPG_HIP(hipGetLastError());
    }
    return NPG_OK;
}

}  // namespace

NPG_API int npg_cg_multi_solve(npg_cg_multi *ws, const npg_csr *A, int precond_kind, double precond_scalar,
                               const npg_vec *precond_diag, int ncol, const npg_vec *y, npg_vec *x, double atol, double rtol,
                               int64_t itmax, npg_solve_stats *stats) {
    NPG_REQUIRE(ws && A && y && x, "npg_cg_multi_solve: NULL argument");
    NPG_REQUIRE(ncol >= 1 && ncol <= ws->ncol_max, "npg_cg_multi_solve: ncol = %d, the workspace holds 1 .. %d columns", ncol,
                ws->ncol_max);
    NPG_REQUIRE(A->ctx == ws->ctx && y->ctx == ws->ctx && x->ctx == ws->ctx &&
                    (precond_kind != NPG_PRECOND_DIAG || !precond_diag || precond_diag->ctx == ws->ctx),
                "npg_cg_multi_solve: the workspace, the matrix and the vectors must belong to one context");
    NPG_REQUIRE(!A->packed && !A->pk9, "npg_cg_multi_solve: matrices with full node records are not served by the CG kernels");
    NPG_REQUIRE(!A->uperm, "npg_cg_multi_solve: the matrix carries an internal renumbering (npg_csr_block_nodes_dofs): npg_spmv and npg_gmres_solve only");
    if (int rc = check_record_view(A, false, "npg_cg_multi_solve")) return rc;
    NPG_REQUIRE(A->nnode() == 0 && !A->drow && !A->grow,
                "npg_cg_multi_solve: the matrix is stored by node blocks or records; the multi-column product reads plain CSR only");
    NPG_REQUIRE(A->m == ws->n && A->n == ws->n && y->n == (int64_t)ncol * ws->n && x->n == (int64_t)ncol * ws->n,
                "npg_cg_multi_solve: workspace is for n=%lld and %d columns want vectors of %lld, but A is %lldx%lld, y has %lld, x has %lld",
                (long long)ws->n, ncol, (long long)ncol * (long long)ws->n, (long long)A->m, (long long)A->n, (long long)y->n,
                (long long)x->n);
    NPG_REQUIRE(precond_kind == NPG_PRECOND_NONE || precond_kind == NPG_PRECOND_SCALAR ||
                    (precond_kind == NPG_PRECOND_DIAG && precond_diag && precond_diag->n == ws->n),
                "npg_cg_multi_solve: bad preconditioner");
    const auto t0 = std::chrono::steady_clock::now();
    npg_ctx *ctx = ws->ctx;
    MDev d;
    memset(&d, 0, sizeof d);
    d.A = csr_view(A);
    d.tile_ptr = A->tile_ptr;
    d.ntiles = A->ntiles;
    d.n = (int)ws->n;
    d.K = ncol;
    d.rs = layout_stacked() ? 1 : ncol;
    d.ks = layout_stacked() ? ws->n : 1;
    d.smax = ws->ncol_max;
    d.pkind = precond_kind;
    d.pscalar = precond_scalar;
    d.pdiag = precond_kind == NPG_PRECOND_DIAG ? precond_diag->d : nullptr;
    d.b = y->d;
    d.x = x->d;
    d.r = ws->r;
    d.z = ws->z;
    d.p = ws->p;
    d.Ap = ws->Ap;
    d.Pg = ws->Pg;
    d.Pp = ws->Pp;
    d.G1 = std::max(1, std::min<int>(A->ntiles, std::min(kMMaxG, ctx->num_cu)));       // as npg_cg_solve
    d.G2 = (int)std::max<int64_t>(1, std::min<int64_t>((ws->n + kMB - 1) / kMB, d.G1));
    d.S = ws->S;
    d.brk = ws->brk;
    d.hist = ws->hist;
    d.hist_cap = ws->hist_cap;
    d.prm = ws->prm;
    if (itmax <= 0) itmax = 2 * ws->n;
    ws->h_prm->atol = atol;
    ws->h_prm->rtol = rtol;
    ws->h_prm->itmax = itmax;
    NPG_HIP(hipMemcpyAsync(ws->prm, ws->h_prm, sizeof(MParams), hipMemcpyHostToDevice, ctx->stream));
    MSnap s0{};
    s0.first = 1;
    MSnap *h_init = ws->h_S + ws->ncol_max;
    for (int k = 0; k < ncol; ++k) h_init[k] = s0;
    NPG_HIP(hipMemcpyAsync(ws->S, h_init, (size_t)ncol * sizeof(MSnap), hipMemcpyHostToDevice, ctx->stream));
    ws->last_ncol = ncol;
    int rc;
    switch (A->lanes) {
        case 4: rc = cgm_run<4>(ws, d, itmax); break;
        case 8: rc = cgm_run<8>(ws, d, itmax); break;
        case 16: rc = cgm_run<16>(ws, d, itmax); break;
        default: rc = cgm_run<32>(ws, d, itmax); break;
    }
    if (rc) return rc;
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (int k = 0; k < ncol; ++k) {
        const MSnap &last = ws->h_S[k];
        ws->hist_len[k] = std::min<int64_t>((int64_t)last.iter + 1, ws->hist_cap);
        if (stats) {
            npg_solve_stats *s = stats + k;
            s->solved = (last.done == 1 || last.done == 4) ? 1 : 0;
            s->niter = last.iter;
            s->npass = 1;
            s->status = last.done;
            s->nreorth = 0;
            s->nflagged = 0;
            s->rnorm0 = last.rnorm0;
            s->rnorm = last.rnorm;
            s->seconds = seconds;
        }
    }
    return NPG_OK;
}

NPG_API int64_t npg_cg_multi_history(npg_cg_multi *ws, int col, double *buf, int64_t cap) {
    if (!ws || !buf || cap <= 0 || col < 0 || col >= ws->last_ncol) return 0;
    const int64_t k = std::min<int64_t>(cap, ws->hist_len[col]);
    if (hipMemcpy(buf, ws->hist + (size_t)col * ws->hist_cap, (size_t)k * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return k;
}
