// Device-resident preconditioned CG: replaces Krylov.krylov_solve!(::CgWorkspace, A, y, x; M=P, ...) as configured at
// /root/reference/src/evolution.jl:118-126 (SPD A = M + theta (Kh + Kv), Jacobi P) and driven from
// /root/reference/src/iterative_solvers.jl:58.  One text serves npg_cg_solve (one right-hand side, any matrix storage, optionally
// distributed) and npg_cg_multi_solve (up to 32 right-hand sides against ONE plain-CSR matrix): a single solve is
// the K = 1 case of everything here but the product.
//
// Three steps per iteration, scalars never leave the device:
//   CS  Ap = A p (tiled CSR SpMV), partial p'Ap
//   CU  alpha = gamma / p'Ap ; x += alpha p ; r -= alpha Ap ; z = P r ; partial r'z
//       p'Ap not positive (zero, negative or NaN): no step, a flag for CP
//   CP  gamma' = r'z ; stopping test sqrt(gamma') <= atol + rtol sqrt(gamma_0) ; beta = gamma'/gamma ; p = z + beta p
//       flag set: status 3 with the iterate, the count and the history of the last completed iteration
// The first CP writes p = z and never reads what an earlier solve left in p.
// State snapshots (one per column) alternate between two slots so that a workgroup never reads what another workgroup of the same
// launch writes.  The host looks at the state every `chunk` iterations only.
//
// Columns: x, y and the internal p, r, z, Ap are STACKED - entry (row, column k) at k n + row.  (Row-major internals measured 1.2 to
// 1.7 times slower, DESIGN.md 19: a column's gathers then touch a cache line per lane instead of sharing lines between neighbouring
// lanes.)  A column whose snapshot says done is frozen: masked out of every kernel, its x / r / z / p / history are not written
// again.  CS and CU serve columns in blocks of C = 1, 2, 4 or 8 (template: the per-column accumulators stay in registers), one
// launch per block; CP serves all columns in one launch.
//
// Contract of the batched solve: every column has the BITS of npg_cg_solve on that column.  CU and CP are the same kernels; the
// build does not contract a*b+c, so the rest holds when each column keeps the single product's order of operations:
//   - products and row sums: spmv_tile_multi (spmv_multi.h) = spmv_tile's plain-CSR path per column, on the matrix's own tiles;
//   - partial sums: the same grids G1 / G2, the same thread-to-row mapping in the init and product kernels, the same
//     block_store_partials / reduce_partials with the column as the value index (kPartStride = 32 values: the column cap).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <type_traits>

#include "common.h"
#include "spmv_multi.h"

namespace npg {

struct CSnap {
    double gamma, eps, rnorm0, rnorm;
    int iter, done, first, pad;
};

struct CParams {
    double atol, rtol;
    long long itmax;
};

struct CDev {
    CsrDev A;
    const TileDesc *tile_ptr;
    int ntiles, n;
    int pkind;
    double pscalar;
    const double *pdiag;
    const double *b;      // stacked
    double *x;            // stacked
    double *r, *z, *p, *Ap;
    double *Pg, *Pp;
    int G1, G2;
    const double *Qp;     // what k_cg_update reduces: Pp on one GPU, the all-reduced row when distributed
    int nQp;
    CSnap *S;             // [2][smax]: two slots
    int *brk;             // [smax]: 1 when the last CU refused the column's step (p'Ap not positive); CU writes it in every iteration, the next CP reads it
    double *hist;         // [smax][hist_cap]
    int hist_cap;
    const CParams *prm;
    int K;                // columns of this solve
    int smax;             // snapshots per slot (the workspace's ncol_max)
};

constexpr int kKB = 1024;                 // threads per Krylov workgroup (see gmres.hip)
constexpr int kKW = kKB / 64;
constexpr int kNS = kKB / kPartStride;
constexpr int kMaxG = 256;
constexpr int kMaxI = kMaxG / kNS;
constexpr int kCols = NPG_CG_MULTI_MAX;
constexpr int kBlockCols = 8;             // columns per CS / CU launch: chosen by measurement
static_assert(kCols <= kPartStride, "a partial row carries one value per column");

struct CShared {
    double tmp[kNS * kPartStride];
    double red[kPartStride];
    double wsum[kKW * kPartStride];
    double beta[kCols];
    int done[kCols];
    int first[kCols];
};

__device__ __forceinline__ double cg_precond(const CDev &d, int64_t row) {
    return d.pkind == NPG_PRECOND_SCALAR ? d.pscalar : (d.pkind == NPG_PRECOND_DIAG ? d.pdiag[row] : 1.0);
}

// k n: where stacked column k starts.  Uniform, and pinned to scalar registers: left to itself the compiler turns every (vector,
// column) pair of an unrolled column loop into a per-thread 64-bit pointer of its own - k_cg_update<8> then takes all 128 VGPRs and
// spills to scratch.
__device__ __forceinline__ int64_t cg_column(const CDev &d, int k) {
    int64_t o = (int64_t)k * d.n;
    asm volatile("" : "+s"(o));
    return o;
}

// bit j: column cb + j exists and is not done in slot `slot`
template <int C>
__device__ __forceinline__ unsigned cg_active(const CDev &d, int slot, int cb) {
    unsigned m = 0;
#pragma unroll
    for (int j = 0; j < C; ++j)
        if (cb + j < d.K && d.S[slot * d.smax + cb + j].done == 0) m |= 1u << j;
    return m;
}

// ---- products of the single solve: spmv_tile, every matrix storage, [owned | ghosts] input (K = 1: one snapshot per slot)

// r = b - A x ; z = P r ; partial r'z
template <int L>
__global__ void __launch_bounds__(kKB) k_cg_init(CDev d) {
    __shared__ double sh[kKW * kPartStride];
    __shared__ TileLds tl;
    __shared__ double sw[kTileRows];
    double acc[1] = {0.0};
    for_each_tile(d.tile_ptr, d.ntiles, [&](const TileDesc &td) {
        const int r0 = td.r0, r1 = td.r0 + td.nrows;
        spmv_tile<kKB, L>(d.A, PlainX{d.x}, td, tl, sw);
        if ((int)threadIdx.x < r1 - r0) {
            const int row = r0 + threadIdx.x;
            const double r = d.b[row] - sw[threadIdx.x];
            const double z = cg_precond(d, row) * r;
            d.r[row] = r;
            d.z[row] = z;
            acc[0] += r * z;
        }
    });
    block_store_partials<1, kKW>(acc, 1, sh, d.Pg);
}

// CS
template <int L>
__global__ void __launch_bounds__(kKB) k_cg_spmv(CDev d, int slot) {
    __shared__ double sh[kKW * kPartStride];
    __shared__ TileLds tl;
    __shared__ double sw[kTileRows];
    if (d.S[slot].done != 0) return;
    double acc[1] = {0.0};
    for_each_tile(d.tile_ptr, d.ntiles, [&](const TileDesc &td) {
        const int r0 = td.r0, r1 = td.r0 + td.nrows;
        spmv_tile<kKB, L>(d.A, PlainX{d.p}, td, tl, sw);
        if ((int)threadIdx.x < r1 - r0) {
            const int row = r0 + threadIdx.x;
            const double ap = sw[threadIdx.x];
            d.Ap[row] = ap;
            acc[0] += d.p[row] * ap;
        }
    });
    block_store_partials<1, kKW>(acc, 1, sh, d.Pp);
}

// ---- products of the batched solve: spmv_tile_multi, plain CSR only, columns [cb, cb + C) on one stream of the matrix

// r = b - A x ; z = P r ; partial r'z
template <int L, int C>
__global__ void __launch_bounds__(kKB) k_cgm_init(CDev d, int cb) {
    __shared__ double sh[kKW * kPartStride];
    __shared__ TileLds tl;
    __shared__ double sw[kTileRows];
    double acc[C];
#pragma unroll
    for (int j = 0; j < C; ++j) acc[j] = 0.0;
    const unsigned active = cb + C <= d.K ? (1u << C) - 1u : (1u << (d.K - cb)) - 1u;
    for_each_tile(d.tile_ptr, d.ntiles, [&](const TileDesc &td) {
        spmv_tile_multi<kKB, L, C>(d.A, d.x + (int64_t)cb * d.n, 1, d.n, active, td, tl, sw, [&](int j) {
            if ((int)threadIdx.x < td.nrows) {
                const int row = td.r0 + threadIdx.x;
                const int64_t i = cg_column(d, cb + j) + row;
                const double r = d.b[i] - sw[threadIdx.x];
                const double z = cg_precond(d, row) * r;
                d.r[i] = r;
                d.z[i] = z;
                acc[j] += r * z;
            }
        });
    });
    block_store_partials<C, kKW>(acc, C, sh, d.Pg + cb);
}

// CS
template <int L, int C>
__global__ void __launch_bounds__(kKB) k_cgm_spmv(CDev d, int slot, int cb) {
    __shared__ double sh[kKW * kPartStride];
    __shared__ TileLds tl;
    __shared__ double sw[kTileRows];
    const unsigned active = cg_active<C>(d, slot, cb);
    if (active == 0) return;
    double acc[C];
#pragma unroll
    for (int j = 0; j < C; ++j) acc[j] = 0.0;
    for_each_tile(d.tile_ptr, d.ntiles, [&](const TileDesc &td) {
        spmv_tile_multi<kKB, L, C>(d.A, d.p + (int64_t)cb * d.n, 1, d.n, active, td, tl, sw, [&](int j) {
            if ((int)threadIdx.x < td.nrows) {
                const int64_t i = cg_column(d, cb + j) + td.r0 + threadIdx.x;
                const double ap = sw[threadIdx.x];
                d.Ap[i] = ap;
                acc[j] += d.p[i] * ap;
            }
        });
    });
    block_store_partials<C, kKW>(acc, C, sh, d.Pp + cb);
}

// ---- the steps both solves share

// CU for columns [cb, cb + C); the single solve is C = 1, cb = 0
template <int C>
__global__ void __launch_bounds__(kKB) k_cg_update(CDev d, int slot, int cb) {
    __shared__ CShared sh;
    unsigned active = cg_active<C>(d, slot, cb);
    if (active == 0) return;
    reduce_partials<kNS, kMaxI>(d.Qp, d.nQp, d.K, sh.tmp, sh.red);
    double alpha[C], acc[C];
#pragma unroll
    for (int j = 0; j < C; ++j) {
        acc[j] = 0.0;
        alpha[j] = 0.0;
        if ((active >> j) & 1u) {
            const double pAp = sh.red[cb + j];
            const bool refuse = !(pAp > 0.0);       // the same in every workgroup (and, distributed, on every rank: Qp is the all-reduced row)
            if (blockIdx.x == 0 && threadIdx.x == 0) d.brk[cb + j] = refuse ? 1 : 0;
            if (refuse)
                active &= ~(1u << j);               // no step for this column, a flag for CP
            else
                alpha[j] = d.S[slot * d.smax + cb + j].gamma / pAp;
        }
    }
    for (int64_t row = blockIdx.x * (int64_t)kKB + threadIdx.x; row < d.n; row += (int64_t)gridDim.x * kKB) {
        const double pc = cg_precond(d, row);
#pragma unroll
        for (int j = 0; j < C; ++j) {
            if (!((active >> j) & 1u)) continue;
            const int64_t i = cg_column(d, cb + j) + row;
            const double pv = d.p[i];
            d.x[i] += alpha[j] * pv;
            const double r = d.r[i] - alpha[j] * d.Ap[i];
            const double z = pc * r;
            d.r[i] = r;
            d.z[i] = z;
            acc[j] += r * z;
        }
    }
    block_store_partials<C, kKW>(acc, C, sh.wsum, d.Pg + cb);
}

// CP for all columns: thread k < K does column k's scalar work; p = z + beta p is element-wise, so any thread-to-entry mapping
// serves.  Reads slot `src`, writes slot `dst`.  qg, ng: the partial rows of r'z to fold (the all-reduced row when distributed).
__global__ void __launch_bounds__(kKB) k_cg_direction(CDev d, int src, int dst, const double *qg, int ng) {
    __shared__ CShared sh;
    reduce_partials<kNS, kMaxI>(qg, ng, d.K, sh.tmp, sh.red);
    if ((int)threadIdx.x < d.K) {
        const int k = threadIdx.x;
        const CSnap prev = d.S[src * d.smax + k];
        CSnap s = prev;
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
                // r'z that is NaN or Inf (y, x0 or the matrix hold one): breakdown, before rnorm0 <= eps = Inf can call it solved
                s.done = !isfinite(g) ? 3 : ((g == 0.0) ? 4 : (s.rnorm0 <= s.eps ? 1 : 0));
                s.pad = 1;   // first step: p = z
                if (blockIdx.x == 0) hist[0] = s.rnorm0;
            } else if (refused) {
                s.done = 3;  // CU took no step: iter, rnorm, gamma and the history stay at the last completed iteration
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
    for (int k = 0; k < d.K; ++k) {
        if (sh.done[k] != 0) continue;
        const double beta = sh.beta[k];
        double *__restrict__ p = d.p + (int64_t)k * d.n;
        const double *__restrict__ z = d.z + (int64_t)k * d.n;
        if (sh.first[k]) {      // first step: the old p is not read (it may hold a NaN of an earlier solve, and 0 * NaN is NaN)
            for (int64_t row = blockIdx.x * (int64_t)kKB + threadIdx.x; row < d.n; row += (int64_t)gridDim.x * kKB) p[row] = z[row];
            continue;
        }
        for (int64_t row = blockIdx.x * (int64_t)kKB + threadIdx.x; row < d.n; row += (int64_t)gridDim.x * kKB) p[row] = z[row] + beta * p[row];
    }
}

}  // namespace npg

using namespace npg;

namespace {

// what a solve of up to ncol_max columns keeps on the device
struct CgWork {
    npg_ctx *ctx = nullptr;
    int64_t n = 0;
    int ncol_max = 0;
    double *r = nullptr, *z = nullptr, *p = nullptr, *Ap = nullptr, *Pg = nullptr, *Pp = nullptr;
    CSnap *S = nullptr;
    int *brk = nullptr;
    CParams *prm = nullptr;
    double *hist = nullptr;
    int hist_cap = 0;
    CSnap *h_S = nullptr;            // pinned: ncol_max snapshots read back + ncol_max initial ones
    CParams *h_prm = nullptr;
    int64_t hist_len[NPG_CG_MULTI_MAX] = {};
};

int cg_work_alloc(CgWork &w, npg_ctx *ctx, int64_t n, int ncol_max) {
    w.ctx = ctx;
    w.n = n;
    w.ncol_max = ncol_max;
    NPG_HIP(hipSetDevice(ctx->device));
    const size_t vb = (size_t)n * (size_t)ncol_max * sizeof(double);
    NPG_HIP(hipMalloc((void **)&w.r, vb));
    NPG_HIP(hipMalloc((void **)&w.z, vb));
    NPG_HIP(hipMalloc((void **)&w.p, vb));
    NPG_HIP(hipMalloc((void **)&w.Ap, vb));
    const size_t pb = (size_t)kMaxG * kPartStride * sizeof(double);
    NPG_HIP(hipMalloc((void **)&w.Pg, pb));
    NPG_HIP(hipMalloc((void **)&w.Pp, pb));
    NPG_HIP(hipMalloc((void **)&w.S, 2 * (size_t)ncol_max * sizeof(CSnap)));
    NPG_HIP(hipMalloc((void **)&w.brk, (size_t)ncol_max * sizeof(int)));
    NPG_HIP(hipMalloc((void **)&w.prm, sizeof(CParams)));
    w.hist_cap = (int)std::min<int64_t>(2 * n + 2, 1 << 22);
    NPG_HIP(hipMalloc((void **)&w.hist, sizeof(double) * (size_t)w.hist_cap * (size_t)ncol_max));
    NPG_HIP(hipHostMalloc((void **)&w.h_S, 2 * (size_t)ncol_max * sizeof(CSnap), hipHostMallocDefault));
    NPG_HIP(hipHostMalloc((void **)&w.h_prm, sizeof(CParams), hipHostMallocDefault));
    NPG_HIP(hipMemsetAsync(w.Pg, 0, pb, ctx->stream));
    NPG_HIP(hipMemsetAsync(w.Pp, 0, pb, ctx->stream));
    NPG_HIP(hipStreamSynchronize(ctx->stream));
    return NPG_OK;
}

void cg_work_free(CgWork &w) {
    hipStreamSynchronize(w.ctx->stream);
    void *ptrs[] = {w.r, w.z, w.p, w.Ap, w.Pg, w.Pp, w.S, w.brk, w.prm, w.hist};
    for (void *p : ptrs)
        if (p) hipFree(p);
    if (w.h_S) hipHostFree(w.h_S);
    if (w.h_prm) hipHostFree(w.h_prm);
}

}  // namespace

struct npg_cg {
    CgWork w;                      // one column
    npg_halo *halo = nullptr;
    double *Rg = nullptr;          // 2 rows of kPartStride doubles: all-reduced p'Ap and r'z in their first entries (distributed mode)
    int64_t n_ghost = 0;
};

struct npg_cg_multi {
    CgWork w;
    int last_ncol = 0;
};

namespace {

// the checks both solves make, before any launch
int cg_check(const char *who, const void *ws, const npg_csr *A, const npg_vec *y, const npg_vec *x, int64_t n, int precond_kind,
             const npg_vec *precond_diag) {
    NPG_REQUIRE(ws && A && y && x, "%s: NULL argument", who);
    NPG_REQUIRE(!A->packed && !A->pk9, "%s: matrices with full node records are not served by the CG kernels", who);
    NPG_REQUIRE(!A->uperm, "%s: the matrix carries an internal renumbering (npg_csr_block_nodes_dofs): npg_spmv and npg_gmres_solve only", who);
    if (int rc = check_record_view(A, false, who)) return rc;
    NPG_REQUIRE(precond_kind == NPG_PRECOND_NONE || precond_kind == NPG_PRECOND_SCALAR ||
                    (precond_kind == NPG_PRECOND_DIAG && precond_diag && precond_diag->n == n),
                "%s: bad preconditioner", who);
    return NPG_OK;
}

// the launch grids: G1 workgroups walk the tiles (init, CS), G2 the rows (CU, CP)
void cg_grids(CDev &d, int num_cu) {
    d.G1 = std::max(1, std::min<int>(d.ntiles, std::min(kMaxG, num_cu)));
    d.G2 = (int)std::max<int64_t>(1, std::min<int64_t>(((int64_t)d.n + kKB - 1) / kKB, d.G1));
}

CDev cg_dev(const CgWork &w, const npg_csr *A, int precond_kind, double precond_scalar, const npg_vec *precond_diag, int ncol,
            const npg_vec *y, npg_vec *x) {
    CDev d;
    memset(&d, 0, sizeof d);
    d.A = csr_view(A);
    d.tile_ptr = A->tile_ptr;
    d.ntiles = A->ntiles;
    d.n = (int)w.n;
    d.K = ncol;
    d.smax = w.ncol_max;
    d.pkind = precond_kind;
    d.pscalar = precond_scalar;
    d.pdiag = precond_kind == NPG_PRECOND_DIAG ? precond_diag->d : nullptr;
    d.b = y->d;
    d.x = x->d;
    d.r = w.r;
    d.z = w.z;
    d.p = w.p;
    d.Ap = w.Ap;
    d.Pg = w.Pg;
    d.Pp = w.Pp;
    cg_grids(d, w.ctx->num_cu);
    d.Qp = d.Pp;
    d.nQp = d.G1;
    d.S = w.S;
    d.brk = w.brk;
    d.hist = w.hist;
    d.hist_cap = w.hist_cap;
    d.prm = w.prm;
    return d;
}

// the parameters and the initial snapshots of K columns, to the device
int cg_upload(CgWork &w, int K, double atol, double rtol, int64_t itmax) {
    w.h_prm->atol = atol;
    w.h_prm->rtol = rtol;
    w.h_prm->itmax = itmax;
    NPG_HIP(hipMemcpyAsync(w.prm, w.h_prm, sizeof(CParams), hipMemcpyHostToDevice, w.ctx->stream));
    CSnap s0{};
    s0.first = 1;
    CSnap *h_init = w.h_S + w.ncol_max;
    for (int k = 0; k < K; ++k) h_init[k] = s0;
    NPG_HIP(hipMemcpyAsync(w.S, h_init, (size_t)K * sizeof(CSnap), hipMemcpyHostToDevice, w.ctx->stream));
    return NPG_OK;
}

// after a solve: the history lengths, and the caller's stats (one per column) from the snapshots read back last
void cg_finish(CgWork &w, int K, npg_solve_stats *stats, std::chrono::steady_clock::time_point t0) {
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (int k = 0; k < K; ++k) {
        const CSnap &last = w.h_S[k];
        w.hist_len[k] = std::min<int64_t>((int64_t)last.iter + 1, w.hist_cap);
        if (!stats) continue;
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

int64_t cg_history(const CgWork &w, int col, double *buf, int64_t cap) {
    const int64_t k = std::min<int64_t>(cap, w.hist_len[col]);
    if (hipMemcpy(buf, w.hist + (size_t)col * w.hist_cap, (size_t)k * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return k;
}

// the column blocks of a solve: kBlockCols at a time, the tail in the smallest instance that holds it; f(cb, C as a type)
template <class F>
void cg_column_blocks(int K, F f) {
    for (int cb = 0; cb < K; cb += kBlockCols) {
        const int rem = K - cb;
        if (rem > 4)
            f(cb, std::integral_constant<int, 8>());
        else if (rem > 2)
            f(cb, std::integral_constant<int, 4>());
        else if (rem == 2)
            f(cb, std::integral_constant<int, 2>());
        else
            f(cb, std::integral_constant<int, 1>());
    }
}

// init (r = b - A x, ...) or CS: the one place that asks which product family serves the workspace
template <int L>
void cg_products(bool batched, bool init, const CDev &d, int slot, hipStream_t st) {
    if (!batched) {
        if (init)
            hipLaunchKernelGGL(k_cg_init<L>, dim3(d.G1), dim3(kKB), 0, st, d);
        else
            hipLaunchKernelGGL(k_cg_spmv<L>, dim3(d.G1), dim3(kKB), 0, st, d, slot);
        return;
    }
    cg_column_blocks(d.K, [&](int cb, auto c) {
        constexpr int C = decltype(c)::value;
        if (init)
            hipLaunchKernelGGL((k_cgm_init<L, C>), dim3(d.G1), dim3(kKB), 0, st, d, cb);
        else
            hipLaunchKernelGGL((k_cgm_spmv<L, C>), dim3(d.G1), dim3(kKB), 0, st, d, slot, cb);
    });
}

// dist: the single workspace of a distributed solve (null otherwise, and always for a batched one).  There the partial rows are
// folded and summed over the ranks - one kernel on the peer transport (comm.hip), fold + collective otherwise - into a row of Rg,
// and CU / CP read that row.  On return w.h_S[0 .. K) holds the columns' last snapshots.
template <int L>
int cg_run(CgWork &w, npg_cg *dist, bool batched, const CDev &d, int64_t itmax) {
    hipStream_t st = w.ctx->stream;
    double *Rp = dist ? dist->Rg : nullptr, *Rz = dist ? dist->Rg + kPartStride : nullptr;
    int rc = NPG_OK;
    if (dist && (rc = halo_exchange_raw(dist->halo, d.x))) return rc;
    cg_products<L>(batched, true, d, 0, st);
    if (dist && (rc = fold_allreduce_rows(w.ctx, d.Pg, d.G1, Rz, st))) return rc;
    // slot 0 = initial state; r'z comes from the init kernel's G1 partial rows (or from the all-reduced row)
    hipLaunchKernelGGL(k_cg_direction, dim3(d.G2), dim3(kKB), 0, st, d, 0, 1, dist ? Rz : d.Pg, dist ? 1 : d.G1);
    int cur = 1;
    const int chunk = 4;
    int64_t it = 0;
    while (true) {
        NPG_HIP(hipMemcpyAsync(w.h_S, w.S + (size_t)cur * w.ncol_max, (size_t)d.K * sizeof(CSnap), hipMemcpyDeviceToHost, st));
        NPG_HIP(hipStreamSynchronize(st));
        bool all = true;
        for (int k = 0; k < d.K; ++k) all = all && w.h_S[k].done != 0;
        if (all || it >= itmax) break;
        for (int c = 0; c < chunk; ++c, ++it) {
            if (dist && (rc = halo_exchange_raw(dist->halo, d.p))) return rc;
            cg_products<L>(batched, false, d, cur, st);
            if (dist && (rc = fold_allreduce_rows(w.ctx, d.Pp, d.G1, Rp, st))) return rc;
            cg_column_blocks(d.K, [&](int cb, auto cc) {
                hipLaunchKernelGGL(k_cg_update<decltype(cc)::value>, dim3(d.G2), dim3(kKB), 0, st, d, cur, cb);
            });
            if (dist && (rc = fold_allreduce_rows(w.ctx, d.Pg, d.G2, Rz, st))) return rc;
            hipLaunchKernelGGL(k_cg_direction, dim3(d.G2), dim3(kKB), 0, st, d, cur, cur ^ 1, dist ? Rz : d.Pg, dist ? 1 : d.G2);
            cur ^= 1;
        }
        NPG_HIP(hipGetLastError());
    }
    return NPG_OK;
}

int cg_run_lanes(CgWork &w, npg_cg *dist, bool batched, int lanes, const CDev &d, int64_t itmax) {
    switch (lanes) {
        case 4: return cg_run<4>(w, dist, batched, d, itmax);
        case 8: return cg_run<8>(w, dist, batched, d, itmax);
        case 16: return cg_run<16>(w, dist, batched, d, itmax);
        default: return cg_run<32>(w, dist, batched, d, itmax);
    }
}

}  // namespace

NPG_API int npg_cg_create(npg_ctx *ctx, int64_t n, npg_cg **out) {
    NPG_REQUIRE(ctx && out && n > 0 && n < INT32_MAX, "npg_cg_create: bad argument");
    npg_cg *ws = new npg_cg();
    if (int rc = cg_work_alloc(ws->w, ctx, n, 1)) return rc;
    *out = ws;
    return NPG_OK;
}

NPG_API int npg_cg_destroy(npg_cg *ws) {
    if (!ws) return NPG_OK;
    cg_work_free(ws->w);
    if (ws->Rg) hipFree(ws->Rg);
    delete ws;
    return NPG_OK;
}

NPG_API int npg_cg_set_halo(npg_cg *ws, npg_halo *h) {
    NPG_REQUIRE(ws, "npg_cg_set_halo: NULL workspace");
    NPG_REQUIRE(!h || h->n_owned == ws->w.n, "npg_cg_set_halo: the plan owns %lld rows, the workspace %lld",
                h ? (long long)h->n_owned : 0LL, (long long)ws->w.n);
    NPG_HIP(hipStreamSynchronize(ws->w.ctx->stream));
    ws->halo = h;
    ws->n_ghost = h ? h->n_ghost : 0;
    NPG_HIP(hipFree(ws->w.p));          // the SpMV input p needs room for the ghost entries
    const size_t nb = (size_t)(ws->w.n + ws->n_ghost) * sizeof(double);
    NPG_HIP(hipMalloc((void **)&ws->w.p, nb));
    NPG_HIP(hipMemset(ws->w.p, 0, nb));
    if (h && !ws->Rg) {
        NPG_HIP(hipMalloc((void **)&ws->Rg, 2 * kPartStride * sizeof(double)));
        NPG_HIP(hipMemset(ws->Rg, 0, 2 * kPartStride * sizeof(double)));
    }
    return NPG_OK;
}

NPG_API int npg_cg_solve(npg_cg *ws, const npg_csr *A, int precond_kind, double precond_scalar, const npg_vec *precond_diag,
                         const npg_vec *y, npg_vec *x, double atol, double rtol, int64_t itmax, npg_solve_stats *stats) {
    if (int rc = cg_check("npg_cg_solve", ws, A, y, x, ws ? ws->w.n : 0, precond_kind, precond_diag)) return rc;
    CgWork &w = ws->w;
    const int64_t nloc = w.n + ws->n_ghost;     // distributed: vectors the SpMV reads hold [owned | ghosts]
    NPG_REQUIRE(A->m == w.n && A->n == nloc && y->n == w.n && x->n == nloc,
                "npg_cg_solve: workspace is for n=%lld (+%lld ghosts) but A is %lldx%lld, y has %lld, x has %lld", (long long)w.n,
                (long long)ws->n_ghost, (long long)A->m, (long long)A->n, (long long)y->n, (long long)x->n);
    const auto t0 = std::chrono::steady_clock::now();
    CDev d = cg_dev(w, A, precond_kind, precond_scalar, precond_diag, 1, y, x);
    if (ws->halo) {
        d.Qp = ws->Rg;
        d.nQp = 1;
    }
    if (itmax <= 0) itmax = 2 * w.n;
    int rc = cg_upload(w, 1, atol, rtol, itmax);
    if (!rc) rc = cg_run_lanes(w, ws->halo ? ws : nullptr, false, A->lanes, d, itmax);
    if (!rc && ws->halo) rc = comm_check(w.ctx);
    if (rc) return rc;
    cg_finish(w, 1, stats, t0);
    return NPG_OK;
}

NPG_API int64_t npg_cg_history(npg_cg *ws, double *buf, int64_t cap) {
    if (!ws || !buf || cap <= 0) return 0;
    return cg_history(ws->w, 0, buf, cap);
}

NPG_API int npg_cg_multi_create(npg_ctx *ctx, int64_t n, int ncol_max, npg_cg_multi **out) {
    NPG_REQUIRE(ctx && out && n > 0 && n < INT32_MAX, "npg_cg_multi_create: bad argument");
    NPG_REQUIRE(ncol_max >= 1 && ncol_max <= NPG_CG_MULTI_MAX, "npg_cg_multi_create: ncol_max = %d, need 1 <= ncol_max <= %d", ncol_max,
                NPG_CG_MULTI_MAX);
    npg_cg_multi *ws = new npg_cg_multi();
    if (int rc = cg_work_alloc(ws->w, ctx, n, ncol_max)) return rc;
    *out = ws;
    return NPG_OK;
}

NPG_API int npg_cg_multi_destroy(npg_cg_multi *ws) {
    if (!ws) return NPG_OK;
    cg_work_free(ws->w);
    delete ws;
    return NPG_OK;
}

NPG_API int npg_cg_multi_solve(npg_cg_multi *ws, const npg_csr *A, int precond_kind, double precond_scalar,
                               const npg_vec *precond_diag, int ncol, const npg_vec *y, npg_vec *x, double atol, double rtol,
                               int64_t itmax, npg_solve_stats *stats) {
    if (int rc = cg_check("npg_cg_multi_solve", ws, A, y, x, ws ? ws->w.n : 0, precond_kind, precond_diag)) return rc;
    CgWork &w = ws->w;
    NPG_REQUIRE(ncol >= 1 && ncol <= w.ncol_max, "npg_cg_multi_solve: ncol = %d, the workspace holds 1 .. %d columns", ncol, w.ncol_max);
    NPG_REQUIRE(A->ctx == w.ctx && y->ctx == w.ctx && x->ctx == w.ctx &&
                    (precond_kind != NPG_PRECOND_DIAG || precond_diag->ctx == w.ctx),
                "npg_cg_multi_solve: the workspace, the matrix and the vectors must belong to one context");
    NPG_REQUIRE(A->nnode() == 0 && !A->drow && !A->grow,
                "npg_cg_multi_solve: the matrix is stored by node blocks or records; the multi-column product reads plain CSR only");
    NPG_REQUIRE(A->m == w.n && A->n == w.n && y->n == (int64_t)ncol * w.n && x->n == (int64_t)ncol * w.n,
                "npg_cg_multi_solve: workspace is for n=%lld and %d columns want vectors of %lld, but A is %lldx%lld, y has %lld, x has %lld",
                (long long)w.n, ncol, (long long)ncol * (long long)w.n, (long long)A->m, (long long)A->n, (long long)y->n,
                (long long)x->n);
    const auto t0 = std::chrono::steady_clock::now();
    const CDev d = cg_dev(w, A, precond_kind, precond_scalar, precond_diag, ncol, y, x);
    if (itmax <= 0) itmax = 2 * w.n;
    int rc = cg_upload(w, ncol, atol, rtol, itmax);
    ws->last_ncol = ncol;
    if (!rc) rc = cg_run_lanes(w, nullptr, true, A->lanes, d, itmax);
    if (rc) return rc;
    cg_finish(w, ncol, stats, t0);
    return NPG_OK;
}

NPG_API int64_t npg_cg_multi_history(npg_cg_multi *ws, int col, double *buf, int64_t cap) {
    if (!ws || !buf || cap <= 0 || col < 0 || col >= ws->last_ncol) return 0;
    return cg_history(ws->w, col, buf, cap);
}
