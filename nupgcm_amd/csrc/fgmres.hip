// Right-preconditioned FLEXIBLE GMRES(m) (npg_fgmres_*): the outer solver of the general preconditioners (npg_precond: mg.hip,
// dense_inv.hip), which are applied inexactly - so every basis vector keeps its own preconditioned copy (Z).  Classical
// Gram-Schmidt with a full second pass (two fused multi-dot reductions per step, one host synchronisation per iteration -
// an iteration costs a V-cycle, i.e. milliseconds on the meshes where this is used, so the host drives the loop).  The
// stopping rule is the reference's: scale * ||r|| <= atol + rtol * scale * ||r0|| with scale = 1/h^dim, the factor its
// Diagonal preconditioner puts on the residual (src/inversion.jl:42-54; right preconditioning leaves r the true residual).
// Of the preconditioner it needs pc->n, precond_apply_raw and axpby (precond.h).
#include <cmath>

#include "precond.h"
#include "device_utils.h"

namespace npg {

// part[block][c] = sum_i V_c[i] w[i] for c < k (k <= 8 NG); V column-major with leading dimension ld
template <int NG>
__global__ void __launch_bounds__(kBlock) k_mdot(const double *__restrict__ V, int64_t ld, int k,
                                                 const double *__restrict__ w, int64_t n, double *__restrict__ part) {
    __shared__ double sh[4 * kPartStride];
    double acc[8 * NG];
#pragma unroll
    for (int c = 0; c < 8 * NG; ++c) acc[c] = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const double wi = w[i];
#pragma unroll
        for (int c = 0; c < 8 * NG; ++c)
            if (c < k) acc[c] += V[(size_t)c * ld + i] * wi;
    }
    block_store_partials<8 * NG, 4>(acc, k, sh, part);
}

// w -= sum_c h[c] V_c ; part[block][0] = sum w_new^2
template <int NG>
__global__ void __launch_bounds__(kBlock) k_mupdate(const double *__restrict__ V, int64_t ld, int k,
                                                    const double *__restrict__ h, double *__restrict__ w, int64_t n,
                                                    double *__restrict__ part) {
    __shared__ double sh[4 * kPartStride];
    double hc[8 * NG];
#pragma unroll
    for (int c = 0; c < 8 * NG; ++c) hc[c] = c < k ? h[c] : 0.0;
    double acc[1] = {0.0};
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        double wi = w[i];
#pragma unroll
        for (int c = 0; c < 8 * NG; ++c)
            if (c < k) wi -= hc[c] * V[(size_t)c * ld + i];
        w[i] = wi;
        acc[0] += wi * wi;
    }
    block_store_partials<1, 4>(acc, 1, sh, part);
}

// out[c] = sum_b part[b][c]  (one block; fixed order)
__global__ void __launch_bounds__(kBlock) k_sum_partials(const double *__restrict__ part, int nblocks, int nvals,
                                                         double *__restrict__ out) {
    __shared__ double tmp[8 * kPartStride], res[kPartStride];
    reduce_partials<8, 128>(part, nblocks, nvals, tmp, res);
    if (threadIdx.x < nvals) out[threadIdx.x] = res[threadIdx.x];
}

// x += sum_c y[c] Z_c
struct Coefs {
    double y[kMaxMem];
};
__global__ void __launch_bounds__(kBlock) k_combine_z(double *__restrict__ x, const double *__restrict__ Z, int64_t ld,
                                                      int k, Coefs cf, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        double s = x[i];
        for (int c = 0; c < k; ++c) s += cf.y[c] * Z[(size_t)c * ld + i];
        x[i] = s;
    }
}

}  // namespace npg

using namespace npg;

struct HostFree {
    void operator()(double *p) const { hipHostFree(p); }
};

struct npg_fgmres {
    npg_ctx *ctx = nullptr;
    int64_t n = 0, ld = 0;
    int mem = 20;
    DevBuf<double> V, Z;                     // (mem + 1) and mem columns of ld doubles
    DevBuf<double> part;                     // partial rows of the reductions
    DevBuf<double> dsc;                      // device scalars: h1 [0,32), h2 [32,64), norm^2 [64]
    std::unique_ptr<double[], HostFree> hsc; // pinned host copy
    std::vector<double> hist;
    // distributed (npg_fgmres_set_halo): n counts OWNED rows; the columns of Z (SpMV inputs) have room for the ghost entries
    npg_halo *halo = nullptr;
    int64_t n_ghost = 0;
};

constexpr int kFgBlocks = 1024;

NPG_API int npg_fgmres_create(npg_ctx *ctx, int64_t n, int memory, npg_fgmres **out) {
    NPG_REQUIRE(ctx && out && n > 0, "npg_fgmres_create: bad argument");
    NPG_REQUIRE(memory >= 1 && memory <= 23, "npg_fgmres_create: memory must be in 1..23");
    std::unique_ptr<npg_fgmres> ws(new npg_fgmres());
    ws->ctx = ctx; ws->n = n; ws->mem = memory;
    ws->ld = (n + 31) / 32 * 32;
    NPG_HIP(hipSetDevice(ctx->device));
    NPG_HIP(ws->V.alloc((size_t)(memory + 1) * ws->ld));
    NPG_HIP(ws->Z.alloc((size_t)memory * ws->ld));
    NPG_HIP(ws->part.alloc((size_t)kFgBlocks * kPartStride));
    NPG_HIP(ws->dsc.zeros(128));                                           // (whole 32-double rows: the all-reduce moves rows)
    double *hsc = nullptr;
    NPG_HIP(hipHostMalloc((void **)&hsc, 128 * sizeof(double), hipHostMallocDefault));
    ws->hsc.reset(hsc);
    *out = ws.release();
    return NPG_OK;
}

// Row-block distributed solves: A is this rank's rows (columns [owned | ghosts]), x holds [owned | ghosts]; the ghosts of every
// SpMV input are filled through `h`, the Gram-Schmidt sums and norms are summed over the ranks (three 32-double all-reduces per
// iteration - an iteration is a whole V-cycle).  Collective: every rank sets its plan before the first solve.
// The wider V and Z are allocated before the old ones are released: a failure leaves the workspace as it was.
NPG_API int npg_fgmres_set_halo(npg_fgmres *ws, npg_halo *h) {
    NPG_REQUIRE(ws && h && h->n_owned == ws->n, "npg_fgmres_set_halo: the plan must own the workspace's %lld rows", ws ? (long long)ws->n : 0LL);
    NPG_HIP(hipStreamSynchronize(ws->ctx->stream));
    const int64_t ld = (ws->n + h->n_ghost + 31) / 32 * 32;
    DevBuf<double> V, Z;
    NPG_HIP(V.alloc((size_t)(ws->mem + 1) * ld));
    NPG_HIP(Z.zeros((size_t)ws->mem * ld));
    ws->V = std::move(V);
    ws->Z = std::move(Z);
    ws->halo = h;
    ws->n_ghost = h->n_ghost;
    ws->ld = ld;
    return NPG_OK;
}

NPG_API int npg_fgmres_destroy(npg_fgmres *ws) {
    if (!ws) return NPG_OK;
    hipStreamSynchronize(ws->ctx->stream);
    delete ws;
    return NPG_OK;
}

NPG_API int64_t npg_fgmres_history(npg_fgmres *ws, double *buf, int64_t cap) {
    if (!ws || !buf) return -1;
    const int64_t k = std::min<int64_t>(cap, (int64_t)ws->hist.size());
    std::copy(ws->hist.begin(), ws->hist.begin() + k, buf);
    return k;
}

template <typename F>
static void by_groups(int k, F f) {
    if (k <= 8) f(std::integral_constant<int, 1>());
    else if (k <= 16) f(std::integral_constant<int, 2>());
    else f(std::integral_constant<int, 3>());
}

NPG_API int npg_fgmres_solve(npg_fgmres *ws, const npg_csr *A, npg_precond *pc, const npg_vec *y, npg_vec *x,
                             double scale, double atol, double rtol, int64_t itmax, npg_solve_stats *stats) {
    NPG_REQUIRE(ws && A && y && x && stats, "npg_fgmres_solve: NULL argument");
    NPG_REQUIRE(!A->uperm, "npg_fgmres_solve: the matrix carries an internal renumbering (npg_csr_block_nodes_dofs): npg_spmv and npg_gmres_solve only");
    const int64_t n = ws->n, ld = ws->ld;
    const int64_t nloc = n + ws->n_ghost;
    NPG_REQUIRE(A->m == n && A->n == nloc && y->n == n && x->n == nloc, "npg_fgmres_solve: system must be %lld x %lld (+%lld ghosts)",
                (long long)n, (long long)n, (long long)ws->n_ghost);
    npg_halo *dh = ws->halo;
    // sum over the ranks of a host scalar (distributed) - the host is synchronised at these points anyway
    auto all_sum = [&](double *v) -> int { return dh ? npg_comm_allreduce_sum(ws->ctx, v, 1) : NPG_OK; };
    NPG_REQUIRE(!pc || pc->n == n, "npg_fgmres_solve: the preconditioner is for %lld unknowns", (long long)(pc ? pc->n : 0));
    NPG_REQUIRE(scale > 0 && atol >= 0 && rtol >= 0, "npg_fgmres_solve: bad tolerance / scale");
    npg_ctx *c = ws->ctx;
    hipStream_t st = c->stream;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    struct EvGuard {
        hipEvent_t &a, &b;
        ~EvGuard() {
            if (a) hipEventDestroy(a);
            if (b) hipEventDestroy(b);
        }
    } evguard{e0, e1};
    NPG_HIP(hipEventCreate(&e0));
    NPG_HIP(hipEventCreate(&e1));
    NPG_HIP(hipEventRecord(e0, st));
    if (itmax <= 0) itmax = 2 * n;
    const int mem = ws->mem;
    const int grid = std::min(kFgBlocks, grid_for(n, kFgBlocks));
    *stats = npg_solve_stats{};
    ws->hist.clear();
    int rc;
    double *V = ws->V, *Z = ws->Z;
    // r0 = y - A x
    {
        if (dh && (rc = halo_exchange_raw(dh, x->d))) return rc;
        SpmvEpi e{};
        e.alpha = -1.0; e.beta = 1.0; e.c = y->d; e.y = V;
        if ((rc = spmv_epi(A, x->d, e))) return rc;
    }
    double dd;
    if ((rc = reduce_dot(c, V, V, n, &dd)) || (rc = all_sum(&dd))) return rc;
    double beta = std::sqrt(dd);
    const double rnorm0 = scale * beta, eps = atol + rtol * rnorm0;
    stats->rnorm0 = rnorm0;
    stats->rnorm = rnorm0;
    ws->hist.push_back(rnorm0);
    int64_t it = 0;
    bool solved = rnorm0 <= eps, breakdown = false;
    if (beta == 0.0) stats->status = 4;
    std::vector<double> H((size_t)(mem + 1) * mem), g(mem + 1), cs(mem), sn(mem), yk(mem);
    while (!solved && !breakdown && it < itmax) {
        ++stats->npass;
        axpby(c, V, 1.0 / beta, V, 0.0, n);
        std::fill(g.begin(), g.end(), 0.0);
        g[0] = beta;
        int k = 0;
        for (int j = 0; j < mem && it < itmax; ++j) {
            double *vj = V + (size_t)j * ld, *zj = Z + (size_t)j * ld, *w = V + (size_t)(j + 1) * ld;
            if (pc) {
                if ((rc = precond_apply_raw(pc, vj, zj))) return rc;
            } else {
                axpby(c, zj, 1.0, vj, 0.0, n);
            }
            if (dh && (rc = halo_exchange_raw(dh, zj))) return rc;
            if ((rc = spmv_raw(A, zj, w, 1.0, 0.0))) return rc;
            const int kk = j + 1;
            // classical Gram-Schmidt, two full passes; everything the host needs arrives in one copy
            for (int pass = 0; pass < 2; ++pass) {
                double *hd = ws->dsc + 32 * pass;
                by_groups(kk, [&](auto ng) {
                    hipLaunchKernelGGL(k_mdot<decltype(ng)::value>, dim3(grid), dim3(kBlock), 0, st, V, ld, kk, w, n, ws->part);
                });
                hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(kBlock), 0, st, ws->part, grid, kk, hd);
                if (dh && (rc = allreduce_sum_device(c, hd, kPartStride))) return rc;
                by_groups(kk, [&](auto ng) {
                    hipLaunchKernelGGL(k_mupdate<decltype(ng)::value>, dim3(grid), dim3(kBlock), 0, st, V, ld, kk, hd, w, n,
                                       ws->part);
                });
            }
            hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(kBlock), 0, st, ws->part, grid, 1, ws->dsc + 64);
            if (dh && (rc = allreduce_sum_device(c, ws->dsc + 64, kPartStride))) return rc;
            NPG_HIP(hipMemcpyAsync(ws->hsc.get(), ws->dsc, 65 * sizeof(double), hipMemcpyDeviceToHost, st));
            NPG_HIP(hipStreamSynchronize(st));
            double *Hj = &H[(size_t)j * (mem + 1)];          // column j
            for (int i = 0; i < kk; ++i) Hj[i] = ws->hsc[i] + ws->hsc[32 + i];
            const double hn = std::sqrt(std::max(0.0, ws->hsc[64]));
            NPG_REQUIRE(std::isfinite(hn), "npg_fgmres_solve: non-finite Arnoldi vector at iteration %lld", (long long)it);
            Hj[kk] = hn;
            for (int i = 0; i < j; ++i) {
                const double t = cs[i] * Hj[i] + sn[i] * Hj[i + 1];
                Hj[i + 1] = -sn[i] * Hj[i] + cs[i] * Hj[i + 1];
                Hj[i] = t;
            }
            const double d = std::hypot(Hj[j], Hj[j + 1]);
            cs[j] = d > 0 ? Hj[j] / d : 1.0;
            sn[j] = d > 0 ? Hj[j + 1] / d : 0.0;
            Hj[j] = d;
            Hj[j + 1] = 0.0;
            g[j + 1] = -sn[j] * g[j];
            g[j] = cs[j] * g[j];
            ++it;
            k = j + 1;
            const double rn = scale * std::fabs(g[j + 1]);
            ws->hist.push_back(rn);
            stats->rnorm = rn;
            if (rn <= eps) break;
            if (hn <= 1e-300 || d == 0.0) { breakdown = true; break; }
            axpby(c, w, 1.0 / hn, w, 0.0, n);
        }
        // x += Z y,  H y = g (upper triangular, columns stored with stride mem + 1)
        for (int i = k - 1; i >= 0; --i) {
            double s = g[i];
            for (int jj = i + 1; jj < k; ++jj) s -= H[(size_t)jj * (mem + 1) + i] * yk[jj];
            const double piv = H[(size_t)i * (mem + 1) + i];
            yk[i] = piv != 0.0 ? s / piv : 0.0;
        }
        Coefs cf{};
        for (int i = 0; i < k; ++i) cf.y[i] = yk[i];
        if (k > 0) hipLaunchKernelGGL(k_combine_z, dim3(grid), dim3(kBlock), 0, st, x->d, Z, ld, k, cf, n);
        // true residual: the next pass starts from it, and a pass that met the estimate is confirmed by it
        {
            if (dh && (rc = halo_exchange_raw(dh, x->d))) return rc;
            SpmvEpi e{};
            e.alpha = -1.0; e.beta = 1.0; e.c = y->d; e.y = V;
            if ((rc = spmv_epi(A, x->d, e))) return rc;
        }
        if ((rc = reduce_dot(c, V, V, n, &dd)) || (rc = all_sum(&dd))) return rc;
        beta = std::sqrt(dd);
        stats->rnorm = scale * beta;
        solved = stats->rnorm <= eps;
        if (beta == 0.0) break;
    }
    NPG_HIP(hipGetLastError());
    NPG_HIP(hipEventRecord(e1, st));
    NPG_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    NPG_HIP(hipEventElapsedTime(&ms, e0, e1));
    stats->seconds = ms * 1e-3;
    stats->solved = solved ? 1 : 0;
    stats->niter = (int32_t)it;
    if (stats->status == 0) stats->status = solved ? 1 : breakdown ? 3 : 2;
    return NPG_OK;
}
