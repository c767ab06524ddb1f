// The explicit dense inverse: A^-1 of a small saddle-point system as a dense array in HBM, built once by rocSOLVER and applied by
// a hand-written split-column GEMV.  Two users (precond.h): the NPG_PC_DENSE kind of npg_precond (npg_precond_dense_set), where the
// whole inversion is one GEMV behind flexible GMRES on the small meshes, and the multigrid's exact coarsest-level solve
// (npg_precond_mg_set_coarse_dense, mg.hip).  The inverse is held in fp64, rounded to fp32, or - the coarse solve only - in fp16
// with every column scaled by its largest magnitude, accepted only where two probe vectors say the rounding is harmless.
#include <rocsolver/rocsolver.h>

#include <cmath>

#include "precond.h"
#include "device_utils.h"

namespace npg {

// ---- explicit dense inverse (NPG_PC_DENSE) ----------------------------------------------------------------------------------
// dA (column-major n x n, zero-filled) <- CSR
__global__ void k_densify(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const double *__restrict__ val,
                          int64_t n, double *__restrict__ dA) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x)
        for (int64_t k = rowptr[r]; k < rowptr[r + 1]; ++k) dA[r + (int64_t)col[k] * n] = val[k];
}

// M (column-major n x n, zero-filled) <- I
__global__ void k_unit_diagonal(double *__restrict__ M, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) M[i + i * n] = 1.0;
}

// part[s][i] = sum over the s-th chunk of columns j of M[i + j n] x[j]: thread = row i, consecutive lanes read consecutive
// doubles of one column (coalesced), eight columns in flight per thread; blockIdx.y = chunk
constexpr int kGemvChunkCols = 512;
template <typename T>
__global__ void __launch_bounds__(kBlock) k_dense_gemv_part(const T *__restrict__ M, int64_t n,
                                                            const double *__restrict__ x, double *__restrict__ part) {
    __shared__ double xs[kGemvChunkCols];
    const int64_t j0 = (int64_t)blockIdx.y * kGemvChunkCols;
    const int nj = (int)min((int64_t)kGemvChunkCols, n - j0);
    for (int j = threadIdx.x; j < nj; j += kBlock) xs[j] = x[j0 + j];
    __syncthreads();
    const int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    if (i >= n) return;
    const T *__restrict__ Mi = M + i + j0 * n;
    double acc = 0.0;
    int j = 0;
    for (; j + 8 <= nj; j += 8) {
        T v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = __builtin_nontemporal_load(Mi + (int64_t)(j + u) * n);
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += (double)v[u] * xs[j + u];
    }
    for (; j < nj; ++j) acc += (double)Mi[(int64_t)j * n] * xs[j];
    part[(int64_t)blockIdx.y * n + i] = acc;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 nt_load4(const float *p) {
    const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}

// fp32 inverse with a padded leading dimension (ld = n rounded up to 4 floats: every column starts 16-byte aligned): thread =
// FOUR adjacent rows (one 16-byte load per column), four columns per trip and the next trip's loads issued before this trip's
// arithmetic (the pattern that took the Krylov row kernels from 3.9 to 5.5 TB/s: profiles/r03_rows_bench.txt)
__global__ void __launch_bounds__(kBlock) k_dense_gemv_part4(const float *__restrict__ M, int64_t n, int64_t ld,
                                                             const double *__restrict__ x, double *__restrict__ part) {
    __shared__ double xs[kGemvChunkCols];
    const int64_t j0 = (int64_t)blockIdx.y * kGemvChunkCols;
    const int nj = (int)min((int64_t)kGemvChunkCols, n - j0);
    for (int j = threadIdx.x; j < nj; j += kBlock) xs[j] = x[j0 + j];
    __syncthreads();
    const int64_t i = 4 * (blockIdx.x * (int64_t)kBlock + threadIdx.x);
    if (i >= n) return;
    const float *__restrict__ Mi = M + i + j0 * ld;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    constexpr int U = 4;
    float4 v[U], vn[U];
    const int ntrip = nj / U;                        // whole trips; the tail columns one by one below
#pragma unroll
    for (int u = 0; u < U; ++u)
        if (ntrip > 0) v[u] = nt_load4(Mi + (int64_t)u * ld);
    for (int tr = 0; tr < ntrip; ++tr) {
        const int j = tr * U;
        if (tr + 1 < ntrip) {
#pragma unroll
            for (int u = 0; u < U; ++u) vn[u] = nt_load4(Mi + (int64_t)(j + U + u) * ld);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const double xv = xs[j + u];
            a0 += (double)v[u].x * xv;
            a1 += (double)v[u].y * xv;
            a2 += (double)v[u].z * xv;
            a3 += (double)v[u].w * xv;
        }
        if (tr + 1 < ntrip) {
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = vn[u];
        }
    }
    for (int j = ntrip * U; j < nj; ++j) {
        const float4 f = *reinterpret_cast<const float4 *>(Mi + (int64_t)j * ld);
        const double xv = xs[j];
        a0 += (double)f.x * xv;
        a1 += (double)f.y * xv;
        a2 += (double)f.z * xv;
        a3 += (double)f.w * xv;
    }
    double *out = part + (int64_t)blockIdx.y * n + i;          // (rows past n are padding of M: computed, not stored)
    out[0] = a0;
    if (i + 1 < n) out[1] = a1;
    if (i + 2 < n) out[2] = a2;
    if (i + 3 < n) out[3] = a3;
}

// fp16 inverse, every column scaled by its largest magnitude (cs[j]; the scale is folded into x when the chunk of x is staged):
// thread = EIGHT adjacent rows (one 16-byte load per column), the same four-columns-per-trip pipeline; products and the sums
// over a chunk's 512 columns in fp32 (the stored numbers carry 11 bits), the sum over the chunks in fp64 (k_dense_gemv_sum)
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ f16x8 nt_load8h(const _Float16 *p) {
    const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(p));
    return __builtin_bit_cast(f16x8, v);
}
__global__ void __launch_bounds__(kBlock) k_dense_gemv_part8h(const _Float16 *__restrict__ M, int64_t n, int64_t ld,
                                                              const double *__restrict__ cs, const double *__restrict__ x,
                                                              double *__restrict__ part) {
    __shared__ float xs[kGemvChunkCols];
    const int64_t j0 = (int64_t)blockIdx.y * kGemvChunkCols;
    const int nj = (int)min((int64_t)kGemvChunkCols, n - j0);
    for (int j = threadIdx.x; j < nj; j += kBlock) xs[j] = (float)(x[j0 + j] * cs[j0 + j]);
    __syncthreads();
    const int64_t i = 8 * (blockIdx.x * (int64_t)kBlock + threadIdx.x);
    if (i >= n) return;
    const _Float16 *__restrict__ Mi = M + i + j0 * ld;
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    constexpr int U = 4;
    f16x8 v[U], vn[U];
    const int ntrip = nj / U;
#pragma unroll
    for (int u = 0; u < U; ++u)
        if (ntrip > 0) v[u] = nt_load8h(Mi + (int64_t)u * ld);
    for (int tr = 0; tr < ntrip; ++tr) {
        const int j = tr * U;
        if (tr + 1 < ntrip) {
#pragma unroll
            for (int u = 0; u < U; ++u) vn[u] = nt_load8h(Mi + (int64_t)(j + U + u) * ld);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float xv = xs[j + u];
#pragma unroll
            for (int k = 0; k < 8; ++k) a[k] = __builtin_fmaf((float)v[u][k], xv, a[k]);
        }
        if (tr + 1 < ntrip) {
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = vn[u];
        }
    }
    for (int j = ntrip * U; j < nj; ++j) {
        const f16x8 f = *reinterpret_cast<const f16x8 *>(Mi + (int64_t)j * ld);
        const float xv = xs[j];
#pragma unroll
        for (int k = 0; k < 8; ++k) a[k] = __builtin_fmaf((float)f[k], xv, a[k]);
    }
    double *out = part + (int64_t)blockIdx.y * n + i;          // (rows past n are padding of M: computed, not stored)
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (i + k < n) out[k] = (double)a[k];
}

// cs[j] = max_i |M[i, j]| of a column-major fp64 n x n array (1 for an all-zero column): one workgroup per column
__global__ void __launch_bounds__(kBlock) k_col_absmax(const double *__restrict__ M, int64_t n, double *__restrict__ cs) {
    __shared__ double sh[kBlock];
    for (int64_t j = blockIdx.x; j < n; j += gridDim.x) {
        double m = 0.0;
        for (int64_t i = threadIdx.x; i < n; i += kBlock) m = fmax(m, fabs(M[j * n + i]));
        sh[threadIdx.x] = m;
        __syncthreads();
        for (int s = kBlock / 2; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + s]);
            __syncthreads();
        }
        if (threadIdx.x == 0) cs[j] = sh[0] > 0.0 ? sh[0] : 1.0;
        __syncthreads();
    }
}

// fp64 column-major n x n -> fp16 with leading dimension ld >= n, column j divided by cs[j] (pad rows zeroed)
__global__ void k_to_half_ld(const double *__restrict__ src, const double *__restrict__ cs, _Float16 *__restrict__ dst, int64_t n,
                             int64_t ld) {
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < ld * n; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = k / ld, i = k - j * ld;
        dst[k] = i < n ? (_Float16)(float)(src[j * n + i] / cs[j]) : (_Float16)0.f;
    }
}

// fp64 column-major n x n -> fp32 with leading dimension ld >= n (pad rows zeroed)
__global__ void k_to_float_ld(const double *__restrict__ src, float *__restrict__ dst, int64_t n, int64_t ld) {
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < ld * n; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = k / ld, i = k - j * ld;
        dst[k] = i < n ? (float)src[j * n + i] : 0.f;
    }
}

// z = a (sum_s part[s]) + b z   (fixed order)
__global__ void __launch_bounds__(kBlock) k_dense_gemv_sum(const double *__restrict__ part, int nsplit, int64_t n, double a,
                                                           double b, double *__restrict__ z) {
    const int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int k = 0; k < nsplit; ++k) s += part[(int64_t)k * n + i];
    z[i] = (b == 0.0) ? a * s : a * s + b * z[i];
}

// z = a A^-1 r + b z, the inverse read from the storage `from` (the one d holds, except while the build compares two)
int dense_apply(npg_ctx *ctx, const DenseInv &d, DenseStorage from, const double *r, double *z, double a, double b) {
    hipStream_t st = ctx->stream;
    if (byte_sink)          // the inverse in the storage that is read, + the split-column partial sums written and re-read, + r, z
        *byte_sink += (from == kDenseF16 ? 2 * d.n * d.ldf : from == kDenseF32 ? 4 * d.n * d.ldf : 8 * d.n * d.n) +
                      16 * (int64_t)d.nsplit * d.n + 24 * d.n;
    const int gx = (int)((d.n + kBlock - 1) / kBlock);
    if (from == kDenseF16)
        hipLaunchKernelGGL(k_dense_gemv_part8h, dim3((unsigned)((d.n + 8 * kBlock - 1) / (8 * kBlock)), d.nsplit), dim3(kBlock), 0, st,
                           (const _Float16 *)d.Mh.p, d.n, d.ldf, (const double *)d.cs.p, r, d.part.p);
    else if (from == kDenseF32)
        hipLaunchKernelGGL(k_dense_gemv_part4, dim3((unsigned)((d.n + 4 * kBlock - 1) / (4 * kBlock)), d.nsplit), dim3(kBlock), 0, st,
                           (const float *)d.Mf.p, d.n, d.ldf, r, d.part.p);
    else
        hipLaunchKernelGGL(k_dense_gemv_part<double>, dim3(gx, d.nsplit), dim3(kBlock), 0, st, d.M.p, d.n, r, d.part.p);
    hipLaunchKernelGGL(k_dense_gemv_sum, dim3(gx), dim3(kBlock), 0, st, d.part.p, d.nsplit, d.n, a, b, z);
    NPG_HIP(hipGetLastError());
    return NPG_OK;
}

// d.Mf <- d.M rounded to fp32 with the padded leading dimension
static int dense_round_fp32(hipStream_t st, DenseInv &d) {
    const int64_t n = d.n;
    d.ldf = (n + 3) / 4 * 4;
    NPG_HIP(d.Mf.alloc((size_t)d.ldf * n));
    hipLaunchKernelGGL(k_to_float_ld, dim3(4096), dim3(kBlock), 0, st, d.M.p, d.Mf.p, n, d.ldf);
    NPG_HIP(hipGetLastError());
    NPG_HIP(hipStreamSynchronize(st));
    return NPG_OK;
}

// Column scaling keeps every column's largest entry exact, but rows of very different magnitude within one column (velocity
// against pressure rows of a Stokes inverse differ by alpha^2 eps^2) may fall below fp16's range and flush to zero: what the
// rounded inverse does to two probe vectors is compared, row by row, with the fp64 inverse while both are in memory; if the
// typical row is off by more than fp16's rounding explains, or any sizeable row is lost, the fp32 storage is taken instead
// (ADVICE round 4).  NPG_MG_COARSE_FP16_CHECK=0 skips the check.
static int dense_fp16_acceptable(npg_ctx *ctx, const DenseInv &d, bool *keep16) {
    static const bool check16 = !getenv("NPG_MG_COARSE_FP16_CHECK") || atoi(getenv("NPG_MG_COARSE_FP16_CHECK")) != 0;
    *keep16 = true;
    if (!check16) return NPG_OK;
    hipStream_t st = ctx->stream;
    const int64_t n = d.n;
    DevBuf<double> rv;
    NPG_HIP(rv.alloc(3 * (size_t)n));
    double *y64 = rv.p + n, *y16 = y64 + n;
    std::vector<double> h((size_t)n), a((size_t)n), b((size_t)n);
    for (int probe = 0; probe < 2 && *keep16; ++probe) {
        for (int64_t i = 0; i < n; ++i)
            h[(size_t)i] = probe == 0 ? std::sin(0.37 * (double)i) + 0.5 : ((i * 2654435761u) & 64 ? 1.0 : -1.0) * (1.0 + (double)(i % 7));
        NPG_HIP(hipMemcpy(rv.p, h.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice));
        int rc;
        if ((rc = dense_apply(ctx, d, kDenseF64, rv.p, y64, 1.0, 0.0)) ||        // fp64 inverse
            (rc = dense_apply(ctx, d, kDenseF16, rv.p, y16, 1.0, 0.0)))          // column-scaled fp16 inverse
            return rc;
        NPG_HIP(hipMemcpyAsync(a.data(), y64, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
        NPG_HIP(hipMemcpyAsync(b.data(), y16, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
        NPG_HIP(hipStreamSynchronize(st));
        double amax = 0.0;
        for (double v : a) amax = std::max(amax, std::fabs(v));
        std::vector<double> rel;
        rel.reserve((size_t)n);
        for (int64_t i = 0; i < n; ++i)
            if (std::fabs(a[(size_t)i]) > 1e-8 * amax) rel.push_back(std::fabs(b[(size_t)i] - a[(size_t)i]) / std::fabs(a[(size_t)i]));
        if (rel.empty()) continue;
        std::sort(rel.begin(), rel.end());
        const double med = rel[rel.size() / 2], p99 = rel[(size_t)(0.99 * (double)(rel.size() - 1))];
        if (!(med <= 5e-3 && p99 <= 0.2)) {
            *keep16 = false;
            fprintf(stderr, "[npg mg] coarsest level: the column-scaled fp16 inverse differs from the fp64 one by %.1e (median row) / "
                            "%.1e (99th percentile) on a probe vector - fp32 storage instead\n", med, p99);
        }
    }
    return NPG_OK;
}

// A^-1 of a plain-CSR matrix as a dense fp64 array in HBM: densify, LU with partial pivoting and the solve against the identity
// by rocSOLVER (set-up; n^2 doubles - 2 GB at 16 k unknowns, 8 GB at 31 k - and as many again while it runs), applied per solve
// by the hand-written GEMV above.  d is a fresh DenseInv of the caller's: whatever an early return leaves in it goes with it.
static int dense_build_raw(npg_ctx *ctx, DenseInv &d, const npg_csr *A, bool fp32, bool fp16) {
    NPG_REQUIRE(A && A->m == A->n && A->nnode() == 0, "dense inverse: a square plain-CSR matrix is required");
    const int64_t n = A->m;
    // (46 340 = floor(sqrt(2^31)): rocSOLVER's getrf addresses the n x n array with 32-bit element offsets - at 58 295 unknowns,
    //  the channel basin's coarsest level, they fault; round 5, profiles/r05_coarse_viscosity.txt)
    NPG_REQUIRE(n > 0 && n <= 46340, "dense inverse: %lld unknowns (limit 46 340: rocSOLVER's getrf / getrs index the n x n array with 32-bit offsets)",
                (long long)n);
    hipStream_t st = ctx->stream;
    d.n = n;
    d.nsplit = (int)((n + kGemvChunkCols - 1) / kGemvChunkCols);
    NPG_HIP(d.M.alloc((size_t)n * n));
    NPG_HIP(d.part.alloc((size_t)d.nsplit * n));
    NPG_HIP(hipMemsetAsync(d.M.p, 0, (size_t)n * n * sizeof(double), st));
    hipLaunchKernelGGL(k_densify, dim3(grid_for(n)), dim3(kBlock), 0, st, A->rowptr, A->col, A->val, n, d.M.p);
    NPG_HIP(hipGetLastError());
    struct Guard {                       // every early return below releases the handle
        rocblas_handle h = nullptr;
        ~Guard() {
            if (h) rocblas_destroy_handle(h);
        }
    } guard;
    NPG_REQUIRE(rocblas_create_handle(&guard.h) == rocblas_status_success, "dense inverse: rocblas_create_handle failed");
    rocblas_handle h = guard.h;
    rocblas_set_stream(h, st);
    DevBuf<rocblas_int> ipiv, info;
    NPG_HIP(ipiv.alloc((size_t)n));
    NPG_HIP(info.alloc(1));
    rocblas_status s1 = rocsolver_dgetrf(h, (rocblas_int)n, (rocblas_int)n, d.M.p, (rocblas_int)n, ipiv.p, info.p);
    rocblas_int i1 = -1, i2 = -1;
    NPG_HIP(hipMemcpyAsync(&i1, info.p, sizeof i1, hipMemcpyDeviceToHost, st));
    NPG_HIP(hipStreamSynchronize(st));
    rocblas_status s2 = rocblas_status_success;
    if (s1 == rocblas_status_success && i1 == 0) {
        // A^-1 = the solution of L U X = P I by getrs, not getri: rocSOLVER 3.32's dgetri returned a wrong inverse at n = 255 and
        // n = 511 (the first (n + 1) / 2 columns, |A X - I| = 1, info = 0; right at 256, 257, 512, 513 -
        // profiles/dense_inverse_getri.txt, tests/test_gpu_dense_inverse.py).  The factors stay in d.M until the solve is
        // done: 2 n^2 doubles at the peak.
        DevBuf<double> X;
        NPG_HIP(X.alloc((size_t)n * n));
        NPG_HIP(hipMemsetAsync(X.p, 0, (size_t)n * n * sizeof(double), st));
        hipLaunchKernelGGL(k_unit_diagonal, dim3(grid_for(n)), dim3(kBlock), 0, st, X.p, n);
        NPG_HIP(hipGetLastError());
        s2 = rocsolver_dgetrs(h, rocblas_operation_none, (rocblas_int)n, (rocblas_int)n, d.M.p, (rocblas_int)n, ipiv.p, X.p, (rocblas_int)n);
        NPG_HIP(hipStreamSynchronize(st));
        i2 = 0;                               // (getrs reports through its status alone)
        if (s2 == rocblas_status_success) d.M.swap(X);      // X goes with the factors - or, after a failure, the unfinished inverse
    }
    NPG_REQUIRE(s1 == rocblas_status_success && i1 == 0 && s2 == rocblas_status_success && i2 == 0,
                "dense inverse: rocSOLVER getrf/getrs failed (status %d/%d, info %d/%d: the matrix is singular to working "
                "precision, or out of memory)", (int)s1, (int)s2, (int)i1, (int)i2);
    d.held = kDenseF64;
    int rc;
    if (fp16) {
        d.ldf = (n + 7) / 8 * 8;
        NPG_HIP(d.cs.alloc((size_t)n));
        NPG_HIP(d.Mh.alloc((size_t)d.ldf * n));
        hipLaunchKernelGGL(k_col_absmax, dim3((unsigned)std::min<int64_t>(n, 4096)), dim3(kBlock), 0, st, d.M.p, n, d.cs.p);
        hipLaunchKernelGGL(k_to_half_ld, dim3(4096), dim3(kBlock), 0, st, d.M.p, d.cs.p, d.Mh.p, n, d.ldf);
        NPG_HIP(hipGetLastError());
        NPG_HIP(hipStreamSynchronize(st));
        bool keep16 = true;
        if ((rc = dense_fp16_acceptable(ctx, d, &keep16))) return rc;
        if (!keep16) {
            d.Mh.reset();
            d.cs.reset();
            if ((rc = dense_round_fp32(st, d))) return rc;
        }
        d.M.reset();
        d.held = keep16 ? kDenseF16 : kDenseF32;
    } else if (fp32) {
        if ((rc = dense_round_fp32(st, d))) return rc;
        d.M.reset();
        d.held = kDenseF32;
    }
    return NPG_OK;
}

// ... and a build that failed leaves no inverse behind: not the factors, not a half-written array, not the previous inverse - an
// application afterwards is refused ("has not been set") instead of multiplying by them.  (The previous inverse is released
// before the build, not after it: the build's own peak is 2 n^2 doubles.)
int dense_build(npg_ctx *ctx, DenseInv &d, const npg_csr *A, bool fp32, bool fp16) {
    dense_free(d);
    DenseInv fresh;
    const int rc = dense_build_raw(ctx, fresh, A, fp32, fp16);
    if (!rc) d = std::move(fresh);
    return rc;
}

}  // namespace npg

using namespace npg;

NPG_API int npg_precond_dense_set(npg_precond *pc, const npg_csr *A, int fp32_storage) {
    NPG_REQUIRE(pc && pc->kind == NPG_PC_DENSE, "npg_precond_dense_set: not a dense-inverse preconditioner");
    int rc = dense_build(pc->ctx, pc->dense, A, fp32_storage != 0);
    if (rc) return rc;
    pc->n = A->m;
    pc->cycle_bytes = 0;       // counted again by the next application: the storage may have changed
    return NPG_OK;
}
