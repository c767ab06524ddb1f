// libnupgcm_host.so - the C ABI of include/nupgcm_hip.h on the HOST (plain C++17 + OpenMP, no HIP), for the reference's CPU()
// architecture (BASELINE.json configs[0]: "bowl3D h = 0.1 mesh, CPU() architecture, 5 timesteps of bowl_mixing - plumbing, runs
// without a GPU"; /root/reference/src/architectures.jl:4-20, src/iterative_solvers.jl:42-58).
//
// What it is: the subset of the entry points that nupgcm_amd's Model(CPU(), ...) drives - context, vectors, plain-CSR matrices,
// SpMV, the element kernels of the path (src/inversion.jl:133-249, src/evolution.jl:209-296, src/model.jl:269-300,
// src/inputs.jl:87-137, src/timesteppers.jl:108-119) and Krylov.jl's restarted GMRES / CG for the sizes and closures where the
// reference's CPU() path iterates instead of factorising (src/iterative_solvers.jl:58).  Same names, argument meaning and
// error behaviour as the HIP library; handles are host memory.  The sparse LU the reference's CPU() path uses wherever it can
// (lu(A) + ldiv!, src/inversion.jl:55-58, src/evolution.jl:150-153) is a LIBRARY there too (UMFPACK): the Python host calls
// SuperLU through scipy for it (nupgcm_amd/iterative_solvers.py).
//
// What it is not: the oracle (oracle/ is numpy test infrastructure; nothing here derives from it) and not a fallback for GPU() -
// a process runs on one architecture, chosen explicitly (nupgcm_amd/_lib.py: select("host") through npg.CPU()).
//
// The element integrals restate csrc/fe.hip statement by statement in scalar loops: same tables, same order of the sums over
// quadrature points and over the cells of a row (row-owner assembly through the inverted index), so the host matrices agree with
// the device's to rounding and repeat bit for bit from run to run whatever OMP_NUM_THREADS is.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <omp.h>
#include <unistd.h>

#include "../../include/nupgcm_hip.h"
#include "../csrc/cell_view.h"
#include "../csrc/tangent_core.h"
#include "../csrc/tangent_adjoint_core.h"
#include "../csrc/tangent_closures_core.h"

#define NPG_API extern "C" __attribute__((visibility("default")))

namespace {
thread_local std::string g_err;
void set_error(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
}
#define REQUIRE(cond, ...)          \
    do {                            \
        if (!(cond)) {              \
            set_error(__VA_ARGS__); \
            return NPG_EINVAL;      \
        }                           \
    } while (0)
// report the message of a shared argument check (the csrc/*_core.h check_* functions; empty: fine)
#define REQUIRE_OK(msg)                            \
    do {                                           \
        const std::string m_ = (msg);              \
        REQUIRE(m_.empty(), "%s", m_.c_str());     \
    } while (0)
}  // namespace

struct npg_ctx {
    std::chrono::steady_clock::time_point t0;
};
struct npg_vec {
    npg_ctx *ctx = nullptr;
    int64_t n = 0;
    double *d = nullptr;
    bool owns = true;
};
struct npg_csr {
    npg_ctx *ctx = nullptr;
    int64_t m = 0, n = 0, nnz = 0;
    std::vector<int64_t> rowptr;
    std::vector<int32_t> col;
    std::vector<double> val;
};

// ---- context -----------------------------------------------------------------------------------------------------------------
NPG_API const char *npg_last_error(void) { return g_err.c_str(); }
NPG_API int npg_ctx_create(int device, npg_ctx **out) {
    REQUIRE(out, "npg_ctx_create: NULL argument");
    (void)device;                       // the host has one "device"
    *out = new npg_ctx();
    return NPG_OK;
}
NPG_API int npg_ctx_destroy(npg_ctx *ctx) {
    delete ctx;
    return NPG_OK;
}
NPG_API int npg_ctx_sync(npg_ctx *) { return NPG_OK; }
NPG_API void *npg_ctx_stream(npg_ctx *) { return nullptr; }
NPG_API int npg_mem_status(npg_ctx *ctx, size_t *free_bytes, size_t *total_bytes) {
    REQUIRE(ctx && free_bytes && total_bytes, "npg_mem_status: NULL argument");
    const size_t page = (size_t)sysconf(_SC_PAGESIZE);
    *total_bytes = page * (size_t)sysconf(_SC_PHYS_PAGES);
    *free_bytes = page * (size_t)sysconf(_SC_AVPHYS_PAGES);
    return NPG_OK;
}
NPG_API int npg_device_name(npg_ctx *ctx, char *buf, size_t cap) {
    REQUIRE(ctx && buf && cap > 0, "npg_device_name: bad argument");
    snprintf(buf, cap, "host CPU (libnupgcm_host, %d OpenMP threads)", omp_get_max_threads());
    return NPG_OK;
}
NPG_API int npg_timer_start(npg_ctx *ctx) {
    REQUIRE(ctx, "npg_timer_start: NULL context");
    ctx->t0 = std::chrono::steady_clock::now();
    return NPG_OK;
}
NPG_API int npg_timer_stop(npg_ctx *ctx, double *ms) {
    REQUIRE(ctx && ms, "npg_timer_stop: NULL argument");
    *ms = 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - ctx->t0).count();
    return NPG_OK;
}

// ---- vectors -----------------------------------------------------------------------------------------------------------------
NPG_API int npg_vec_create(npg_ctx *ctx, int64_t n, npg_vec **out) {
    REQUIRE(ctx && out && n >= 0, "npg_vec_create: bad argument");
    npg_vec *v = new npg_vec();
    v->ctx = ctx;
    v->n = n;
    v->d = (double *)calloc((size_t)std::max<int64_t>(n, 1), sizeof(double));
    if (!v->d) {
        delete v;
        set_error("npg_vec_create: out of memory (%lld doubles)", (long long)n);
        return NPG_ENOMEM;
    }
    *out = v;
    return NPG_OK;
}
NPG_API int npg_vec_destroy(npg_vec *v) {
    if (!v) return NPG_OK;
    if (v->owns) free(v->d);
    delete v;
    return NPG_OK;
}
NPG_API int npg_vec_view(npg_vec *v, int64_t offset, int64_t n, npg_vec **out) {
    REQUIRE(v && out && offset >= 0 && n >= 0 && offset + n <= v->n, "npg_vec_view: window out of range");
    npg_vec *w = new npg_vec();
    w->ctx = v->ctx;
    w->n = n;
    w->d = v->d + offset;
    w->owns = false;
    *out = w;
    return NPG_OK;
}
NPG_API int64_t npg_vec_len(const npg_vec *v) { return v ? v->n : -1; }
NPG_API int npg_vec_upload(npg_vec *v, const double *host) {
    REQUIRE(v && host, "npg_vec_upload: NULL argument");
    memcpy(v->d, host, (size_t)v->n * sizeof(double));
    return NPG_OK;
}
NPG_API int npg_vec_download(const npg_vec *v, double *host) {
    REQUIRE(v && host, "npg_vec_download: NULL argument");
    memcpy(host, v->d, (size_t)v->n * sizeof(double));
    return NPG_OK;
}
// v[i] = host[perm[i]]   /   host[i] = v[perm[i]]        (as the HIP library: the gathers of src/model.jl:274-275,282,312)
NPG_API int npg_vec_upload_perm(npg_vec *v, const double *host, const int64_t *perm) {
    REQUIRE(v && host && perm, "npg_vec_upload_perm: NULL argument");
    for (int64_t i = 0; i < v->n; ++i) v->d[i] = host[perm[i]];
    return NPG_OK;
}
NPG_API int npg_vec_download_perm(const npg_vec *v, double *host, const int64_t *perm) {
    REQUIRE(v && host && perm, "npg_vec_download_perm: NULL argument");
    for (int64_t i = 0; i < v->n; ++i) {
        REQUIRE(perm[i] >= 0 && perm[i] < v->n, "npg_vec_download_perm: index out of range");
        host[i] = v->d[perm[i]];
    }
    return NPG_OK;
}
NPG_API int npg_vec_fill(npg_vec *v, double a) {
    REQUIRE(v, "npg_vec_fill: NULL vector");
    std::fill(v->d, v->d + v->n, a);
    return NPG_OK;
}
NPG_API int npg_vec_copy(npg_vec *dst, const npg_vec *src) {
    REQUIRE(dst && src && dst->n == src->n, "npg_vec_copy: length mismatch");
    if (dst->d != src->d) memmove(dst->d, src->d, (size_t)dst->n * sizeof(double));
    return NPG_OK;
}
NPG_API int npg_vec_axpby(npg_vec *y, double a, const npg_vec *x, double b) {
    REQUIRE(y && x && y->n == x->n, "npg_vec_axpby: length mismatch");
    const int64_t n = y->n;
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; ++i) y->d[i] = a * x->d[i] + (b == 0.0 ? 0.0 : b * y->d[i]);
    return NPG_OK;
}
static double dot_fixed(const double *x, const double *y, int64_t n) {
    // fixed blocking (independent of the thread count): bit-reproducible whatever OMP_NUM_THREADS is
    constexpr int64_t B = 4096;
    const int64_t nb = (n + B - 1) / B;
    std::vector<double> part((size_t)nb);
#pragma omp parallel for schedule(static)
    for (int64_t b = 0; b < nb; ++b) {
        double s = 0.0;
        for (int64_t i = b * B; i < std::min(n, (b + 1) * B); ++i) s += x[i] * y[i];
        part[(size_t)b] = s;
    }
    double s = 0.0;
    for (double p : part) s += p;
    return s;
}
NPG_API int npg_vec_dot(const npg_vec *x, const npg_vec *y, double *out) {
    REQUIRE(x && y && out && x->n == y->n, "npg_vec_dot: length mismatch");
    *out = dot_fixed(x->d, y->d, x->n);
    return NPG_OK;
}
NPG_API int npg_vec_nrm2(const npg_vec *x, double *out) {
    REQUIRE(x && out, "npg_vec_nrm2: NULL argument");
    *out = std::sqrt(dot_fixed(x->d, x->d, x->n));
    return NPG_OK;
}
NPG_API int npg_vec_maxabs(const npg_vec *x, double *out, int *has_nan) {
    REQUIRE(x && out, "npg_vec_maxabs: NULL argument");
    double m = 0.0;
    int nan = 0;
    for (int64_t i = 0; i < x->n; ++i) {
        const double a = std::fabs(x->d[i]);
        if (a != a) nan = 1;
        else m = std::max(m, a);
    }
    *out = m;
    if (has_nan) *has_nan = nan;
    return NPG_OK;
}
NPG_API int npg_vec_is_constant(const npg_vec *x, double *value, int *is_constant) {
    REQUIRE(x && value && is_constant && x->n > 0, "npg_vec_is_constant: bad argument");
    double lo = x->d[0], hi = x->d[0];
    for (int64_t i = 1; i < x->n; ++i) {
        lo = std::min(lo, x->d[i]);
        hi = std::max(hi, x->d[i]);
    }
    *value = lo;
    *is_constant = lo == hi;
    return NPG_OK;
}
NPG_API int npg_vec_lincomb(npg_vec *y, int nterms, const double *coef, const npg_vec *const *xs) {
    REQUIRE(y && nterms >= 1 && nterms <= 8 && coef && xs, "npg_vec_lincomb: 1 to 8 terms");
    for (int k = 0; k < nterms; ++k) REQUIRE(xs[k] && xs[k]->n == y->n, "npg_vec_lincomb: length mismatch in term %d", k);
    const int64_t n = y->n;
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; ++i) {
        double s = 0.0;
        for (int k = 0; k < nterms; ++k) s += coef[k] * xs[k]->d[i];
        y->d[i] = s;
    }
    return NPG_OK;
}
NPG_API int npg_vec_mul(npg_vec *y, const npg_vec *d, const npg_vec *x) {
    REQUIRE(y && d && x && y->n == d->n && y->n == x->n, "npg_vec_mul: length mismatch");
    for (int64_t i = 0; i < y->n; ++i) y->d[i] = d->d[i] * x->d[i];
    return NPG_OK;
}

// ---- CSR matrices ------------------------------------------------------------------------------------------------------------------
static int csr_check(int64_t m, int64_t n, const std::vector<int64_t> &rp, const std::vector<int32_t> &col, const char *who) {
    REQUIRE(rp.size() == (size_t)m + 1 && rp[0] == 0, "%s: bad row offsets", who);
    for (int64_t r = 0; r < m; ++r) {
        REQUIRE(rp[r] <= rp[r + 1], "%s: row offsets must not decrease", who);
        for (int64_t k = rp[r]; k < rp[r + 1]; ++k) {
            REQUIRE(col[k] >= 0 && col[k] < n, "%s: column index %d out of range in row %lld", who, col[k], (long long)r);
            REQUIRE(k == rp[r] || col[k - 1] < col[k], "%s: columns of row %lld are not strictly ascending", who, (long long)r);
        }
    }
    return NPG_OK;
}
NPG_API int npg_csr_create(npg_ctx *ctx, int64_t m, int64_t n, const int64_t *rowptr, const int32_t *colind, const double *val,
                           npg_csr **out) {
    REQUIRE(ctx && out && rowptr && m >= 0 && n >= 0 && n < INT32_MAX, "npg_csr_create: bad argument");
    npg_csr *A = new npg_csr();
    A->ctx = ctx;
    A->m = m;
    A->n = n;
    A->rowptr.assign(rowptr, rowptr + m + 1);
    A->nnz = rowptr[m];
    REQUIRE(A->nnz == 0 || colind, "npg_csr_create: NULL column array");
    A->col.assign(colind, colind + A->nnz);
    if (val) A->val.assign(val, val + A->nnz);
    else A->val.assign((size_t)A->nnz, 0.0);
    const int rc = csr_check(m, n, A->rowptr, A->col, "npg_csr_create");
    if (rc) {
        delete A;
        return rc;
    }
    *out = A;
    return NPG_OK;
}
NPG_API int npg_csr_create_from_csc(npg_ctx *ctx, int64_t m, int64_t n, const int64_t *colptr, const int64_t *rowval,
                                    const double *nzval, int drop_zeros, npg_csr **out) {
    REQUIRE(ctx && out && colptr && m >= 0 && n >= 0 && n < INT32_MAX, "npg_csr_create_from_csc: bad argument");
    const int64_t nz = colptr[n];
    REQUIRE(nz == 0 || (rowval && nzval), "npg_csr_create_from_csc: NULL arrays");
    npg_csr *A = new npg_csr();
    A->ctx = ctx;
    A->m = m;
    A->n = n;
    A->rowptr.assign((size_t)m + 1, 0);
    for (int64_t j = 0; j < n; ++j)
        for (int64_t k = colptr[j]; k < colptr[j + 1]; ++k) {
            if (rowval[k] < 0 || rowval[k] >= m) {
                delete A;
                set_error("npg_csr_create_from_csc: row index out of range");
                return NPG_EINVAL;
            }
            if (!drop_zeros || nzval[k] != 0.0) ++A->rowptr[(size_t)rowval[k] + 1];
        }
    for (int64_t r = 0; r < m; ++r) A->rowptr[r + 1] += A->rowptr[r];
    A->nnz = A->rowptr[m];
    A->col.resize((size_t)A->nnz);
    A->val.resize((size_t)A->nnz);
    std::vector<int64_t> next(A->rowptr.begin(), A->rowptr.end() - 1);
    for (int64_t j = 0; j < n; ++j)            // columns ascending => every row's entries arrive in ascending column order
        for (int64_t k = colptr[j]; k < colptr[j + 1]; ++k)
            if (!drop_zeros || nzval[k] != 0.0) {
                const int64_t s = next[(size_t)rowval[k]]++;
                A->col[(size_t)s] = (int32_t)j;
                A->val[(size_t)s] = nzval[k];
            }
    const int rc = csr_check(m, n, A->rowptr, A->col, "npg_csr_create_from_csc");
    if (rc) {
        delete A;
        return rc;
    }
    *out = A;
    return NPG_OK;
}
NPG_API int npg_csr_destroy(npg_csr *A) {
    delete A;
    return NPG_OK;
}
NPG_API int npg_csr_shape(const npg_csr *A, int64_t *m, int64_t *n, int64_t *nnz) {
    REQUIRE(A, "npg_csr_shape: NULL matrix");
    if (m) *m = A->m;
    if (n) *n = A->n;
    if (nnz) *nnz = A->nnz;
    return NPG_OK;
}
NPG_API int npg_csr_storage(const npg_csr *A, int64_t *nodes, int64_t *records, int64_t *csr_entries) {
    REQUIRE(A, "npg_csr_storage: NULL matrix");
    if (nodes) *nodes = 0;              // plain CSR only on the host
    if (records) *records = 0;
    if (csr_entries) *csr_entries = A->nnz;
    return NPG_OK;
}
NPG_API int npg_csr_spmv_bytes(const npg_csr *A, int64_t *matrix_bytes) {
    REQUIRE(A && matrix_bytes, "npg_csr_spmv_bytes: NULL argument");
    *matrix_bytes = 8 * (A->m + 1) + 12 * A->nnz;
    return NPG_OK;
}
NPG_API int npg_csr_block_nodes(npg_csr *A, int64_t, int64_t, double, int *blocked) {
    REQUIRE(A && blocked, "npg_csr_block_nodes: NULL argument");
    *blocked = 0;                       // the record layouts are HBM layouts: the host keeps plain CSR
    return NPG_OK;
}
NPG_API int npg_csr_download(const npg_csr *A, int64_t *rowptr, int32_t *colind, double *val) {
    REQUIRE(A, "npg_csr_download: NULL matrix");
    if (rowptr) memcpy(rowptr, A->rowptr.data(), A->rowptr.size() * sizeof(int64_t));
    if (colind && A->nnz) memcpy(colind, A->col.data(), (size_t)A->nnz * sizeof(int32_t));
    if (val && A->nnz) memcpy(val, A->val.data(), (size_t)A->nnz * sizeof(double));
    return NPG_OK;
}
NPG_API int npg_csr_to_csc(const npg_csr *A, int64_t *colptr, int64_t *rowval, double *nzval) {
    REQUIRE(A && colptr && (A->nnz == 0 || (rowval && nzval)), "npg_csr_to_csc: NULL argument");
    std::fill(colptr, colptr + A->n + 1, 0);
    for (int64_t k = 0; k < A->nnz; ++k) ++colptr[A->col[(size_t)k] + 1];
    for (int64_t j = 0; j < A->n; ++j) colptr[j + 1] += colptr[j];
    std::vector<int64_t> next(colptr, colptr + A->n);
    for (int64_t r = 0; r < A->m; ++r)
        for (int64_t k = A->rowptr[r]; k < A->rowptr[r + 1]; ++k) {
            const int64_t s = next[(size_t)A->col[(size_t)k]]++;
            rowval[s] = r;
            nzval[s] = A->val[(size_t)k];
        }
    return NPG_OK;
}
NPG_API int npg_csr_clone(const npg_csr *A, npg_csr **out) {
    REQUIRE(A && out, "npg_csr_clone: NULL argument");
    *out = new npg_csr(*A);
    return NPG_OK;
}
NPG_API int npg_csr_zero_values(npg_csr *A) {
    REQUIRE(A, "npg_csr_zero_values: NULL matrix");
    std::fill(A->val.begin(), A->val.end(), 0.0);
    return NPG_OK;
}
NPG_API int npg_csr_combine(npg_csr *out, double a, const npg_csr *X, double b, const npg_csr *Y, const npg_csr *Z) {
    REQUIRE(out && X && Y && Z, "npg_csr_combine: NULL argument");
    REQUIRE(out->nnz == X->nnz && X->nnz == Y->nnz && Y->nnz == Z->nnz && out->m == X->m && X->m == Y->m && Y->m == Z->m,
            "npg_csr_combine: operands must share one sparsity pattern");
    for (int64_t k = 0; k < out->nnz; ++k) out->val[(size_t)k] = a * X->val[(size_t)k] + b * (Y->val[(size_t)k] + Z->val[(size_t)k]);
    return NPG_OK;
}
NPG_API int npg_csr_axpy(npg_csr *out, double a, const npg_csr *X) {
    REQUIRE(out && X, "npg_csr_axpy: NULL argument");
    REQUIRE(out != X, "npg_csr_axpy: out must not be X");
    REQUIRE(out->ctx == X->ctx && out->nnz == X->nnz && out->m == X->m && out->n == X->n, "npg_csr_axpy: operands must share one sparsity pattern");
    for (int64_t k = 0; k < out->nnz; ++k) out->val[(size_t)k] = out->val[(size_t)k] + a * X->val[(size_t)k];
    return NPG_OK;
}
NPG_API int npg_csr_inv_diag(const npg_csr *A, npg_vec *d) {
    REQUIRE(A && d && A->m <= A->n && d->n == A->m, "npg_csr_inv_diag: shape mismatch");
    for (int64_t r = 0; r < A->m; ++r) {
        double v = 0.0;
        for (int64_t k = A->rowptr[r]; k < A->rowptr[r + 1]; ++k)
            if (A->col[(size_t)k] == r) v = A->val[(size_t)k];
        d->d[r] = 1.0 / v;
    }
    return NPG_OK;
}
static void spmv_raw(const npg_csr *A, const double *x, double *y, double alpha, double beta) {
    const int64_t m = A->m;
#pragma omp parallel for schedule(static)
    for (int64_t r = 0; r < m; ++r) {
        double s = 0.0;
        for (int64_t k = A->rowptr[r]; k < A->rowptr[r + 1]; ++k) s += A->val[(size_t)k] * x[A->col[(size_t)k]];
        y[r] = alpha * s + (beta == 0.0 ? 0.0 : beta * y[r]);
    }
}
NPG_API int npg_spmv(const npg_csr *A, const npg_vec *x, npg_vec *y, double alpha, double beta) {
    REQUIRE(A && x && y && x->n == A->n && y->n == A->m && x->d != y->d, "npg_spmv: shape mismatch (A %lldx%lld, x %lld, y %lld)",
            A ? (long long)A->m : 0LL, A ? (long long)A->n : 0LL, x ? (long long)x->n : 0LL, y ? (long long)y->n : 0LL);
    spmv_raw(A, x->d, y->d, alpha, beta);
    return NPG_OK;
}

// ---- Krylov.jl's gmres! / cg! as the reference configures them (src/inversion.jl:74-94, src/evolution.jl:118-126) ---------------------
struct npg_gmres {
    npg_ctx *ctx = nullptr;
    int64_t n = 0;
    int mem = 20;
    std::vector<double> V, w, q, dx, hist;
};
struct npg_cg {
    npg_ctx *ctx = nullptr;
    int64_t n = 0;
    std::vector<double> r, z, p, Ap, hist;
};
static inline double pre(int kind, double scalar, const npg_vec *diag, int64_t i) {
    return kind == NPG_PRECOND_SCALAR ? scalar : (kind == NPG_PRECOND_DIAG ? diag->d[i] : 1.0);
}
NPG_API int npg_gmres_create(npg_ctx *ctx, int64_t n, int memory, npg_gmres **out) {
    REQUIRE(ctx && out && n > 0 && memory >= 1 && memory <= 31, "npg_gmres_create: bad argument");
    npg_gmres *ws = new npg_gmres();
    ws->ctx = ctx;
    ws->n = n;
    ws->mem = memory;
    ws->V.assign((size_t)n * (size_t)memory, 0.0);
    ws->w.assign((size_t)n, 0.0);
    ws->q.assign((size_t)n, 0.0);
    ws->dx.assign((size_t)n, 0.0);
    *out = ws;
    return NPG_OK;
}
NPG_API int npg_gmres_destroy(npg_gmres *ws) {
    delete ws;
    return NPG_OK;
}
// knobs of the HBM layouts: accepted and ignored on the host
NPG_API int npg_gmres_set_split(npg_gmres *ws, int) { return ws ? NPG_OK : NPG_EINVAL; }
NPG_API int npg_gmres_set_basis(npg_gmres *ws, int) { return ws ? NPG_OK : NPG_EINVAL; }
NPG_API int npg_gmres_set_gather(npg_gmres *ws, int) { return ws ? NPG_OK : NPG_EINVAL; }
NPG_API int npg_gmres_set_profile(npg_gmres *ws, int) { return ws ? NPG_OK : NPG_EINVAL; }
NPG_API int npg_gmres_get_profile(npg_gmres *ws, double *ms_total, int64_t *launches) {
    REQUIRE(ws && ms_total && launches, "npg_gmres_get_profile: NULL argument");
    *ms_total = 0.0;
    *launches = 0;
    return NPG_OK;
}
NPG_API int64_t npg_gmres_history(npg_gmres *ws, double *buf, int64_t cap) {
    if (!ws || !buf || cap <= 0) return 0;
    const int64_t k = std::min<int64_t>(cap, (int64_t)ws->hist.size());
    memcpy(buf, ws->hist.data(), (size_t)k * sizeof(double));
    return k;
}
static void sym_givens(double a, double b, double &c, double &s, double &rho) {
    if (b == 0.0) {
        c = a == 0.0 ? 1.0 : std::copysign(1.0, a);
        s = 0.0;
        rho = std::fabs(a);
    } else if (a == 0.0) {
        c = 0.0;
        s = std::copysign(1.0, b);
        rho = std::fabs(b);
    } else if (std::fabs(b) > std::fabs(a)) {
        const double t = a / b;
        s = std::copysign(1.0, b) / std::sqrt(1.0 + t * t);
        c = s * t;
        rho = b / s;
    } else {
        const double t = b / a;
        c = std::copysign(1.0, a) / std::sqrt(1.0 + t * t);
        s = c * t;
        rho = a / c;
    }
}
// Left-preconditioned restarted GMRES(memory) with modified Gram-Schmidt: residual estimate |zeta|, stop at
// ||M r|| <= atol + rtol ||M r0||, warm start (x in/out), itmax == 0 means 2 n, breakdown tolerance eps^(3/4).
NPG_API int npg_gmres_solve(npg_gmres *ws, const npg_csr *A, int precond_kind, double precond_scalar, const npg_vec *precond_diag,
                            const npg_vec *y, npg_vec *x, double atol, double rtol, int64_t itmax, double, npg_solve_stats *stats) {
    REQUIRE(ws && A && y && x, "npg_gmres_solve: NULL argument");
    REQUIRE(A->m == ws->n && A->n == ws->n && y->n == ws->n && x->n == ws->n, "npg_gmres_solve: workspace is for n=%lld",
            (long long)ws->n);
    REQUIRE(precond_kind == NPG_PRECOND_NONE || precond_kind == NPG_PRECOND_SCALAR ||
                (precond_kind == NPG_PRECOND_DIAG && precond_diag && precond_diag->n == ws->n),
            "npg_gmres_solve: bad preconditioner");
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t n = ws->n;
    const int mem = ws->mem;
    if (itmax <= 0) itmax = 2 * n;
    const double btol = std::pow(2.220446049250313e-16, 0.75);
    double *w = ws->w.data(), *q = ws->q.data();
    std::vector<double> c((size_t)mem), s((size_t)mem), z((size_t)mem + 1), R((size_t)mem * (mem + 1) / 2), yk((size_t)mem);
    ws->hist.clear();
    int64_t iter = 0;
    int npass = 0, status = 0;
    double rnorm0 = 0.0, rnorm = 0.0, eps = 0.0;
    bool first = true;
    while (status == 0) {
        // true residual q = M (b - A x)
        spmv_raw(A, x->d, w, 1.0, 0.0);
        for (int64_t i = 0; i < n; ++i) q[i] = pre(precond_kind, precond_scalar, precond_diag, i) * (y->d[i] - w[i]);
        const double beta = std::sqrt(dot_fixed(q, q, n));
        if (first) {
            rnorm0 = rnorm = beta;
            eps = atol + rtol * beta;
            ws->hist.push_back(beta);
            first = false;
            if (beta == 0.0) {
                status = 4;
                break;
            }
            if (beta <= eps) {      // (atol alone can satisfy the rule at the start)
                status = 1;
                break;
            }
        }
        ++npass;
        double zeta = beta;
        z[0] = beta;
        double *V = ws->V.data();
        for (int64_t i = 0; i < n; ++i) V[i] = q[i] / beta;
        int k = 0;
        for (; k < mem && status == 0; ++k) {
            double *vk = V + (size_t)k * (size_t)n;
            spmv_raw(A, vk, w, 1.0, 0.0);
            for (int64_t i = 0; i < n; ++i) q[i] = pre(precond_kind, precond_scalar, precond_diag, i) * w[i];
            double *Rk = R.data() + (size_t)k * (k + 1) / 2;
            for (int i = 0; i <= k; ++i) {          // modified Gram-Schmidt
                const double *vi = V + (size_t)i * (size_t)n;
                const double h = dot_fixed(vi, q, n);
                Rk[i] = h;
                for (int64_t t = 0; t < n; ++t) q[t] -= h * vi[t];
            }
            const double hbis = std::sqrt(dot_fixed(q, q, n));
            for (int i = 0; i < k; ++i) {           // previous rotations
                const double hi = Rk[i], hn = Rk[i + 1];
                Rk[i] = c[(size_t)i] * hi + s[(size_t)i] * hn;
                Rk[i + 1] = s[(size_t)i] * hi - c[(size_t)i] * hn;
            }
            double ck, sk, rho;
            sym_givens(Rk[k], hbis, ck, sk, rho);
            c[(size_t)k] = ck;
            s[(size_t)k] = sk;
            Rk[k] = rho;
            const double znext = sk * zeta;
            z[(size_t)k] = ck * zeta;
            zeta = znext;
            rnorm = std::fabs(zeta);
            ++iter;
            ws->hist.push_back(rnorm);
            const bool solved = rnorm <= eps || rnorm + 1.0 <= 1.0;
            if (solved) status = 1;
            else if (iter >= itmax) status = 2;
            else if (hbis <= btol) status = 3;
            if (status == 0 && k + 1 < mem) {
                double *vn = V + (size_t)(k + 1) * (size_t)n;
                for (int64_t t = 0; t < n; ++t) vn[t] = q[t] / hbis;
            }
        }
        const int kk = std::min(k, mem);
        // back substitution R y = z, x += V y
        for (int i = kk - 1; i >= 0; --i) {
            double v = z[(size_t)i];
            for (int j = i + 1; j < kk; ++j) v -= R[(size_t)j * (j + 1) / 2 + i] * yk[(size_t)j];
            const double rii = R[(size_t)i * (i + 1) / 2 + i];
            yk[(size_t)i] = std::fabs(rii) <= btol ? 0.0 : v / rii;
        }
        for (int i = 0; i < kk; ++i) {
            const double *vi = V + (size_t)i * (size_t)n;
            const double a = yk[(size_t)i];
            for (int64_t t = 0; t < n; ++t) x->d[t] += a * vi[t];
        }
    }
    if (stats) {
        stats->solved = (status == 1 || status == 4) ? 1 : 0;
        stats->niter = (int32_t)iter;
        stats->npass = npass;
        stats->status = status;
        stats->nreorth = 0;
        stats->nflagged = 0;
        stats->rnorm0 = rnorm0;
        stats->rnorm = rnorm;
        stats->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    return NPG_OK;
}
NPG_API int npg_cg_create(npg_ctx *ctx, int64_t n, npg_cg **out) {
    REQUIRE(ctx && out && n > 0, "npg_cg_create: bad argument");
    npg_cg *ws = new npg_cg();
    ws->ctx = ctx;
    ws->n = n;
    for (auto *v : {&ws->r, &ws->z, &ws->p, &ws->Ap}) v->assign((size_t)n, 0.0);
    *out = ws;
    return NPG_OK;
}
NPG_API int npg_cg_destroy(npg_cg *ws) {
    delete ws;
    return NPG_OK;
}
NPG_API int64_t npg_cg_history(npg_cg *ws, double *buf, int64_t cap) {
    if (!ws || !buf || cap <= 0) return 0;
    const int64_t k = std::min<int64_t>(cap, (int64_t)ws->hist.size());
    memcpy(buf, ws->hist.data(), (size_t)k * sizeof(double));
    return k;
}
// Krylov.jl cg!: gamma = r'z, stop at sqrt(gamma) <= atol + rtol sqrt(gamma_0); warm start; itmax == 0 means 2 n
NPG_API int npg_cg_solve(npg_cg *ws, const npg_csr *A, int precond_kind, double precond_scalar, const npg_vec *precond_diag,
                         const npg_vec *y, npg_vec *x, double atol, double rtol, int64_t itmax, npg_solve_stats *stats) {
    REQUIRE(ws && A && y && x, "npg_cg_solve: NULL argument");
    REQUIRE(A->m == ws->n && A->n == ws->n && y->n == ws->n && x->n == ws->n, "npg_cg_solve: workspace is for n=%lld", (long long)ws->n);
    REQUIRE(precond_kind == NPG_PRECOND_NONE || precond_kind == NPG_PRECOND_SCALAR ||
                (precond_kind == NPG_PRECOND_DIAG && precond_diag && precond_diag->n == ws->n),
            "npg_cg_solve: bad preconditioner");
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t n = ws->n;
    if (itmax <= 0) itmax = 2 * n;
    double *r = ws->r.data(), *z = ws->z.data(), *p = ws->p.data(), *Ap = ws->Ap.data();
    spmv_raw(A, x->d, Ap, 1.0, 0.0);
    for (int64_t i = 0; i < n; ++i) {
        r[i] = y->d[i] - Ap[i];
        z[i] = pre(precond_kind, precond_scalar, precond_diag, i) * r[i];
        p[i] = z[i];
    }
    double gamma = dot_fixed(r, z, n);
    double rnorm = std::sqrt(std::max(gamma, 0.0));
    const double rnorm0 = rnorm, eps = atol + rtol * rnorm;
    ws->hist.assign(1, rnorm);
    int64_t iter = 0;
    // r'z that is NaN or Inf: breakdown, before rnorm <= eps = Inf can call it solved (as the device library)
    int status = !std::isfinite(gamma) ? 3 : (rnorm == 0.0 ? 4 : (rnorm <= eps ? 1 : 0));
    while (status == 0) {
        spmv_raw(A, p, Ap, 1.0, 0.0);
        const double pAp = dot_fixed(p, Ap, n);
        if (!(pAp > 0.0)) {
            status = 3;             // not positive definite / breakdown
            break;
        }
        const double alpha = gamma / pAp;
        for (int64_t i = 0; i < n; ++i) {
            x->d[i] += alpha * p[i];
            r[i] -= alpha * Ap[i];
            z[i] = pre(precond_kind, precond_scalar, precond_diag, i) * r[i];
        }
        const double gnext = dot_fixed(r, z, n);
        rnorm = std::sqrt(std::max(gnext, 0.0));
        ++iter;
        ws->hist.push_back(rnorm);
        if (rnorm <= eps) status = 1;
        else if (iter >= itmax) status = 2;
        const double beta = gnext / gamma;
        gamma = gnext;
        for (int64_t i = 0; i < n; ++i) p[i] = z[i] + beta * p[i];
    }
    if (stats) {
        stats->solved = (status == 1 || status == 4) ? 1 : 0;
        stats->niter = (int32_t)iter;
        stats->npass = 0;
        stats->status = status;
        stats->nreorth = stats->nflagged = 0;
        stats->rnorm0 = rnorm0;
        stats->rnorm = rnorm;
        stats->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    return NPG_OK;
}

// Several right-hand sides against one matrix: the same C ABI as the device library's batched solver; here a loop over the columns
// that runs the CG above on each column's slice, so every column has that solver's bits, statistics and history.
struct npg_cg_multi {
    npg_ctx *ctx = nullptr;
    int64_t n = 0;
    int ncol_max = 0, last_ncol = 0;
    npg_cg *one = nullptr;
    std::vector<std::vector<double>> hist;
};
NPG_API int npg_cg_multi_create(npg_ctx *ctx, int64_t n, int ncol_max, npg_cg_multi **out) {
    REQUIRE(ctx && out && n > 0, "npg_cg_multi_create: bad argument");
    REQUIRE(ncol_max >= 1 && ncol_max <= NPG_CG_MULTI_MAX, "npg_cg_multi_create: ncol_max = %d, need 1 <= ncol_max <= %d", ncol_max,
            NPG_CG_MULTI_MAX);
    npg_cg_multi *ws = new npg_cg_multi();
    ws->ctx = ctx;
    ws->n = n;
    ws->ncol_max = ncol_max;
    if (int rc = npg_cg_create(ctx, n, &ws->one)) {
        delete ws;
        return rc;
    }
    ws->hist.resize((size_t)ncol_max);
    *out = ws;
    return NPG_OK;
}
NPG_API int npg_cg_multi_destroy(npg_cg_multi *ws) {
    if (!ws) return NPG_OK;
    npg_cg_destroy(ws->one);
    delete ws;
    return NPG_OK;
}
NPG_API int npg_cg_multi_solve(npg_cg_multi *ws, const npg_csr *A, int precond_kind, double precond_scalar, const npg_vec *precond_diag,
                               int ncol, const npg_vec *y, npg_vec *x, double atol, double rtol, int64_t itmax, npg_solve_stats *stats) {
    REQUIRE(ws && A && y && x, "npg_cg_multi_solve: NULL argument");
    REQUIRE(ncol >= 1 && ncol <= ws->ncol_max, "npg_cg_multi_solve: ncol = %d, the workspace holds 1 .. %d columns", ncol, ws->ncol_max);
    REQUIRE(A->ctx == ws->ctx && y->ctx == ws->ctx && x->ctx == ws->ctx &&
                (precond_kind != NPG_PRECOND_DIAG || !precond_diag || precond_diag->ctx == ws->ctx),
            "npg_cg_multi_solve: the workspace, the matrix and the vectors must belong to one context");
    REQUIRE(A->m == ws->n && A->n == ws->n && y->n == (int64_t)ncol * ws->n && x->n == (int64_t)ncol * ws->n,
            "npg_cg_multi_solve: workspace is for n=%lld and %d columns want vectors of %lld, but A is %lldx%lld, y has %lld, x has %lld",
            (long long)ws->n, ncol, (long long)ncol * (long long)ws->n, (long long)A->m, (long long)A->n, (long long)y->n, (long long)x->n);
    REQUIRE(precond_kind == NPG_PRECOND_NONE || precond_kind == NPG_PRECOND_SCALAR ||
                (precond_kind == NPG_PRECOND_DIAG && precond_diag && precond_diag->n == ws->n),
            "npg_cg_multi_solve: bad preconditioner");
    const auto t0 = std::chrono::steady_clock::now();
    ws->last_ncol = ncol;
    for (int k = 0; k < ncol; ++k) {
        npg_vec yk, xk;
        yk.ctx = xk.ctx = ws->ctx;
        yk.n = xk.n = ws->n;
        yk.owns = xk.owns = false;
        yk.d = y->d + (size_t)k * (size_t)ws->n;
        xk.d = x->d + (size_t)k * (size_t)ws->n;
        if (int rc = npg_cg_solve(ws->one, A, precond_kind, precond_scalar, precond_diag, &yk, &xk, atol, rtol, itmax, stats ? stats + k : nullptr))
            return rc;
        ws->hist[(size_t)k] = ws->one->hist;
    }
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (int k = 0; stats && k < ncol; ++k) stats[k].seconds = seconds;
    return NPG_OK;
}
NPG_API int64_t npg_cg_multi_history(npg_cg_multi *ws, int col, double *buf, int64_t cap) {
    if (!ws || !buf || cap <= 0 || col < 0 || col >= ws->last_ncol) return 0;
    const std::vector<double> &h = ws->hist[(size_t)col];
    const int64_t k = std::min<int64_t>(cap, (int64_t)h.size());
    memcpy(buf, h.data(), (size_t)k * sizeof(double));
    return k;
}

// ---- element kernels ---------------------------------------------------------------------------------------------------------------------
struct npg_fe {
    npg_ctx *ctx = nullptr;
    int64_t ncell = 0, n_inv = 0, n_b = 0;
    int nq = 0, nb = 0;
    std::vector<double> G, wdet, qw, N2, dN2, Nb, dNb, N1, u_diri, b_diri;       // G: [ncell][12] (4 gradients x 3 components)
    std::vector<int32_t> cu, cp, cb;                                              // [ncell][30], [ncell][4], [ncell][nb]
    std::vector<int64_t> gptr, iptr;                                              // inverted indices: row -> (cell, local DoF)
    std::vector<int64_t> gidx, iidx;                                              // cell * nb + i   /   cell * 34 + l
    std::vector<double> coef[4], kv0, hcell, loc;                                 // nu, kappa_h, kappa_v, f: [ncell][nq]
    std::vector<double> loc_inv;                                                  // [ncell][34], as iidx addresses it (npg_fe_tangent_adjoint)
};
static inline double fval(const double *x, const std::vector<double> &diri, int32_t idx) { return npg::field_val(x, diri.data(), idx); }
namespace {
// the engine's tables as the diagnostics read them, cell by cell (csrc/cell_view.h; [cell][component] here)
using HostView = npg::CellView<npg::CellMajor>;
inline const double *data_or_null(const std::vector<double> &v) { return v.empty() ? nullptr : v.data(); }
inline HostView host_view(const npg_fe *fe) {
    return HostView{fe->cu.data(), fe->cp.data(), fe->cb.data(), fe->G.data(), fe->u_diri.data(), fe->b_diri.data(), fe->ncell, fe->nb,
                    fe->wdet.data(), data_or_null(fe->coef[0]), data_or_null(fe->coef[1]), data_or_null(fe->coef[2]), fe->nq};
}
struct HostShape {       // and its shape tables as cell_integrals and cell_tracers read them
    const double *qw, *N2, *dN2, *Nb, *dNb, *N1;
};
inline HostShape host_shape(const npg_fe *fe) {
    return HostShape{fe->qw.data(), fe->N2.data(), fe->dN2.data(), fe->Nb.data(), fe->dNb.data(), fe->N1.data()};
}
}  // namespace

NPG_API int npg_fe_create(npg_ctx *ctx, const npg_fe_desc *d, npg_fe **out) {
    REQUIRE(ctx && d && out, "npg_fe_create: NULL argument");
    REQUIRE(d->ncell > 0 && d->nq > 0 && d->nq <= 16, "npg_fe_create: need 1 <= nq <= 16");
    REQUIRE(d->nloc_b == 10 || d->nloc_b == 4, "npg_fe_create: nloc_b must be 10 (P2) or 4 (P1)");
    REQUIRE(d->grad_lambda && d->wdet && d->qw && d->N2 && d->dN2 && d->Nb && d->dNb && d->N1 && d->cell_u && d->cell_p && d->cell_b,
            "npg_fe_create: NULL table");
    const int64_t nc = d->ncell;
    const int nb = d->nloc_b, nq = d->nq;
    for (int64_t k = 0; k < nc * 30; ++k)
        REQUIRE(d->cell_u[k] < d->n_inv && (d->cell_u[k] >= 0 || -1 - (int64_t)d->cell_u[k] < d->n_u_diri),
                "npg_fe_create: cell_u[%lld] = %d out of range", (long long)k, d->cell_u[k]);
    for (int64_t k = 0; k < nc * 4; ++k) REQUIRE(d->cell_p[k] < d->n_inv, "npg_fe_create: cell_p[%lld] = %d out of range", (long long)k, d->cell_p[k]);
    for (int64_t k = 0; k < nc * nb; ++k)
        REQUIRE(d->cell_b[k] < d->n_b && (d->cell_b[k] >= 0 || -1 - (int64_t)d->cell_b[k] < d->n_b_diri),
                "npg_fe_create: cell_b[%lld] = %d out of range", (long long)k, d->cell_b[k]);
    npg_fe *fe = new npg_fe();
    fe->ctx = ctx;
    fe->ncell = nc;
    fe->nq = nq;
    fe->nb = nb;
    fe->n_inv = d->n_inv;
    fe->n_b = d->n_b;
    fe->G.assign(d->grad_lambda, d->grad_lambda + nc * 12);
    fe->wdet.assign(d->wdet, d->wdet + nc);
    fe->qw.assign(d->qw, d->qw + nq);
    fe->N2.assign(d->N2, d->N2 + nq * 10);
    fe->dN2.assign(d->dN2, d->dN2 + nq * 40);
    fe->Nb.assign(d->Nb, d->Nb + nq * nb);
    fe->dNb.assign(d->dNb, d->dNb + nq * nb * 4);
    fe->N1.assign(d->N1, d->N1 + nq * 4);
    fe->cu.assign(d->cell_u, d->cell_u + nc * 30);
    fe->cp.assign(d->cell_p, d->cell_p + nc * 4);
    fe->cb.assign(d->cell_b, d->cell_b + nc * nb);
    fe->u_diri.assign(d->u_diri, d->u_diri + std::max<int64_t>(0, d->n_u_diri));
    fe->b_diri.assign(d->b_diri, d->b_diri + std::max<int64_t>(0, d->n_b_diri));
    fe->u_diri.push_back(0.0);
    fe->b_diri.push_back(0.0);
    // inverted indices, cell-ascending: the order in which a row's cell contributions are added
    fe->gptr.assign((size_t)d->n_b + 1, 0);
    for (int64_t k = 0; k < nc * nb; ++k)
        if (fe->cb[(size_t)k] >= 0) ++fe->gptr[(size_t)fe->cb[(size_t)k] + 1];
    for (int64_t r = 0; r < d->n_b; ++r) fe->gptr[r + 1] += fe->gptr[r];
    fe->gidx.resize((size_t)fe->gptr[d->n_b]);
    {
        std::vector<int64_t> next(fe->gptr.begin(), fe->gptr.end() - 1);
        for (int64_t k = 0; k < nc * nb; ++k)
            if (fe->cb[(size_t)k] >= 0) fe->gidx[(size_t)next[(size_t)fe->cb[(size_t)k]]++] = k;
    }
    fe->iptr.assign((size_t)d->n_inv + 1, 0);
    for (int64_t k = 0; k < nc * 30; ++k)
        if (fe->cu[(size_t)k] >= 0) ++fe->iptr[(size_t)fe->cu[(size_t)k] + 1];
    for (int64_t k = 0; k < nc * 4; ++k)
        if (fe->cp[(size_t)k] >= 0) ++fe->iptr[(size_t)fe->cp[(size_t)k] + 1];
    for (int64_t r = 0; r < d->n_inv; ++r) fe->iptr[r + 1] += fe->iptr[r];
    fe->iidx.resize((size_t)fe->iptr[d->n_inv]);
    {
        std::vector<int64_t> next(fe->iptr.begin(), fe->iptr.end() - 1);
        for (int64_t c = 0; c < nc; ++c) {
            for (int l = 0; l < 30; ++l) {
                const int32_t r = fe->cu[(size_t)c * 30 + l];
                if (r >= 0) fe->iidx[(size_t)next[(size_t)r]++] = c * 34 + l;
            }
            for (int m = 0; m < 4; ++m) {
                const int32_t r = fe->cp[(size_t)c * 4 + m];
                if (r >= 0) fe->iidx[(size_t)next[(size_t)r]++] = c * 34 + 30 + m;
            }
        }
    }
    fe->loc.assign((size_t)nc * nb, 0.0);
    *out = fe;
    return NPG_OK;
}
NPG_API int npg_fe_destroy(npg_fe *fe) {
    delete fe;
    return NPG_OK;
}
NPG_API int npg_fe_set_precision(npg_fe *fe, int precision) {
    REQUIRE(fe, "npg_fe_set_precision: NULL handle");
    REQUIRE(precision == NPG_FE_FP64, "npg_fe_set_precision: the host element kernels are fp64 (Gridap's arithmetic); the fp32-local mode "
                                      "is a device option");
    return NPG_OK;
}
NPG_API int npg_fe_get_precision(const npg_fe *fe) { return fe ? NPG_FE_FP64 : NPG_EINVAL; }
static int coef_index(const char *name) {
    return !strcmp(name, "nu") ? 0 : !strcmp(name, "kappa_h") ? 1 : !strcmp(name, "kappa_v") ? 2 : !strcmp(name, "f") ? 3 : -1;
}
NPG_API int npg_fe_set_coeff(npg_fe *fe, const char *name, const double *values) {
    REQUIRE(fe && name && values, "npg_fe_set_coeff: NULL argument");
    const int k = coef_index(name);
    REQUIRE(k >= 0, "npg_fe_set_coeff: unknown coefficient '%s'", name);
    fe->coef[k].assign(values, values + fe->ncell * fe->nq);
    if (k == 2) fe->kv0 = fe->coef[2];
    return NPG_OK;
}
// physical gradient of local function i (table dN: [nq][nloc][4]) at quadrature point q of a cell with gradients G[4][3]
static inline void grad_of(const double *dN, int nloc, const double *G, int q, int i, double g[3]) {
    const double *dn = dN + ((size_t)q * nloc + i) * 4;
    for (int a = 0; a < 3; ++a) g[a] = dn[0] * G[a] + dn[1] * G[3 + a] + dn[2] * G[6 + a] + dn[3] * G[9 + a];
}
// pass 2 of the vector assembly: every destination row adds its cells' local entries in cell order
static void gather_rows(const npg_fe *fe, double theta, double dt, const npg_vec *rhs_diff, const npg_vec *rhs_flux, const npg_vec *rhs_M,
                        const npg_vec *rhs_h, const npg_vec *rhs_v, double *out) {
    const int64_t n = fe->n_b;
#pragma omp parallel for schedule(static)
    for (int64_t r = 0; r < n; ++r) {
        double s = 0.0;
        for (int64_t k = fe->gptr[r]; k < fe->gptr[r + 1]; ++k) s += fe->loc[(size_t)fe->gidx[(size_t)k]];
        if (rhs_diff) s += theta * rhs_diff->d[r];
        if (rhs_flux) s += dt * rhs_flux->d[r];
        double lift = 0.0;
        if (rhs_h) lift += rhs_h->d[r];
        if (rhs_v) lift += rhs_v->d[r];
        lift *= theta;
        if (rhs_M) lift += rhs_M->d[r];
        out[r] = s - lift;
    }
}
// loc[cell][i] = int ( c1 b + c2 b_prev - cdt ( u~ . grad b~ + u~_z N2 ) ) phi_i         (src/model.jl:292-300)
static int advection_pass1(npg_fe *fe, int scheme, double dt, double N2, const npg_vec *b, const npg_vec *bp, const npg_vec *xi,
                           const npg_vec *xip) {
    REQUIRE(scheme == NPG_BDF1 || scheme == NPG_BDF2, "fe: scheme must be NPG_BDF1 or NPG_BDF2");
    REQUIRE(b && bp && xi && xip, "fe: NULL state vector");
    REQUIRE(b->n == fe->n_b && bp->n == fe->n_b, "fe: buoyancy vectors must have %lld entries", (long long)fe->n_b);
    REQUIRE(xi->n == fe->n_inv && xip->n == fe->n_inv, "fe: inversion vectors must have %lld entries", (long long)fe->n_inv);
    const bool bdf2 = scheme == NPG_BDF2;
    const double c1 = bdf2 ? 4.0 / 3.0 : 1.0, c2 = bdf2 ? -1.0 / 3.0 : 0.0, e1 = bdf2 ? 2.0 : 1.0, e2 = bdf2 ? -1.0 : 0.0;
    const double cdt = bdf2 ? 2.0 / 3.0 * dt : dt;
    const int nb = fe->nb, nq = fe->nq;
    const int64_t nc = fe->ncell;
#pragma omp parallel for schedule(static)
    for (int64_t cell = 0; cell < nc; ++cell) {
        const double *G = &fe->G[(size_t)cell * 12];
        double bm[10], bt[10], ut[30], acc[10];
        for (int i = 0; i < nb; ++i) {
            const int32_t idx = fe->cb[(size_t)cell * nb + i];
            const double v = fval(b->d, fe->b_diri, idx), vp = fval(bp->d, fe->b_diri, idx);
            bm[i] = c1 * v + c2 * vp;
            bt[i] = e1 * v + e2 * vp;
            acc[i] = 0.0;
        }
        for (int k = 0; k < 30; ++k) {
            const int32_t idx = fe->cu[(size_t)cell * 30 + k];
            ut[k] = e1 * fval(xi->d, fe->u_diri, idx) + e2 * fval(xip->d, fe->u_diri, idx);
        }
        for (int q = 0; q < nq; ++q) {
            double bq = 0.0, gl[4] = {0, 0, 0, 0};
            for (int i = 0; i < nb; ++i) {
                bq += fe->Nb[(size_t)q * nb + i] * bm[i];
                const double *dn = &fe->dNb[((size_t)q * nb + i) * 4];
                for (int k = 0; k < 4; ++k) gl[k] += dn[k] * bt[i];
            }
            double u[3] = {0, 0, 0};
            for (int i = 0; i < 10; ++i) {
                const double nn = fe->N2[(size_t)q * 10 + i];
                u[0] += nn * ut[3 * i];
                u[1] += nn * ut[3 * i + 1];
                u[2] += nn * ut[3 * i + 2];
            }
            double g[3];
            for (int a = 0; a < 3; ++a) g[a] = gl[0] * G[a] + gl[1] * G[3 + a] + gl[2] * G[6 + a] + gl[3] * G[9 + a];
            const double integrand = bq - cdt * (u[0] * g[0] + u[1] * g[1] + u[2] * g[2] + u[2] * N2);
            const double wq = fe->qw[(size_t)q] * fe->wdet[(size_t)cell] * integrand;
            for (int i = 0; i < nb; ++i) acc[i] += wq * fe->Nb[(size_t)q * nb + i];
        }
        for (int i = 0; i < nb; ++i) fe->loc[(size_t)cell * nb + i] = acc[i];
    }
    return NPG_OK;
}
NPG_API int npg_fe_advection_rhs(npg_fe *fe, int scheme, double dt, double N2, const npg_vec *b, const npg_vec *b_prev, const npg_vec *x_inv,
                                 const npg_vec *x_inv_prev, npg_vec *out) {
    REQUIRE(fe && out && out->n == fe->n_b, "npg_fe_advection_rhs: bad argument");
    const int rc = advection_pass1(fe, scheme, dt, N2, b, b_prev, x_inv, x_inv_prev);
    if (rc) return rc;
    gather_rows(fe, 0.0, 0.0, nullptr, nullptr, nullptr, nullptr, nullptr, out->d);
    return NPG_OK;
}
NPG_API int npg_fe_evolution_rhs(npg_fe *fe, int scheme, double dt, double N2, double theta, const npg_vec *b, const npg_vec *b_prev,
                                 const npg_vec *x_inv, const npg_vec *x_inv_prev, const npg_vec *rhs_diff, const npg_vec *rhs_flux,
                                 const npg_vec *rhs_M, const npg_vec *rhs_h, const npg_vec *rhs_v, npg_vec *y) {
    REQUIRE(fe && y && y->n == fe->n_b, "npg_fe_evolution_rhs: bad argument");
    for (const npg_vec *v : {rhs_diff, rhs_flux, rhs_M, rhs_h, rhs_v})
        REQUIRE(!v || v->n == fe->n_b, "npg_fe_evolution_rhs: rhs_* vectors must have %lld entries", (long long)fe->n_b);
    const int rc = advection_pass1(fe, scheme, dt, N2, b, b_prev, x_inv, x_inv_prev);
    if (rc) return rc;
    gather_rows(fe, theta, dt, rhs_diff, rhs_flux, rhs_M, rhs_h, rhs_v, y->d);
    return NPG_OK;
}
// the tangent of the advection load (csrc/linearized.hip on the host; the arithmetic and its order are csrc/tangent_core.h)
NPG_API int npg_fe_tangent_rhs(npg_fe *fe, double N2, const npg_vec *b_base, const npg_vec *x_base, const npg_vec *db, const npg_vec *dx,
                               npg_vec *out) {
    REQUIRE(fe, "npg_fe_tangent_rhs: NULL handle");
    const bool any_null = !(b_base && x_base && db && dx && out);
    REQUIRE_OK(npg::check_tangent(any_null, N2, fe->n_inv, fe->n_b, any_null ? 0 : b_base->n, any_null ? 0 : x_base->n, any_null ? 0 : db->n,
                                  any_null ? 0 : dx->n, any_null ? 0 : out->n, true));
    const HostShape s = host_shape(fe);
    const HostView t = host_view(fe);
    const int64_t nc = fe->ncell;
#pragma omp parallel for schedule(static)
    for (int64_t cell = 0; cell < nc; ++cell) {
        if (fe->nb == 10) npg::cell_tangent<10>(s, t, fe->nq, N2, b_base->d, x_base->d, db->d, dx->d, cell, fe->loc.data());
        else npg::cell_tangent<4>(s, t, fe->nq, N2, b_base->d, x_base->d, db->d, dx->d, cell, fe->loc.data());
    }
    gather_rows(fe, 0.0, 0.0, nullptr, nullptr, nullptr, nullptr, nullptr, out->d);
    return NPG_OK;
}
// the adjoint of the tangent load (csrc/tangent_adjoint.hip on the host; the arithmetic and its order are csrc/tangent_adjoint_core.h)
NPG_API int npg_fe_tangent_adjoint(npg_fe *fe, double N2, const npg_vec *b_base, const npg_vec *x_base, const npg_vec *lam, npg_vec *out_b,
                                   npg_vec *out_x) {
    REQUIRE(fe, "npg_fe_tangent_adjoint: NULL handle");
    const bool any_null = !(b_base && x_base && lam && out_b && out_x);
    const bool aliased = !any_null && npg::adjoint_outputs_alias(b_base, x_base, lam, out_b, out_x);
    REQUIRE_OK(npg::check_tangent_adjoint(any_null, aliased, N2, fe->n_inv, fe->n_b, any_null ? 0 : b_base->n, any_null ? 0 : x_base->n,
                                          any_null ? 0 : lam->n, any_null ? 0 : out_b->n, any_null ? 0 : out_x->n, true));
    const HostShape s = host_shape(fe);
    const HostView t = host_view(fe);
    const int64_t nc = fe->ncell;
    if (fe->loc_inv.empty()) fe->loc_inv.assign((size_t)nc * 34, 0.0);      // the pressure entries stay the zeros set here
#pragma omp parallel for schedule(static)
    for (int64_t cell = 0; cell < nc; ++cell) {
        if (fe->nb == 10) npg::cell_tangent_adjoint<10>(s, t, fe->nq, N2, b_base->d, x_base->d, lam->d, cell, fe->loc.data(), fe->loc_inv.data());
        else npg::cell_tangent_adjoint<4>(s, t, fe->nq, N2, b_base->d, x_base->d, lam->d, cell, fe->loc.data(), fe->loc_inv.data());
    }
    gather_rows(fe, 0.0, 0.0, nullptr, nullptr, nullptr, nullptr, nullptr, out_b->d);
    const int64_t n = fe->n_inv;
#pragma omp parallel for schedule(static)
    for (int64_t r = 0; r < n; ++r) {
        double acc = 0.0;
        for (int64_t k = fe->iptr[(size_t)r]; k < fe->iptr[(size_t)r + 1]; ++k) acc += fe->loc_inv[(size_t)fe->iidx[(size_t)k]];
        out_x->d[r] = acc;
    }
    return NPG_OK;
}
// the derivatives of the convection and eddy closures (csrc/tangent_closures.hip on the host; the arithmetic and its order are
// csrc/tangent_closures_core.h)
static void gather_inv_rows(const npg_fe *fe, double *out) {
    const int64_t n = fe->n_inv;
#pragma omp parallel for schedule(static)
    for (int64_t r = 0; r < n; ++r) {
        double acc = 0.0;
        for (int64_t k = fe->iptr[(size_t)r]; k < fe->iptr[(size_t)r + 1]; ++k) acc += fe->loc_inv[(size_t)fe->iidx[(size_t)k]];
        out[r] = acc;
    }
}
NPG_API int npg_fe_tangent_diffusion(npg_fe *fe, double kappa_c, double N2min, double alpha, double N2, const npg_vec *b_base,
                                     const npg_vec *db, npg_vec *out) {
    REQUIRE(fe, "npg_fe_tangent_diffusion: NULL handle");
    const bool any_null = !(b_base && db && out);
    REQUIRE_OK(npg::check_tangent_diffusion(any_null, !any_null && (out == b_base || out == db), !fe->kv0.empty(), kappa_c, N2min, alpha, N2,
                                            fe->n_b, any_null ? 0 : b_base->n, any_null ? 0 : db->n, any_null ? 0 : out->n, true));
    const HostShape s = host_shape(fe);
    const HostView t = host_view(fe);
    const npg::ConvClosure cl{kappa_c, N2min};
    const int64_t nc = fe->ncell;
#pragma omp parallel for schedule(static)
    for (int64_t cell = 0; cell < nc; ++cell) {
        if (fe->nb == 10) npg::cell_tangent_diffusion<10>(s, t, fe->nq, cl, alpha, N2, fe->kv0.data(), b_base->d, db->d, cell, fe->loc.data());
        else npg::cell_tangent_diffusion<4>(s, t, fe->nq, cl, alpha, N2, fe->kv0.data(), b_base->d, db->d, cell, fe->loc.data());
    }
    gather_rows(fe, 0.0, 0.0, nullptr, nullptr, nullptr, nullptr, nullptr, out->d);
    return NPG_OK;
}
NPG_API int npg_fe_tangent_eddy(npg_fe *fe, double a2e2, int full_stress, double N2min, double alpha, double N2, double smoothing,
                                double nu_min, const npg_vec *b_base, const npg_vec *x_base, const npg_vec *db, npg_vec *out_x) {
    REQUIRE(fe, "npg_fe_tangent_eddy: NULL handle");
    const bool any_null = !(b_base && x_base && db && out_x);
    REQUIRE_OK(npg::check_tangent_eddy(false, any_null, !any_null && (out_x == b_base || out_x == x_base || out_x == db), !fe->coef[3].empty(),
                                       a2e2, full_stress, N2min, alpha, N2, smoothing, nu_min, fe->n_inv, fe->n_b, any_null ? 0 : b_base->n,
                                       any_null ? 0 : x_base->n, any_null ? 0 : db->n, any_null ? 0 : out_x->n, true));
    const HostShape s = host_shape(fe);
    const HostView t = host_view(fe);
    const npg::EddyClosure cl{N2min, smoothing, nu_min};
    const int64_t nc = fe->ncell;
    if (fe->loc_inv.empty()) fe->loc_inv.assign((size_t)nc * 34, 0.0);      // the pressure entries stay the zeros set here
    const double *f = fe->coef[3].data();
#pragma omp parallel for schedule(static)
    for (int64_t cell = 0; cell < nc; ++cell) {
        if (fe->nb == 10)
            npg::cell_tangent_eddy<10>(s, t, fe->nq, a2e2, full_stress, cl, alpha, N2, f, b_base->d, x_base->d, db->d, cell, fe->loc_inv.data());
        else
            npg::cell_tangent_eddy<4>(s, t, fe->nq, a2e2, full_stress, cl, alpha, N2, f, b_base->d, x_base->d, db->d, cell, fe->loc_inv.data());
    }
    gather_inv_rows(fe, out_x->d);
    return NPG_OK;
}
NPG_API int npg_fe_tangent_eddy_adjoint(npg_fe *fe, double a2e2, int full_stress, double N2min, double alpha, double N2, double smoothing,
                                        double nu_min, const npg_vec *b_base, const npg_vec *x_base, const npg_vec *mu, npg_vec *out_b) {
    REQUIRE(fe, "npg_fe_tangent_eddy_adjoint: NULL handle");
    const bool any_null = !(b_base && x_base && mu && out_b);
    REQUIRE_OK(npg::check_tangent_eddy(true, any_null, !any_null && (out_b == b_base || out_b == x_base || out_b == mu), !fe->coef[3].empty(),
                                       a2e2, full_stress, N2min, alpha, N2, smoothing, nu_min, fe->n_inv, fe->n_b, any_null ? 0 : b_base->n,
                                       any_null ? 0 : x_base->n, any_null ? 0 : mu->n, any_null ? 0 : out_b->n, true));
    const HostShape s = host_shape(fe);
    const HostView t = host_view(fe);
    const npg::EddyClosure cl{N2min, smoothing, nu_min};
    const int64_t nc = fe->ncell;
    const double *f = fe->coef[3].data();
#pragma omp parallel for schedule(static)
    for (int64_t cell = 0; cell < nc; ++cell) {
        if (fe->nb == 10)
            npg::cell_tangent_eddy_adjoint<10>(s, t, fe->nq, a2e2, full_stress, cl, alpha, N2, f, b_base->d, x_base->d, mu->d, cell, fe->loc.data());
        else
            npg::cell_tangent_eddy_adjoint<4>(s, t, fe->nq, a2e2, full_stress, cl, alpha, N2, f, b_base->d, x_base->d, mu->d, cell, fe->loc.data());
    }
    gather_rows(fe, 0.0, 0.0, nullptr, nullptr, nullptr, nullptr, nullptr, out_b->d);
    return NPG_OK;
}
// the read-back of npg_fe_set_coeff: the table as it stands
NPG_API int npg_fe_get_coeff(npg_fe *fe, const char *name, double *host_out) {
    const bool any_null = !(fe && name && host_out);
    const int k = any_null ? -1 : coef_index(name);
    REQUIRE_OK(npg::check_get_coeff(any_null, k, any_null ? "" : name, k >= 0 && !fe->coef[k].empty()));
    memcpy(host_out, fe->coef[k].data(), fe->coef[k].size() * sizeof(double));
    return NPG_OK;
}
// rhs_diff = -N2 int kappa_v d_z phi_i        (src/evolution.jl:269-278)
NPG_API int npg_fe_assemble_rhs_diff(npg_fe *fe, double N2, npg_vec *out) {
    REQUIRE(fe && out && out->n == fe->n_b, "npg_fe_assemble_rhs_diff: bad argument");
    REQUIRE(!fe->coef[2].empty(), "npg_fe_assemble_rhs_diff: coefficient kappa_v has not been set");
    const int nb = fe->nb, nq = fe->nq;
#pragma omp parallel for schedule(static)
    for (int64_t cell = 0; cell < fe->ncell; ++cell) {
        const double *G = &fe->G[(size_t)cell * 12];
        double acc[10] = {0};
        for (int q = 0; q < nq; ++q) {
            const double wq = -N2 * fe->qw[(size_t)q] * fe->wdet[(size_t)cell] * fe->coef[2][(size_t)cell * nq + q];
            for (int i = 0; i < nb; ++i) {
                const double *dn = &fe->dNb[((size_t)q * nb + i) * 4];
                acc[i] += wq * (dn[0] * G[2] + dn[1] * G[5] + dn[2] * G[8] + dn[3] * G[11]);
            }
        }
        for (int i = 0; i < nb; ++i) fe->loc[(size_t)cell * nb + i] = acc[i];
    }
    gather_rows(fe, 0.0, 0.0, nullptr, nullptr, nullptr, nullptr, nullptr, out->d);
    return NPG_OK;
}
static inline int64_t slot_of(const npg_csr *A, int64_t row, int32_t c) {
    const auto b = A->col.begin() + A->rowptr[(size_t)row], e = A->col.begin() + A->rowptr[(size_t)row + 1];
    const auto it = std::lower_bound(b, e, c);
    return (it != e && *it == c) ? (int64_t)(it - A->col.begin()) : -1;
}
// Row-owner matrix assembly (as csrc/fe.hip: the owner of a CSR row walks the (cell, local DoF) pairs that carry the row's DoF,
// cell-ascending, and adds the local rows into its own row - no races, the same bits on every run).
NPG_API int npg_fe_assemble_matrix(npg_fe *fe, int which, double scale, int full_stress, npg_csr *A, npg_vec *lift) {
    REQUIRE(fe && A, "npg_fe_assemble_matrix: NULL argument");
    const int nb = fe->nb, nq = fe->nq;
    std::fill(A->val.begin(), A->val.end(), 0.0);
    if (lift) std::fill(lift->d, lift->d + lift->n, 0.0);
    int64_t missing = 0;
    if (which == NPG_MAT_M || which == NPG_MAT_KH || which == NPG_MAT_KV) {
        REQUIRE(A->m <= fe->n_b && A->n <= fe->n_b && A->m <= A->n, "npg_fe_assemble_matrix: matrix must be n_b x n_b");
        REQUIRE(!lift || (lift->n >= A->m && lift->n <= fe->n_b), "npg_fe_assemble_matrix: lift must have n_b entries");
        const std::vector<double> *kap = which == NPG_MAT_KH ? &fe->coef[1] : which == NPG_MAT_KV ? &fe->coef[2] : nullptr;
        REQUIRE(which == NPG_MAT_M || !kap->empty(), "npg_fe_assemble_matrix: diffusivity coefficient has not been set");
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : missing)
        for (int64_t r = 0; r < A->m; ++r) {
            double lf = 0.0;
            for (int64_t k = fe->gptr[r]; k < fe->gptr[r + 1]; ++k) {
                const int64_t cell = fe->gidx[(size_t)k] / nb;
                const int i = (int)(fe->gidx[(size_t)k] % nb);
                const double *G = &fe->G[(size_t)cell * 12];
                double acc[10] = {0};
                for (int q = 0; q < nq; ++q) {
                    double wq = fe->qw[(size_t)q] * fe->wdet[(size_t)cell];
                    if (which == NPG_MAT_M) {
                        wq *= fe->Nb[(size_t)q * nb + i];
                        for (int j = 0; j < nb; ++j) acc[j] += wq * fe->Nb[(size_t)q * nb + j];
                    } else {
                        double gi[3];
                        grad_of(fe->dNb.data(), nb, G, q, i, gi);
                        wq *= (*kap)[(size_t)cell * nq + q];
                        for (int j = 0; j < nb; ++j) {
                            double gj[3];
                            grad_of(fe->dNb.data(), nb, G, q, j, gj);
                            acc[j] += wq * (which == NPG_MAT_KH ? gi[0] * gj[0] + gi[1] * gj[1] : gi[2] * gj[2]);
                        }
                    }
                }
                for (int j = 0; j < nb; ++j) {
                    const int32_t c = fe->cb[(size_t)cell * nb + j];
                    if (c >= 0) {
                        const int64_t s = slot_of(A, r, c);
                        if (s >= 0) A->val[(size_t)s] += acc[j];
                        else if (acc[j] != 0.0) ++missing;
                    } else {
                        lf += acc[j] * fe->b_diri[(size_t)(-1 - c)];
                    }
                }
            }
            if (lift) lift->d[r] = lf;
        }
    } else if (which == NPG_MAT_B) {
        // rows (u node i, component z), columns buoyancy nodes: scale * int phi_i phib_j          (src/inversion.jl:208)
        REQUIRE(A->m <= fe->n_inv && A->n == fe->n_b, "npg_fe_assemble_matrix: B must be n_inv x n_b");
        REQUIRE(!lift || (lift->n >= A->m && lift->n <= fe->n_inv), "npg_fe_assemble_matrix: lift must have n_inv entries");
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : missing)
        for (int64_t r = 0; r < A->m; ++r) {
            double lf = 0.0;
            for (int64_t k = fe->iptr[r]; k < fe->iptr[r + 1]; ++k) {
                const int64_t cell = fe->iidx[(size_t)k] / 34;
                const int l = (int)(fe->iidx[(size_t)k] % 34);
                if (l >= 30 || l % 3 != 2) continue;
                const int i = l / 3;
                double acc[10] = {0};
                for (int q = 0; q < nq; ++q) {
                    const double wq = fe->qw[(size_t)q] * fe->wdet[(size_t)cell] * scale * fe->N2[(size_t)q * 10 + i];
                    for (int j = 0; j < nb; ++j) acc[j] += wq * fe->Nb[(size_t)q * nb + j];
                }
                for (int j = 0; j < nb; ++j) {
                    const int32_t c = fe->cb[(size_t)cell * nb + j];
                    if (c >= 0) {
                        const int64_t s = slot_of(A, r, c);
                        if (s >= 0) A->val[(size_t)s] += acc[j];
                        else if (acc[j] != 0.0) ++missing;
                    } else {
                        lf += acc[j] * fe->b_diri[(size_t)(-1 - c)];
                    }
                }
            }
            if (lift) lift->d[r] = lf;
        }
    } else if (which == NPG_MAT_A) {
        //   [(i,a),(j,c)] += a2e2 int nu ( d_ac grad phi_i . grad phi_j  [+ d_c phi_i d_a phi_j  if full_stress] )
        //   [(i,x),(j,y)] -= int f phi_i phi_j ; [(i,y),(j,x)] += int f phi_i phi_j
        //   [(i,a), p_m ] -= int d_a phi_i psi_m ; [p_m, (i,a)] += int psi_m d_a phi_i          (src/inversion.jl:172-192)
        REQUIRE(A->m <= fe->n_inv && A->n <= fe->n_inv && A->m <= A->n, "npg_fe_assemble_matrix: A must be n_inv x n_inv");
        REQUIRE(!fe->coef[0].empty() && !fe->coef[3].empty(), "npg_fe_assemble_matrix: coefficients nu and f must be set");
        auto add = [&](int64_t r, int32_t c, double v, int64_t &miss) {
            const int64_t s = slot_of(A, r, c);
            if (s >= 0) A->val[(size_t)s] += v;
            else if (v != 0.0) ++miss;
        };
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : missing)
        for (int64_t r = 0; r < A->m; ++r) {
            for (int64_t k = fe->iptr[r]; k < fe->iptr[r + 1]; ++k) {
                const int64_t cell = fe->iidx[(size_t)k] / 34;
                const int l = (int)(fe->iidx[(size_t)k] % 34);
                const double *G = &fe->G[(size_t)cell * 12];
                const double *nu = &fe->coef[0][(size_t)cell * nq], *ff = &fe->coef[3][(size_t)cell * nq];
                if (l < 30) {
                    const int i = l / 3, a = l % 3;
                    for (int j = 0; j < 10; ++j) {
                        double kk = 0.0, cc = 0.0, fs[3] = {0, 0, 0};
                        for (int q = 0; q < nq; ++q) {
                            const double wq = fe->qw[(size_t)q] * fe->wdet[(size_t)cell];
                            double gi[3], gj[3];
                            grad_of(fe->dN2.data(), 10, G, q, i, gi);
                            grad_of(fe->dN2.data(), 10, G, q, j, gj);
                            const double wn = wq * scale * nu[q];
                            kk += wn * (gi[0] * gj[0] + gi[1] * gj[1] + gi[2] * gj[2]);
                            cc += wq * ff[q] * fe->N2[(size_t)q * 10 + i] * fe->N2[(size_t)q * 10 + j];
                            if (full_stress)
                                for (int c = 0; c < 3; ++c) fs[c] += wn * gi[c] * gj[a];
                        }
                        for (int c = 0; c < 3; ++c) {
                            const int32_t cj = fe->cu[(size_t)cell * 30 + 3 * j + c];
                            if (cj < 0) continue;               // homogeneous velocity Dirichlet data: no lift
                            double v = full_stress ? fs[c] : 0.0;
                            if (a == c) v += kk;
                            if (a == 0 && c == 1) v -= cc;
                            if (a == 1 && c == 0) v += cc;
                            if (a == c || full_stress || (a < 2 && c < 2)) add(r, cj, v, missing);
                        }
                    }
                    for (int m = 0; m < 4; ++m) {
                        const int32_t pm = fe->cp[(size_t)cell * 4 + m];
                        if (pm < 0) continue;
                        double dd = 0.0;
                        for (int q = 0; q < nq; ++q) {
                            double gi[3];
                            grad_of(fe->dN2.data(), 10, G, q, i, gi);
                            dd += fe->qw[(size_t)q] * fe->wdet[(size_t)cell] * fe->N1[(size_t)q * 4 + m] * gi[a];
                        }
                        add(r, pm, -dd, missing);
                    }
                } else {
                    const int m = l - 30;
                    for (int i = 0; i < 10; ++i) {
                        double dsum[3] = {0, 0, 0};
                        for (int q = 0; q < nq; ++q) {
                            double gi[3];
                            grad_of(fe->dN2.data(), 10, G, q, i, gi);
                            const double wm = fe->qw[(size_t)q] * fe->wdet[(size_t)cell] * fe->N1[(size_t)q * 4 + m];
                            for (int a = 0; a < 3; ++a) dsum[a] += wm * gi[a];
                        }
                        for (int a = 0; a < 3; ++a) {
                            const int32_t ci = fe->cu[(size_t)cell * 30 + 3 * i + a];
                            if (ci >= 0) add(r, ci, dsum[a], missing);
                        }
                    }
                }
            }
        }
    } else {
        REQUIRE(false, "npg_fe_assemble_matrix: unknown matrix id %d", which);
    }
    REQUIRE(missing == 0, "npg_fe_assemble_matrix: %lld non-zero local entries fall outside the CSR pattern", (long long)missing);
    return NPG_OK;
}
// closures at the quadrature points from d_z b          (src/inputs.jl:87-91, 130-137)
static void coeff_from_bz(const npg_fe *fe, int mode, const npg_vec *b, const std::vector<double> &base, double p0, double p1, double alpha,
                          double N2, double p2, double p3, std::vector<double> &out) {
    const int nb = fe->nb, nq = fe->nq;
    out.resize((size_t)fe->ncell * nq);
#pragma omp parallel for schedule(static)
    for (int64_t cell = 0; cell < fe->ncell; ++cell) {
        const double *G = &fe->G[(size_t)cell * 12];
        double bn[10];
        for (int i = 0; i < nb; ++i) bn[i] = fval(b->d, fe->b_diri, fe->cb[(size_t)cell * nb + i]);
        for (int q = 0; q < nq; ++q) {
            double bz = 0.0;
            for (int i = 0; i < nb; ++i) {
                const double *dn = &fe->dNb[((size_t)q * nb + i) * 4];
                bz += bn[i] * (dn[0] * G[2] + dn[1] * G[5] + dn[2] * G[8] + dn[3] * G[11]);
            }
            const double abz = alpha * (N2 + bz);
            const size_t o = (size_t)cell * nq + q;
            if (mode == 0) {
                out[o] = base[o] + p0 * (1.0 + std::tanh(-abz / p1)) / 2.0;
            } else {
                const double f = fe->coef[3][o];
                const double nu = f * (f / std::sqrt(p1 * p1 + abz * abz));
                const double m = std::fmax(p2 * p3, p2 * nu);
                out[o] = (m + std::log(std::exp(p2 * p3 - m) + std::exp(p2 * nu - m))) / p2;
            }
        }
    }
}
NPG_API int npg_fe_update_kappa_convection(npg_fe *fe, const double *kappa_v0_host_or_null, double kappa_c, double N2min, double alpha,
                                           double N2, const npg_vec *b) {
    REQUIRE(fe && b && b->n == fe->n_b, "npg_fe_update_kappa_convection: bad argument");
    if (kappa_v0_host_or_null) {
        const int rc = npg_fe_set_coeff(fe, "kappa_v", kappa_v0_host_or_null);
        if (rc) return rc;
    }
    REQUIRE(!fe->kv0.empty(), "npg_fe_update_kappa_convection: background kappa_v has not been set");
    coeff_from_bz(fe, 0, b, fe->kv0, kappa_c, N2min, alpha, N2, 0.0, 0.0, fe->coef[2]);
    return NPG_OK;
}
NPG_API int npg_fe_update_nu_eddy(npg_fe *fe, double N2min, double alpha, double N2, double smoothing, double nu_min, const npg_vec *b) {
    REQUIRE(fe && b && b->n == fe->n_b, "npg_fe_update_nu_eddy: bad argument");
    REQUIRE(!fe->coef[3].empty(), "npg_fe_update_nu_eddy: coefficient f has not been set");
    coeff_from_bz(fe, 1, b, fe->coef[3], 0.0, N2min, alpha, N2, smoothing, nu_min, fe->coef[0]);
    return NPG_OK;
}
// min_K h_K / max(max_q |u|, u_min)          (update_dt!, src/timesteppers.jl:108-119)
NPG_API int npg_fe_cfl_ratio(npg_fe *fe, const double *h_cells_host, double u_min, const npg_vec *x_inv, double *out) {
    REQUIRE(fe && x_inv && out && x_inv->n == fe->n_inv, "npg_fe_cfl_ratio: bad argument");
    if (h_cells_host) fe->hcell.assign(h_cells_host, h_cells_host + fe->ncell);
    REQUIRE(!fe->hcell.empty(), "npg_fe_cfl_ratio: cell sizes have not been provided");
    double best = 1e300;
    for (int64_t cell = 0; cell < fe->ncell; ++cell) {
        double un[30];
        for (int k = 0; k < 30; ++k) un[k] = fval(x_inv->d, fe->u_diri, fe->cu[(size_t)cell * 30 + k]);
        double smax = 0.0;
        for (int q = 0; q < fe->nq; ++q) {
            double u[3] = {0, 0, 0};
            for (int i = 0; i < 10; ++i) {
                const double nn = fe->N2[(size_t)q * 10 + i];
                u[0] += nn * un[3 * i];
                u[1] += nn * un[3 * i + 1];
                u[2] += nn * un[3 * i + 2];
            }
            smax = std::fmax(smax, std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]));
        }
        best = std::fmin(best, fe->hcell[(size_t)cell] / std::fmax(smax, u_min));
    }
    *out = best;
    return NPG_OK;
}

// ---- point sampling of the state (csrc/sample.hip on the host): the bins, the acceptance rule, the tie-break and the shape
// functions are the SAME code (csrc/sample_core.h), looped over the points with OpenMP --------------------------------------------
#include "../csrc/sample_core.h"

struct npg_locator {
    npg_ctx *ctx = nullptr;
    int64_t ncell = 0;
    npg::BinTables t;
};
struct npg_located {
    npg_ctx *ctx = nullptr;
    int64_t n = 0;
    std::vector<int32_t> cell;
    std::vector<double> lam;
};
NPG_API int npg_locator_create(npg_fe *fe, const double *anchor, int64_t nbins, npg_locator **out) {
    REQUIRE(fe && anchor && out, "npg_locator_create: NULL argument");
    REQUIRE(nbins >= 0 && nbins <= ((int64_t)1 << 26), "npg_locator_create: nbins must be 0 (automatic) .. 2^26");
    npg_locator *loc = new npg_locator();
    loc->ctx = fe->ctx;
    loc->ncell = fe->ncell;
    const char *err = npg::build_bins(fe->G.data(), anchor, fe->ncell, nbins, loc->t);
    if (err) {
        delete loc;
        REQUIRE(false, "%s", err);
    }
    *out = loc;
    return NPG_OK;
}
NPG_API int npg_locator_destroy(npg_locator *loc) {
    delete loc;
    return NPG_OK;
}
NPG_API int npg_locator_info(const npg_locator *loc, int64_t *dims, double *box, int64_t *nentries, int64_t *max_per_bin) {
    REQUIRE(loc, "npg_locator_info: NULL handle");
    for (int a = 0; a < 3; ++a) {
        if (dims) dims[a] = loc->t.grid.nb[a];
        if (box) box[a] = loc->t.grid.lo[a], box[3 + a] = loc->t.grid.hi[a];
    }
    if (nentries) *nentries = (int64_t)loc->t.bin_cells.size();
    if (max_per_bin) *max_per_bin = loc->t.max_per_bin;
    return NPG_OK;
}
NPG_API int npg_located_create(npg_ctx *ctx, int64_t n, npg_located **out) {
    REQUIRE(ctx && out && n >= 0, "npg_located_create: bad argument");
    REQUIRE(n <= ((int64_t)1 << 32), "npg_located_create: too many points for one launch (sample in chunks)");
    npg_located *p = new npg_located();
    p->ctx = ctx;
    p->n = n;
    p->cell.assign((size_t)n, -1);
    p->lam.assign((size_t)n * 4, NAN);
    *out = p;
    return NPG_OK;
}
NPG_API int npg_located_destroy(npg_located *p) {
    delete p;
    return NPG_OK;
}
NPG_API int npg_located_upload(npg_located *p, const int32_t *cell, const double *lambda) {
    REQUIRE(p && (p->n == 0 || (cell && lambda)), "npg_located_upload: NULL argument");
    std::copy(cell, cell + p->n, p->cell.begin());
    std::copy(lambda, lambda + 4 * p->n, p->lam.begin());
    return NPG_OK;
}
NPG_API int npg_located_download(const npg_located *p, int32_t *cell, double *lambda) {
    REQUIRE(p, "npg_located_download: NULL handle");
    if (cell) std::copy(p->cell.begin(), p->cell.end(), cell);
    if (lambda) std::copy(p->lam.begin(), p->lam.end(), lambda);
    return NPG_OK;
}
NPG_API int npg_locator_find(npg_locator *loc, const npg_vec *points, int64_t n, npg_located *out) {
    REQUIRE(loc && points && out, "npg_locator_find: NULL argument");
    REQUIRE(n >= 0 && points->n == 3 * n && out->n == n, "npg_locator_find: points must hold 3 n doubles and out n points");
    const npg::BinTables &t = loc->t;
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; ++i)
        npg::locate_point(t.grid, t.bin_ptr.data(), t.bin_cells.data(), t.geo.data(), points->d + 3 * i, &out->cell[(size_t)i],
                          &out->lam[(size_t)4 * i]);
    return NPG_OK;
}
NPG_API int npg_fe_sample(npg_fe *fe, int field, const npg_vec *vec, const npg_located *pts, npg_vec *out) {
    REQUIRE(fe && vec && pts && out, "npg_fe_sample: NULL argument");
    REQUIRE(field >= NPG_SAMPLE_U && field <= NPG_SAMPLE_GRAD_B, "npg_fe_sample: unknown field %d", field);
    const bool flow = field == NPG_SAMPLE_U || field == NPG_SAMPLE_P;
    REQUIRE(vec->n == (flow ? fe->n_inv : fe->n_b), "npg_fe_sample: the field's vector has %lld entries, expected %lld",
            (long long)vec->n, (long long)(flow ? fe->n_inv : fe->n_b));
    const int64_t n = pts->n;
    const int nc = npg::sample_ncomp(field);
    REQUIRE(out->n == n * nc, "npg_fe_sample: out must hold %d values per point", nc);
    const HostView t = host_view(fe);
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; ++i) {
        const int32_t c = pts->cell[(size_t)i];
        if (c >= 0 && c < fe->ncell)         // cell ids may come from the caller (npg_located_upload)
            npg::sample_point(t, field, vec->d, c, &pts->lam[(size_t)4 * i], out->d + (size_t)nc * i);
        else
            for (int a = 0; a < nc; ++a) out->d[(size_t)nc * i + a] = NAN;
    }
    return NPG_OK;
}
NPG_API int npg_fe_grid_integrals(npg_fe *fe, npg_locator *loc, const npg_vec *x_inv, const npg_vec *b, double N2, const npg_vec *axes,
                                  int64_t nx, int64_t ny, int64_t nz, npg_vec *col, npg_vec *zon) {
    REQUIRE(fe && loc && x_inv && b && axes && col && zon, "npg_fe_grid_integrals: NULL argument");
    REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, "npg_fe_grid_integrals: every axis needs at least 2 points");
    REQUIRE(nx <= 65536 && ny <= 65536 && nz <= 65536, "npg_fe_grid_integrals: at most 65536 points per axis");
    REQUIRE(loc->ctx == fe->ctx && x_inv->ctx == fe->ctx && b->ctx == fe->ctx && axes->ctx == fe->ctx && col->ctx == fe->ctx &&
                zon->ctx == fe->ctx, "npg_fe_grid_integrals: arguments of different contexts");
    REQUIRE(loc->ncell == fe->ncell, "npg_fe_grid_integrals: the locator was built for another mesh");
    REQUIRE_OK(npg::check_state_vectors("npg_fe_grid_integrals", fe->n_inv, fe->n_b, x_inv->n, b->n));
    REQUIRE(axes->n == nx + ny + nz, "npg_fe_grid_integrals: axes must hold nx + ny + nz doubles");
    REQUIRE(col->n == npg::kGridCol * nx * ny && zon->n == npg::kGridZon * ny * nz,
            "npg_fe_grid_integrals: col must hold %d nx ny and zon %d ny nz doubles", npg::kGridCol, npg::kGridZon);
    const double *ax = axes->d, *ay = ax + nx, *az = ay + ny;
    const int64_t len[3] = {nx, ny, nz};
    const double *a = ax;
    for (int d = 0; d < 3; a += len[d], ++d) {
        const char *err = npg::check_axis(a, len[d]);
        REQUIRE(!err, "npg_fe_grid_integrals: %s (axis %c)", err, "xyz"[d]);
    }
    const npg::BinTables &bt = loc->t;
    const HostView t = host_view(fe);
    auto values = [&](int64_t i, int64_t j, int64_t k, double v[npg::kGridVal]) {
        const double p[3] = {ax[i], ay[j], az[k]};
        int32_t c;
        double l[4];
        npg::locate_point(bt.grid, bt.bin_ptr.data(), bt.bin_cells.data(), bt.geo.data(), p, &c, l);
        npg::grid_point_values(t, x_inv->d, b->d, N2, p[2], c, l, v);
    };
    // every point is evaluated twice, once for its column and once for its zonal line: each output entry then has one owner and
    // one summation order (columns: k ascending; zonal lines: chunks of kGridChunk x indices, folded in order, as the device does)
#pragma omp parallel for collapse(2) schedule(dynamic, 16)
    for (int64_t i = 0; i < nx; ++i)
        for (int64_t j = 0; j < ny; ++j) {
            double s[npg::kGridCol] = {0.0, 0.0, 0.0, 0.0};
            for (int64_t k = 0; k < nz; ++k) {
                double v[npg::kGridVal], term[npg::kGridCol];
                values(i, j, k, v);
                npg::grid_col_terms(npg::trapezoid_weight(az, nz, k), v, term);
                for (int ch = 0; ch < npg::kGridCol; ++ch) s[ch] += term[ch];
            }
            for (int ch = 0; ch < npg::kGridCol; ++ch) col->d[((size_t)ch * nx + i) * ny + j] = s[ch];
        }
#pragma omp parallel for collapse(2) schedule(dynamic, 16)
    for (int64_t j = 0; j < ny; ++j)
        for (int64_t k = 0; k < nz; ++k) {
            double s[npg::kGridZon] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            for (int64_t i0 = 0; i0 < nx; i0 += npg::kGridChunk) {
                double acc[npg::kGridZon] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                for (int64_t i = i0; i < std::min(nx, i0 + npg::kGridChunk); ++i) {
                    double v[npg::kGridVal];
                    values(i, j, k, v);
                    npg::grid_zon_add(npg::trapezoid_weight(ax, nx, i), v, acc);
                }
                for (int ch = 0; ch < npg::kGridZon; ++ch) s[ch] += acc[ch];
            }
            for (int ch = 0; ch < npg::kGridZon; ++ch) zon->d[((size_t)ch * ny + j) * nz + k] = s[ch];
        }
    return NPG_OK;
}

// ---- quadrature integrals of the state over the mesh (csrc/integrals.hip on the host): the per-cell arithmetic is the SAME code
// (csrc/integrals_core.h).  Fixed chunks of kIntChunk cells give one partial row each, folded in chunk order: the sums do not depend
// on the number of threads. -----------------------------------------------------------------------------------------------------------
#include "../csrc/integrals_core.h"
static_assert(NPG_NINT == npg::kNInt, "NPG_NINT of the header and kNInt of integrals_core.h must agree");

struct npg_integrals {
    npg_fe *fe = nullptr;
    std::vector<double> cz;          // [ncell][4]
    std::vector<uint8_t> mask;       // [ncell] or empty
    std::vector<double> part;        // [nchunk][NPG_NINT]
};
NPG_API int npg_integrals_create(npg_fe *fe, const double *cell_z, const uint8_t *cell_mask, npg_integrals **out) {
    REQUIRE_OK(npg::check_integrals_create(fe && out, cell_z, fe ? fe->ncell : 0));
    const int64_t nc = fe->ncell;
    npg_integrals *I = new npg_integrals();
    I->fe = fe;
    I->cz.assign(cell_z, cell_z + nc * 4);
    if (cell_mask) I->mask.assign(cell_mask, cell_mask + nc);
    I->part.assign((size_t)((nc + npg::kIntChunk - 1) / npg::kIntChunk) * NPG_NINT, 0.0);
    *out = I;
    return NPG_OK;
}
NPG_API int npg_integrals_destroy(npg_integrals *I) {
    delete I;
    return NPG_OK;
}
NPG_API int npg_integrals_compute(npg_integrals *I, const npg_vec *x_inv, const npg_vec *b, int full_stress, npg_vec *out) {
    REQUIRE_OK(npg::check_integrals_compute(I, x_inv, b, full_stress, (const npg_vec *)out));
    const npg_fe *fe = I->fe;
    const int64_t nc = fe->ncell, nchunk = (nc + npg::kIntChunk - 1) / npg::kIntChunk;
    const HostShape s = host_shape(fe);
    const npg::CellsYZ<HostView> t{host_view(fe), nullptr, I->cz.data()};
    const uint8_t *mask = I->mask.empty() ? nullptr : I->mask.data();
#pragma omp parallel for schedule(static)
    for (int64_t k = 0; k < nchunk; ++k) {
        double acc[NPG_NINT];
        for (int a = 0; a < NPG_NINT; ++a) acc[a] = 0.0;
        for (int64_t c = k * npg::kIntChunk; c < std::min(nc, (k + 1) * npg::kIntChunk); ++c) {
            if (mask && !mask[c]) continue;
            if (fe->nb == 10) npg::cell_integrals<10>(s, t, fe->nq, x_inv->d, b->d, c, full_stress != 0, acc);
            else npg::cell_integrals<4>(s, t, fe->nq, x_inv->d, b->d, c, full_stress != 0, acc);
        }
        for (int a = 0; a < NPG_NINT; ++a) I->part[(size_t)k * NPG_NINT + a] = acc[a];
    }
    for (int a = 0; a < NPG_NINT; ++a) {
        double sum = 0.0;
        for (int64_t k = 0; k < nchunk; ++k) sum += I->part[(size_t)k * NPG_NINT + a];
        out->d[a] = sum;
    }
    return NPG_OK;
}

// ---- quadrature integrals of the state over the mesh's boundary faces (csrc/boundary.hip on the host): the per-face arithmetic, the
// validation, the sort by group and the rows of kBndChunk faces are the SAME code (csrc/boundary_core.h).  One partial row per row of
// faces, a group's rows folded in index order: the sums do not depend on the number of threads. ------------------------------------------
#include "../csrc/boundary_core.h"
static_assert(NPG_NBND == npg::kNBnd, "NPG_NBND of the header and kNBnd of boundary_core.h must agree");
static_assert(NPG_BND_NU == npg::kBndNu && NPG_BND_KH == npg::kBndKh && NPG_BND_KV == npg::kBndKv && NPG_BND_TAUX == npg::kBndTauX &&
                  NPG_BND_TAUY == npg::kBndTauY && NPG_BND_FLUX == npg::kBndFlux,
              "the coefficient codes of the header and of boundary_core.h must agree");

struct npg_boundary {
    npg_fe *fe = nullptr;
    int64_t nface = 0;
    int ngroup = 0;
    npg::BndLayout lay;
    npg::BndShape shape;
    npg::MixClosure cl{0.0, 0.0, 0.0, 0.0};
    std::vector<int32_t> cell;               // the faces that count, sorted: [nkept]
    std::vector<uint8_t> local;
    std::vector<double> area2, normal, z;    // [nkept], [3][nkept], [3][nkept]
    std::vector<double> coef[npg::kBndNCoef];   // [9][nkept] or empty
    std::vector<double> part;                // [nrows][NPG_NBND]
};
NPG_API int npg_boundary_create(npg_fe *fe, int64_t nface, const int32_t *face_cell, const uint8_t *face_local, const uint8_t *face_group,
                                int ngroup, const double *face_xyz, const double *face_normal, const double *face_area2,
                                const uint8_t *face_mask, npg_boundary **out) {
    REQUIRE(fe && out, "npg_boundary_create: NULL argument");
    {   // an embedded 2-D engine keeps every quadrature point on the face lambda_4 = 0 of its padded tetrahedra: it has no boundary faces
        bool flat = true;
        for (int q = 0; q < fe->nq; ++q) flat = flat && fe->N1[(size_t)q * 4 + 3] == 0.0;
        REQUIRE(!flat, "npg_boundary_create: an embedded 2-D engine is refused (its boundary is made of segments, not of faces)");
    }
    std::unique_ptr<npg_boundary> B(new npg_boundary());
    REQUIRE_OK(npg::bnd_build_layout(fe->ncell, nface, face_cell, face_local, face_group, ngroup, face_xyz, face_normal, face_area2, face_mask,
                                     B->lay));
    B->fe = fe;
    B->nface = nface;
    B->ngroup = ngroup;
    npg::bnd_shape_tables(B->shape);
    const size_t n = B->lay.orig.size();
    B->cell.resize(n), B->local.resize(n), B->area2.resize(n), B->normal.resize(3 * n), B->z.resize(3 * n);
    for (size_t i = 0; i < n; ++i) {
        const size_t f = (size_t)B->lay.orig[i];
        B->cell[i] = face_cell[f], B->local[i] = face_local[f], B->area2[i] = face_area2[f];
        for (int a = 0; a < 3; ++a)
            B->normal[a * n + i] = face_normal[(size_t)a * nface + f], B->z[a * n + i] = face_xyz[(size_t)(3 * a + 2) * nface + f];
    }
    B->part.assign(B->lay.rows.size() * NPG_NBND, 0.0);
    *out = B.release();
    return NPG_OK;
}
NPG_API int npg_boundary_destroy(npg_boundary *B) {
    delete B;
    return NPG_OK;
}
NPG_API int npg_boundary_set_coeff(npg_boundary *B, int which, const double *table) {
    REQUIRE(B, "npg_boundary_set_coeff: NULL argument");
    REQUIRE(which >= 0 && which < npg::kBndNCoef, "npg_boundary_set_coeff: which must be NPG_BND_NU .. NPG_BND_FLUX, got %d", which);
    const size_t n = B->lay.orig.size();
    std::vector<double> t;
    if (table) {
        t.resize(npg::kBndQ * n);
        for (int q = 0; q < npg::kBndQ; ++q)
            for (size_t i = 0; i < n; ++i) {
                const double v = table[(size_t)q * B->nface + B->lay.orig[i]];
                REQUIRE(std::isfinite(v), "npg_boundary_set_coeff: table %d is not finite at point %d of face %d", which, q, B->lay.orig[i]);
                t[q * n + i] = v;
            }
    }
    B->coef[which].swap(t);
    return NPG_OK;
}
NPG_API int npg_boundary_set_closure(npg_boundary *B, double kappa_c, double N2min, double alpha, double N2c) {
    REQUIRE(B, "npg_boundary_set_closure: NULL argument");
    REQUIRE(std::isfinite(kappa_c) && kappa_c >= 0.0 && std::isfinite(N2min) && std::isfinite(alpha) && std::isfinite(N2c),
            "npg_boundary_set_closure: kappa_c must be finite and >= 0, N2min, alpha and N2c finite");
    REQUIRE(kappa_c == 0.0 || N2min > 0.0, "npg_boundary_set_closure: kappa_c > 0 needs N2min > 0, got %g", N2min);
    B->cl = npg::MixClosure{kappa_c, N2min, alpha, N2c};
    return NPG_OK;
}
NPG_API int npg_boundary_compute(npg_boundary *B, const npg_vec *x_inv, const npg_vec *b, int full_stress, npg_vec *out, npg_vec *faces_out) {
    REQUIRE(B && x_inv && b && out, "npg_boundary_compute: NULL argument");
    const npg_fe *fe = B->fe;
    REQUIRE_OK(npg::check_state_vectors("npg_boundary_compute", fe->n_inv, fe->n_b, x_inv->n, b->n));
    REQUIRE(out->n >= (int64_t)B->ngroup * NPG_NBND, "npg_boundary_compute: out holds %lld doubles, needs ngroup * NPG_NBND = %d",
            (long long)out->n, B->ngroup * NPG_NBND);
    REQUIRE(!faces_out || faces_out->n >= B->nface * NPG_NBND, "npg_boundary_compute: faces_out holds %lld doubles, needs NPG_NBND * nface = %lld",
            (long long)faces_out->n, (long long)(B->nface * NPG_NBND));
    REQUIRE(full_stress == 0 || full_stress == 1, "npg_boundary_compute: full_stress must be 0 or 1, got %d", full_stress);
    npg::FaceTables<HostView> t{host_view(fe), (int64_t)B->lay.orig.size(), B->cell.data(), B->local.data(), B->area2.data(), B->normal.data(),
                                B->z.data(), {}};
    for (int i = 0; i < npg::kBndNCoef; ++i) t.coef_[i] = data_or_null(B->coef[i]);
    const int64_t nrows = (int64_t)B->lay.rows.size();
    double *fo = faces_out ? faces_out->d : nullptr;
    if (fo) std::fill(fo, fo + B->nface * NPG_NBND, 0.0);      // faces that do not count keep zeros
#pragma omp parallel for schedule(static)
    for (int64_t r = 0; r < nrows; ++r) {
        const npg::BndRow row = B->lay.rows[(size_t)r];
        double sum[NPG_NBND];
        for (int a = 0; a < NPG_NBND; ++a) sum[a] = 0.0;
        for (int64_t f = row.first; f < row.first + row.count; ++f) {
            double acc[NPG_NBND];
            for (int a = 0; a < NPG_NBND; ++a) acc[a] = 0.0;
            if (fe->nb == 10) npg::face_integrals<10>(B->shape, t, x_inv->d, b->d, f, full_stress != 0, B->cl, acc);
            else npg::face_integrals<4>(B->shape, t, x_inv->d, b->d, f, full_stress != 0, B->cl, acc);
            for (int a = 0; a < NPG_NBND; ++a) sum[a] += acc[a];
            if (fo)
                for (int a = 0; a < NPG_NBND; ++a) fo[(size_t)a * B->nface + B->lay.orig[(size_t)f]] = acc[a];
        }
        for (int a = 0; a < NPG_NBND; ++a) B->part[(size_t)r * NPG_NBND + a] = sum[a];
    }
    for (int g = 0; g < B->ngroup; ++g)
        for (int a = 0; a < NPG_NBND; ++a) {
            double sum = 0.0;
            for (int64_t r = B->lay.row0[g]; r < B->lay.row0[g + 1]; ++r) sum += B->part[(size_t)r * NPG_NBND + a];
            out->d[(size_t)g * NPG_NBND + a] = sum;
        }
    return NPG_OK;
}

// ---- time-dependent surface forcing (csrc/forcing.hip on the host): the per-face arithmetic, the row and entry gathers, the plan and
// the argument checks are the SAME code (csrc/forcing_core.h); every row and every entry is one thread's own sum. ------------------------
#include "../csrc/forcing_core.h"
static_assert(NPG_FRC_NSERIES == npg::kFrcNSeries, "NPG_FRC_NSERIES of the header and kFrcNSeries of forcing_core.h must agree");

struct npg_forcing {
    npg_fe *fe = nullptr;
    int64_t nface = 0;
    npg::FrcPlan plan;
    int32_t nkey[npg::kFrcNSeries] = {0, 0, 0, 0};
    bool has_ser[npg::kFrcNSeries] = {false, false, false, false}, has_gamma = false;
    std::vector<double> area2, ser[npg::kFrcNSeries], gamma, loc;
};
static npg::FrcFaces frc_faces(const npg_forcing *F) {
    npg::FrcFaces t{};
    t.nface = F->nface;
    t.area2 = F->area2.data();
    for (int c = 0; c < npg::kFrcNSeries; ++c) t.ser[c] = F->has_ser[c] ? F->ser[c].data() : nullptr, t.nkey[c] = F->nkey[c];
    t.gamma = F->has_gamma ? F->gamma.data() : nullptr;
    return t;
}
NPG_API int npg_forcing_create(npg_fe *fe, int64_t nface, const int32_t *face_cell, const uint8_t *face_local, const double *face_area2,
                               const npg_csr *pattern, npg_forcing **out) {
    REQUIRE(fe && out, "npg_forcing_create: NULL argument");
    REQUIRE(!pattern || pattern->ctx == fe->ctx, "npg_forcing_create: the pattern must be a plain-CSR matrix of the engine's context");
    {
        bool flat = true;
        for (int q = 0; q < fe->nq; ++q) flat = flat && fe->N1[(size_t)q * 4 + 3] == 0.0;
        REQUIRE(!flat, "npg_forcing_create: an embedded 2-D engine is refused (its boundary is made of segments, not of faces)");
    }
    std::unique_ptr<npg_forcing> F(new npg_forcing());
    REQUIRE_OK(npg::frc_build_plan(host_view(fe), fe->n_inv, fe->n_b, nface, face_cell, face_local, face_area2, pattern ? pattern->m : 0,
                                   pattern ? pattern->rowptr.data() : nullptr, pattern ? pattern->col.data() : nullptr, F->plan));
    F->fe = fe;
    F->nface = nface;
    F->area2.assign(face_area2, face_area2 + nface);
    F->loc.assign((size_t)npg::kFrcNLoad * npg::kFrcK * (size_t)nface + 1, 0.0);
    *out = F.release();
    return NPG_OK;
}
NPG_API int npg_forcing_destroy(npg_forcing *F) {
    delete F;
    return NPG_OK;
}
NPG_API int npg_forcing_set_series(npg_forcing *F, int which, int nkey, const double *tables) {
    REQUIRE(F, "npg_forcing_set_series: NULL argument");
    REQUIRE(which >= 0 && which < npg::kFrcNSeries, "npg_forcing_set_series: which must be NPG_FRC_TAUX .. NPG_FRC_TARGET, got %d", which);
    REQUIRE(!tables || nkey >= 1, "npg_forcing_set_series: nkey must be >= 1, got %d", nkey);
    if (tables) REQUIRE_OK(npg::frc_check_table("npg_forcing_set_series", tables, nkey, F->nface, false));
    F->ser[which].assign(1, 0.0);
    if (tables && F->nface > 0) F->ser[which].assign(tables, tables + (size_t)nkey * npg::kBndQ * (size_t)F->nface);
    F->has_ser[which] = tables != nullptr;
    F->nkey[which] = tables ? nkey : 0;
    return NPG_OK;
}
NPG_API int npg_forcing_set_gamma(npg_forcing *F, const double *table) {
    REQUIRE(F, "npg_forcing_set_gamma: NULL argument");
    if (table) REQUIRE_OK(npg::frc_check_table("npg_forcing_set_gamma", table, 1, F->nface, true));
    F->gamma.assign(1, 0.0);
    if (table && F->nface > 0) F->gamma.assign(table, table + npg::kBndQ * (size_t)F->nface);
    F->has_gamma = table != nullptr;
    return NPG_OK;
}
NPG_API int npg_forcing_apply(npg_forcing *F, const int32_t *key, const double *w, double alpha, const npg_vec *b_inv_base, npg_vec *b_inv_out,
                              npg_vec *rhs_flux_out) {
    REQUIRE(F, "npg_forcing_apply: NULL argument");
    const npg_fe *fe = F->fe;
    const bool all = b_inv_base && b_inv_out && rhs_flux_out;
    REQUIRE_OK(npg::frc_check_apply(key, w, alpha, F->nkey, fe->n_inv, fe->n_b, all, all ? b_inv_base->n : 0, all ? b_inv_out->n : 0,
                                    all ? rhs_flux_out->n : 0, all && b_inv_base->d == b_inv_out->d,
                                    all && b_inv_base->ctx == fe->ctx && b_inv_out->ctx == fe->ctx && rhs_flux_out->ctx == fe->ctx));
    npg::FrcFaces t = frc_faces(F);
    for (int c = 0; c < npg::kFrcNSeries; ++c) t.key[c] = F->nkey[c] ? key[c] : 0, t.w[c] = F->nkey[c] ? w[c] : 0.0;
    const int64_t nf = F->nface, nrow = fe->n_inv + fe->n_b;
    double *loc = F->loc.data();
#pragma omp parallel for schedule(static)
    for (int64_t f = 0; f < nf; ++f) {
        if (F->plan.kb == 6) npg::frc_face_loads<6>(t, f, loc);
        else npg::frc_face_loads<3>(t, f, loc);
    }
    const int32_t *ptr = F->plan.gptr.data(), *slot = F->plan.gslot.data();
#pragma omp parallel for schedule(static)
    for (int64_t r = 0; r < nrow; ++r) npg::frc_gather_row(r, fe->n_inv, ptr, slot, loc, alpha, b_inv_base->d, b_inv_out->d, rhs_flux_out->d);
    return NPG_OK;
}
NPG_API int npg_forcing_surface_matrix(npg_forcing *F, double scale, npg_csr *S) {
    REQUIRE(F && S, "npg_forcing_surface_matrix: NULL argument");
    REQUIRE(std::isfinite(scale), "npg_forcing_surface_matrix: scale is not finite");
    REQUIRE(F->plan.has_pattern, "npg_forcing_surface_matrix: the handle was created without a pattern");
    REQUIRE(F->has_gamma, "npg_forcing_surface_matrix: no gamma table (npg_forcing_set_gamma)");
    REQUIRE(S->ctx == F->fe->ctx && S->m == F->plan.pat_m && S->nnz == F->plan.pat_nnz,
            "npg_forcing_surface_matrix: S must be a plain-CSR matrix with the pattern given at create");
    std::fill(S->val.begin(), S->val.end(), 0.0);
    const npg::FrcFaces t = frc_faces(F);
    const npg::FrcPlan &pl = F->plan;
    const int64_t nent = (int64_t)pl.epos.size();
#pragma omp parallel for schedule(static)
    for (int64_t e = 0; e < nent; ++e) {
        const double s = pl.kb == 6 ? npg::frc_matrix_entry<6>(t, pl.eptr.data(), pl.eface.data(), pl.ecode.data(), e)
                                    : npg::frc_matrix_entry<3>(t, pl.eptr.data(), pl.eface.data(), pl.ecode.data(), e);
        S->val[(size_t)pl.epos[(size_t)e]] = scale * s;
    }
    return NPG_OK;
}
NPG_API int npg_forcing_info(const npg_forcing *F, int64_t *nface, int64_t *wind_slots, int64_t *flux_slots, int64_t *matrix_entries,
                             int64_t *matrix_slots) {
    REQUIRE(F, "npg_forcing_info: NULL argument");
    if (nface) *nface = F->nface;
    if (wind_slots) *wind_slots = F->plan.wind_slots;
    if (flux_slots) *flux_slots = F->plan.flux_slots;
    if (matrix_entries) *matrix_entries = (int64_t)F->plan.epos.size();
    if (matrix_slots) *matrix_slots = (int64_t)F->plan.eface.size();
    return NPG_OK;
}

// ---- interior buoyancy forcing (csrc/interior.hip on the host): the per-cell arithmetic, the row and entry gathers, the plan and the
// argument checks are the SAME code (csrc/interior_core.h); every row and every entry is one thread's own sum.  The budget: fixed chunks
// of kItrChunk kept cells give one partial row each, folded in chunk order - the sums do not depend on the number of threads. ------------
#include "../csrc/interior_core.h"
static_assert(NPG_ITR_NSERIES == npg::kItrNSeries, "NPG_ITR_NSERIES of the header and kItrNSeries of interior_core.h must agree");
static_assert(NPG_ITR_NBUDGET == npg::kItrNBudget, "NPG_ITR_NBUDGET of the header and kItrNBudget of interior_core.h must agree");

struct npg_interior {
    npg_fe *fe = nullptr;
    int64_t nkept = 0;
    npg::ItrPlan plan;
    int32_t nkey[npg::kItrNSeries] = {0, 0};
    bool has_ser[npg::kItrNSeries] = {false, false}, has_gamma = false;
    std::vector<int32_t> cell;
    std::vector<double> ser[npg::kItrNSeries], gamma, loc, part;
};
static npg::ItrCells itr_cells(const npg_interior *F, const int32_t *key, const double *w) {
    npg::ItrCells t{};
    t.nkept = F->nkept;
    t.nq = F->fe->nq;
    t.cell = F->cell.data();
    for (int c = 0; c < npg::kItrNSeries; ++c) {
        t.ser[c] = F->has_ser[c] ? F->ser[c].data() : nullptr, t.nkey[c] = F->nkey[c];
        t.key[c] = key && F->nkey[c] ? key[c] : 0, t.w[c] = w && F->nkey[c] ? w[c] : 0.0;
    }
    t.gamma = F->has_gamma ? F->gamma.data() : nullptr;
    return t;
}
NPG_API int npg_interior_create(npg_fe *fe, int64_t nkept, const int32_t *cells, const npg_csr *pattern, npg_interior **out) {
    REQUIRE(fe && out, "npg_interior_create: NULL argument");
    REQUIRE(!pattern || pattern->ctx == fe->ctx, "npg_interior_create: the pattern must be a plain-CSR matrix of the engine's context");
    std::unique_ptr<npg_interior> F(new npg_interior());
    REQUIRE_OK(npg::itr_build_plan(host_view(fe), fe->n_b, nkept, cells, pattern ? pattern->m : 0, pattern ? pattern->rowptr.data() : nullptr,
                                   pattern ? pattern->col.data() : nullptr, F->plan));
    F->fe = fe;
    F->nkept = nkept;
    F->cell.assign(cells, cells + nkept);
    F->loc.assign((size_t)fe->nb * (size_t)nkept + 1, 0.0);
    F->part.assign((size_t)((nkept + npg::kItrChunk - 1) / npg::kItrChunk) * npg::kItrNBudget + 1, 0.0);
    *out = F.release();
    return NPG_OK;
}
NPG_API int npg_interior_destroy(npg_interior *F) {
    delete F;
    return NPG_OK;
}
NPG_API int npg_interior_set_series(npg_interior *F, int which, int nkey, const double *tables) {
    REQUIRE_OK(npg::check_interior_set_series(F != nullptr, which, nkey, tables, F ? F->fe->nq : 0, F ? F->nkept : 0));
    F->ser[which].assign(1, 0.0);
    if (tables && F->nkept > 0) F->ser[which].assign(tables, tables + (size_t)nkey * F->fe->nq * (size_t)F->nkept);
    F->has_ser[which] = tables != nullptr;
    F->nkey[which] = tables ? nkey : 0;
    return NPG_OK;
}
NPG_API int npg_interior_set_gamma(npg_interior *F, const double *table) {
    REQUIRE_OK(npg::check_interior_set_gamma(F != nullptr, table, F ? F->fe->nq : 0, F ? F->nkept : 0));
    F->gamma.assign(1, 0.0);
    if (table && F->nkept > 0) F->gamma.assign(table, table + (size_t)F->fe->nq * (size_t)F->nkept);
    F->has_gamma = table != nullptr;
    return NPG_OK;
}
NPG_API int npg_interior_apply(npg_interior *F, const int32_t *key, const double *w, npg_vec *rhs_src_out) {
    const bool all = F && rhs_src_out;
    REQUIRE_OK(npg::check_interior_apply(all, key, w, all ? F->nkey : nullptr, all ? F->fe->n_b : 0, all ? rhs_src_out->n : 0,
                                         all && rhs_src_out->ctx == F->fe->ctx));
    const npg_fe *fe = F->fe;
    const npg::ItrCells t = itr_cells(F, key, w);
    const HostShape s = host_shape(fe);
    const HostView v = host_view(fe);
    const int64_t nk = F->nkept, nrow = fe->n_b;
    double *loc = F->loc.data();
#pragma omp parallel for schedule(static)
    for (int64_t kc = 0; kc < nk; ++kc) {
        if (fe->nb == 10) npg::itr_cell_load<10>(s, v, t, kc, loc);
        else npg::itr_cell_load<4>(s, v, t, kc, loc);
    }
    const int32_t *ptr = F->plan.gptr.data(), *slot = F->plan.gslot.data();
#pragma omp parallel for schedule(static)
    for (int64_t r = 0; r < nrow; ++r) npg::itr_gather_row(r, ptr, slot, loc, rhs_src_out->d);
    return NPG_OK;
}
NPG_API int npg_interior_matrix(npg_interior *F, npg_csr *R) {
    const bool all = F && R;
    REQUIRE_OK(npg::check_interior_matrix(all, all && F->plan.has_pattern, all && F->has_gamma,
                                          all && R->ctx == F->fe->ctx && R->m == F->plan.pat_m && R->nnz == F->plan.pat_nnz));
    std::fill(R->val.begin(), R->val.end(), 0.0);
    const npg_fe *fe = F->fe;
    const npg::ItrCells t = itr_cells(F, nullptr, nullptr);
    const HostShape s = host_shape(fe);
    const HostView v = host_view(fe);
    const npg::ItrPlan &pl = F->plan;
    const int64_t nent = (int64_t)pl.epos.size();
#pragma omp parallel for schedule(static)
    for (int64_t e = 0; e < nent; ++e) {
        R->val[(size_t)pl.epos[(size_t)e]] = fe->nb == 10 ? npg::itr_matrix_entry<10>(s, v, t, pl.eptr.data(), pl.ecell.data(), pl.ecode.data(), e)
                                                          : npg::itr_matrix_entry<4>(s, v, t, pl.eptr.data(), pl.ecell.data(), pl.ecode.data(), e);
    }
    return NPG_OK;
}
NPG_API int npg_interior_budget(npg_interior *F, const int32_t *key, const double *w, const npg_vec *b, npg_vec *out) {
    const bool all = F && b && out;
    REQUIRE_OK(npg::check_interior_budget(all, key, w, all ? F->nkey : nullptr, all ? F->fe->n_b : 0, all ? b->n : 0, all ? out->n : 0,
                                          all && b->ctx == F->fe->ctx && out->ctx == F->fe->ctx));
    const npg_fe *fe = F->fe;
    const npg::ItrCells t = itr_cells(F, key, w);
    const HostShape s = host_shape(fe);
    const HostView v = host_view(fe);
    const int64_t nk = F->nkept, nchunk = (nk + npg::kItrChunk - 1) / npg::kItrChunk;
#pragma omp parallel for schedule(static)
    for (int64_t k = 0; k < nchunk; ++k) {
        double acc[npg::kItrNBudget] = {0.0, 0.0, 0.0};
        for (int64_t kc = k * npg::kItrChunk; kc < std::min(nk, (k + 1) * npg::kItrChunk); ++kc) {
            if (fe->nb == 10) npg::itr_cell_budget<10>(s, v, t, b->d, kc, acc);
            else npg::itr_cell_budget<4>(s, v, t, b->d, kc, acc);
        }
        for (int a = 0; a < npg::kItrNBudget; ++a) F->part[(size_t)k * npg::kItrNBudget + a] = acc[a];
    }
    for (int a = 0; a < npg::kItrNBudget; ++a) {
        double sum = 0.0;
        for (int64_t k = 0; k < nchunk; ++k) sum += F->part[(size_t)k * npg::kItrNBudget + a];
        out->d[a] = sum;
    }
    return NPG_OK;
}
NPG_API int npg_interior_info(const npg_interior *F, int64_t *nkept, int64_t *load_slots, int64_t *matrix_entries, int64_t *matrix_slots) {
    REQUIRE(F, "npg_interior_info: NULL argument");
    if (nkept) *nkept = F->nkept;
    if (load_slots) *load_slots = (int64_t)F->plan.gslot.size();
    if (matrix_entries) *matrix_entries = (int64_t)F->plan.epos.size();
    if (matrix_slots) *matrix_slots = (int64_t)F->plan.ecell.size();
    return NPG_OK;
}

// ---- time means and co-moments of the running state (csrc/tavg.hip on the host): the per-node and per-entry arithmetic and the argument
// checks are the SAME code (csrc/tavg_core.h); every node and every entry is one thread's own. -------------------------------------------
#include "../csrc/tavg_core.h"

struct npg_tavg {
    npg_ctx *ctx = nullptr;
    int64_t n_inv = 0, n_b = 0, nnode = 0;
    std::vector<int32_t> iu, ib;
};
NPG_API int npg_tavg_create(npg_ctx *ctx, int64_t n_inv, int64_t n_b, int64_t nnode, const int32_t *iu, const int32_t *ib, npg_tavg **out) {
    REQUIRE(ctx && out, "npg_tavg_create: NULL argument");
    REQUIRE_OK(npg::tavg_check_create(n_inv, n_b, nnode, iu, ib));
    std::unique_ptr<npg_tavg> T(new npg_tavg());
    T->ctx = ctx;
    T->n_inv = n_inv, T->n_b = n_b, T->nnode = nnode;
    if (nnode > 0) T->iu.assign(iu, iu + 3 * nnode), T->ib.assign(ib, ib + 2 * nnode);
    *out = T.release();
    return NPG_OK;
}
NPG_API int npg_tavg_destroy(npg_tavg *T) {
    delete T;
    return NPG_OK;
}
NPG_API int npg_tavg_info(const npg_tavg *T, int64_t *nnode, int64_t *n_inv, int64_t *n_b) {
    REQUIRE(T, "npg_tavg_info: NULL argument");
    if (nnode) *nnode = T->nnode;
    if (n_inv) *n_inv = T->n_inv;
    if (n_b) *n_b = T->n_b;
    return NPG_OK;
}
NPG_API int npg_tavg_accumulate(npg_tavg *T, double r, double q, const npg_vec *x_inv, const npg_vec *b, npg_vec *mean_x, npg_vec *mean_b,
                                npg_vec *comom) {
    REQUIRE(T, "npg_tavg_accumulate: NULL argument");
    const bool all = x_inv && b && mean_x && mean_b;
    const bool aliased = all && (mean_x->d == x_inv->d || mean_b->d == b->d || mean_x->d == mean_b->d ||
                                 (comom && (comom->d == x_inv->d || comom->d == b->d || comom->d == mean_x->d || comom->d == mean_b->d)));
    const bool one_ctx = all && x_inv->ctx == T->ctx && b->ctx == T->ctx && mean_x->ctx == T->ctx && mean_b->ctx == T->ctx &&
                         (!comom || comom->ctx == T->ctx);
    REQUIRE_OK(npg::tavg_check_accumulate(r, q, T->n_inv, T->n_b, T->nnode, all, all ? x_inv->n : 0, all ? b->n : 0, all ? mean_x->n : 0,
                                          all ? mean_b->n : 0, comom ? comom->n : -1, aliased, one_ctx));
    const int64_t nnode = T->nnode, n_inv = T->n_inv, n = T->n_inv + T->n_b;
    if (comom && nnode > 0) {
        const npg::TavgTable t{nnode, T->iu.data(), T->ib.data()};
#pragma omp parallel for schedule(static)
        for (int64_t j = 0; j < nnode; ++j) npg::tavg_node(t, j, q, x_inv->d, b->d, mean_x->d, mean_b->d, comom->d);
    }
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; ++i) npg::tavg_mean(i, n_inv, r, x_inv->d, b->d, mean_x->d, mean_b->d);
    return NPG_OK;
}

// ---- gradients of the state recovered at the mesh's P2 nodes (csrc/nodal.hip on the host): the per-cell vertex gradients, the per-node
// sum and the argument checks are the SAME code (csrc/nodal_core.h); every cell's record and every node's row is one thread's own. --------
#include "../csrc/nodal_core.h"
static_assert(NPG_NODAL_U == npg::kNodalU && NPG_NODAL_B == npg::kNodalB && NPG_NODAL_P == npg::kNodalP && NPG_NODAL_NCH == npg::kNodalMaxCh,
              "the field codes of the header and of nodal_core.h must agree");

struct npg_nodal {
    npg_fe *fe = nullptr;
    int64_t nsel = 0, max_valence = 0;
    int weight_mode = 0;
    std::vector<int64_t> ptr;
    std::vector<int32_t> inc;
    std::vector<double> scratch;
};
NPG_API int npg_nodal_create(npg_fe *fe, int64_t nsel, const int64_t *inc_ptr, const int32_t *inc, int weight_mode, npg_nodal **out) {
    REQUIRE(fe && out, "npg_nodal_create: NULL argument");
    {   // an embedded 2-D engine pads its triangles to tetrahedra with a zero fourth gradient: its nodes have other local numbers
        bool flat = true;
        for (int q = 0; q < fe->nq; ++q) flat = flat && fe->N1[(size_t)q * 4 + 3] == 0.0;
        REQUIRE(!flat, "npg_nodal_create: an embedded 2-D engine is refused (the recovery is written for tetrahedra)");
    }
    int64_t vmax = 0;
    REQUIRE_OK(npg::check_nodal_create(fe->ncell, nsel, inc_ptr, inc, weight_mode, &vmax));
    std::unique_ptr<npg_nodal> N(new npg_nodal());
    N->fe = fe;
    N->nsel = nsel, N->max_valence = vmax, N->weight_mode = weight_mode;
    N->ptr.assign(inc_ptr, inc_ptr + nsel + 1);
    if (nsel > 0) N->inc.assign(inc, inc + inc_ptr[nsel]);
    *out = N.release();
    return NPG_OK;
}
NPG_API int npg_nodal_destroy(npg_nodal *N) {
    delete N;
    return NPG_OK;
}
NPG_API int npg_nodal_info(const npg_nodal *N, int64_t *nsel, int64_t *ninc, int64_t *max_valence, int64_t *scratch_doubles) {
    REQUIRE(N, "npg_nodal_info: NULL argument");
    if (nsel) *nsel = N->nsel;
    if (ninc) *ninc = (int64_t)N->inc.size();
    if (max_valence) *max_valence = N->max_valence;
    if (scratch_doubles) *scratch_doubles = (int64_t)N->scratch.size();
    return NPG_OK;
}
NPG_API int npg_nodal_compute(npg_nodal *N, const npg_vec *x_inv, const npg_vec *b, int fields_mask, npg_vec *out) {
    REQUIRE(N && x_inv && b && out, "npg_nodal_compute: NULL argument");
    const npg_fe *fe = N->fe;
    REQUIRE_OK(npg::check_nodal_compute(fe->n_inv, fe->n_b, fe->nb, N->nsel, x_inv->n, b->n, fields_mask, out->n,
                                        x_inv->ctx == fe->ctx && b->ctx == fe->ctx && out->ctx == fe->ctx));
    if (N->nsel == 0) return NPG_OK;
    const npg::NodalPlan pl = npg::nodal_plan(fields_mask, fe->nb);
    const int64_t ncell = fe->ncell, nsel = N->nsel;
    if (N->scratch.size() < (size_t)ncell * pl.nslot) N->scratch.resize((size_t)ncell * pl.nslot);
    const HostView t = host_view(fe);
    double *scr = N->scratch.data();
    if (fe->nb == 10) {
#pragma omp parallel for schedule(static)
        for (int64_t c = 0; c < ncell; ++c) npg::nodal_cell<HostView, 10>(t, pl, x_inv->d, b->d, c, scr + (size_t)c * pl.nslot);
    } else {
#pragma omp parallel for schedule(static)
        for (int64_t c = 0; c < ncell; ++c) npg::nodal_cell<HostView, 4>(t, pl, x_inv->d, b->d, c, scr + (size_t)c * pl.nslot);
    }
    const npg::NodalTable tab{nsel, N->ptr.data(), N->inc.data(), fe->wdet.data(), N->weight_mode};
#pragma omp parallel for schedule(static)
    for (int64_t j = 0; j < nsel; ++j) npg::nodal_node(tab, pl, scr, j, out->d);
    return NPG_OK;
}

// ---- transports through sections (csrc/sections.hip on the host): the plan, the per-piece arithmetic, the fold order and the argument
// checks are the SAME code (csrc/sections_core.h); every piece's terms and every (bin, channel) sum is one thread's own. -----------------
#include "../csrc/sections_core.h"
static_assert(NPG_NSEC == npg::kNSec, "NPG_NSEC of the header and kNSec of sections_core.h must agree");
static_assert(NPG_SEC_KH == npg::kSecKh && NPG_SEC_KV == npg::kSecKv, "the coefficient codes of the header and of sections_core.h must agree");

struct npg_sections {
    npg_fe *fe = nullptr;
    npg::SecPlan plan;
    npg::MixClosure cl{0.0, 0.0, 0.0, 0.0};
    std::vector<double> cz;                      // [ncell][4]
    std::vector<double> lam;                     // [12][npiece]
    std::vector<double> coef[npg::kSecNCoef];    // [6][npiece] or empty
    std::vector<double> terms;                   // [NPG_NSEC][npiece]
};
NPG_API int npg_sections_create(npg_fe *fe, const double *cell_xyz, int nsec, const double *frames, const int32_t *n1, const int32_t *n2,
                                const double *edges1, const double *edges2, const uint8_t *cell_mask, npg_sections **out) {
    REQUIRE(fe && out, "npg_sections_create: NULL argument");
    bool flat = true;                   // an embedded 2-D engine keeps every quadrature point on the face lambda_4 = 0 of its padded tetrahedra
    for (int q = 0; q < fe->nq; ++q) flat = flat && fe->N1[(size_t)q * 4 + 3] == 0.0;
    std::unique_ptr<npg_sections> S(new npg_sections());
    const int64_t nc = fe->ncell;
    REQUIRE_OK(npg::sec_build_plan(true, flat, nc, cell_xyz, nsec, frames, n1, n2, edges1, edges2, cell_mask, S->plan));
    S->fe = fe;
    const size_t np = (size_t)S->plan.npiece();
    S->cz.resize((size_t)nc * 4), S->lam.resize(12 * np), S->terms.resize(NPG_NSEC * np);
    for (int64_t c = 0; c < nc; ++c)
        for (int k = 0; k < 4; ++k) S->cz[(size_t)c * 4 + k] = cell_xyz[(size_t)c * 12 + 3 * k + 2];
    for (size_t i = 0; i < np; ++i)
        for (int k = 0; k < 12; ++k) S->lam[(size_t)k * np + i] = S->plan.lam[12 * i + k];
    *out = S.release();
    return NPG_OK;
}
NPG_API int npg_sections_destroy(npg_sections *S) {
    delete S;
    return NPG_OK;
}
NPG_API int npg_sections_info(const npg_sections *S, int64_t *npiece, int64_t *nbin, int64_t *ncut_cells, int64_t *max_per_bin) {
    REQUIRE(S, "npg_sections_info: NULL argument");
    if (npiece) *npiece = S->plan.npiece();
    if (nbin) *nbin = S->plan.nbin;
    if (ncut_cells) *ncut_cells = S->plan.ncut_cells;
    if (max_per_bin) *max_per_bin = S->plan.max_per_bin;
    return NPG_OK;
}
NPG_API int npg_sections_pieces(const npg_sections *S, int32_t *cell, int32_t *bin, double *lam, double *area) {
    REQUIRE(S, "npg_sections_pieces: NULL argument");
    const npg::SecPlan &pl = S->plan;
    if (cell) std::copy(pl.cell.begin(), pl.cell.end(), cell);
    if (bin) std::copy(pl.bin.begin(), pl.bin.end(), bin);
    if (lam) std::copy(pl.lam.begin(), pl.lam.end(), lam);
    if (area) std::copy(pl.area.begin(), pl.area.end(), area);
    return NPG_OK;
}
NPG_API int npg_sections_set_coeff(npg_sections *S, int which, const double *table) {
    REQUIRE_OK(npg::check_sections_coeff(S != nullptr, which, table, S ? S->plan.npiece() : 0));
    std::vector<double> t;
    if (table) t.assign(table, table + (size_t)npg::kSecQ * (size_t)S->plan.npiece());
    S->coef[which].swap(t);
    return NPG_OK;
}
NPG_API int npg_sections_set_closure(npg_sections *S, double kappa_c, double N2min, double alpha, double N2c) {
    REQUIRE_OK(npg::check_sections_closure(S != nullptr, kappa_c, N2min, alpha, N2c));
    S->cl = npg::MixClosure{kappa_c, N2min, alpha, N2c};
    return NPG_OK;
}
NPG_API int npg_sections_compute(npg_sections *S, const npg_vec *x_inv, const npg_vec *b, npg_vec *out, npg_vec *pieces_out) {
    REQUIRE(S && x_inv && b && out, "npg_sections_compute: NULL argument");
    const npg_fe *fe = S->fe;
    const npg::SecPlan &pl = S->plan;
    const int64_t np = pl.npiece(), nbin = pl.nbin;
    REQUIRE_OK(npg::check_sections_compute(true, fe->n_inv, fe->n_b, x_inv->n, b->n, nbin, np, out->n, pieces_out ? pieces_out->n : -1,
                                           x_inv->ctx == fe->ctx && b->ctx == fe->ctx && out->ctx == fe->ctx &&
                                               (!pieces_out || pieces_out->ctx == fe->ctx)));
    npg::SecPieces<HostView> t{{host_view(fe), nullptr, S->cz.data()}, np, pl.cell.data(), pl.sec.data(), S->lam.data(), pl.area.data(),
                               pl.normal.data(), {}};
    // (a set_coeff table of a plan without pieces is empty, hence "missing": nothing reads it)
    for (int w = 0; w < npg::kSecNCoef; ++w) t.coef_[w] = data_or_null(S->coef[w]);
    double *terms = pieces_out ? pieces_out->d : S->terms.data();
    const npg::MixClosure cl = S->cl;
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < np; ++i) {
        double term[NPG_NSEC];
        if (fe->nb == 10) npg::section_piece<10>(t, x_inv->d, b->d, i, cl, term);
        else npg::section_piece<4>(t, x_inv->d, b->d, i, cl, term);
        for (int k = 0; k < NPG_NSEC; ++k) terms[(size_t)k * (size_t)np + i] = term[k];
    }
#pragma omp parallel for schedule(static)
    for (int64_t j = 0; j < nbin * NPG_NSEC; ++j) out->d[j] = npg::section_fold(pl.bin_ptr.data(), terms, np, j / NPG_NSEC, (int)(j % NPG_NSEC));
    return NPG_OK;
}

// ---- the state binned into (latitude band, buoyancy class) (csrc/classes.hip on the host): the per-sample arithmetic and the edge
// search are the SAME code (csrc/classes_core.h).  Pass 1 in fixed chunks of kClsChunk cells, folded in chunk order; pass 2 adds the
// quantised terms as 64-bit integers (relaxed atomics on one table, a run of samples in one bin added up first): integer addition is
// associative, so the table does not depend on the number of threads. ------------------------------------------------------------------
#include "../csrc/classes_core.h"
#include "../csrc/mixing_core.h"
static_assert(NPG_NMIX == npg::kNMix, "NPG_NMIX of the header and kNMix of mixing_core.h must agree");
static_assert(NPG_NCLS == npg::kNCls, "NPG_NCLS of the header and kNCls of classes_core.h must agree");

struct npg_classes {
    npg_fe *fe = nullptr;
    std::vector<double> cy, cz;      // [ncell][4]
    std::vector<uint8_t> mask;       // [ncell] or empty
    std::vector<double> lam, wq;     // [ns][4], [ns] (= w[s] qsum)
    std::vector<double> y_edges, b_edges;
    std::vector<double> part;        // [nchunk][kClsInfo]
    std::vector<int64_t> itab;       // [(ny + 1)(nb + 1)][NPG_NCLS]
    int64_t nbins = 0;
    // the diffusivities of npg_classes_mixing (npg_classes_set_diffusivity): [ncell][ns], empty where the scalar holds
    std::vector<double> kh, kv0;
    double kh_s = 0.0, kv0_s = 0.0;
    bool kap_set = false;
};
namespace {
inline void classes_flush(int64_t *itab, int64_t bin, const int64_t run[NPG_NCLS]) {
    for (int k = 0; k < NPG_NCLS; ++k)
        if (run[k] != 0) __atomic_fetch_add(&itab[bin * NPG_NCLS + k], run[k], __ATOMIC_RELAXED);
}
// PASS 1: acc += {|term|, dropped} of cell c; PASS 2: the cell's quantised terms into itab, run by run.  sm: the sampler
// (csrc/classes_core.h: CensusSampler; csrc/mixing_core.h: MixSampler)
template <int NB, int PASS, class Sampler>
inline void class_cell(const npg::ClsRule &r, const npg::CellsYZ<HostView> &t, const Sampler &sm, int64_t c, double *acc, const double *scale,
                       int64_t *itab) {
    typename Sampler::template Cell<NB> n;
    sm.template load<NB>(t, c, n);
    int64_t run[NPG_NCLS] = {0, 0, 0, 0, 0, 0, 0, 0}, cur = -1;
    for (int s = 0; s < r.ns; ++s) {
        double term[NPG_NCLS];
        int64_t band = 0, cls = 0;
        const bool ok = sm.template sample<NB, PASS == 2>(t, n, r, s, c, &band, &cls, term);
        if (PASS == 1) {
            if (ok) for (int k = 0; k < NPG_NCLS; ++k) acc[k] += std::fabs(term[k]);
            else acc[NPG_NCLS] += 1.0;
        } else if (ok) {
            const int64_t bin = band * (r.nb + 1) + cls;
            if (bin != cur) {
                if (cur >= 0) classes_flush(itab, cur, run);
                cur = bin;
                for (int k = 0; k < NPG_NCLS; ++k) run[k] = 0;
            }
            for (int k = 0; k < NPG_NCLS; ++k) run[k] += npg::class_quantise(term[k], scale[k]);
        }
    }
    if (PASS == 2 && cur >= 0) classes_flush(itab, cur, run);
}
// the two passes of a class table with the sampler sm: zero, sum per chunk, fold, scale, bin, convert
template <class Sampler>
int class_passes(npg_classes *K, const Sampler &sm, npg_vec *table, npg_vec *info) {
    const npg_fe *fe = K->fe;
    const int64_t nc = fe->ncell, nchunk = (nc + npg::kClsChunk - 1) / npg::kClsChunk, nent = K->nbins * NPG_NCLS;
    const npg::ClsRule r{K->lam.data(), K->wq.data(), K->y_edges.data(), K->b_edges.data(), (int)K->wq.size(), (int64_t)K->y_edges.size(),
                         (int64_t)K->b_edges.size()};
    const npg::CellsYZ<HostView> t{host_view(fe), K->cy.data(), K->cz.data()};
    const uint8_t *mask = K->mask.empty() ? nullptr : K->mask.data();
    int64_t *itab = K->itab.data();
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < nent; ++i) itab[i] = 0;
#pragma omp parallel for schedule(static)
    for (int64_t k = 0; k < nchunk; ++k) {
        double acc[npg::kClsInfo];
        for (int a = 0; a < npg::kClsInfo; ++a) acc[a] = 0.0;
        for (int64_t c = k * npg::kClsChunk; c < std::min(nc, (k + 1) * npg::kClsChunk); ++c) {
            if (mask && !mask[c]) continue;
            if (fe->nb == 10) class_cell<10, 1>(r, t, sm, c, acc, nullptr, nullptr);
            else class_cell<4, 1>(r, t, sm, c, acc, nullptr, nullptr);
        }
        for (int a = 0; a < npg::kClsInfo; ++a) K->part[(size_t)k * npg::kClsInfo + a] = acc[a];
    }
    double scale[NPG_NCLS];
    for (int a = 0; a < npg::kClsInfo; ++a) {
        double sum = 0.0;
        for (int64_t k = 0; k < nchunk; ++k) sum += K->part[(size_t)k * npg::kClsInfo + a];
        if (a < NPG_NCLS) info->d[1 + a] = sum, scale[a] = npg::class_scale(sum);
        else info->d[0] = sum;
    }
#pragma omp parallel for schedule(static)
    for (int64_t c = 0; c < nc; ++c) {
        if (mask && !mask[c]) continue;
        if (fe->nb == 10) class_cell<10, 2>(r, t, sm, c, nullptr, scale, itab);
        else class_cell<4, 2>(r, t, sm, c, nullptr, scale, itab);
    }
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < nent; ++i) table->d[i] = (double)itab[i] / scale[i % NPG_NCLS];
    return NPG_OK;
}
}  // namespace

NPG_API int npg_classes_create(npg_fe *fe, const double *cell_y, const double *cell_z, const uint8_t *cell_mask, const double *rule_lam,
                               const double *rule_w, int ns, const double *y_edges, int64_t ny, const double *b_edges, int64_t nb,
                               npg_classes **out) {
    REQUIRE_OK(npg::check_classes_create(fe && out, fe ? fe->ncell : 0, cell_y, cell_z, rule_lam, rule_w, ns, y_edges, ny, b_edges, nb));
    const int64_t nc = fe->ncell;
    double qsum = 0.0;                       // the measure of a sample is w[s] wdet qsum, qsum from the engine's own weights
    for (double w : fe->qw) qsum += w;
    npg_classes *K = new npg_classes();
    K->fe = fe;
    K->cy.assign(cell_y, cell_y + nc * 4);
    K->cz.assign(cell_z, cell_z + nc * 4);
    if (cell_mask) K->mask.assign(cell_mask, cell_mask + nc);
    K->lam.assign(rule_lam, rule_lam + (size_t)4 * ns);
    K->wq.resize((size_t)ns);
    for (int s = 0; s < ns; ++s) K->wq[(size_t)s] = rule_w[s] * qsum;
    if (ny) K->y_edges.assign(y_edges, y_edges + ny);
    if (nb) K->b_edges.assign(b_edges, b_edges + nb);
    K->nbins = (ny + 1) * (nb + 1);
    K->part.assign((size_t)((nc + npg::kClsChunk - 1) / npg::kClsChunk) * npg::kClsInfo, 0.0);
    K->itab.assign((size_t)K->nbins * NPG_NCLS, 0);
    *out = K;
    return NPG_OK;
}
NPG_API int npg_classes_destroy(npg_classes *K) {
    delete K;
    return NPG_OK;
}
NPG_API int npg_classes_compute(npg_classes *K, const npg_vec *x_inv, const npg_vec *b, double N2, npg_vec *table, npg_vec *info) {
    REQUIRE_OK(npg::check_classes_compute(K, x_inv, b, N2, (const npg_vec *)table, (const npg_vec *)info));
    return class_passes(K, npg::CensusSampler{x_inv->d, b->d, N2}, table, info);
}

// ---- water-mass transformation by mixing (csrc/classes.hip with the mixing sampler): the per-sample arithmetic is the SAME code
// (csrc/mixing_core.h); the passes, the chunks, the scales and the integer table are those of npg_classes_compute (class_passes) ------
NPG_API int npg_classes_set_diffusivity(npg_classes *K, const double *kappa_h, double kappa_h_scalar, const double *kappa_v0,
                                        double kappa_v0_scalar) {
    const int ns = K ? (int)K->wq.size() : 1;
    const int64_t nc = K ? K->fe->ncell : 0;
    REQUIRE_OK(npg::check_classes_set_diffusivity(K != nullptr, nc * ns, ns, kappa_h, kappa_h_scalar, kappa_v0, kappa_v0_scalar));
    if (kappa_h) K->kh.assign(kappa_h, kappa_h + nc * ns);
    else K->kh.clear();
    if (kappa_v0) K->kv0.assign(kappa_v0, kappa_v0 + nc * ns);
    else K->kv0.clear();
    K->kh_s = kappa_h_scalar, K->kv0_s = kappa_v0_scalar;
    K->kap_set = true;
    return NPG_OK;
}

NPG_API int npg_classes_mixing(npg_classes *K, const npg_vec *b, double N2, double kappa_c, double N2min, double alpha, double N2c,
                               npg_vec *table, npg_vec *info) {
    const npg::MixClosure cl{kappa_c, N2min, alpha, N2c};
    REQUIRE_OK(npg::check_classes_mixing(K, b, N2, cl, (const npg_vec *)table, (const npg_vec *)info));
    const npg::MixSampler sm{data_or_null(K->kh), data_or_null(K->kv0), K->kh_s, K->kv0_s, cl, b->d, N2};
    return class_passes(K, sm, table, info);
}

// ---- Lagrangian particles in the flow (csrc/particles.hip on the host): the RK4 step, the remembered cell, the periodic wrap and the
// rule for leaving the mesh are the SAME code (csrc/particles_core.h), looped over the particles with OpenMP -------------------------
#include "../csrc/particles_core.h"
#include "../csrc/particles_walk_core.h"

struct npg_particles {
    npg_ctx *ctx = nullptr;
    int64_t n = 0;
    double t = 0.0;
    double L[3] = {0.0, 0.0, 0.0};
    std::vector<double> xyz, t_lost;
    std::vector<int32_t> cell, status, wind;
    // npg_particles_walk: the wall tables, the diffusivities, the generator's key and the count of steps since npg_particles_set
    int64_t wall_ncell = -1, kappa_ncell = -1;       // -1 = not set
    bool wall_axis[3] = {false, false, false};
    std::vector<int32_t> nbr, nreflect;
    std::vector<int8_t> shift;
    std::vector<double> kappa_h, kappa_v;
    double cd = 0.0;
    uint64_t seed = 0, step = 0;
};

NPG_API int npg_particles_create(npg_ctx *ctx, int64_t n, npg_particles **out) {
    REQUIRE(ctx && out, "npg_particles_create: NULL argument");
    REQUIRE(n >= 0 && n <= ((int64_t)1 << 32), "npg_particles_create: 0 .. 2^32 particles, got %lld", (long long)n);
    npg_particles *P = new npg_particles();
    P->ctx = ctx;
    P->n = n;
    P->xyz.assign((size_t)n * 3, 0.0);
    P->t_lost.assign((size_t)n, NAN);
    P->cell.assign((size_t)n, -1);
    P->status.assign((size_t)n, 0);
    P->wind.assign((size_t)n * 3, 0);
    *out = P;
    return NPG_OK;
}
NPG_API int npg_particles_destroy(npg_particles *P) {
    delete P;
    return NPG_OK;
}
NPG_API int npg_particles_set(npg_particles *P, const double *xyz, double t0) {
    REQUIRE(P && (P->n == 0 || xyz), "npg_particles_set: NULL argument");
    REQUIRE(std::isfinite(t0), "npg_particles_set: t0 is not finite");
    P->t = t0;
    P->step = 0;
    std::fill(P->nreflect.begin(), P->nreflect.end(), 0);
    if (P->n) std::copy(xyz, xyz + 3 * P->n, P->xyz.begin());
    std::fill(P->t_lost.begin(), P->t_lost.end(), NAN);
    std::fill(P->cell.begin(), P->cell.end(), -1);
    std::fill(P->status.begin(), P->status.end(), 0);
    std::fill(P->wind.begin(), P->wind.end(), 0);
    return NPG_OK;
}
NPG_API int npg_particles_set_period(npg_particles *P, const double *L) {
    REQUIRE(P && L, "npg_particles_set_period: NULL argument");
    for (int a = 0; a < 3; ++a)
        REQUIRE(std::isfinite(L[a]) && L[a] >= 0.0, "npg_particles_set_period: L[%d] = %g must be finite and >= 0 (0 = not periodic)", a, L[a]);
    for (int a = 0; a < 3; ++a) P->L[a] = L[a];
    return NPG_OK;
}
NPG_API int npg_particles_advance(npg_particles *P, npg_fe *fe, npg_locator *loc, const npg_vec *x_a, const npg_vec *x_b, double s0,
                                  double s1, double dt, int64_t nsub) {
    REQUIRE(P && fe && loc && x_a && x_b, "npg_particles_advance: NULL argument");
    REQUIRE(fe->ctx == P->ctx && loc->ctx == P->ctx && x_a->ctx == P->ctx && x_b->ctx == P->ctx,
            "npg_particles_advance: arguments of different contexts");
    REQUIRE(loc->ncell == fe->ncell, "npg_particles_advance: the locator was built for another mesh (an embedded 2-D engine has no "
            "locator: particles need a tetrahedral mesh)");
    REQUIRE(x_a->n == fe->n_inv && x_b->n == fe->n_inv, "npg_particles_advance: the flow vectors have %lld and %lld entries, expected %lld",
            (long long)x_a->n, (long long)x_b->n, (long long)fe->n_inv);
    const char *err = npg::check_particle_call(s0, s1, dt, nsub);
    REQUIRE(!err, "npg_particles_advance: %s", err);
    const npg::ParticleCall call = npg::make_particle_call(P->t, s0, s1, dt, nsub);
    const HostView t = host_view(fe);
    const npg::BinTables &bt = loc->t;
    const npg::ParticleMesh m{bt.grid, bt.bin_ptr.data(), bt.bin_cells.data(), bt.geo.data(), {P->L[0], P->L[1], P->L[2]}};
    const bool blend = x_a->d != x_b->d;
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < P->n; ++i) {
        if (P->status[(size_t)i] != 0) continue;         // lost: nothing moves it
        npg::ParticleState p;
        for (int a = 0; a < 3; ++a) p.x[a] = P->xyz[(size_t)3 * i + a], p.wind[a] = P->wind[(size_t)3 * i + a];
        p.c = P->cell[(size_t)i];
        const int64_t done = blend ? npg::particle_advance<true>(m, t, x_a->d, x_b->d, call, nsub, p)
                                   : npg::particle_advance<false>(m, t, x_a->d, x_a->d, call, nsub, p);
        if (done < nsub) {
            P->status[(size_t)i] = 1;
            P->t_lost[(size_t)i] = done > 0 ? call.t + (double)done * call.h : call.t;
            if (done < 0) continue;                      // lost where the call found it: the seed stays as it was given
        }
        for (int a = 0; a < 3; ++a) P->xyz[(size_t)3 * i + a] = p.x[a], P->wind[(size_t)3 * i + a] = p.wind[a];
        P->cell[(size_t)i] = p.c;
    }
    P->t += dt;
    return NPG_OK;
}
NPG_API int npg_particles_set_walls(npg_particles *P, const int32_t *nbr, const int8_t *shift, int64_t ncell) {
    REQUIRE(P && nbr && shift, "npg_particles_set_walls: NULL argument");
    REQUIRE(ncell >= 1 && ncell <= INT32_MAX, "npg_particles_set_walls: ncell = %lld", (long long)ncell);
    bool has[3];
    const char *err = npg::check_wall_tables(nbr, shift, ncell, P->L, has);
    REQUIRE(!err, "npg_particles_set_walls: %s", err);
    P->nbr.assign(nbr, nbr + ncell * 4);
    P->shift.assign(shift, shift + ncell * 12);
    P->nreflect.resize((size_t)P->n, 0);
    P->wall_ncell = ncell;
    for (int a = 0; a < 3; ++a) P->wall_axis[a] = has[a];
    return NPG_OK;
}
NPG_API int npg_particles_set_diffusion(npg_particles *P, const double *kappa_h, const double *kappa_v, int64_t ncell, double c_d,
                                        uint64_t seed) {
    REQUIRE(P, "npg_particles_set_diffusion: NULL handle");
    if (!kappa_h && !kappa_v) {              // diffusion off
        P->kappa_h.clear(), P->kappa_v.clear(), P->kappa_ncell = -1;
        return NPG_OK;
    }
    REQUIRE(kappa_h && kappa_v, "npg_particles_set_diffusion: NULL argument (kappa_h and kappa_v are given together)");
    REQUIRE(ncell >= 1 && ncell <= INT32_MAX, "npg_particles_set_diffusion: ncell = %lld", (long long)ncell);
    REQUIRE(P->wall_ncell < 0 || P->wall_ncell == ncell, "npg_particles_set_diffusion: ncell = %lld, the wall tables have %lld cells",
            (long long)ncell, (long long)P->wall_ncell);
    const char *err = npg::check_kappa_tables(kappa_h, kappa_v, ncell, c_d);
    REQUIRE(!err, "npg_particles_set_diffusion: %s", err);
    P->kappa_h.assign(kappa_h, kappa_h + ncell * 4);
    P->kappa_v.assign(kappa_v, kappa_v + ncell * 4);
    P->kappa_ncell = ncell, P->cd = c_d, P->seed = seed;
    return NPG_OK;
}
NPG_API int npg_particles_walk(npg_particles *P, npg_fe *fe, npg_locator *loc, const npg_vec *x_a, const npg_vec *x_b, double s0,
                               double s1, double dt, int64_t nsub) {
    REQUIRE(P && fe && loc && x_a && x_b, "npg_particles_walk: NULL argument");
    REQUIRE(fe->ctx == P->ctx && loc->ctx == P->ctx && x_a->ctx == P->ctx && x_b->ctx == P->ctx,
            "npg_particles_walk: arguments of different contexts");
    REQUIRE(loc->ncell == fe->ncell, "npg_particles_walk: the locator was built for another mesh (an embedded 2-D engine has no "
            "locator: particles need a tetrahedral mesh)");
    REQUIRE(x_a->n == fe->n_inv && x_b->n == fe->n_inv, "npg_particles_walk: the flow vectors have %lld and %lld entries, expected %lld",
            (long long)x_a->n, (long long)x_b->n, (long long)fe->n_inv);
    const char *err = npg::check_particle_call(s0, s1, dt, nsub);
    REQUIRE(!err, "npg_particles_walk: %s", err);
    REQUIRE(P->wall_ncell >= 0, "npg_particles_walk: no walls - call npg_particles_set_walls first");
    REQUIRE(P->wall_ncell == loc->ncell, "npg_particles_walk: the wall tables have ncell = %lld, the locator %lld",
            (long long)P->wall_ncell, (long long)loc->ncell);
    REQUIRE(P->kappa_ncell < 0 || P->kappa_ncell == loc->ncell, "npg_particles_walk: the diffusivity tables have ncell = %lld, the locator %lld",
            (long long)P->kappa_ncell, (long long)loc->ncell);
    for (int a = 0; a < 3; ++a)
        REQUIRE(P->wall_axis[a] == (P->L[a] > 0.0), "npg_particles_walk: axis %d has period %g but the wall tables carry %s seam "
                "shift on it - a walked particle crosses a seam through the table", a, P->L[a], P->wall_axis[a] ? "a" : "no");
    const npg::ParticleCall call = npg::make_particle_call(P->t, s0, s1, dt, nsub);
    const uint64_t step0 = P->step;
    const HostView t = host_view(fe);
    const npg::BinTables &bt = loc->t;
    const npg::ParticleMesh m{bt.grid, bt.bin_ptr.data(), bt.bin_cells.data(), bt.geo.data(), {P->L[0], P->L[1], P->L[2]}};
    const bool blend = x_a->d != x_b->d, diffuse = P->kappa_ncell >= 0;
    const npg::WalkTables w{P->nbr.data(), P->shift.data(), P->kappa_h.data(), P->kappa_v.data(), P->cd, (uint32_t)P->seed,
                            (uint32_t)(P->seed >> 32)};
    const double *xa = x_a->d, *xb = blend ? x_b->d : x_a->d;
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < P->n; ++i) {
        if (P->status[(size_t)i] != 0) continue;         // lost or stuck: nothing moves it
        npg::ParticleState p;
        for (int a = 0; a < 3; ++a) p.x[a] = P->xyz[(size_t)3 * i + a], p.wind[a] = P->wind[(size_t)3 * i + a];
        p.c = P->cell[(size_t)i];
        int32_t nrefl = P->nreflect[(size_t)i];
        const uint64_t idx = (uint64_t)i;
        const int64_t done = blend ? (diffuse ? npg::particle_walk<true, true>(m, w, t, xa, xb, call, nsub, idx, step0, p, nrefl)
                                              : npg::particle_walk<true, false>(m, w, t, xa, xb, call, nsub, idx, step0, p, nrefl))
                                   : (diffuse ? npg::particle_walk<false, true>(m, w, t, xa, xb, call, nsub, idx, step0, p, nrefl)
                                              : npg::particle_walk<false, false>(m, w, t, xa, xb, call, nsub, idx, step0, p, nrefl));
        if (done < nsub) {
            P->status[(size_t)i] = done < 0 ? 1 : 2;
            P->t_lost[(size_t)i] = done > 0 ? call.t + (double)done * call.h : call.t;
            if (done < 0) continue;                      // lost where the call found it: the seed stays as it was given
        }
        for (int a = 0; a < 3; ++a) P->xyz[(size_t)3 * i + a] = p.x[a], P->wind[(size_t)3 * i + a] = p.wind[a];
        P->cell[(size_t)i] = p.c;
        P->nreflect[(size_t)i] = nrefl;
    }
    P->t += dt, P->step += (uint64_t)nsub;
    return NPG_OK;
}
NPG_API int npg_particles_download_walk(const npg_particles *P, int32_t *nreflect, uint64_t *step) {
    REQUIRE(P, "npg_particles_download_walk: NULL handle");
    if (step) *step = P->step;
    if (nreflect) {
        std::fill(nreflect, nreflect + P->n, 0);
        std::copy(P->nreflect.begin(), P->nreflect.end(), nreflect);
    }
    return NPG_OK;
}
NPG_API int npg_particles_uniforms(npg_ctx *ctx, uint64_t seed, uint64_t first_index, int64_t n, uint64_t step, npg_vec *out) {
    REQUIRE(ctx && out, "npg_particles_uniforms: NULL argument");
    REQUIRE(n >= 0 && out->ctx == ctx && out->n == 3 * n, "npg_particles_uniforms: out must hold 3 n = %lld doubles of this context",
            (long long)(3 * n));
    for (int64_t i = 0; i < n; ++i)
        npg::particle_uniforms((uint32_t)seed, (uint32_t)(seed >> 32), first_index + (uint64_t)i, step, out->d + 3 * i);
    return NPG_OK;
}
NPG_API int npg_particles_download(const npg_particles *P, double *xyz, int32_t *cell, int32_t *status, int32_t *wind, double *t_lost) {
    REQUIRE(P, "npg_particles_download: NULL handle");
    if (xyz) std::copy(P->xyz.begin(), P->xyz.end(), xyz);
    if (cell) std::copy(P->cell.begin(), P->cell.end(), cell);
    if (status) std::copy(P->status.begin(), P->status.end(), status);
    if (wind) std::copy(P->wind.begin(), P->wind.end(), wind);
    if (t_lost) std::copy(P->t_lost.begin(), P->t_lost.end(), t_lost);
    return NPG_OK;
}
NPG_API int npg_particles_positions(const npg_particles *P, npg_vec *out) {
    REQUIRE(P && out, "npg_particles_positions: NULL argument");
    REQUIRE(out->ctx == P->ctx && out->n == 3 * P->n, "npg_particles_positions: out must hold 3 n = %lld doubles of the particles' context",
            (long long)(3 * P->n));
    std::copy(P->xyz.begin(), P->xyz.end(), out->d);
    return NPG_OK;
}

// ---- maps on buoyancy surfaces (csrc/surfaces.hip on the host): the tiling of the columns and the scan of one column are the SAME
// code (csrc/surfaces_core.h), looped over the columns with OpenMP ------------------------------------------------------------------
#include "../csrc/surfaces_core.h"
static_assert(NPG_NSURF == npg::kNSurf, "NPG_NSURF of the header and kNSurf of surfaces_core.h must agree");

struct npg_surfaces {
    npg_ctx *ctx = nullptr;
    npg_fe *fe = nullptr;
    npg_locator *loc = nullptr;
    int64_t ncol = 0;
    std::vector<double> xy;
    npg::ColumnTables t;
};

NPG_API int npg_surfaces_create(npg_fe *fe, npg_locator *loc, const double *xy, int64_t ncol, npg_surfaces **out) {
    REQUIRE(fe && loc && out && (xy || ncol == 0), "npg_surfaces_create: NULL argument");
    REQUIRE(ncol >= 0 && ncol <= ((int64_t)1 << 30), "npg_surfaces_create: 0 .. 2^30 columns, got %lld", (long long)ncol);
    REQUIRE(loc->ctx == fe->ctx, "npg_surfaces_create: arguments of different contexts");
    REQUIRE(loc->ncell == fe->ncell, "npg_surfaces_create: the locator was built for another mesh (an embedded 2-D engine has no "
            "locator: buoyancy surfaces need a tetrahedral mesh)");
    npg_surfaces *S = new npg_surfaces();
    S->ctx = fe->ctx, S->fe = fe, S->loc = loc, S->ncol = ncol;
    if (ncol) S->xy.assign(xy, xy + 2 * ncol);
    const char *err = npg::build_columns(loc->t.geo.data(), loc->ncell, loc->t.grid.lo[2], loc->t.grid.hi[2], xy, ncol, S->t);
    if (err) {
        delete S;
        REQUIRE(false, "%s", err);
    }
    *out = S;
    return NPG_OK;
}
NPG_API int npg_surfaces_destroy(npg_surfaces *S) {
    delete S;
    return NPG_OK;
}
NPG_API int npg_surfaces_info(const npg_surfaces *S, int64_t *nseg, int64_t *max_per_col, int64_t *ndry) {
    REQUIRE(S, "npg_surfaces_info: NULL handle");
    if (nseg) *nseg = S->t.col_ptr[(size_t)S->ncol];
    if (max_per_col) *max_per_col = S->t.max_per_col;
    if (ndry) *ndry = S->t.ndry;
    return NPG_OK;
}
NPG_API int npg_surfaces_columns(const npg_surfaces *S, double *z_top, double *z_bot, int32_t *nseg) {
    REQUIRE(S, "npg_surfaces_columns: NULL handle");
    for (int64_t j = 0; j < S->ncol; ++j) {
        const int64_t s0 = S->t.col_ptr[(size_t)j], s1 = S->t.col_ptr[(size_t)j + 1];
        if (z_top) z_top[j] = s1 > s0 ? S->t.seg_ztop[(size_t)s0] : NAN;
        if (z_bot) z_bot[j] = s1 > s0 ? S->t.seg_zbot[(size_t)s1 - 1] : NAN;
        if (nseg) nseg[j] = (int32_t)(s1 - s0);
    }
    return NPG_OK;
}
NPG_API int npg_surfaces_segments(const npg_surfaces *S, int32_t *cell, double *z_top, double *z_bot) {
    REQUIRE(S, "npg_surfaces_segments: NULL handle");
    if (cell) std::copy(S->t.seg_cell.begin(), S->t.seg_cell.end(), cell);
    if (z_top) std::copy(S->t.seg_ztop.begin(), S->t.seg_ztop.end(), z_top);
    if (z_bot) std::copy(S->t.seg_zbot.begin(), S->t.seg_zbot.end(), z_bot);
    return NPG_OK;
}
NPG_API int npg_surfaces_compute(npg_surfaces *S, const npg_vec *x_inv, const npg_vec *b, double N2, const double *levels, int nlev,
                                 npg_vec *out, npg_vec *cols) {
    REQUIRE(S && x_inv && b && out && cols, "npg_surfaces_compute: NULL argument");
    const char *err = npg::check_levels(levels, nlev, N2);
    REQUIRE(!err, "npg_surfaces_compute: %s", err);
    REQUIRE(x_inv->ctx == S->ctx && b->ctx == S->ctx && out->ctx == S->ctx && cols->ctx == S->ctx,
            "npg_surfaces_compute: arguments of different contexts");
    const npg_fe *fe = S->fe;
    REQUIRE_OK(npg::check_state_vectors("npg_surfaces_compute", fe->n_inv, fe->n_b, x_inv->n, b->n));
    REQUIRE(out->n == (int64_t)npg::kNSurf * nlev * S->ncol && cols->n == (int64_t)npg::kNSurfCol * S->ncol,
            "npg_surfaces_compute: out must hold %d nlev ncol = %lld and cols %d ncol = %lld entries, got %lld and %lld", npg::kNSurf,
            (long long)npg::kNSurf * nlev * S->ncol, npg::kNSurfCol, (long long)npg::kNSurfCol * S->ncol, (long long)out->n,
            (long long)cols->n);
    const HostView t = host_view(fe);
    const npg::SurfaceColumns sc{S->t.col_ptr.data(), S->t.seg_cell.data(), S->t.seg_ztop.data(), S->t.seg_zbot.data(), S->xy.data(),
                                 S->loc->t.geo.data(), S->ncol};
    std::vector<int32_t> cross((size_t)nlev * (size_t)S->ncol);
#pragma omp parallel for schedule(dynamic, 64)
    for (int64_t j = 0; j < S->ncol; ++j) {
        if (fe->nb == 10) npg::column_surfaces<10>(sc, t, b->d, N2, levels, nlev, j, out->d, cross.data(), cols->d);
        else npg::column_surfaces<4>(sc, t, b->d, N2, levels, nlev, j, out->d, cross.data(), cols->d);
    }
#pragma omp parallel for schedule(static)
    for (int64_t o = 0; o < (int64_t)cross.size(); ++o) npg::surface_fields(sc, t, x_inv->d, b->d, N2, nlev, o, cross.data(), out->d);
    return NPG_OK;
}

// ---- column integrals (csrc/columns.hip on the host): the tiling, a segment's terms, the order of the fold and the end values are
// the SAME code (csrc/columns_core.h), looped over the columns with OpenMP ---------------------------------------------------------------
#include "../csrc/columns_core.h"
static_assert(NPG_NCOLI == npg::kNColI && NPG_NCOLE == npg::kNColE, "NPG_NCOLI / NPG_NCOLE of the header and columns_core.h must agree");

struct npg_columns {
    npg_ctx *ctx = nullptr;
    npg_fe *fe = nullptr;
    npg_locator *loc = nullptr;
    int64_t ncol = 0;
    std::vector<double> xy;
    npg::ColumnTables t;
};

NPG_API int npg_columns_create(npg_fe *fe, npg_locator *loc, const double *xy, int64_t ncol, npg_columns **out) {
    const bool null_arg = !(fe && loc && xy && out);
    REQUIRE_OK(npg::check_columns_create(null_arg, ncol, null_arg || loc->ctx == fe->ctx, false, null_arg ? 0 : loc->ncell,
                                         null_arg ? 0 : fe->ncell));
    npg_columns *S = new npg_columns();
    S->ctx = fe->ctx, S->fe = fe, S->loc = loc, S->ncol = ncol;
    S->xy.assign(xy, xy + 2 * ncol);
    const char *err = npg::build_columns(loc->t.geo.data(), loc->ncell, loc->t.grid.lo[2], loc->t.grid.hi[2], xy, ncol, S->t);
    if (err) {
        delete S;
        REQUIRE(false, "npg_columns_create: %s", err);
    }
    *out = S;
    return NPG_OK;
}
NPG_API int npg_columns_destroy(npg_columns *S) {
    delete S;
    return NPG_OK;
}
NPG_API int npg_columns_info(const npg_columns *S, int64_t *nseg, int64_t *max_per_col, int64_t *ndry) {
    REQUIRE(S, "npg_columns_info: NULL handle");
    if (nseg) *nseg = S->t.col_ptr[(size_t)S->ncol];
    if (max_per_col) *max_per_col = S->t.max_per_col;
    if (ndry) *ndry = S->t.ndry;
    return NPG_OK;
}
NPG_API int npg_columns_columns(const npg_columns *S, double *z_top, double *z_bot, int32_t *nseg) {
    REQUIRE(S, "npg_columns_columns: NULL handle");
    for (int64_t j = 0; j < S->ncol; ++j) {
        const int64_t s0 = S->t.col_ptr[(size_t)j], s1 = S->t.col_ptr[(size_t)j + 1];
        if (z_top) z_top[j] = s1 > s0 ? S->t.seg_ztop[(size_t)s0] : NAN;
        if (z_bot) z_bot[j] = s1 > s0 ? S->t.seg_zbot[(size_t)s1 - 1] : NAN;
        if (nseg) nseg[j] = (int32_t)(s1 - s0);
    }
    return NPG_OK;
}
NPG_API int npg_columns_segments(const npg_columns *S, int32_t *cell, double *z_top, double *z_bot) {
    REQUIRE(S, "npg_columns_segments: NULL handle");
    if (cell) std::copy(S->t.seg_cell.begin(), S->t.seg_cell.end(), cell);
    if (z_top) std::copy(S->t.seg_ztop.begin(), S->t.seg_ztop.end(), z_top);
    if (z_bot) std::copy(S->t.seg_zbot.begin(), S->t.seg_zbot.end(), z_bot);
    return NPG_OK;
}
namespace {
template <int NB>
void columns_compute(const npg_columns *S, const double *xu, const double *xb, double *out, double *seg_out) {
    const HostView t = host_view(S->fe);
    const npg::ColumnTables &ct = S->t;
    const double *geo = S->loc->t.geo.data();
    const int64_t ncol = S->ncol;
    const size_t nseg = (size_t)ct.col_ptr[(size_t)ncol];
#pragma omp parallel for schedule(dynamic, 64)
    for (int64_t j = 0; j < ncol; ++j) {
        const int64_t s0 = ct.col_ptr[(size_t)j], s1 = ct.col_ptr[(size_t)j + 1];
        if (s1 == s0) {
            for (int ch = 0; ch < npg::kNColI + npg::kNColE; ++ch) out[(size_t)ch * ncol + j] = NAN;
            continue;
        }
        const double x = S->xy[2 * (size_t)j], y = S->xy[2 * (size_t)j + 1];
        double acc[npg::kNColI], term[npg::kNColI];
        for (int ch = 0; ch < npg::kNColI; ++ch) acc[ch] = 0.0;
        for (int64_t s = s0; s < s1; ++s) {            // top to bottom from 0.0: the fold of columns_core.h
            const int64_t c = ct.seg_cell[(size_t)s];
            npg::segment_terms<NB>(t, geo + (size_t)c * npg::kGeoStride, xu, xb, c, x, y, ct.seg_ztop[(size_t)s], ct.seg_zbot[(size_t)s], term, 1);
            for (int ch = 0; ch < npg::kNColI; ++ch) {
                acc[ch] += term[ch];
                if (seg_out) seg_out[(size_t)ch * nseg + (size_t)s] = term[ch];
            }
        }
        for (int ch = 0; ch < npg::kNColI; ++ch) out[(size_t)ch * ncol + j] = acc[ch];
        npg::column_ends<NB>(t, geo, xu, xb, x, y, ct.seg_cell[(size_t)s0], ct.seg_ztop[(size_t)s0], ct.seg_cell[(size_t)s1 - 1],
                             ct.seg_zbot[(size_t)s1 - 1], out + (size_t)npg::kNColI * ncol + j, (size_t)ncol);
    }
}
}  // namespace
NPG_API int npg_columns_compute(npg_columns *S, const npg_vec *x_inv, const npg_vec *b, npg_vec *out, npg_vec *segments_out) {
    const bool null_arg = !(S && x_inv && b && out);
    REQUIRE_OK(npg::check_columns_compute(
        null_arg, null_arg || (x_inv->ctx == S->ctx && b->ctx == S->ctx && out->ctx == S->ctx && (!segments_out || segments_out->ctx == S->ctx)),
        null_arg ? 0 : S->fe->n_inv, null_arg ? 0 : S->fe->n_b, null_arg ? 0 : x_inv->n, null_arg ? 0 : b->n, null_arg ? 0 : out->n,
        segments_out ? segments_out->n : -1, null_arg ? 0 : S->ncol, null_arg ? 0 : S->t.col_ptr[(size_t)S->ncol]));
    double *seg = segments_out && segments_out->n ? segments_out->d : nullptr;
    if (S->fe->nb == 10) columns_compute<10>(S, x_inv->d, b->d, out->d, seg);
    else columns_compute<4>(S, x_inv->d, b->d, out->d, seg);
    return NPG_OK;
}

// ---- passive tracers carried by the flow (csrc/tracers.hip on the host): the per-cell arithmetic is the SAME code
// (csrc/tracers_core.h); pass 2 walks the engine's inverted index in cell order, as gather_rows does. ----------------------------------
#include "../csrc/redi_core.h"
#include "../csrc/tracers_core.h"
#include "../csrc/transport_core.h"

struct npg_tracers {
    npg_fe *fe = nullptr;
    int ntracer = 0;
    int64_t n_diri = 0;
    std::vector<double> loc, diri, gamma, source;        // [K][ncell][nb], [K][n_diri], [K], [K]
    std::vector<uint8_t> lift;
    // isoneutral mixing (csrc/redi_core.h): kappa_iso and the tensor tables [ncell][nq], the counts of the last update
    int iso = npg::kRediOff;
    double slope_max = 0.0, bz_min = 0.0;
    std::vector<double> kiso, kxz, kyz, kzz;
    int64_t nfloor = 0, nclip = 0;
    // the transport operator (csrc/transport_core.h): the velocity tables [ncell][nq]
    int transport = npg::kTransportOff;
    std::vector<double> tux, tuy, tuz;
};
namespace {
struct HostTrVel {       // a cell's velocities at the quadrature points
    double a[3 * npg::kTrMaxQ];
    double &operator()(int j) { return a[j]; }
};
}  // namespace

NPG_API int npg_tracers_create(npg_fe *fe, int ntracer, npg_tracers **out) {
    REQUIRE(fe && out, "npg_tracers_create: NULL argument");
    REQUIRE(ntracer >= 1, "npg_tracers_create: ntracer must be at least 1, got %d", ntracer);
    REQUIRE(ntracer <= 65535, "npg_tracers_create: at most 65535 tracers, got %d", ntracer);
    npg_tracers *T = new npg_tracers();
    T->fe = fe;
    T->ntracer = ntracer;
    T->n_diri = (int64_t)fe->b_diri.size();              // (the engine keeps one spare zero behind its n_b_diri values)
    T->loc.assign((size_t)ntracer * fe->ncell * fe->nb, 0.0);
    T->diri.assign((size_t)ntracer * T->n_diri, 0.0);
    T->gamma.assign((size_t)ntracer, 0.0);
    T->source.assign((size_t)ntracer, 0.0);
    T->lift.assign((size_t)ntracer, 0);
    *out = T;
    return NPG_OK;
}
NPG_API int npg_tracers_destroy(npg_tracers *T) {
    delete T;
    return NPG_OK;
}
NPG_API int npg_tracers_set(npg_tracers *T, int k, const double *diri_or_null, double gamma, double source) {
    REQUIRE(T, "npg_tracers_set: NULL handle");
    REQUIRE(k >= 0 && k < T->ntracer, "npg_tracers_set: tracer %d out of range (ntracer = %d)", k, T->ntracer);
    REQUIRE(std::isfinite(gamma) && std::isfinite(source), "npg_tracers_set: gamma and source must be finite");
    const int64_t nd = T->n_diri - 1;
    bool any = false;
    if (diri_or_null)
        for (int64_t j = 0; j < nd; ++j) {
            REQUIRE(std::isfinite(diri_or_null[j]), "npg_tracers_set: Dirichlet value %lld is not finite", (long long)j);
            any = any || diri_or_null[j] != 0.0;
        }
    for (int64_t j = 0; j < nd; ++j) T->diri[(size_t)k * T->n_diri + j] = diri_or_null ? diri_or_null[j] : 0.0;
    T->gamma[(size_t)k] = gamma;
    T->source[(size_t)k] = source;
    T->lift[(size_t)k] = any;
    return NPG_OK;
}
NPG_API int npg_tracers_rhs(npg_tracers *T, int scheme, double dt, double theta, const npg_vec *c, const npg_vec *c_prev,
                            const npg_vec *x_inv, const npg_vec *x_inv_prev, const npg_vec *rhs_diff1_or_null, const npg_vec *flux_or_null,
                            npg_vec *y) {
    REQUIRE(T, "npg_tracers_rhs: NULL handle");
    REQUIRE(c && c_prev && x_inv && x_inv_prev && y, "npg_tracers_rhs: NULL state vector");
    npg_fe *fe = T->fe;
    const int K = T->ntracer;
    const int64_t nb = fe->n_b, nc = fe->ncell;
    REQUIRE(scheme == NPG_BDF1 || scheme == NPG_BDF2, "npg_tracers_rhs: scheme must be NPG_BDF1 or NPG_BDF2, got %d", scheme);
    REQUIRE(c->n == K * nb && c_prev->n == K * nb, "npg_tracers_rhs: tracer vectors must have ntracer * n_b = %lld entries", (long long)(K * nb));
    REQUIRE(y->n == K * nb, "npg_tracers_rhs: the output vector must have ntracer * n_b = %lld entries", (long long)(K * nb));
    REQUIRE(x_inv->n == fe->n_inv && x_inv_prev->n == fe->n_inv, "npg_tracers_rhs: inversion vectors must have %lld entries",
            (long long)fe->n_inv);
    REQUIRE(!rhs_diff1_or_null || rhs_diff1_or_null->n == nb, "npg_tracers_rhs: rhs_diff1 must have n_b = %lld entries", (long long)nb);
    REQUIRE(!flux_or_null || flux_or_null->n == K * nb, "npg_tracers_rhs: flux must have ntracer * n_b = %lld entries", (long long)(K * nb));
    const bool iso = T->iso != npg::kRediOff;
    if (iso) {
        npg::RediCheck a{"npg_tracers_rhs"};
        a.need = npg::kRediUpdated, a.state = T->iso;
        REQUIRE_OK(npg::check_redi(a));
    }
    bool lift = false;
    for (int k = 0; k < K; ++k) {
        REQUIRE(iso || T->gamma[(size_t)k] == 0.0 || rhs_diff1_or_null,
                "npg_tracers_rhs: tracer %d has a background gradient (gamma = %g) but rhs_diff1 is NULL", k, T->gamma[(size_t)k]);
        lift = lift || T->lift[(size_t)k] || (iso && T->gamma[(size_t)k] != 0.0);
    }
    REQUIRE(!lift || ((iso || !fe->coef[1].empty()) && !fe->coef[2].empty()),
            "npg_tracers_rhs: a tracer has non-zero Dirichlet values but the coefficients kappa_h / kappa_v have not been set");
    const HostShape s = host_shape(fe);
    const npg::TracerCells<HostView> t{host_view(fe)};
    const npg::RediCells<HostView> ti{host_view(fe), T->kiso.data(), T->kxz.data(), T->kyz.data(), T->kzz.data()};
    const npg::TracerSet ts{K, nb, T->n_diri, nc * fe->nb, c->d, c_prev->d, T->diri.data(), T->gamma.data(), T->source.data(), T->loc.data()};
    const bool bdf2 = scheme == NPG_BDF2;
#pragma omp parallel for schedule(static)
    for (int64_t cell = 0; cell < nc; ++cell) {
        HostTrVel uq;
        if (iso) {
            if (fe->nb == 10) npg::cell_tracers<double, 10, true>(s, ti, uq, fe->nq, bdf2, dt, theta, x_inv->d, x_inv_prev->d, ts, cell);
            else npg::cell_tracers<double, 4, true>(s, ti, uq, fe->nq, bdf2, dt, theta, x_inv->d, x_inv_prev->d, ts, cell);
        } else if (fe->nb == 10) npg::cell_tracers<double, 10>(s, t, uq, fe->nq, bdf2, dt, theta, x_inv->d, x_inv_prev->d, ts, cell);
        else npg::cell_tracers<double, 4>(s, t, uq, fe->nq, bdf2, dt, theta, x_inv->d, x_inv_prev->d, ts, cell);
    }
#pragma omp parallel for schedule(static) collapse(2)
    for (int k = 0; k < K; ++k)
        for (int64_t r = 0; r < nb; ++r)
            y->d[(size_t)k * nb + r] = npg::tracer_row(fe->gptr.data(), fe->gidx.data(), T->loc.data() + (size_t)k * ts.loc_stride, r,
                                                       theta * T->gamma[(size_t)k], dt, rhs_diff1_or_null && !iso ? rhs_diff1_or_null->d : nullptr,
                                                       flux_or_null ? flux_or_null->d + (size_t)k * nb : nullptr);
    return NPG_OK;
}

// ---- isoneutral mixing of the tracers (csrc/tracers.hip on the host; the arithmetic is csrc/redi_core.h) ------------------------------
NPG_API int npg_tracers_set_isoneutral(npg_tracers *T, const double *kappa_iso_or_null, double slope_max, double bz_min) {
    REQUIRE(T, "npg_tracers_set_isoneutral: NULL handle");
    npg_fe *fe = T->fe;
    const int64_t nc = fe->ncell;
    const int nq = fe->nq;
    npg::RediCheck a{"npg_tracers_set_isoneutral"};
    a.set = true, a.kiso = kappa_iso_or_null, a.npts = nc * nq, a.slope_max = slope_max, a.bz_min = bz_min;
    a.flat = true;
    for (int q = 0; q < nq; ++q) a.flat = a.flat && fe->N1[(size_t)q * 4 + 3] == 0.0;
    REQUIRE_OK(npg::check_redi(a));
    if (!kappa_iso_or_null) {
        T->iso = npg::kRediOff;
        T->kiso.clear(), T->kxz.clear(), T->kyz.clear(), T->kzz.clear();
        return NPG_OK;
    }
    T->kiso.resize((size_t)nc * nq);
    for (int64_t c = 0; c < nc; ++c)                       // [nq][ncell] -> the host tables' [cell][q]
        for (int q = 0; q < nq; ++q) T->kiso[(size_t)c * nq + q] = kappa_iso_or_null[(size_t)q * nc + c];
    T->kxz.assign((size_t)nc * nq, 0.0), T->kyz.assign((size_t)nc * nq, 0.0), T->kzz.assign((size_t)nc * nq, 0.0);
    T->slope_max = slope_max, T->bz_min = bz_min;
    T->nfloor = T->nclip = 0;
    T->iso = npg::kRediSet;
    return NPG_OK;
}
NPG_API int npg_tracers_isoneutral_update(npg_tracers *T, double N2, const npg_vec *b) {
    REQUIRE(T && b, "npg_tracers_isoneutral_update: NULL argument");
    npg_fe *fe = T->fe;
    npg::RediCheck a{"npg_tracers_isoneutral_update"};
    a.need = npg::kRediSet, a.state = T->iso, a.n_b = fe->n_b, a.vec_n = b->n, a.N2 = N2;
    REQUIRE_OK(npg::check_redi(a));
    const HostShape s = host_shape(fe);
    const HostView t = host_view(fe);
    int64_t nfloor = 0, nclip = 0;
#pragma omp parallel for schedule(static) reduction(+ : nfloor, nclip)
    for (int64_t cell = 0; cell < fe->ncell; ++cell) {
        int nf = 0, ncl = 0;
        if (fe->nb == 10)
            npg::cell_redi_update<10>(s, t, fe->nq, N2, b->d, T->kiso.data(), T->slope_max, T->bz_min, cell, T->kxz.data(), T->kyz.data(),
                                      T->kzz.data(), nf, ncl);
        else
            npg::cell_redi_update<4>(s, t, fe->nq, N2, b->d, T->kiso.data(), T->slope_max, T->bz_min, cell, T->kxz.data(), T->kyz.data(),
                                     T->kzz.data(), nf, ncl);
        nfloor += nf, nclip += ncl;
    }
    T->nfloor = nfloor, T->nclip = nclip;
    T->iso = npg::kRediUpdated;
    return NPG_OK;
}
NPG_API int npg_tracers_isoneutral_matrix(npg_tracers *T, npg_csr *K) {
    REQUIRE(T && K, "npg_tracers_isoneutral_matrix: NULL argument");
    npg_fe *fe = T->fe;
    npg::RediCheck a{"npg_tracers_isoneutral_matrix"};
    a.need = npg::kRediUpdated, a.state = T->iso, a.n_b = fe->n_b, a.mat_m = K->m, a.mat_n = K->n;
    REQUIRE_OK(npg::check_redi(a));
    const int nb = fe->nb, nq = fe->nq;
    std::fill(K->val.begin(), K->val.end(), 0.0);
    int64_t missing = 0;
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : missing)
    for (int64_t r = 0; r < K->m; ++r) {
        for (int64_t k = fe->gptr[(size_t)r]; k < fe->gptr[(size_t)r + 1]; ++k) {
            const int64_t cell = fe->gidx[(size_t)k] / nb;
            const int i = (int)(fe->gidx[(size_t)k] % nb);
            const double *G = &fe->G[(size_t)cell * 12];
            double acc[10] = {0};
            for (int q = 0; q < nq; ++q) {
                const double w = fe->qw[(size_t)q] * fe->wdet[(size_t)cell];
                const size_t o = (size_t)cell * nq + q;
                double gi[3];
                grad_of(fe->dNb.data(), nb, G, q, i, gi);
                for (int j = 0; j < nb; ++j) {
                    double gj[3];
                    grad_of(fe->dNb.data(), nb, G, q, j, gj);
                    acc[j] += npg::redi_entry(w, T->kiso[o], T->kxz[o], T->kyz[o], T->kzz[o], gi[0], gi[1], gi[2], gj[0], gj[1], gj[2]);
                }
            }
            for (int j = 0; j < nb; ++j) {
                const int32_t c = fe->cb[(size_t)cell * nb + j];
                if (c < 0) continue;                       // Dirichlet columns: the lift is per tracer (npg_tracers_rhs)
                const int64_t sl = slot_of(K, r, c);
                if (sl >= 0) K->val[(size_t)sl] += acc[j];
                else if (acc[j] != 0.0) ++missing;
            }
        }
    }
    REQUIRE(missing == 0, "npg_tracers_isoneutral_matrix: %lld non-zero local entries fall outside the matrix's pattern: it is not the buoyancy pattern",
            (long long)missing);
    return NPG_OK;
}
NPG_API int npg_tracers_isoneutral_tables(npg_tracers *T, double *kxz, double *kyz, double *kzz) {
    REQUIRE(T && kxz && kyz && kzz, "npg_tracers_isoneutral_tables: NULL argument");
    npg::RediCheck a{"npg_tracers_isoneutral_tables"};
    a.need = npg::kRediUpdated, a.state = T->iso;
    REQUIRE_OK(npg::check_redi(a));
    const int64_t nc = T->fe->ncell;
    const int nq = T->fe->nq;
    for (int64_t c = 0; c < nc; ++c)
        for (int q = 0; q < nq; ++q) {
            const size_t o = (size_t)c * nq + q, e = (size_t)q * nc + c;
            kxz[e] = T->kxz[o], kyz[e] = T->kyz[o], kzz[e] = T->kzz[o];
        }
    return NPG_OK;
}
// ---- the tracers' transport operator as a matrix (csrc/tracers.hip on the host; the arithmetic is csrc/transport_core.h) -----------------
NPG_API int npg_tracers_transport_update(npg_tracers *T, const npg_vec *x_inv, double scale) {
    REQUIRE(T && x_inv, "npg_tracers_transport_update: NULL argument");
    npg_fe *fe = T->fe;
    const int64_t nc = fe->ncell;
    const int nq = fe->nq;
    npg::TransportCheck a{"npg_tracers_transport_update"};
    a.same_ctx = x_inv->ctx == fe->ctx;
    a.update = true, a.scale = scale, a.n_inv = fe->n_inv, a.vec_n = x_inv->n;
    a.flat = true;
    for (int q = 0; q < nq; ++q) a.flat = a.flat && fe->N1[(size_t)q * 4 + 3] == 0.0;
    REQUIRE_OK(npg::check_transport(a));
    T->tux.resize((size_t)nc * nq), T->tuy.resize((size_t)nc * nq), T->tuz.resize((size_t)nc * nq);
    const HostShape s = host_shape(fe);
    const HostView t = host_view(fe);
#pragma omp parallel for schedule(static)
    for (int64_t cell = 0; cell < nc; ++cell)
        npg::cell_transport_velocity(s, t, nq, scale, x_inv->d, cell, T->tux.data(), T->tuy.data(), T->tuz.data());
    T->transport = npg::kTransportUpdated;
    return NPG_OK;
}
NPG_API int npg_tracers_transport_matrix(npg_tracers *T, npg_csr *Cm) {
    REQUIRE(T && Cm, "npg_tracers_transport_matrix: NULL argument");
    npg_fe *fe = T->fe;
    npg::TransportCheck a{"npg_tracers_transport_matrix"};
    a.same_ctx = Cm->ctx == fe->ctx;
    a.need = npg::kTransportUpdated, a.state = T->transport, a.n_b = fe->n_b, a.mat_m = Cm->m, a.mat_n = Cm->n;
    REQUIRE_OK(npg::check_transport(a));
    const int nb = fe->nb, nq = fe->nq;
    std::fill(Cm->val.begin(), Cm->val.end(), 0.0);
    int64_t missing = 0;
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : missing)
    for (int64_t r = 0; r < Cm->m; ++r) {
        for (int64_t k = fe->gptr[(size_t)r]; k < fe->gptr[(size_t)r + 1]; ++k) {
            const int64_t cell = fe->gidx[(size_t)k] / nb;
            const int i = (int)(fe->gidx[(size_t)k] % nb);
            const double *G = &fe->G[(size_t)cell * 12];
            double acc[10] = {0};
            for (int q = 0; q < nq; ++q) {
                const double w = fe->qw[(size_t)q] * fe->wdet[(size_t)cell];
                const size_t o = (size_t)cell * nq + q;
                const double phi = fe->Nb[(size_t)q * nb + i];
                for (int j = 0; j < nb; ++j) {
                    double gj[3];
                    grad_of(fe->dNb.data(), nb, G, q, j, gj);
                    acc[j] += npg::transport_entry(w, phi, T->tux[o], T->tuy[o], T->tuz[o], gj[0], gj[1], gj[2]);
                }
            }
            for (int j = 0; j < nb; ++j) {
                const int32_t c = fe->cb[(size_t)cell * nb + j];
                if (c < 0) continue;                       // Dirichlet columns: the lift is per tracer (the load)
                const int64_t sl = slot_of(Cm, r, c);
                if (sl >= 0) Cm->val[(size_t)sl] += acc[j];
                else if (acc[j] != 0.0) ++missing;
            }
        }
    }
    REQUIRE(missing == 0, "npg_tracers_transport_matrix: %lld non-zero local entries fall outside the matrix's pattern: it is not the buoyancy pattern",
            (long long)missing);
    return NPG_OK;
}
NPG_API int npg_tracers_transport_load(npg_tracers *T, double kappa_hat, const double *decay_or_null, const npg_vec *rhs_diff1_or_null,
                                       const npg_vec *flux_or_null, npg_vec *out) {
    REQUIRE(T && out, "npg_tracers_transport_load: NULL argument");
    npg_fe *fe = T->fe;
    const int K = T->ntracer;
    const int64_t nb = fe->n_b, nc = fe->ncell;
    npg::TransportCheck a{"npg_tracers_transport_load"};
    for (const npg_vec *v : {rhs_diff1_or_null, flux_or_null, (const npg_vec *)out}) a.same_ctx = a.same_ctx && (!v || v->ctx == fe->ctx);
    a.load = true, a.kappa_hat = kappa_hat, a.decay = decay_or_null, a.ntracer = K, a.n_b = nb;
    a.need = npg::kTransportUpdated, a.state = T->transport;
    a.out_n = out->n, a.flux_n = flux_or_null ? flux_or_null->n : -1, a.diff1_n = rhs_diff1_or_null ? rhs_diff1_or_null->n : -1;
    bool lift = false;
    for (int k = 0; k < K; ++k) {
        a.need_diff1 = a.need_diff1 || T->gamma[(size_t)k] != 0.0;
        lift = lift || T->lift[(size_t)k];
    }
    a.need_coeff = lift && (fe->coef[1].empty() || fe->coef[2].empty());
    REQUIRE_OK(npg::check_transport(a));
    const HostShape s = host_shape(fe);
    const npg::TransportCells<HostView> t{host_view(fe), T->tux.data(), T->tuy.data(), T->tuz.data()};
    const npg::TracerSet ts{K, nb, T->n_diri, nc * fe->nb, nullptr, nullptr, T->diri.data(), T->gamma.data(), T->source.data(), T->loc.data()};
#pragma omp parallel for schedule(static)
    for (int64_t cell = 0; cell < nc; ++cell) {
        HostTrVel uq;
        if (fe->nb == 10) npg::cell_transport_load<10>(s, t, uq, fe->nq, kappa_hat, decay_or_null, ts, cell);
        else npg::cell_transport_load<4>(s, t, uq, fe->nq, kappa_hat, decay_or_null, ts, cell);
    }
#pragma omp parallel for schedule(static) collapse(2)
    for (int k = 0; k < K; ++k)
        for (int64_t r = 0; r < nb; ++r)
            out->d[(size_t)k * nb + r] = npg::tracer_row(fe->gptr.data(), fe->gidx.data(), T->loc.data() + (size_t)k * ts.loc_stride, r,
                                                         kappa_hat * T->gamma[(size_t)k], 1.0, rhs_diff1_or_null ? rhs_diff1_or_null->d : nullptr,
                                                         flux_or_null ? flux_or_null->d + (size_t)k * nb : nullptr);
    return NPG_OK;
}
NPG_API int npg_tracers_transport_tables(npg_tracers *T, double *ux, double *uy, double *uz) {
    REQUIRE(T && ux && uy && uz, "npg_tracers_transport_tables: NULL argument");
    npg::TransportCheck a{"npg_tracers_transport_tables"};
    a.need = npg::kTransportUpdated, a.state = T->transport;
    REQUIRE_OK(npg::check_transport(a));
    const int64_t nc = T->fe->ncell;
    const int nq = T->fe->nq;
    for (int64_t c = 0; c < nc; ++c)
        for (int q = 0; q < nq; ++q) {
            const size_t o = (size_t)c * nq + q, e = (size_t)q * nc + c;
            ux[e] = T->tux[o], uy[e] = T->tuy[o], uz[e] = T->tuz[o];
        }
    return NPG_OK;
}
NPG_API int npg_tracers_transport_info(npg_tracers *T, int *state, double *umax) {
    REQUIRE(T, "npg_tracers_transport_info: NULL handle");
    double um = 0.0;
    if (T->transport == npg::kTransportUpdated)
        for (size_t o = 0; o < T->tux.size(); ++o) um = std::max(um, std::sqrt(T->tux[o] * T->tux[o] + T->tuy[o] * T->tuy[o] + T->tuz[o] * T->tuz[o]));
    if (state) *state = T->transport;
    if (umax) *umax = um;
    return NPG_OK;
}
NPG_API int npg_tracers_isoneutral_info(npg_tracers *T, int64_t *nfloored, int64_t *nclipped, int64_t *npoints, int *state) {
    REQUIRE(T, "npg_tracers_isoneutral_info: NULL handle");
    const bool up = T->iso == npg::kRediUpdated;
    if (nfloored) *nfloored = up ? T->nfloor : 0;
    if (nclipped) *nclipped = up ? T->nclip : 0;
    if (npoints) *npoints = T->iso == npg::kRediOff ? 0 : T->fe->ncell * T->fe->nq;
    if (state) *state = T->iso;
    return NPG_OK;
}
