// Passive tracers carried by the flow (npg_tracers_rhs): the right-hand sides of K advection-diffusion equations that share the
// model's velocity, matrix and time scheme, in two launches.  The reference has no counterpart (it evolves b' alone).
//   k_tracers_local<R, NB>  pass 1, one lane per cell: u~ at the quadrature points ONCE (30 scattered velocity values, 12 geometry
//                           values, the velocity shape table), then a run-time loop over the tracers that reloads only the tracer's
//                           nodal values (cell_tracers, tracers_core.h).  Writes loc[k][i][cell] into the handle's own buffer;
//                           fe->loc is not touched.  The nq x 3 velocities of a lane live in a column of dynamic LDS
//                           (uq[3 q + a][lane]: consecutive lanes, consecutive words - no bank conflict): as a register array they
//                           are indexed at run time and go to scratch, and fully unrolled the kernel spills.  kTrBlock = 128 lanes
//                           keep 3 nq columns of doubles beside the staged tables within 64 KiB; no instance uses scratch.
//   k_tracers_gather        pass 2, one thread per (tracer, row): the row's local entries through the engine's inverted index in cell
//                           order, + theta Gamma_k rhs_diff1[r] + dt flux_k[r].  No atomics: the same bits on every call.
#include <cmath>

#include "common.h"
#include "device_utils.h"
#include "fe_dev.h"
#include "tracers_core.h"

static_assert(npg::kTrMaxQ == npg::kMaxQ, "a lane column holds the engine's largest rule");

namespace npg {

constexpr int kTrBlock = 128;

// a lane's nq x 3 velocities: column `lane` of uq[3 nq][kTrBlock]
template <typename R>
struct LaneColumn {
    R *p;
    __device__ __forceinline__ R &operator()(int j) const { return p[j * kTrBlock]; }
};

template <typename R, int NB>
__global__ void __launch_bounds__(kTrBlock) __attribute__((amdgpu_waves_per_eu(2))) k_tracers_local(FeDev d, int bdf2, double dt, double theta, const double *xi,
                                                          const double *xip, TracerSet ts) {
    __shared__ FeTablesT<R> t;
    stage_tables(d, t);
    extern __shared__ double uq_lds[];                                   // 3 nq kTrBlock values of R
    const int64_t cell = blockIdx.x * (int64_t)kTrBlock + threadIdx.x;
    if (cell >= d.ncell) return;
    const TracerCells<DevCells> cells{cell_view(d)};
    LaneColumn<R> uq{reinterpret_cast<R *>(uq_lds) + threadIdx.x};
    cell_tracers<R, NB>(t, cells, uq, d.nq, bdf2 != 0, dt, theta, xi, xip, ts, cell);
}

// out[k][r], k = blockIdx.y
__global__ void __launch_bounds__(kBlock) k_tracers_gather(const int64_t *gptr, const int32_t *gidx, int64_t n, TracerSet ts,
                                                           double theta, double dt, const double *rhs_diff1, const double *flux,
                                                           double *out) {
    const int k = blockIdx.y;
    const double *lock = ts.loc + (size_t)k * ts.loc_stride;
    const double *fk = flux ? flux + (size_t)k * n : nullptr;
    const double tg = theta * ts.gamma[k];
    for (int64_t r = blockIdx.x * (int64_t)kBlock + threadIdx.x; r < n; r += (int64_t)gridDim.x * kBlock)
        out[(size_t)k * n + r] = tracer_row(gptr, gidx, lock, r, tg, dt, rhs_diff1, fk);
}

}  // namespace npg

using namespace npg;

struct npg_tracers {
    npg_ctx *ctx = nullptr;
    npg_fe *fe = nullptr;
    int ntracer = 0;
    int64_t n_diri = 0;              // Dirichlet values per tracer (at least 1 stored)
    DevBuf<double> loc;              // [ntracer][nb][ncell]
    DevBuf<double> diri;             // [ntracer][max(1, n_b_diri)]
    DevBuf<double> gamma;            // [ntracer]
    DevBuf<double> source;           // [ntracer]
    std::vector<double> h_gamma;
    std::vector<uint8_t> h_lift;     // tracer k has a non-zero Dirichlet value
};

NPG_API int npg_tracers_destroy(npg_tracers *T) {
    if (!T) return NPG_OK;
    hipStreamSynchronize(T->ctx->stream);
    delete T;
    return NPG_OK;
}

NPG_API int npg_tracers_create(npg_fe *fe, int ntracer, npg_tracers **out) {
    NPG_REQUIRE(fe && out, "npg_tracers_create: NULL argument");
    NPG_REQUIRE(ntracer >= 1, "npg_tracers_create: ntracer must be at least 1, got %d", ntracer);
    NPG_REQUIRE(ntracer <= 65535, "npg_tracers_create: at most 65535 tracers, got %d", ntracer);
    NPG_HIP(hipSetDevice(fe->ctx->device));
    std::unique_ptr<npg_tracers> T(new npg_tracers());
    T->ctx = fe->ctx;
    T->fe = fe;
    T->ntracer = ntracer;
    T->n_diri = std::max<int64_t>(1, fe->n_b_diri);
    T->h_gamma.assign((size_t)ntracer, 0.0);
    T->h_lift.assign((size_t)ntracer, 0);
    const size_t nloc = (size_t)ntracer * fe->d.nb * fe->d.ncell, nd = (size_t)ntracer * T->n_diri;
    NPG_HIP(T->loc.alloc(nloc));
    NPG_HIP(T->diri.zeros(nd));
    NPG_HIP(T->gamma.zeros((size_t)ntracer));
    NPG_HIP(T->source.zeros((size_t)ntracer));
    *out = T.release();
    return NPG_OK;
}

NPG_API int npg_tracers_set(npg_tracers *T, int k, const double *diri_or_null, double gamma, double source) {
    NPG_REQUIRE(T, "npg_tracers_set: NULL handle");
    NPG_REQUIRE(k >= 0 && k < T->ntracer, "npg_tracers_set: tracer %d out of range (ntracer = %d)", k, T->ntracer);
    NPG_REQUIRE(std::isfinite(gamma) && std::isfinite(source), "npg_tracers_set: gamma and source must be finite");
    const int64_t nd = T->fe->n_b_diri;
    std::vector<double> dv((size_t)T->n_diri, 0.0);
    bool any = false;
    if (diri_or_null)
        for (int64_t j = 0; j < nd; ++j) {
            NPG_REQUIRE(std::isfinite(diri_or_null[j]), "npg_tracers_set: Dirichlet value %lld is not finite", (long long)j);
            dv[(size_t)j] = diri_or_null[j];
            any = any || diri_or_null[j] != 0.0;
        }
    NPG_HIP(hipSetDevice(T->ctx->device));
    // kernels that read these tables run on ctx->stream (not ordered with the null stream) - drain it first
    NPG_HIP(hipStreamSynchronize(T->ctx->stream));
    NPG_HIP(hipMemcpy(T->diri + (size_t)k * T->n_diri, dv.data(), dv.size() * sizeof(double), hipMemcpyHostToDevice));
    NPG_HIP(hipMemcpy(T->gamma + k, &gamma, sizeof(double), hipMemcpyHostToDevice));
    NPG_HIP(hipMemcpy(T->source + k, &source, sizeof(double), hipMemcpyHostToDevice));
    T->h_gamma[(size_t)k] = gamma;
    T->h_lift[(size_t)k] = any;
    return NPG_OK;
}

NPG_API int npg_tracers_rhs(npg_tracers *T, int scheme, double dt, double theta, const npg_vec *c, const npg_vec *c_prev,
                            const npg_vec *x_inv, const npg_vec *x_inv_prev, const npg_vec *rhs_diff1_or_null,
                            const npg_vec *flux_or_null, npg_vec *y) {
    NPG_REQUIRE(T, "npg_tracers_rhs: NULL handle");
    NPG_REQUIRE(c && c_prev && x_inv && x_inv_prev && y, "npg_tracers_rhs: NULL state vector");
    npg_fe *fe = T->fe;
    const int K = T->ntracer;
    const int64_t nb = fe->n_b;
    NPG_REQUIRE(scheme == NPG_BDF1 || scheme == NPG_BDF2, "npg_tracers_rhs: scheme must be NPG_BDF1 or NPG_BDF2, got %d", scheme);
    NPG_REQUIRE(c->n == K * nb && c_prev->n == K * nb, "npg_tracers_rhs: tracer vectors must have ntracer * n_b = %lld entries",
                (long long)(K * nb));
    NPG_REQUIRE(y->n == K * nb, "npg_tracers_rhs: the output vector must have ntracer * n_b = %lld entries", (long long)(K * nb));
    NPG_REQUIRE(x_inv->n == fe->n_inv && x_inv_prev->n == fe->n_inv, "npg_tracers_rhs: inversion vectors must have %lld entries",
                (long long)fe->n_inv);
    NPG_REQUIRE(!rhs_diff1_or_null || rhs_diff1_or_null->n == nb, "npg_tracers_rhs: rhs_diff1 must have n_b = %lld entries", (long long)nb);
    NPG_REQUIRE(!flux_or_null || flux_or_null->n == K * nb, "npg_tracers_rhs: flux must have ntracer * n_b = %lld entries",
                (long long)(K * nb));
    bool lift = false;
    for (int k = 0; k < K; ++k) {
        NPG_REQUIRE(T->h_gamma[(size_t)k] == 0.0 || rhs_diff1_or_null,
                    "npg_tracers_rhs: tracer %d has a background gradient (gamma = %g) but rhs_diff1 is NULL", k, T->h_gamma[(size_t)k]);
        lift = lift || T->h_lift[(size_t)k];
    }
    NPG_REQUIRE(!lift || (fe->d.kh && fe->d.kv),
                "npg_tracers_rhs: a tracer has non-zero Dirichlet values but the coefficients kappa_h / kappa_v have not been set");
    for (const npg_vec *v : {c, c_prev, x_inv, x_inv_prev, rhs_diff1_or_null, flux_or_null, (const npg_vec *)y})
        NPG_REQUIRE(!v || v->ctx == fe->ctx, "npg_tracers_rhs: arguments of different contexts");
    NPG_HIP(hipSetDevice(fe->ctx->device));
    hipStream_t st = fe->ctx->stream;
    const FeDev &d = fe->d;
    TracerSet ts{K, nb, T->n_diri, (int64_t)d.nb * d.ncell, c->d, c_prev->d, T->diri, T->gamma, T->source, T->loc};
    const bool f32 = fe->precision == NPG_FE_FP32;
    const int grid = (int)((d.ncell + kTrBlock - 1) / kTrBlock);
    const size_t lds = (size_t)3 * d.nq * kTrBlock * (f32 ? sizeof(float) : sizeof(double));
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(kTrBlock), lds, st, d, (int)(scheme == NPG_BDF2), dt, theta, x_inv->d, x_inv_prev->d, ts);
    };
    if (d.nb == 10) f32 ? go(k_tracers_local<float, 10>) : go(k_tracers_local<double, 10>);
    else f32 ? go(k_tracers_local<float, 4>) : go(k_tracers_local<double, 4>);
    NPG_HIP(hipGetLastError());
    const int ggrid = (int)std::min<int64_t>(2048, (nb + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_tracers_gather, dim3(ggrid, K), dim3(kBlock), 0, st, fe->gptr, fe->gidx, nb, ts, theta, dt,
                       rhs_diff1_or_null ? rhs_diff1_or_null->d : nullptr, flux_or_null ? flux_or_null->d : nullptr, y->d);
    NPG_HIP(hipGetLastError());
    return NPG_OK;
}
