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
// Isoneutral mixing (npg_tracers_set_isoneutral, redi_core.h): the tracers' own rotated diffusion tensor.
//   k_redi_update<NB>       one lane per cell, shape tables in LDS as k_coeff_from_bz: grad B at the cell's quadrature points, the floor
//                           and the clip, the three tensor tables, and the workgroup's floored / clipped counts (wave sums folded in
//                           wave order: no atomics).
//   k_redi_matrix<NB>       K_iso on the buoyancy pattern with the skeleton of k_assemble_b: sixteen lanes own a CSR row, lane =
//                           quadrature point, the row's (cell, local DoF) pairs in cell order, the DPP tree, row_add.  fp64 always.
//   k_tracers_local_iso     pass 1 with the rotated tensor in the second integral (cell_tracers<R, NB, true>); the instances of
//                           k_tracers_local are not touched by the flag.
// The transport operator as a matrix (npg_tracers_transport_*, transport_core.h): equilibria and implicit steps.
//   k_transport_velocity    one lane per cell, shape tables in LDS as k_redi_update: the three velocity tables ux, uy, uz at the cell's
//                           quadrature points from its 30 velocity values.
//   k_transport_matrix<NB>  C on the buoyancy pattern with the skeleton of k_redi_matrix: sixteen lanes own a CSR row, lane =
//                           quadrature point, three tables and three products per pair.  fp64 always, no atomics.
//   k_transport_load<NB>    one lane per cell: the local loads of all K tracers (cell_transport_load); the cell's velocities are read
//                           from the tables once into the lane's LDS column (as k_tracers_local), then a run-time loop over the
//                           tracers.  The rows are then gathered by k_tracers_gather.
#include <cmath>

#include "common.h"
#include "device_utils.h"
#include "fe_dev.h"
#include "redi_core.h"
#include "tracers_core.h"
#include "transport_core.h"

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

// the mode's tables, [nq][ncell] each
struct RediDev {
    const double *kiso, *kxz, *kyz, *kzz;
};

template <typename R, int NB>
__global__ void __launch_bounds__(kTrBlock) __attribute__((amdgpu_waves_per_eu(2))) k_tracers_local_iso(FeDev d, RediDev rd, int bdf2, double dt, double theta,
                                                              const double *xi, const double *xip, TracerSet ts) {
    __shared__ FeTablesT<R> t;
    stage_tables(d, t);
    extern __shared__ double uq_lds[];
    const int64_t cell = blockIdx.x * (int64_t)kTrBlock + threadIdx.x;
    if (cell >= d.ncell) return;
    const RediCells<DevCells> cells{cell_view(d), rd.kiso, rd.kxz, rd.kyz, rd.kzz};
    LaneColumn<R> uq{reinterpret_cast<R *>(uq_lds) + threadIdx.x};
    cell_tracers<R, NB, true>(t, cells, uq, d.nq, bdf2 != 0, dt, theta, xi, xip, ts, cell);
}

// counts[2 blockIdx.x + {0, 1}] = the workgroup's floored / clipped points
template <int NB>
__global__ void __launch_bounds__(kBlock) k_redi_update(FeDev d, double N2, const double *b, const double *kiso, double slope_max, double bz_min,
                                                        double *kxz, double *kyz, double *kzz, int32_t *counts) {
    __shared__ FeTables t;
    __shared__ int32_t shc[2 * (kBlock / kWave)];
    stage_tables(d, t);
    const int64_t cell = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    int nfloor = 0, nclip = 0;
    if (cell < d.ncell) cell_redi_update<NB>(t, cell_view(d), d.nq, N2, b, kiso, slope_max, bz_min, cell, kxz, kyz, kzz, nfloor, nclip);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        nfloor += __shfl_xor(nfloor, off, kWave);
        nclip += __shfl_xor(nclip, off, kWave);
    }
    if ((threadIdx.x & (kWave - 1)) == 0) shc[2 * (threadIdx.x / kWave)] = nfloor, shc[2 * (threadIdx.x / kWave) + 1] = nclip;
    __syncthreads();
    if (threadIdx.x < 2) {
        int32_t s = 0;
#pragma unroll
        for (int w = 0; w < kBlock / kWave; ++w) s += shc[2 * w + threadIdx.x];
        counts[2 * (size_t)blockIdx.x + threadIdx.x] = s;
    }
}

template <int NB>
__global__ void __launch_bounds__(kBlock) k_redi_matrix(FeDev d, RediDev rd, const int64_t *gptr, const int32_t *gidx, int64_t nrows,
                                                        const int64_t *rowptr, const int32_t *col, double *val, int *missing) {
    __shared__ FeTables t;
    stage_tables(d, t);
    const int64_t r = (blockIdx.x * (int64_t)kBlock + threadIdx.x) / kQL;
    const int q = threadIdx.x % kQL;
    if (r >= nrows) return;                                  // whole lane groups leave together
    const int32_t row = (int32_t)r;
    const bool on = q < d.nq;
    for (int64_t k = gptr[r]; k < gptr[r + 1]; ++k) {
        const int64_t cell = gidx[k] % d.ncell;
        const int i = (int)(gidx[k] / d.ncell);
        double acc[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[j] = 0.0;
        if (on) {
            const double w = t.qw[q] * d.wdet[cell];
            const size_t o = (size_t)q * d.ncell + cell;
            const double ki = rd.kiso[o], kxz = rd.kxz[o], kyz = rd.kyz[o], kzz = rd.kzz[o];
            double G[12];
#pragma unroll
            for (int e = 0; e < 12; ++e) G[e] = d.G[(size_t)e * d.ncell + cell];
            double gix, giy, giz;
            grad_b<double, NB>(t, G, q, i, gix, giy, giz);
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                double gx, gy, gz;
                grad_b<double, NB>(t, G, q, j, gx, gy, gz);
                acc[j] = redi_entry(w, ki, kxz, kyz, kzz, gix, giy, giz, gx, gy, gz);
            }
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[j] = group_sum_dpp<kQL>(acc[j]);
        // lane j adds column j; Dirichlet columns are skipped (their lift is per tracer: the right-hand side)
        double mine = 0.0;
#pragma unroll
        for (int j = 0; j < NB; ++j) mine = (q == j) ? acc[j] : mine;
        if (q < NB) {
            const int32_t c = d.cb[(size_t)q * d.ncell + cell];
            if (c >= 0) row_add(rowptr, col, val, row, c, mine, missing);
        }
        __builtin_amdgcn_s_waitcnt(0);                       // this cell's stores are out before the next cell's loads
    }
}

// the velocity tables, [nq][ncell] each
struct TransportDev {
    const double *ux, *uy, *uz;
};

__global__ void __launch_bounds__(kBlock) k_transport_velocity(FeDev d, double scale, const double *xi, double *ux, double *uy, double *uz) {
    __shared__ FeTables t;
    stage_tables(d, t);
    const int64_t cell = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    if (cell < d.ncell) cell_transport_velocity(t, cell_view(d), d.nq, scale, xi, cell, ux, uy, uz);
}

template <int NB>
__global__ void __launch_bounds__(kBlock) k_transport_matrix(FeDev d, TransportDev td, const int64_t *gptr, const int32_t *gidx, int64_t nrows,
                                                             const int64_t *rowptr, const int32_t *col, double *val, int *missing) {
    __shared__ FeTables t;
    stage_tables(d, t);
    const int64_t r = (blockIdx.x * (int64_t)kBlock + threadIdx.x) / kQL;
    const int q = threadIdx.x % kQL;
    if (r >= nrows) return;                                  // whole lane groups leave together
    const int32_t row = (int32_t)r;
    const bool on = q < d.nq;
    for (int64_t k = gptr[r]; k < gptr[r + 1]; ++k) {
        const int64_t cell = gidx[k] % d.ncell;
        const int i = (int)(gidx[k] / d.ncell);
        double acc[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[j] = 0.0;
        if (on) {
            const double w = t.qw[q] * d.wdet[cell];
            const size_t o = (size_t)q * d.ncell + cell;
            const double ux = td.ux[o], uy = td.uy[o], uz = td.uz[o];
            const double phi = t.Nb[q * NB + i];
            double G[12];
#pragma unroll
            for (int e = 0; e < 12; ++e) G[e] = d.G[(size_t)e * d.ncell + cell];
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                double gx, gy, gz;
                grad_b<double, NB>(t, G, q, j, gx, gy, gz);
                acc[j] = transport_entry(w, phi, ux, uy, uz, gx, gy, gz);
            }
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[j] = group_sum_dpp<kQL>(acc[j]);
        // lane j adds column j; Dirichlet columns are skipped (their lift is per tracer: the load)
        double mine = 0.0;
#pragma unroll
        for (int j = 0; j < NB; ++j) mine = (q == j) ? acc[j] : mine;
        if (q < NB) {
            const int32_t c = d.cb[(size_t)q * d.ncell + cell];
            if (c >= 0) row_add(rowptr, col, val, row, c, mine, missing);
        }
        __builtin_amdgcn_s_waitcnt(0);                       // this cell's stores are out before the next cell's loads
    }
}

// (kTrBlock lanes and the nq x 3 velocities of a lane in a column of dynamic LDS, as k_tracers_local)
template <int NB>
__global__ void __launch_bounds__(kTrBlock) k_transport_load(FeDev d, TransportDev td, double kappa_hat, const double *decay, TracerSet ts) {
    __shared__ FeTables t;
    stage_tables(d, t);
    extern __shared__ double uq_lds[];                                   // 3 nq kTrBlock doubles
    const int64_t cell = blockIdx.x * (int64_t)kTrBlock + threadIdx.x;
    if (cell >= d.ncell) return;
    const TransportCells<DevCells> cells{cell_view(d), td.ux, td.uy, td.uz};
    LaneColumn<double> uq{uq_lds + threadIdx.x};
    cell_transport_load<NB>(t, cells, uq, d.nq, kappa_hat, decay, ts, cell);
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
    // isoneutral mixing (npg_tracers_set_isoneutral): kappa_iso and the tensor tables [nq][ncell], the update's per-workgroup counts
    int iso = kRediOff;
    double slope_max = 0.0, bz_min = 0.0;
    DevBuf<double> kiso, kxz, kyz, kzz;
    DevBuf<int32_t> counts;          // [2 iso_grid]
    DevBuf<int> missing;
    int iso_grid = 0;
    // the transport operator (npg_tracers_transport_update): the velocity tables [nq][ncell], the decay rates of the last load
    int transport = kTransportOff;
    int flat = -1;                   // the engine is an embedded 2-D one (-1: not looked at yet)
    DevBuf<double> tux, tuy, tuz, decay;
};

static bool engine_is_flat(const npg_fe *fe, int *rc) {   // an embedded 2-D engine pads its triangles to tetrahedra: N1[q][3] = 0
    std::vector<double> n1((size_t)fe->d.nq * 4);
    *rc = hipMemcpy(n1.data(), fe->d.N1, n1.size() * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess ? NPG_OK : NPG_EHIP;
    bool flat = true;
    for (int q = 0; q < fe->d.nq; ++q) flat = flat && n1[(size_t)q * 4 + 3] == 0.0;
    return flat;
}

NPG_API int npg_tracers_set_isoneutral(npg_tracers *T, const double *kappa_iso_or_null, double slope_max, double bz_min) {
    NPG_REQUIRE(T, "npg_tracers_set_isoneutral: NULL handle");
    npg_fe *fe = T->fe;
    NPG_HIP(hipSetDevice(T->ctx->device));
    const size_t npts = (size_t)fe->d.nq * fe->d.ncell;
    RediCheck a{"npg_tracers_set_isoneutral"};
    a.set = true, a.kiso = kappa_iso_or_null, a.npts = (int64_t)npts, a.slope_max = slope_max, a.bz_min = bz_min;
    int rc = NPG_OK;
    a.flat = engine_is_flat(fe, &rc);
    NPG_REQUIRE(rc == NPG_OK, "npg_tracers_set_isoneutral: reading the engine's shape tables failed");
    NPG_REQUIRE_OK(check_redi(a));
    NPG_HIP(hipStreamSynchronize(T->ctx->stream));          // kernels that read the tables run on ctx->stream
    if (!kappa_iso_or_null) {
        T->iso = kRediOff;
        T->kiso.reset(), T->kxz.reset(), T->kyz.reset(), T->kzz.reset(), T->counts.reset(), T->missing.reset();
        return NPG_OK;
    }
    T->iso_grid = (int)((fe->d.ncell + kBlock - 1) / kBlock);
    NPG_HIP(T->kiso.upload(kappa_iso_or_null, npts));       // [nq][ncell]: the engine's own [q][cell] layout
    NPG_HIP(T->kxz.zeros(npts));
    NPG_HIP(T->kyz.zeros(npts));
    NPG_HIP(T->kzz.zeros(npts));
    NPG_HIP(T->counts.zeros((size_t)2 * T->iso_grid));
    NPG_HIP(T->missing.zeros(1));
    T->slope_max = slope_max, T->bz_min = bz_min;
    T->iso = kRediSet;
    return NPG_OK;
}

NPG_API int npg_tracers_isoneutral_update(npg_tracers *T, double N2, const npg_vec *b) {
    NPG_REQUIRE(T && b, "npg_tracers_isoneutral_update: NULL argument");
    npg_fe *fe = T->fe;
    RediCheck a{"npg_tracers_isoneutral_update"};
    a.need = kRediSet, a.state = T->iso, a.n_b = fe->n_b, a.vec_n = b->n, a.N2 = N2;
    NPG_REQUIRE_OK(check_redi(a));
    NPG_REQUIRE(b->ctx == fe->ctx, "npg_tracers_isoneutral_update: arguments of different contexts");
    NPG_HIP(hipSetDevice(T->ctx->device));
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(T->iso_grid), dim3(kBlock), 0, T->ctx->stream, fe->d, N2, b->d, T->kiso, T->slope_max, T->bz_min,
                           T->kxz, T->kyz, T->kzz, T->counts);
    };
    fe->d.nb == 10 ? go(k_redi_update<10>) : go(k_redi_update<4>);
    NPG_HIP(hipGetLastError());
    T->iso = kRediUpdated;
    return NPG_OK;
}

NPG_API int npg_tracers_isoneutral_matrix(npg_tracers *T, npg_csr *K) {
    NPG_REQUIRE(T && K, "npg_tracers_isoneutral_matrix: NULL argument");
    npg_fe *fe = T->fe;
    RediCheck a{"npg_tracers_isoneutral_matrix"};
    a.need = kRediUpdated, a.state = T->iso, a.n_b = fe->n_b, a.mat_m = K->m, a.mat_n = K->n;
    a.mat_plain = K->nnode() == 0 && K->lb.nblocks == 0 && !K->uperm;
    NPG_REQUIRE_OK(check_redi(a));
    NPG_REQUIRE(K->ctx == fe->ctx, "npg_tracers_isoneutral_matrix: arguments of different contexts");
    NPG_HIP(hipSetDevice(T->ctx->device));
    hipStream_t st = T->ctx->stream;
    const FeDev &d = fe->d;
    NPG_HIP(hipMemsetAsync(K->val, 0, (size_t)K->nnz * sizeof(double), st));
    NPG_HIP(hipMemsetAsync(T->missing, 0, sizeof(int), st));
    const RediDev rd{T->kiso, T->kxz, T->kyz, T->kzz};
    const int grid = (int)((K->m * kQL + kBlock - 1) / kBlock);
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), 0, st, d, rd, fe->gptr, fe->gidx, K->m, K->rowptr, K->col, K->val, T->missing);
    };
    d.nb == 10 ? go(k_redi_matrix<10>) : go(k_redi_matrix<4>);
    NPG_HIP(hipGetLastError());
    int miss = 0;
    NPG_HIP(hipMemcpyAsync(&miss, T->missing, sizeof(int), hipMemcpyDeviceToHost, st));
    NPG_HIP(hipStreamSynchronize(st));
    NPG_REQUIRE(miss == 0, "npg_tracers_isoneutral_matrix: %d non-zero local entries fall outside the matrix's pattern: it is not the buoyancy pattern",
                miss);
    return csr_repack(K);
}

NPG_API int npg_tracers_isoneutral_tables(npg_tracers *T, double *kxz, double *kyz, double *kzz) {
    NPG_REQUIRE(T && kxz && kyz && kzz, "npg_tracers_isoneutral_tables: NULL argument");
    RediCheck a{"npg_tracers_isoneutral_tables"};
    a.need = kRediUpdated, a.state = T->iso;
    NPG_REQUIRE_OK(check_redi(a));
    NPG_HIP(hipSetDevice(T->ctx->device));
    NPG_HIP(hipStreamSynchronize(T->ctx->stream));
    const size_t bytes = (size_t)T->fe->d.nq * T->fe->d.ncell * sizeof(double);
    NPG_HIP(hipMemcpy(kxz, T->kxz, bytes, hipMemcpyDeviceToHost));
    NPG_HIP(hipMemcpy(kyz, T->kyz, bytes, hipMemcpyDeviceToHost));
    NPG_HIP(hipMemcpy(kzz, T->kzz, bytes, hipMemcpyDeviceToHost));
    return NPG_OK;
}

NPG_API int npg_tracers_isoneutral_info(npg_tracers *T, int64_t *nfloored, int64_t *nclipped, int64_t *npoints, int *state) {
    NPG_REQUIRE(T, "npg_tracers_isoneutral_info: NULL handle");
    int64_t nf = 0, ncl = 0;
    if (T->iso == kRediUpdated) {
        NPG_HIP(hipSetDevice(T->ctx->device));
        std::vector<int32_t> h((size_t)2 * T->iso_grid);
        NPG_HIP(hipStreamSynchronize(T->ctx->stream));
        NPG_HIP(hipMemcpy(h.data(), T->counts, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int g = 0; g < T->iso_grid; ++g) nf += h[(size_t)2 * g], ncl += h[(size_t)2 * g + 1];      // workgroup order
    }
    if (nfloored) *nfloored = nf;
    if (nclipped) *nclipped = ncl;
    if (npoints) *npoints = T->iso == kRediOff ? 0 : (int64_t)T->fe->d.nq * T->fe->d.ncell;
    if (state) *state = T->iso;
    return NPG_OK;
}

// ---- the transport operator as a matrix (transport_core.h) ----------------------------------------------------------------------------
NPG_API int npg_tracers_transport_update(npg_tracers *T, const npg_vec *x_inv, double scale) {
    NPG_REQUIRE(T && x_inv, "npg_tracers_transport_update: NULL argument");
    npg_fe *fe = T->fe;
    NPG_HIP(hipSetDevice(T->ctx->device));
    if (T->flat < 0) {
        int rc = NPG_OK;
        const bool flat = engine_is_flat(fe, &rc);
        NPG_REQUIRE(rc == NPG_OK, "npg_tracers_transport_update: reading the engine's shape tables failed");
        T->flat = flat;
    }
    TransportCheck a{"npg_tracers_transport_update"};
    a.same_ctx = x_inv->ctx == fe->ctx;
    a.update = true, a.scale = scale, a.n_inv = fe->n_inv, a.vec_n = x_inv->n, a.flat = T->flat != 0;
    NPG_REQUIRE_OK(check_transport(a));
    const FeDev &d = fe->d;
    const size_t npts = (size_t)d.nq * d.ncell;
    if (!T->tux) {
        NPG_HIP(T->tux.zeros(npts));
        NPG_HIP(T->tuy.zeros(npts));
        NPG_HIP(T->tuz.zeros(npts));
        NPG_HIP(T->decay.zeros((size_t)T->ntracer));
    }
    const int grid = (int)((d.ncell + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_transport_velocity, dim3(grid), dim3(kBlock), 0, T->ctx->stream, d, scale, x_inv->d, T->tux, T->tuy, T->tuz);
    NPG_HIP(hipGetLastError());
    T->transport = kTransportUpdated;
    return NPG_OK;
}

NPG_API int npg_tracers_transport_matrix(npg_tracers *T, npg_csr *Cm) {
    NPG_REQUIRE(T && Cm, "npg_tracers_transport_matrix: NULL argument");
    npg_fe *fe = T->fe;
    TransportCheck a{"npg_tracers_transport_matrix"};
    a.same_ctx = Cm->ctx == fe->ctx;
    a.need = kTransportUpdated, a.state = T->transport, a.n_b = fe->n_b, a.mat_m = Cm->m, a.mat_n = Cm->n;
    a.mat_plain = Cm->nnode() == 0 && Cm->lb.nblocks == 0 && !Cm->uperm;
    NPG_REQUIRE_OK(check_transport(a));
    NPG_HIP(hipSetDevice(T->ctx->device));
    hipStream_t st = T->ctx->stream;
    const FeDev &d = fe->d;
    if (!T->missing) NPG_HIP(T->missing.zeros(1));          // (shared with the isoneutral mode, which frees it when switched off)
    NPG_HIP(hipMemsetAsync(Cm->val, 0, (size_t)Cm->nnz * sizeof(double), st));
    NPG_HIP(hipMemsetAsync(T->missing, 0, sizeof(int), st));
    const TransportDev td{T->tux, T->tuy, T->tuz};
    const int grid = (int)((Cm->m * kQL + kBlock - 1) / kBlock);
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), 0, st, d, td, fe->gptr, fe->gidx, Cm->m, Cm->rowptr, Cm->col, Cm->val, T->missing);
    };
    d.nb == 10 ? go(k_transport_matrix<10>) : go(k_transport_matrix<4>);
    NPG_HIP(hipGetLastError());
    int miss = 0;
    NPG_HIP(hipMemcpyAsync(&miss, T->missing, sizeof(int), hipMemcpyDeviceToHost, st));
    NPG_HIP(hipStreamSynchronize(st));
    NPG_REQUIRE(miss == 0, "npg_tracers_transport_matrix: %d non-zero local entries fall outside the matrix's pattern: it is not the buoyancy pattern",
                miss);
    return csr_repack(Cm);
}

NPG_API int npg_tracers_transport_load(npg_tracers *T, double kappa_hat, const double *decay_or_null, const npg_vec *rhs_diff1_or_null,
                                       const npg_vec *flux_or_null, npg_vec *out) {
    NPG_REQUIRE(T && out, "npg_tracers_transport_load: NULL argument");
    npg_fe *fe = T->fe;
    const int K = T->ntracer;
    const int64_t nb = fe->n_b;
    TransportCheck a{"npg_tracers_transport_load"};
    for (const npg_vec *v : {rhs_diff1_or_null, flux_or_null, (const npg_vec *)out}) a.same_ctx = a.same_ctx && (!v || v->ctx == fe->ctx);
    a.load = true, a.kappa_hat = kappa_hat, a.decay = decay_or_null, a.ntracer = K, a.n_b = nb;
    a.need = kTransportUpdated, a.state = T->transport;
    a.out_n = out->n, a.flux_n = flux_or_null ? flux_or_null->n : -1, a.diff1_n = rhs_diff1_or_null ? rhs_diff1_or_null->n : -1;
    bool lift = false;
    for (int k = 0; k < K; ++k) {
        a.need_diff1 = a.need_diff1 || T->h_gamma[(size_t)k] != 0.0;
        lift = lift || T->h_lift[(size_t)k];
    }
    a.need_coeff = lift && !(fe->d.kh && fe->d.kv);
    NPG_REQUIRE_OK(check_transport(a));
    NPG_HIP(hipSetDevice(T->ctx->device));
    hipStream_t st = T->ctx->stream;
    if (decay_or_null) {
        NPG_HIP(hipStreamSynchronize(st));                  // an earlier load on the stream may still read the rates
        NPG_HIP(hipMemcpy(T->decay, decay_or_null, (size_t)K * sizeof(double), hipMemcpyHostToDevice));
    }
    const FeDev &d = fe->d;
    TracerSet ts{K, nb, T->n_diri, (int64_t)d.nb * d.ncell, nullptr, nullptr, T->diri, T->gamma, T->source, T->loc};
    const TransportDev td{T->tux, T->tuy, T->tuz};
    const int grid = (int)((d.ncell + kTrBlock - 1) / kTrBlock);
    const size_t lds = (size_t)3 * d.nq * kTrBlock * sizeof(double);
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(kTrBlock), lds, st, d, td, kappa_hat, decay_or_null ? (const double *)T->decay : nullptr, ts);
    };
    d.nb == 10 ? go(k_transport_load<10>) : go(k_transport_load<4>);
    NPG_HIP(hipGetLastError());
    const int ggrid = (int)std::min<int64_t>(2048, (nb + kBlock - 1) / kBlock);
    // (tracer_row with theta = kappa_hat and dt = 1: + kappa_hat gamma_k rhs_diff1 + flux_k)
    hipLaunchKernelGGL(k_tracers_gather, dim3(ggrid, K), dim3(kBlock), 0, st, fe->gptr, fe->gidx, nb, ts, kappa_hat, 1.0,
                       rhs_diff1_or_null ? rhs_diff1_or_null->d : nullptr, flux_or_null ? flux_or_null->d : nullptr, out->d);
    NPG_HIP(hipGetLastError());
    return NPG_OK;
}

NPG_API int npg_tracers_transport_tables(npg_tracers *T, double *ux, double *uy, double *uz) {
    NPG_REQUIRE(T && ux && uy && uz, "npg_tracers_transport_tables: NULL argument");
    TransportCheck a{"npg_tracers_transport_tables"};
    a.need = kTransportUpdated, a.state = T->transport;
    NPG_REQUIRE_OK(check_transport(a));
    NPG_HIP(hipSetDevice(T->ctx->device));
    NPG_HIP(hipStreamSynchronize(T->ctx->stream));
    const size_t bytes = (size_t)T->fe->d.nq * T->fe->d.ncell * sizeof(double);
    NPG_HIP(hipMemcpy(ux, T->tux, bytes, hipMemcpyDeviceToHost));
    NPG_HIP(hipMemcpy(uy, T->tuy, bytes, hipMemcpyDeviceToHost));
    NPG_HIP(hipMemcpy(uz, T->tuz, bytes, hipMemcpyDeviceToHost));
    return NPG_OK;
}

NPG_API int npg_tracers_transport_info(npg_tracers *T, int *state, double *umax) {
    NPG_REQUIRE(T, "npg_tracers_transport_info: NULL handle");
    double um = 0.0;
    if (umax && T->transport == kTransportUpdated) {
        const size_t npts = (size_t)T->fe->d.nq * T->fe->d.ncell;
        std::vector<double> x(npts), y(npts), z(npts);
        const int rc = npg_tracers_transport_tables(T, x.data(), y.data(), z.data());
        if (rc != NPG_OK) return rc;
        for (size_t o = 0; o < npts; ++o) um = std::max(um, std::sqrt(x[o] * x[o] + y[o] * y[o] + z[o] * z[o]));
    }
    if (state) *state = T->transport;
    if (umax) *umax = um;
    return NPG_OK;
}

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
    const bool iso = T->iso != kRediOff;
    if (iso) {
        RediCheck a{"npg_tracers_rhs"};
        a.need = kRediUpdated, a.state = T->iso;
        NPG_REQUIRE_OK(check_redi(a));
    }
    bool lift = false;
    for (int k = 0; k < K; ++k) {
        NPG_REQUIRE(iso || T->h_gamma[(size_t)k] == 0.0 || rhs_diff1_or_null,
                    "npg_tracers_rhs: tracer %d has a background gradient (gamma = %g) but rhs_diff1 is NULL", k, T->h_gamma[(size_t)k]);
        lift = lift || T->h_lift[(size_t)k] || (iso && T->h_gamma[(size_t)k] != 0.0);
    }
    NPG_REQUIRE(!lift || ((iso || fe->d.kh) && fe->d.kv),
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
    const RediDev rd{T->kiso, T->kxz, T->kyz, T->kzz};
    auto go_iso = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(kTrBlock), lds, st, d, rd, (int)(scheme == NPG_BDF2), dt, theta, x_inv->d, x_inv_prev->d, ts);
    };
    if (iso) {
        if (d.nb == 10) f32 ? go_iso(k_tracers_local_iso<float, 10>) : go_iso(k_tracers_local_iso<double, 10>);
        else f32 ? go_iso(k_tracers_local_iso<float, 4>) : go_iso(k_tracers_local_iso<double, 4>);
    } else if (d.nb == 10) f32 ? go(k_tracers_local<float, 10>) : go(k_tracers_local<double, 10>);
    else f32 ? go(k_tracers_local<float, 4>) : go(k_tracers_local<double, 4>);
    NPG_HIP(hipGetLastError());
    const int ggrid = (int)std::min<int64_t>(2048, (nb + kBlock - 1) / kBlock);
    // (the mode on: the background gradient's diffusion went through the rotated tensor in pass 1; rhs_diff1 is not added)
    hipLaunchKernelGGL(k_tracers_gather, dim3(ggrid, K), dim3(kBlock), 0, st, fe->gptr, fe->gidx, nb, ts, theta, dt,
                       rhs_diff1_or_null && !iso ? rhs_diff1_or_null->d : nullptr, flux_or_null ? flux_or_null->d : nullptr, y->d);
    NPG_HIP(hipGetLastError());
    return NPG_OK;
}
