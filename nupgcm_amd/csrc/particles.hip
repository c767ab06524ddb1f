// Lagrangian particles advected through the device-resident flow (npg_particles_advance): where a water parcel goes,
// answered while the velocity is still in HBM instead of from velocities saved every timestep.
//   k_particles_advance<BLEND>   one lane per particle, nsub classical RK4 steps per launch (particles_core.h: locate -> evaluate ->
//                                next stage).  Position, cell, lambda, wind and status live in registers across the substeps and are
//                                written once at the end; the cell remembered from the last location is tried first, so a particle
//                                that stays in its cell reads one 128-byte record per stage and never the bins.  BLEND: the velocity
//                                is (1 - s) u_a + s u_b, the two vectors evaluated one after the other from the same lambda;
//                                BLEND = false (the same vector twice): one evaluation.  The period is a runtime branch.
//   k_particles_walk<BLEND, DIFFUSE>   npg_particles_walk (particles_walk_core.h): the same step with every move walked
//                                through the neighbour table - reflection at boundary faces, translation across periodic seams - and
//                                (DIFFUSE) Visser's random displacement after it, from a counter-based generator.  The same layout:
//                                one lane per particle, the state in registers across the substeps, written once.
//   k_particles_uniforms         the generator alone (npg_particles_uniforms), for its test
// No LDS, no atomics: a particle is one lane's own, so the result does not depend on the order or the number of particles.
// Always fp64 (npg_fe_set_precision does not apply).
#include <cmath>

#include "common.h"
#include "fe_dev.h"
#include "particles_core.h"
#include "particles_walk_core.h"
#include "sample_dev.h"

namespace npg {

template <bool BLEND>
__global__ void __launch_bounds__(kBlock) k_particles_advance(ParticleMesh m, DevCells t, const double *__restrict__ xa,
                                                              const double *__restrict__ xb, ParticleCall call, int64_t nsub,
                                                              int64_t n, double *__restrict__ xyz, int32_t *__restrict__ cell,
                                                              int32_t *__restrict__ status, int32_t *__restrict__ wind,
                                                              double *__restrict__ t_lost) {
    const int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    if (i >= n) return;
    if (status[i] != 0) return;              // lost: nothing moves it
    ParticleState p;
#pragma unroll
    for (int a = 0; a < 3; ++a) p.x[a] = xyz[3 * i + a], p.wind[a] = wind[3 * i + a];
    p.c = cell[i];
    const int64_t done = particle_advance<BLEND>(m, t, xa, xb, call, nsub, p);
    if (done < nsub) {
        status[i] = 1;
        t_lost[i] = done > 0 ? call.t + (double)done * call.h : call.t;
        if (done < 0) return;                // lost where the call found it: the seed stays as it was given
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) xyz[3 * i + a] = p.x[a], wind[3 * i + a] = p.wind[a];
    cell[i] = p.c;
}

template <bool BLEND, bool DIFFUSE>
__global__ void __launch_bounds__(kBlock) k_particles_walk(ParticleMesh m, WalkTables w, DevCells t, const double *__restrict__ xa,
                                                           const double *__restrict__ xb, ParticleCall call, int64_t nsub,
                                                           uint64_t step0, int64_t n, double *__restrict__ xyz,
                                                           int32_t *__restrict__ cell, int32_t *__restrict__ status,
                                                           int32_t *__restrict__ wind, double *__restrict__ t_lost,
                                                           int32_t *__restrict__ nreflect) {
    const int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    if (i >= n) return;
    if (status[i] != 0) return;              // lost or stuck: nothing moves it
    ParticleState p;
#pragma unroll
    for (int a = 0; a < 3; ++a) p.x[a] = xyz[3 * i + a], p.wind[a] = wind[3 * i + a];
    p.c = cell[i];
    int32_t nrefl = nreflect[i];
    const int64_t done = particle_walk<BLEND, DIFFUSE>(m, w, t, xa, xb, call, nsub, (uint64_t)i, step0, p, nrefl);
    if (done < nsub) {
        status[i] = done < 0 ? 1 : 2;
        t_lost[i] = done > 0 ? call.t + (double)done * call.h : call.t;
        if (done < 0) return;                // lost where the call found it: the seed stays as it was given
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) xyz[3 * i + a] = p.x[a], wind[3 * i + a] = p.wind[a];
    cell[i] = p.c;
    nreflect[i] = nrefl;
}

__global__ void __launch_bounds__(kBlock) k_particles_uniforms(uint32_t key0, uint32_t key1, uint64_t first, uint64_t step, int64_t n,
                                                               double *__restrict__ out) {
    const int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    if (i >= n) return;
    double R[3];
    particle_uniforms(key0, key1, first + (uint64_t)i, step, R);
#pragma unroll
    for (int a = 0; a < 3; ++a) out[3 * i + a] = R[a];
}

}  // namespace npg

using namespace npg;

struct npg_particles {
    npg_ctx *ctx = nullptr;
    int64_t n = 0;
    double t = 0.0;              // the time the particles are at
    double L[3] = {0.0, 0.0, 0.0};
    DevBuf<double> xyz;          // [n][3]
    DevBuf<double> t_lost;       // [n], NaN while alive
    DevBuf<int32_t> cell;        // [n] the remembered cell, -1 = none
    DevBuf<int32_t> status;      // [n] 0 alive, 1 lost
    DevBuf<int32_t> wind;        // [n][3]
    // npg_particles_walk: the wall tables, the diffusivities, the generator's key and the count of steps since npg_particles_set
    int64_t wall_ncell = -1, kappa_ncell = -1;       // -1 = not set
    bool wall_axis[3] = {false, false, false};       // some face carries a translation on this axis
    DevBuf<int32_t> nbr;         // [ncell][4]
    DevBuf<int8_t> shift;        // [ncell][4][3]
    DevBuf<double> kappa;        // [2][ncell][4]: kappa_h, kappa_v
    DevBuf<int32_t> nreflect;    // [n], allocated with the walls
    double cd = 0.0;
    uint64_t seed = 0, step = 0;
};

NPG_API int npg_particles_destroy(npg_particles *P) {
    if (!P) return NPG_OK;
    hipStreamSynchronize(P->ctx->stream);
    delete P;
    return NPG_OK;
}

NPG_API int npg_particles_create(npg_ctx *ctx, int64_t n, npg_particles **out) {
    NPG_REQUIRE(ctx && out, "npg_particles_create: NULL argument");
    NPG_REQUIRE(n >= 0 && n <= ((int64_t)1 << 32), "npg_particles_create: 0 .. 2^32 particles, got %lld", (long long)n);
    NPG_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<npg_particles> P(new npg_particles());
    P->ctx = ctx;
    P->n = n;
    const size_t m = std::max<size_t>(1, (size_t)n);
    NPG_HIP(P->xyz.alloc(m * 3));
    NPG_HIP(P->t_lost.alloc(m));
    NPG_HIP(P->cell.alloc(m));
    NPG_HIP(P->status.alloc(m));
    NPG_HIP(P->wind.alloc(m * 3));
    *out = P.release();
    const std::vector<double> zero(m * 3, 0.0);
    return npg_particles_set(*out, zero.data(), 0.0);
}

NPG_API int npg_particles_set(npg_particles *P, const double *xyz, double t0) {
    NPG_REQUIRE(P && (P->n == 0 || xyz), "npg_particles_set: NULL argument");
    NPG_REQUIRE(std::isfinite(t0), "npg_particles_set: t0 is not finite");
    NPG_HIP(hipSetDevice(P->ctx->device));
    NPG_HIP(hipStreamSynchronize(P->ctx->stream));
    const size_t n = (size_t)P->n;
    P->t = t0;
    P->step = 0;
    if (n == 0) return NPG_OK;
    if (P->nreflect) NPG_HIP(hipMemset(P->nreflect, 0, n * sizeof(int32_t)));
    const std::vector<double> nan(n, std::numeric_limits<double>::quiet_NaN());
    NPG_HIP(hipMemcpy(P->xyz, xyz, n * 3 * sizeof(double), hipMemcpyHostToDevice));
    NPG_HIP(hipMemcpy(P->t_lost, nan.data(), n * sizeof(double), hipMemcpyHostToDevice));
    NPG_HIP(hipMemset(P->cell, 0xff, n * sizeof(int32_t)));          // -1
    NPG_HIP(hipMemset(P->status, 0, n * sizeof(int32_t)));
    NPG_HIP(hipMemset(P->wind, 0, n * 3 * sizeof(int32_t)));
    NPG_HIP(hipDeviceSynchronize());
    return NPG_OK;
}

NPG_API int npg_particles_set_period(npg_particles *P, const double *L) {
    NPG_REQUIRE(P && L, "npg_particles_set_period: NULL argument");
    for (int a = 0; a < 3; ++a)
        NPG_REQUIRE(std::isfinite(L[a]) && L[a] >= 0.0, "npg_particles_set_period: L[%d] = %g must be finite and >= 0 (0 = not periodic)", a, L[a]);
    for (int a = 0; a < 3; ++a) P->L[a] = L[a];
    return NPG_OK;
}

NPG_API int npg_particles_advance(npg_particles *P, npg_fe *fe, npg_locator *loc, const npg_vec *x_a, const npg_vec *x_b, double s0,
                                  double s1, double dt, int64_t nsub) {
    NPG_REQUIRE(P && fe && loc && x_a && x_b, "npg_particles_advance: NULL argument");
    NPG_REQUIRE(fe->ctx == P->ctx && loc->ctx == P->ctx && x_a->ctx == P->ctx && x_b->ctx == P->ctx,
                "npg_particles_advance: arguments of different contexts");
    NPG_REQUIRE(!loc->part, "npg_particles_advance: a partitioned locator (npg_locator_create_cells) is refused - a particle that "
                "leaves the rank's cells would have to be handed to another rank, which is not implemented");
    NPG_REQUIRE(loc->ncell == fe->d.ncell, "npg_particles_advance: the locator was built for another mesh (an embedded 2-D engine "
                "has no locator: particles need a tetrahedral mesh)");
    NPG_REQUIRE(x_a->n == fe->n_inv && x_b->n == fe->n_inv, "npg_particles_advance: the flow vectors have %lld and %lld entries, expected %lld",
                (long long)x_a->n, (long long)x_b->n, (long long)fe->n_inv);
    const char *err = check_particle_call(s0, s1, dt, nsub);
    NPG_REQUIRE(!err, "npg_particles_advance: %s", err);
    const ParticleCall call = make_particle_call(P->t, s0, s1, dt, nsub);
    if (P->n == 0) {
        P->t += dt;
        return NPG_OK;
    }
    NPG_HIP(hipSetDevice(P->ctx->device));
    const FeDev &d = fe->d;
    const DevCells t = cell_view(d);
    const ParticleMesh m{loc->grid, loc->bin_ptr, loc->bin_cells, loc->geo, {P->L[0], P->L[1], P->L[2]}};
    const dim3 grid((unsigned)((P->n + kBlock - 1) / kBlock)), block(kBlock);
    hipStream_t st = P->ctx->stream;
    if (x_a->d != x_b->d)
        hipLaunchKernelGGL(k_particles_advance<true>, grid, block, 0, st, m, t, x_a->d, x_b->d, call, nsub, P->n, P->xyz, P->cell,
                           P->status, P->wind, P->t_lost);
    else
        hipLaunchKernelGGL(k_particles_advance<false>, grid, block, 0, st, m, t, x_a->d, x_a->d, call, nsub, P->n, P->xyz, P->cell,
                           P->status, P->wind, P->t_lost);
    NPG_HIP(hipGetLastError());
    P->t += dt;
    return NPG_OK;
}

NPG_API int npg_particles_set_walls(npg_particles *P, const int32_t *nbr, const int8_t *shift, int64_t ncell) {
    NPG_REQUIRE(P && nbr && shift, "npg_particles_set_walls: NULL argument");
    NPG_REQUIRE(ncell >= 1 && ncell <= INT32_MAX, "npg_particles_set_walls: ncell = %lld", (long long)ncell);
    bool has[3];
    const char *err = check_wall_tables(nbr, shift, ncell, P->L, has);
    NPG_REQUIRE(!err, "npg_particles_set_walls: %s", err);
    NPG_HIP(hipSetDevice(P->ctx->device));
    NPG_HIP(hipStreamSynchronize(P->ctx->stream));
    DevBuf<int32_t> d_nbr, d_refl;               // the handle keeps its tables unless every step succeeds
    DevBuf<int8_t> d_shift;
    NPG_HIP(d_nbr.upload(nbr, (size_t)ncell * 4));
    NPG_HIP(d_shift.upload(shift, (size_t)ncell * 12));
    if (!P->nreflect) {
        NPG_HIP(d_refl.zeros(std::max<size_t>(1, (size_t)P->n)));
        P->nreflect.swap(d_refl);
    }
    P->nbr.swap(d_nbr), P->shift.swap(d_shift), P->wall_ncell = ncell;
    for (int a = 0; a < 3; ++a) P->wall_axis[a] = has[a];
    return NPG_OK;
}

NPG_API int npg_particles_set_diffusion(npg_particles *P, const double *kappa_h, const double *kappa_v, int64_t ncell, double c_d,
                                        uint64_t seed) {
    NPG_REQUIRE(P, "npg_particles_set_diffusion: NULL handle");
    NPG_HIP(hipSetDevice(P->ctx->device));
    if (!kappa_h && !kappa_v) {              // diffusion off
        NPG_HIP(hipStreamSynchronize(P->ctx->stream));
        P->kappa.reset(), P->kappa_ncell = -1;
        return NPG_OK;
    }
    NPG_REQUIRE(kappa_h && kappa_v, "npg_particles_set_diffusion: NULL argument (kappa_h and kappa_v are given together)");
    NPG_REQUIRE(ncell >= 1 && ncell <= INT32_MAX, "npg_particles_set_diffusion: ncell = %lld", (long long)ncell);
    NPG_REQUIRE(P->wall_ncell < 0 || P->wall_ncell == ncell, "npg_particles_set_diffusion: ncell = %lld, the wall tables have %lld cells",
                (long long)ncell, (long long)P->wall_ncell);
    const char *err = check_kappa_tables(kappa_h, kappa_v, ncell, c_d);
    NPG_REQUIRE(!err, "npg_particles_set_diffusion: %s", err);
    NPG_HIP(hipStreamSynchronize(P->ctx->stream));
    DevBuf<double> d;
    const size_t bytes = (size_t)ncell * 4 * sizeof(double);
    NPG_HIP(d.alloc((size_t)ncell * 8));
    NPG_HIP(hipMemcpy(d, kappa_h, bytes, hipMemcpyHostToDevice));
    NPG_HIP(hipMemcpy(d + (size_t)ncell * 4, kappa_v, bytes, hipMemcpyHostToDevice));
    P->kappa.swap(d), P->kappa_ncell = ncell, P->cd = c_d, P->seed = seed;
    return NPG_OK;
}

NPG_API int npg_particles_walk(npg_particles *P, npg_fe *fe, npg_locator *loc, const npg_vec *x_a, const npg_vec *x_b, double s0,
                               double s1, double dt, int64_t nsub) {
    NPG_REQUIRE(P && fe && loc && x_a && x_b, "npg_particles_walk: NULL argument");
    NPG_REQUIRE(fe->ctx == P->ctx && loc->ctx == P->ctx && x_a->ctx == P->ctx && x_b->ctx == P->ctx,
                "npg_particles_walk: arguments of different contexts");
    NPG_REQUIRE(!loc->part, "npg_particles_walk: a partitioned locator (npg_locator_create_cells) is refused - a particle that "
                "leaves the rank's cells would have to be handed to another rank, which is not implemented");
    NPG_REQUIRE(loc->ncell == fe->d.ncell, "npg_particles_walk: the locator was built for another mesh (an embedded 2-D engine "
                "has no locator: particles need a tetrahedral mesh)");
    NPG_REQUIRE(x_a->n == fe->n_inv && x_b->n == fe->n_inv, "npg_particles_walk: the flow vectors have %lld and %lld entries, expected %lld",
                (long long)x_a->n, (long long)x_b->n, (long long)fe->n_inv);
    const char *err = check_particle_call(s0, s1, dt, nsub);
    NPG_REQUIRE(!err, "npg_particles_walk: %s", err);
    NPG_REQUIRE(P->wall_ncell >= 0, "npg_particles_walk: no walls - call npg_particles_set_walls first");
    NPG_REQUIRE(P->wall_ncell == loc->ncell, "npg_particles_walk: the wall tables have ncell = %lld, the locator %lld",
                (long long)P->wall_ncell, (long long)loc->ncell);
    NPG_REQUIRE(P->kappa_ncell < 0 || P->kappa_ncell == loc->ncell, "npg_particles_walk: the diffusivity tables have ncell = %lld, the locator %lld",
                (long long)P->kappa_ncell, (long long)loc->ncell);
    for (int a = 0; a < 3; ++a)
        NPG_REQUIRE(P->wall_axis[a] == (P->L[a] > 0.0), "npg_particles_walk: axis %d has period %g but the wall tables carry %s seam "
                    "shift on it - a walked particle crosses a seam through the table", a, P->L[a], P->wall_axis[a] ? "a" : "no");
    const ParticleCall call = make_particle_call(P->t, s0, s1, dt, nsub);
    const uint64_t step0 = P->step;
    if (P->n == 0) {
        P->t += dt, P->step += (uint64_t)nsub;
        return NPG_OK;
    }
    NPG_HIP(hipSetDevice(P->ctx->device));
    const FeDev &d = fe->d;
    const DevCells t = cell_view(d);
    const ParticleMesh m{loc->grid, loc->bin_ptr, loc->bin_cells, loc->geo, {P->L[0], P->L[1], P->L[2]}};
    const bool diffuse = P->kappa_ncell >= 0;
    const WalkTables w{P->nbr, P->shift, P->kappa, diffuse ? P->kappa + (size_t)P->kappa_ncell * 4 : nullptr, P->cd,
                       (uint32_t)P->seed, (uint32_t)(P->seed >> 32)};
    const dim3 grid((unsigned)((P->n + kBlock - 1) / kBlock)), block(kBlock);
    hipStream_t st = P->ctx->stream;
    const bool blend = x_a->d != x_b->d;
#define NPG_WALK(B, D)                                                                                                              \
    hipLaunchKernelGGL((k_particles_walk<B, D>), grid, block, 0, st, m, w, t, x_a->d, blend ? x_b->d : x_a->d, call, nsub, step0, \
                       P->n, P->xyz, P->cell, P->status, P->wind, P->t_lost, P->nreflect)
    if (blend && diffuse) NPG_WALK(true, true);
    else if (blend) NPG_WALK(true, false);
    else if (diffuse) NPG_WALK(false, true);
    else NPG_WALK(false, false);
#undef NPG_WALK
    NPG_HIP(hipGetLastError());
    P->t += dt, P->step += (uint64_t)nsub;
    return NPG_OK;
}

NPG_API int npg_particles_download_walk(const npg_particles *P, int32_t *nreflect, uint64_t *step) {
    NPG_REQUIRE(P, "npg_particles_download_walk: NULL handle");
    NPG_HIP(hipSetDevice(P->ctx->device));
    NPG_HIP(hipStreamSynchronize(P->ctx->stream));
    if (step) *step = P->step;
    if (nreflect && P->n > 0) {
        if (P->nreflect) NPG_HIP(hipMemcpy(nreflect, P->nreflect, (size_t)P->n * sizeof(int32_t), hipMemcpyDeviceToHost));
        else std::fill(nreflect, nreflect + P->n, 0);
    }
    return NPG_OK;
}

NPG_API int npg_particles_uniforms(npg_ctx *ctx, uint64_t seed, uint64_t first_index, int64_t n, uint64_t step, npg_vec *out) {
    NPG_REQUIRE(ctx && out, "npg_particles_uniforms: NULL argument");
    NPG_REQUIRE(n >= 0 && out->ctx == ctx && out->n == 3 * n, "npg_particles_uniforms: out must hold 3 n = %lld doubles of this context",
                (long long)(3 * n));
    if (n == 0) return NPG_OK;
    NPG_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_particles_uniforms, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, (uint32_t)seed,
                       (uint32_t)(seed >> 32), first_index, step, n, out->d);
    NPG_HIP(hipGetLastError());
    return NPG_OK;
}

NPG_API int npg_particles_download(const npg_particles *P, double *xyz, int32_t *cell, int32_t *status, int32_t *wind, double *t_lost) {
    NPG_REQUIRE(P, "npg_particles_download: NULL handle");
    NPG_HIP(hipSetDevice(P->ctx->device));
    NPG_HIP(hipStreamSynchronize(P->ctx->stream));
    const size_t n = (size_t)P->n;
    if (n == 0) return NPG_OK;
    if (xyz) NPG_HIP(hipMemcpy(xyz, P->xyz, n * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (cell) NPG_HIP(hipMemcpy(cell, P->cell, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (status) NPG_HIP(hipMemcpy(status, P->status, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (wind) NPG_HIP(hipMemcpy(wind, P->wind, n * 3 * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (t_lost) NPG_HIP(hipMemcpy(t_lost, P->t_lost, n * sizeof(double), hipMemcpyDeviceToHost));
    return NPG_OK;
}

NPG_API int npg_particles_positions(const npg_particles *P, npg_vec *out) {
    NPG_REQUIRE(P && out, "npg_particles_positions: NULL argument");
    NPG_REQUIRE(out->ctx == P->ctx && out->n == 3 * P->n, "npg_particles_positions: out must hold 3 n = %lld doubles of the particles' context",
                (long long)(3 * P->n));
    if (P->n == 0) return NPG_OK;
    NPG_HIP(hipMemcpyAsync(out->d, P->xyz, (size_t)P->n * 3 * sizeof(double), hipMemcpyDeviceToDevice, P->ctx->stream));
    return NPG_OK;
}
