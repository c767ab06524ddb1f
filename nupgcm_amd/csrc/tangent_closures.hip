// The derivatives of the convection and eddy closures: three loads of the linearised model (nupgcm_amd/linearized.py,
// closures="tangent") for models whose kappa_v and nu depend on the buoyancy, and the read-back of a coefficient table.
//   npg_fe_tangent_diffusion      out   = D_v db    the derivative of the vertical diffusion with the convection closure
//   npg_fe_tangent_eddy           out_x = r_x(db)   the right-hand side that the derivative of nu adds to the tangent inversion
//   npg_fe_tangent_eddy_adjoint   out_b = g(mu)     its adjoint: <mu, r_x(db)> = <g(mu), db>
// The arithmetic, the order of its sums and the argument checks are tangent_closures_core.h's, shared with the host library.
//   pass 1  k_tangent_diffusion_local<NB> / k_tangent_eddy_local<NB> / k_tangent_eddy_adjoint_local<NB>: one lane per cell at kBlock,
//           the shape tables from LDS (stage_tables); the closure derivatives are evaluated on the fly from b_base, fe->kv0 and the f
//           table - coef[*] is neither read (f apart) nor written
//   pass 2  the engine's fixed-order gather of fe.hip: gptr / gidx over loc, or iptr / iidx over loc_inv (whose pressure planes are
//           zeroed once and never written: the pressure rows of r_x are sums of zeros)
// No atomics: the bits of the host library on every call.  Always fp64.
#include "common.h"
#include "device_utils.h"
#include "fe_dev.h"
#include "tangent_closures_core.h"

namespace npg {

template <int NB>
__global__ void __launch_bounds__(kBlock) k_tangent_diffusion_local(FeDev d, ConvClosure cl, double alpha, double N2,
                                                                    const double *__restrict__ kv0, const double *__restrict__ b_base,
                                                                    const double *__restrict__ db, double *__restrict__ loc) {
    __shared__ FeTables t;
    stage_tables(d, t);
    const int64_t cell = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    if (cell >= d.ncell) return;
    cell_tangent_diffusion<NB>(t, cell_view(d), d.nq, cl, alpha, N2, kv0, b_base, db, cell, loc);
}

template <int NB>
__global__ void __launch_bounds__(kBlock) k_tangent_eddy_local(FeDev d, double a2e2, int full_stress, EddyClosure cl, double alpha, double N2,
                                                               const double *__restrict__ b_base, const double *__restrict__ x_base,
                                                               const double *__restrict__ db, double *__restrict__ loc_x) {
    __shared__ FeTables t;
    stage_tables(d, t);
    const int64_t cell = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    if (cell >= d.ncell) return;
    cell_tangent_eddy<NB>(t, cell_view(d), d.nq, a2e2, full_stress, cl, alpha, N2, d.f, b_base, x_base, db, cell, loc_x);
}

template <int NB>
__global__ void __launch_bounds__(kBlock) k_tangent_eddy_adjoint_local(FeDev d, double a2e2, int full_stress, EddyClosure cl, double alpha,
                                                                       double N2, const double *__restrict__ b_base,
                                                                       const double *__restrict__ x_base, const double *__restrict__ mu,
                                                                       double *__restrict__ loc) {
    __shared__ FeTables t;
    stage_tables(d, t);
    const int64_t cell = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    if (cell >= d.ncell) return;
    cell_tangent_eddy_adjoint<NB>(t, cell_view(d), d.nq, a2e2, full_stress, cl, alpha, N2, d.f, b_base, x_base, mu, cell, loc);
}

static dim3 cells_grid(const npg_fe *fe) { return dim3((unsigned)((fe->d.ncell + kBlock - 1) / kBlock)); }

}  // namespace npg

using namespace npg;

NPG_API int npg_fe_tangent_diffusion(npg_fe *fe, double kappa_c, double N2min, double alpha, double N2, const npg_vec *b_base,
                                     const npg_vec *db, npg_vec *out) {
    NPG_REQUIRE(fe, "npg_fe_tangent_diffusion: NULL handle");
    const bool any_null = !(b_base && db && out);
    NPG_REQUIRE_OK(check_tangent_diffusion(any_null, !any_null && (out == b_base || out == db), fe->kv0 != nullptr, kappa_c, N2min, alpha, N2,
                                           fe->n_b, any_null ? 0 : b_base->n, any_null ? 0 : db->n, any_null ? 0 : out->n,
                                           any_null || (b_base->ctx == fe->ctx && db->ctx == fe->ctx && out->ctx == fe->ctx)));
    NPG_HIP(hipSetDevice(fe->ctx->device));
    const ConvClosure cl{kappa_c, N2min};
    const dim3 block(kBlock);
    if (fe->d.nb == 10)
        hipLaunchKernelGGL(k_tangent_diffusion_local<10>, cells_grid(fe), block, 0, fe->ctx->stream, fe->d, cl, alpha, N2, fe->kv0, b_base->d,
                           db->d, fe->loc);
    else
        hipLaunchKernelGGL(k_tangent_diffusion_local<4>, cells_grid(fe), block, 0, fe->ctx->stream, fe->d, cl, alpha, N2, fe->kv0, b_base->d,
                           db->d, fe->loc);
    NPG_HIP(hipGetLastError());
    return fe_gather_rows(fe, out);
}

NPG_API int npg_fe_tangent_eddy(npg_fe *fe, double a2e2, int full_stress, double N2min, double alpha, double N2, double smoothing,
                                double nu_min, const npg_vec *b_base, const npg_vec *x_base, const npg_vec *db, npg_vec *out_x) {
    NPG_REQUIRE(fe, "npg_fe_tangent_eddy: NULL handle");
    const bool any_null = !(b_base && x_base && db && out_x);
    NPG_REQUIRE_OK(check_tangent_eddy(false, any_null, !any_null && (out_x == b_base || out_x == x_base || out_x == db), fe->d.f != nullptr,
                                      a2e2, full_stress, N2min, alpha, N2, smoothing, nu_min, fe->n_inv, fe->n_b, any_null ? 0 : b_base->n,
                                      any_null ? 0 : x_base->n, any_null ? 0 : db->n, any_null ? 0 : out_x->n,
                                      any_null || (b_base->ctx == fe->ctx && x_base->ctx == fe->ctx && db->ctx == fe->ctx &&
                                                   out_x->ctx == fe->ctx)));
    NPG_HIP(hipSetDevice(fe->ctx->device));
    int rc = fe_ensure_loc_inv(fe);
    if (rc) return rc;
    const EddyClosure cl{N2min, smoothing, nu_min};
    const dim3 block(kBlock);
    if (fe->d.nb == 10)
        hipLaunchKernelGGL(k_tangent_eddy_local<10>, cells_grid(fe), block, 0, fe->ctx->stream, fe->d, a2e2, full_stress, cl, alpha, N2,
                           b_base->d, x_base->d, db->d, fe->loc_inv);
    else
        hipLaunchKernelGGL(k_tangent_eddy_local<4>, cells_grid(fe), block, 0, fe->ctx->stream, fe->d, a2e2, full_stress, cl, alpha, N2,
                           b_base->d, x_base->d, db->d, fe->loc_inv);
    NPG_HIP(hipGetLastError());
    return fe_gather_index(fe, fe->iptr, fe->iidx, fe->loc_inv, fe->n_inv, out_x);
}

NPG_API int npg_fe_tangent_eddy_adjoint(npg_fe *fe, double a2e2, int full_stress, double N2min, double alpha, double N2, double smoothing,
                                        double nu_min, const npg_vec *b_base, const npg_vec *x_base, const npg_vec *mu, npg_vec *out_b) {
    NPG_REQUIRE(fe, "npg_fe_tangent_eddy_adjoint: NULL handle");
    const bool any_null = !(b_base && x_base && mu && out_b);
    NPG_REQUIRE_OK(check_tangent_eddy(true, any_null, !any_null && (out_b == b_base || out_b == x_base || out_b == mu), fe->d.f != nullptr,
                                      a2e2, full_stress, N2min, alpha, N2, smoothing, nu_min, fe->n_inv, fe->n_b, any_null ? 0 : b_base->n,
                                      any_null ? 0 : x_base->n, any_null ? 0 : mu->n, any_null ? 0 : out_b->n,
                                      any_null || (b_base->ctx == fe->ctx && x_base->ctx == fe->ctx && mu->ctx == fe->ctx &&
                                                   out_b->ctx == fe->ctx)));
    NPG_HIP(hipSetDevice(fe->ctx->device));
    const EddyClosure cl{N2min, smoothing, nu_min};
    const dim3 block(kBlock);
    if (fe->d.nb == 10)
        hipLaunchKernelGGL(k_tangent_eddy_adjoint_local<10>, cells_grid(fe), block, 0, fe->ctx->stream, fe->d, a2e2, full_stress, cl, alpha, N2,
                           b_base->d, x_base->d, mu->d, fe->loc);
    else
        hipLaunchKernelGGL(k_tangent_eddy_adjoint_local<4>, cells_grid(fe), block, 0, fe->ctx->stream, fe->d, a2e2, full_stress, cl, alpha, N2,
                           b_base->d, x_base->d, mu->d, fe->loc);
    NPG_HIP(hipGetLastError());
    return fe_gather_rows(fe, out_b);
}

// the read-back of npg_fe_set_coeff: host_out[cell][q], the table as it stands (after a closure update: the updated one)
NPG_API int npg_fe_get_coeff(npg_fe *fe, const char *name, double *host_out) {
    const bool any_null = !(fe && name && host_out);
    const int k = any_null ? -1 : !strcmp(name, "nu") ? 0 : !strcmp(name, "kappa_h") ? 1 : !strcmp(name, "kappa_v") ? 2 : !strcmp(name, "f") ? 3 : -1;
    NPG_REQUIRE_OK(check_get_coeff(any_null, k, any_null ? "" : name, k >= 0 && fe->coef[k] != nullptr));
    NPG_HIP(hipSetDevice(fe->ctx->device));
    const int64_t nc = fe->d.ncell;
    const int nq = fe->d.nq;
    std::vector<double> tmp((size_t)nc * nq);
    NPG_HIP(hipStreamSynchronize(fe->ctx->stream));          // a closure update on the engine's stream is finished first
    NPG_HIP(hipMemcpy(tmp.data(), fe->coef[k], tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int64_t c = 0; c < nc; ++c)
        for (int q = 0; q < nq; ++q) host_out[(size_t)c * nq + q] = tmp[(size_t)q * nc + c];
    return NPG_OK;
}
