// The tangent of the advection load (npg_fe_tangent_rhs): the directional derivative of int (u . grad b + w N2) phi_i at
// a base state along a perturbation - the one ingredient of the linearised model (nupgcm_amd/linearized.py) that was not on the device.
// The arithmetic, the order of its sums and the argument checks are tangent_core.h's, shared with the host library.
//   pass 1  k_tangent_local<NB>  one lane per cell at kBlock: unit-stride reads of the engine's [component][cell] tables, the shape
//                                tables from LDS (stage_tables; all lanes of a wave read the same entry: a broadcast), the two terms one
//                                after the other so that one velocity and one scalar are live at a time; writes loc[i][cell]
//   pass 2  the engine's fixed-order gather of fe.hip (k_gather_rows with empty RhsTerms) through the inverted index
// No atomics: the bits of the host library on every call.  Always fp64, whatever npg_fe_set_precision says.
#include "common.h"
#include "device_utils.h"
#include "fe_dev.h"
#include "tangent_core.h"

namespace npg {

template <int NB>
__global__ void __launch_bounds__(kBlock) k_tangent_local(FeDev d, double N2, const double *__restrict__ b_base,
                                                          const double *__restrict__ x_base, const double *__restrict__ db,
                                                          const double *__restrict__ dx, double *__restrict__ loc) {
    __shared__ FeTables t;
    stage_tables(d, t);
    const int64_t cell = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    if (cell >= d.ncell) return;
    cell_tangent<NB>(t, cell_view(d), d.nq, N2, b_base, x_base, db, dx, cell, loc);
}

}  // namespace npg

using namespace npg;

NPG_API int npg_fe_tangent_rhs(npg_fe *fe, double N2, const npg_vec *b_base, const npg_vec *x_base, const npg_vec *db, const npg_vec *dx,
                               npg_vec *out) {
    NPG_REQUIRE(fe, "npg_fe_tangent_rhs: NULL handle");
    const bool any_null = !(b_base && x_base && db && dx && out);
    NPG_REQUIRE_OK(check_tangent(any_null, N2, fe->n_inv, fe->n_b, any_null ? 0 : b_base->n, any_null ? 0 : x_base->n, any_null ? 0 : db->n,
                                 any_null ? 0 : dx->n, any_null ? 0 : out->n,
                                 any_null || (b_base->ctx == fe->ctx && x_base->ctx == fe->ctx && db->ctx == fe->ctx && dx->ctx == fe->ctx &&
                                              out->ctx == fe->ctx)));
    NPG_HIP(hipSetDevice(fe->ctx->device));
    const dim3 grid((unsigned)((fe->d.ncell + kBlock - 1) / kBlock)), block(kBlock);
    if (fe->d.nb == 10)
        hipLaunchKernelGGL(k_tangent_local<10>, grid, block, 0, fe->ctx->stream, fe->d, N2, b_base->d, x_base->d, db->d, dx->d, fe->loc);
    else
        hipLaunchKernelGGL(k_tangent_local<4>, grid, block, 0, fe->ctx->stream, fe->d, N2, b_base->d, x_base->d, db->d, dx->d, fe->loc);
    NPG_HIP(hipGetLastError());
    return fe_gather_rows(fe, out);
}
