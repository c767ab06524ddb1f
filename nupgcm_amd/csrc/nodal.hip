// Gradients of the device-resident state recovered at the mesh's P2 nodes (npg_nodal_*): d_j u_a, grad b', grad p, the
// weight and the valence per selected node - what vorticity, divergence, N^2 and the planetary PV are made of.  The arithmetic and the
// argument checks are nodal_core.h's, shared with the host library.  The no-atomics scatter in two launches:
//   k_nodal_cells<NB>  one lane per cell: unit-stride reads of the engine's [component][cell] tables, the state gathered through the DoF
//                      codes, one field at a time; the cell's vertex gradients go to its own record of the scratch with plain stores
//   k_nodal_nodes      one lane per selected node: walks its incidence list in ascending cell order, reads one record entry per channel
//                      for a vertex and two for a mid-node, sums from 0.0, divides once, writes out[channel][node] (unit stride)
// Deterministic: every sum has one order, no atomics, no LDS - the bits of the host library on every call.  The handle owns the
// incidence table and the scratch ([ncell][nslot] doubles, grown to the largest fields_mask asked for so far).
#include "common.h"
#include "device_utils.h"
#include "fe_dev.h"
#include "nodal_core.h"

static_assert(NPG_NODAL_U == npg::kNodalU && NPG_NODAL_B == npg::kNodalB && NPG_NODAL_P == npg::kNodalP && NPG_NODAL_NCH == npg::kNodalMaxCh,
              "the field codes of the header and of nodal_core.h must agree");

namespace npg {

constexpr int kNodalBlock = NPG_NODAL_BLOCK;
static_assert(kNodalBlock % kWave == 0 && kNodalBlock <= 1024, "whole waves");

template <int NB>
__global__ void __launch_bounds__(kNodalBlock) k_nodal_cells(DevCells t, NodalPlan pl, const double *__restrict__ xu, const double *__restrict__ xb,
                                                             double *__restrict__ scr) {
    const int64_t c = (int64_t)blockIdx.x * kNodalBlock + threadIdx.x;
    if (c < t.ncell) nodal_cell<DevCells, NB>(t, pl, xu, xb, c, scr + (size_t)c * (size_t)pl.nslot);
}

__global__ void __launch_bounds__(kNodalBlock) k_nodal_nodes(NodalTable t, NodalPlan pl, const double *__restrict__ scr, double *__restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * kNodalBlock + threadIdx.x;
    if (j < t.nsel) nodal_node(t, pl, scr, j, out);
}

}  // namespace npg

using namespace npg;

struct npg_nodal {
    npg_ctx *ctx = nullptr;
    npg_fe *fe = nullptr;
    int64_t nsel = 0, ninc = 0, max_valence = 0;
    int weight_mode = 0;
    DevBuf<int64_t> ptr;
    DevBuf<int32_t> inc;
    DevBuf<double> scratch;
    size_t scratch_n = 0;           // doubles held
};

NPG_API int npg_nodal_create(npg_fe *fe, int64_t nsel, const int64_t *inc_ptr, const int32_t *inc, int weight_mode, npg_nodal **out) {
    NPG_REQUIRE(fe && out, "npg_nodal_create: NULL argument");
    NPG_HIP(hipSetDevice(fe->ctx->device));
    {   // an embedded 2-D engine pads its triangles to tetrahedra with a zero fourth gradient: its nodes have other local numbers
        std::vector<double> n1((size_t)fe->d.nq * 4);
        NPG_HIP(hipMemcpy(n1.data(), fe->d.N1, n1.size() * sizeof(double), hipMemcpyDeviceToHost));
        bool flat = true;
        for (int q = 0; q < fe->d.nq; ++q) flat = flat && n1[(size_t)q * 4 + 3] == 0.0;
        NPG_REQUIRE(!flat, "npg_nodal_create: an embedded 2-D engine is refused (the recovery is written for tetrahedra)");
    }
    int64_t vmax = 0;
    NPG_REQUIRE_OK(check_nodal_create(fe->d.ncell, nsel, inc_ptr, inc, weight_mode, &vmax));
    std::unique_ptr<npg_nodal> N(new npg_nodal());
    N->ctx = fe->ctx;
    N->fe = fe;
    N->nsel = nsel, N->ninc = inc_ptr[nsel], N->max_valence = vmax, N->weight_mode = weight_mode;
    NPG_HIP(N->ptr.upload(inc_ptr, (size_t)nsel + 1));
    NPG_HIP(N->inc.upload(inc, (size_t)N->ninc));
    *out = N.release();
    return NPG_OK;
}

NPG_API int npg_nodal_destroy(npg_nodal *N) {
    if (!N) return NPG_OK;
    hipStreamSynchronize(N->ctx->stream);
    delete N;
    return NPG_OK;
}

NPG_API int npg_nodal_info(const npg_nodal *N, int64_t *nsel, int64_t *ninc, int64_t *max_valence, int64_t *scratch_doubles) {
    NPG_REQUIRE(N, "npg_nodal_info: NULL argument");
    if (nsel) *nsel = N->nsel;
    if (ninc) *ninc = N->ninc;
    if (max_valence) *max_valence = N->max_valence;
    if (scratch_doubles) *scratch_doubles = (int64_t)N->scratch_n;
    return NPG_OK;
}

NPG_API int npg_nodal_compute(npg_nodal *N, const npg_vec *x_inv, const npg_vec *b, int fields_mask, npg_vec *out) {
    NPG_REQUIRE(N && x_inv && b && out, "npg_nodal_compute: NULL argument");
    npg_fe *fe = N->fe;
    NPG_REQUIRE_OK(check_nodal_compute(fe->n_inv, fe->n_b, fe->d.nb, N->nsel, x_inv->n, b->n, fields_mask, out->n,
                                       x_inv->ctx == fe->ctx && b->ctx == fe->ctx && out->ctx == fe->ctx));
    if (N->nsel == 0) return NPG_OK;
    NPG_HIP(hipSetDevice(fe->ctx->device));
    hipStream_t st = fe->ctx->stream;
    const NodalPlan pl = nodal_plan(fields_mask, fe->d.nb);
    const size_t need = (size_t)fe->d.ncell * (size_t)pl.nslot;
    if (need > N->scratch_n) {
        NPG_HIP(hipStreamSynchronize(st));                  // a compute still in flight reads the scratch this call replaces
        N->scratch_n = 0;
        NPG_HIP(N->scratch.alloc(need));
        N->scratch_n = need;
    }
    const dim3 block(kNodalBlock), gcells((unsigned)((fe->d.ncell + kNodalBlock - 1) / kNodalBlock));
    if (fe->d.nb == 10)
        hipLaunchKernelGGL(k_nodal_cells<10>, gcells, block, 0, st, cell_view(fe->d), pl, x_inv->d, b->d, N->scratch.p);
    else
        hipLaunchKernelGGL(k_nodal_cells<4>, gcells, block, 0, st, cell_view(fe->d), pl, x_inv->d, b->d, N->scratch.p);
    NPG_HIP(hipGetLastError());
    const NodalTable t{N->nsel, N->ptr.p, N->inc.p, fe->d.wdet, N->weight_mode};
    hipLaunchKernelGGL(k_nodal_nodes, dim3((unsigned)((N->nsel + kNodalBlock - 1) / kNodalBlock)), block, 0, st, t, pl, N->scratch.p, out->d);
    NPG_HIP(hipGetLastError());
    return NPG_OK;
}
