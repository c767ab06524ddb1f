// Quadrature integrals of the device-resident state over the mesh's boundary faces (npg_boundary_compute): area, normals, volume and
// buoyancy fluxes, pressure force and work, viscous traction and work, diffusive flux, wind work, the prescribed flux, the stratification
// and the tangential flow at the boundary - the NPG_NBND channels of boundary_core.h, per GROUP of faces (surface, bottom, coastline,
// ...) and, on request, per face.  The reference has no counterpart.
//   k_boundary_faces<NB>  one lane per face, one face per lane; the faces that count are sorted by group and every workgroup of
//                         kBndChunk lanes gets faces of ONE group (rows[blockIdx.x] = first face, count, group).  The lane loads its
//                         cell's nodal values once, walks the 9 face points with the face shape tables in LDS and keeps its NPG_NBND
//                         accumulators in registers; they ARE the face's integrals and go to faces_out[ch][face] when asked for; then
//                         wave_sum, the waves added in order: one partial row per workgroup (block_store_partials)
//   k_boundary_fold       one workgroup per group adds that group's rows in one fixed order
// Deterministic: the rows are a function of the face counts alone (not of the device, not of the environment), every sum has one
// order, no atomics - two calls on the same state give the same bits.  The workgroup (kBndChunk = 256 lanes) is a compile-time
// constant: the boundary is small (43 k faces at 527 k cells) and the kernel is bound by latency - of which staging the 15.8 KB of
// shape tables once per workgroup is a large part, so 256 lanes beat 64 (43 against 59 us).
#include <cmath>

#include "common.h"
#include "device_utils.h"
#include "fe_dev.h"
#include "boundary_core.h"

static_assert(NPG_NBND == npg::kNBnd, "NPG_NBND of the header and kNBnd of boundary_core.h must agree");
static_assert(npg::kNBnd <= npg::kPartStride, "a partial row holds the channels");
static_assert(NPG_BND_NU == npg::kBndNu && NPG_BND_KH == npg::kBndKh && NPG_BND_KV == npg::kBndKv && NPG_BND_TAUX == npg::kBndTauX &&
                  NPG_BND_TAUY == npg::kBndTauY && NPG_BND_FLUX == npg::kBndFlux,
              "the coefficient codes of the header and of boundary_core.h must agree");

namespace npg {

constexpr int kBndBlock = kBndChunk;        // one face per lane, one partial row per workgroup
static_assert(kBndBlock % kWave == 0 && kBndBlock <= 1024, "whole waves");
constexpr int kBndFoldSlices = kBlock / kPartStride;

using BndFaces = FaceTables<DevCells>;

// the face shape tables into LDS, as stage_tables does for the engine's
__device__ __forceinline__ void stage_face_tables(const BndShape *__restrict__ g, BndShape &t) {
    const double *src = reinterpret_cast<const double *>(g);
    double *dst = reinterpret_cast<double *>(&t);
    for (int i = threadIdx.x; i < (int)(sizeof(BndShape) / sizeof(double)); i += blockDim.x) dst[i] = src[i];
    __syncthreads();
}

// part[blockIdx.x][kPartStride]: the sums of the NPG_NBND channels over the faces of row blockIdx.x; faces_out[ch][orig[face]] if asked
template <int NB>
__global__ void __launch_bounds__(kBndBlock) k_boundary_faces(BndFaces t, const BndShape *__restrict__ shape, const BndRow *__restrict__ rows,
                                                              const int32_t *__restrict__ orig, const double *__restrict__ xu,
                                                              const double *__restrict__ xb, int full_stress, MixClosure cl,
                                                              double *__restrict__ part, double *__restrict__ faces_out, int64_t nface) {
    __shared__ BndShape s;
    __shared__ double sh[(kBndBlock / kWave) * kPartStride];
    stage_face_tables(shape, s);
    double acc[kNBnd];
#pragma unroll
    for (int k = 0; k < kNBnd; ++k) acc[k] = 0.0;
    const BndRow row = rows[blockIdx.x];
    if ((int)threadIdx.x < row.count) {
        const int64_t f = (int64_t)row.first + threadIdx.x;
        face_integrals<NB>(s, t, xu, xb, f, full_stress != 0, cl, acc);
        if (faces_out) {
#pragma unroll
            for (int k = 0; k < kNBnd; ++k) faces_out[(size_t)k * nface + orig[f]] = acc[k];
        }
    }
    block_store_partials<kNBnd, kBndBlock / kWave>(acc, kNBnd, sh, part);
}

// out[g][ch] = the rows of group g = blockIdx.x added up: thread (slice, ch) adds rows slice, slice + kBndFoldSlices, ... in index
// order, then the slices are added in order - one order whatever the number of rows; a group without rows gives zeros
__global__ void __launch_bounds__(kBlock) k_boundary_fold(const double *__restrict__ part, BndRowRange rr, double *__restrict__ out) {
    __shared__ double tmp[kBndFoldSlices * kPartStride];
    const int g = blockIdx.x, k = threadIdx.x & (kPartStride - 1), slice = threadIdx.x >> 5;
    double sum = 0.0;
    for (int r = rr.row0[g] + slice; r < rr.row0[g + 1]; r += kBndFoldSlices) sum += part[(size_t)r * kPartStride + k];
    tmp[slice * kPartStride + k] = sum;
    __syncthreads();
    if (threadIdx.x < kNBnd) {
        double t = 0.0;
#pragma unroll
        for (int sl = 0; sl < kBndFoldSlices; ++sl) t += tmp[sl * kPartStride + threadIdx.x];
        out[(size_t)g * kNBnd + threadIdx.x] = t;
    }
}

}  // namespace npg

using namespace npg;

struct npg_boundary {
    npg_ctx *ctx = nullptr;
    npg_fe *fe = nullptr;
    int64_t nface = 0, nkept = 0;       // the caller's faces; those that count
    int ngroup = 0, nrows = 0;
    BndLayout lay;                      // host: the sort and the rows
    BndRowRange rr{};
    MixClosure cl{0.0, 0.0, 0.0, 0.0};
    DevBuf<int32_t> cell, orig;         // device, sorted faces
    DevBuf<uint8_t> local;
    DevBuf<double> area2, normal, z;    // [nkept], [3][nkept], [3][nkept]
    DevBuf<double> coef[kBndNCoef];     // [9][nkept] or null
    DevBuf<BndShape> shape;
    DevBuf<BndRow> rows;
    DevBuf<double> part;                // [nrows][kPartStride]
};

NPG_API int npg_boundary_destroy(npg_boundary *B) {
    if (!B) return NPG_OK;
    hipStreamSynchronize(B->ctx->stream);
    delete B;
    return NPG_OK;
}

NPG_API int npg_boundary_create(npg_fe *fe, int64_t nface, const int32_t *face_cell, const uint8_t *face_local, const uint8_t *face_group,
                                int ngroup, const double *face_xyz, const double *face_normal, const double *face_area2,
                                const uint8_t *face_mask, npg_boundary **out) {
    NPG_REQUIRE(fe && out, "npg_boundary_create: NULL argument");
    NPG_HIP(hipSetDevice(fe->ctx->device));
    {   // an embedded 2-D engine keeps every quadrature point on the face lambda_4 = 0 of its padded tetrahedra: it has no boundary faces
        std::vector<double> n1((size_t)fe->d.nq * 4);
        NPG_HIP(hipMemcpy(n1.data(), fe->d.N1, n1.size() * sizeof(double), hipMemcpyDeviceToHost));
        bool flat = true;
        for (int q = 0; q < fe->d.nq; ++q) flat = flat && n1[(size_t)q * 4 + 3] == 0.0;
        NPG_REQUIRE(!flat, "npg_boundary_create: an embedded 2-D engine is refused (its boundary is made of segments, not of faces)");
    }
    std::unique_ptr<npg_boundary> B(new npg_boundary());
    NPG_REQUIRE_OK(bnd_build_layout(fe->d.ncell, nface, face_cell, face_local, face_group, ngroup, face_xyz, face_normal, face_area2, face_mask,
                                    B->lay));
    B->ctx = fe->ctx;
    B->fe = fe;
    B->nface = nface;
    B->ngroup = ngroup;
    B->nkept = (int64_t)B->lay.orig.size();
    B->nrows = (int)B->lay.rows.size();
    for (int g = 0; g <= kBndMaxGroups; ++g) B->rr.row0[g] = B->lay.row0[g];
    const size_t n = (size_t)B->nkept;
    std::vector<int32_t> cell(n);
    std::vector<uint8_t> local(n);
    std::vector<double> area2(n), normal(3 * n), z(3 * n);
    for (size_t i = 0; i < n; ++i) {
        const size_t f = (size_t)B->lay.orig[i];
        cell[i] = face_cell[f], local[i] = face_local[f], area2[i] = face_area2[f];
        for (int a = 0; a < 3; ++a) normal[a * n + i] = face_normal[(size_t)a * nface + f], z[a * n + i] = face_xyz[(size_t)(3 * a + 2) * nface + f];
    }
    std::vector<BndShape> shape(1);
    bnd_shape_tables(shape[0]);
    NPG_HIP(B->cell.upload(cell));
    NPG_HIP(B->orig.upload(B->lay.orig));
    NPG_HIP(B->local.upload(local));
    NPG_HIP(B->area2.upload(area2));
    NPG_HIP(B->normal.upload(normal));
    NPG_HIP(B->z.upload(z));
    NPG_HIP(B->shape.upload(shape));
    NPG_HIP(B->rows.upload(B->lay.rows));
    NPG_HIP(B->part.alloc((size_t)B->nrows * kPartStride));
    *out = B.release();
    return NPG_OK;
}

NPG_API int npg_boundary_set_coeff(npg_boundary *B, int which, const double *table) {
    NPG_REQUIRE(B, "npg_boundary_set_coeff: NULL argument");
    NPG_REQUIRE(which >= 0 && which < kBndNCoef, "npg_boundary_set_coeff: which must be NPG_BND_NU .. NPG_BND_FLUX, got %d", which);
    const size_t n = (size_t)B->nkept;
    std::vector<double> t;
    if (table) {
        t.resize(kBndQ * n);
        for (int q = 0; q < kBndQ; ++q)
            for (size_t i = 0; i < n; ++i) {
                const double v = table[(size_t)q * B->nface + B->lay.orig[i]];
                NPG_REQUIRE(std::isfinite(v), "npg_boundary_set_coeff: table %d is not finite at point %d of face %d", which, q, B->lay.orig[i]);
                t[q * n + i] = v;
            }
    }
    NPG_HIP(hipSetDevice(B->ctx->device));
    NPG_HIP(hipStreamSynchronize(B->ctx->stream));          // a compute still in flight reads the table this call replaces
    NPG_HIP(B->coef[which].upload(t));
    return NPG_OK;
}

NPG_API int npg_boundary_set_closure(npg_boundary *B, double kappa_c, double N2min, double alpha, double N2c) {
    NPG_REQUIRE(B, "npg_boundary_set_closure: NULL argument");
    NPG_REQUIRE(std::isfinite(kappa_c) && kappa_c >= 0.0 && std::isfinite(N2min) && std::isfinite(alpha) && std::isfinite(N2c),
                "npg_boundary_set_closure: kappa_c must be finite and >= 0, N2min, alpha and N2c finite");
    NPG_REQUIRE(kappa_c == 0.0 || N2min > 0.0, "npg_boundary_set_closure: kappa_c > 0 needs N2min > 0, got %g", N2min);
    B->cl = MixClosure{kappa_c, N2min, alpha, N2c};
    return NPG_OK;
}

NPG_API int npg_boundary_compute(npg_boundary *B, const npg_vec *x_inv, const npg_vec *b, int full_stress, npg_vec *out, npg_vec *faces_out) {
    NPG_REQUIRE(B && x_inv && b && out, "npg_boundary_compute: NULL argument");
    npg_fe *fe = B->fe;
    NPG_REQUIRE_OK(check_state_vectors("npg_boundary_compute", fe->n_inv, fe->n_b, x_inv->n, b->n));
    NPG_REQUIRE(out->n >= (int64_t)B->ngroup * NPG_NBND, "npg_boundary_compute: out holds %lld doubles, needs ngroup * NPG_NBND = %d",
                (long long)out->n, B->ngroup * NPG_NBND);
    NPG_REQUIRE(!faces_out || faces_out->n >= B->nface * NPG_NBND, "npg_boundary_compute: faces_out holds %lld doubles, needs NPG_NBND * nface = %lld",
                (long long)faces_out->n, (long long)(B->nface * NPG_NBND));
    NPG_REQUIRE(full_stress == 0 || full_stress == 1, "npg_boundary_compute: full_stress must be 0 or 1, got %d", full_stress);
    NPG_REQUIRE(x_inv->ctx == fe->ctx && b->ctx == fe->ctx && out->ctx == fe->ctx && (!faces_out || faces_out->ctx == fe->ctx),
                "npg_boundary_compute: arguments of different contexts");
    NPG_HIP(hipSetDevice(fe->ctx->device));
    hipStream_t st = fe->ctx->stream;
    if (faces_out && B->nface > 0)      // faces that do not count keep zeros
        NPG_HIP(hipMemsetAsync(faces_out->d, 0, (size_t)B->nface * NPG_NBND * sizeof(double), st));
    if (B->nrows > 0) {
        BndFaces t{cell_view(fe->d), B->nkept, B->cell, B->local, B->area2, B->normal, B->z, {}};
        for (int i = 0; i < kBndNCoef; ++i) t.coef_[i] = B->coef[i];
        const dim3 grid((unsigned)B->nrows), block(kBndBlock);
        double *fo = faces_out ? faces_out->d : nullptr;
        if (fe->d.nb == 10)
            hipLaunchKernelGGL(k_boundary_faces<10>, grid, block, 0, st, t, B->shape.p, B->rows.p, B->orig.p, x_inv->d, b->d, full_stress, B->cl,
                               B->part.p, fo, B->nface);
        else
            hipLaunchKernelGGL(k_boundary_faces<4>, grid, block, 0, st, t, B->shape.p, B->rows.p, B->orig.p, x_inv->d, b->d, full_stress, B->cl,
                               B->part.p, fo, B->nface);
        NPG_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_boundary_fold, dim3((unsigned)B->ngroup), dim3(kBlock), 0, st, B->part.p, B->rr, out->d);
    NPG_HIP(hipGetLastError());
    return NPG_OK;
}
