// The element engine's device tables and handle, shared by the translation units that read them (fe.hip: assembly; sample.hip:
// point evaluation of the state; integrals.hip: quadrature integrals of the state), and the shape tables they stage in LDS.
#pragma once
#include "cell_view.h"
#include "common.h"

namespace npg {

struct FeDev {
    int64_t ncell;
    int nq, nb;                 // nb = buoyancy nodes per cell (10 or 4)
    const double *G;            // [12][ncell]   grad lambda_k, component a at (3k+a)
    const double *wdet;         // [ncell]
    const double *qw, *N2, *dN2, *Nb, *dNb, *N1;
    const int32_t *cu;          // [30][ncell]  (3*i + a)
    const int32_t *cp;          // [4][ncell]
    const int32_t *cb;          // [nb][ncell]
    const double *u_diri, *b_diri;
    const double *nu, *kh, *kv, *f;   // [nq][ncell] or null
};

constexpr int kMaxQ = 16;

// R = the arithmetic type of the element-LOCAL work (shape tables, geometry, nodal values, the integrand at a quadrature
// point): double, or float for the mixed mode of BASELINE.json configs[4] ("fp32 assembly / fp64 solve").  Whatever R is,
// sums over quadrature points, over the cells of a row and everything downstream (CSR values, right-hand sides, solvers)
// are fp64, and all HBM tables stay fp64 (converted on load).
template <typename R>
struct FeTablesT {
    R qw[kMaxQ];
    R N2[kMaxQ * 10];
    R dN2[kMaxQ * 40];
    R Nb[kMaxQ * 10];
    R dNb[kMaxQ * 40];
    R N1[kMaxQ * 4];
};
using FeTables = FeTablesT<double>;

template <typename R>
__device__ __forceinline__ void stage_tables(const FeDev &d, FeTablesT<R> &t) {
    for (int i = threadIdx.x; i < d.nq; i += blockDim.x) t.qw[i] = (R)d.qw[i];
    for (int i = threadIdx.x; i < d.nq * 10; i += blockDim.x) t.N2[i] = (R)d.N2[i];
    for (int i = threadIdx.x; i < d.nq * 40; i += blockDim.x) t.dN2[i] = (R)d.dN2[i];
    for (int i = threadIdx.x; i < d.nq * d.nb; i += blockDim.x) t.Nb[i] = (R)d.Nb[i];
    for (int i = threadIdx.x; i < d.nq * d.nb * 4; i += blockDim.x) t.dNb[i] = (R)d.dNb[i];
    for (int i = threadIdx.x; i < d.nq * 4; i += blockDim.x) t.N1[i] = (R)d.N1[i];
    __syncthreads();
}

// ---- row-owner matrix assembly (fe.hip: k_assemble_*; tracers.hip: k_redi_matrix) ----------------------------------------
constexpr int kQL = 16;      // lanes per CSR row = kMaxQ: lane = quadrature point

#if defined(__HIPCC__)
__device__ __forceinline__ int64_t csr_slot(const int64_t *rowptr, const int32_t *col, int32_t row, int32_t c) {
    int64_t lo = rowptr[row], hi = rowptr[row + 1] - 1;
    while (lo <= hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int32_t v = col[mid];
        if (v == c) return mid;
        if (v < c) lo = mid + 1; else hi = mid - 1;
    }
    return -1;
}

// a row owner adds into its own row: no atomic, contributions arrive in the fixed order of its adjacency list
__device__ __forceinline__ void row_add(const int64_t *rowptr, const int32_t *col, double *val, int32_t row, int32_t c,
                                        double v, int *missing) {
    const int64_t s = csr_slot(rowptr, col, row, c);
    if (s >= 0) val[s] += v;
    else if (v != 0.0) atomicAdd(missing, 1);    // a numerically non-zero entry outside the pattern is an error
}

// physical gradient of buoyancy basis function i at quadrature point q
template <typename R, int NB>
__device__ __forceinline__ void grad_b(const FeTablesT<R> &t, const R *G, int q, int i, R &gx, R &gy, R &gz) {
    const R *dn = &t.dNb[(q * NB + i) * 4];
    gx = dn[0] * G[0] + dn[1] * G[3] + dn[2] * G[6] + dn[3] * G[9];
    gy = dn[0] * G[1] + dn[1] * G[4] + dn[2] * G[7] + dn[3] * G[10];
    gz = dn[0] * G[2] + dn[1] * G[5] + dn[2] * G[8] + dn[3] * G[11];
}
#endif

// the engine's cell tables as the diagnostics read them (cell_view.h)
using DevCells = CellView<CompMajor>;
__host__ __device__ __forceinline__ DevCells cell_view(const FeDev &d) {
    return DevCells{d.cu, d.cp, d.cb, d.G, d.u_diri, d.b_diri, d.ncell, d.nb, d.wdet, d.nu, d.kh, d.kv, d.nq};
}

}  // namespace npg

struct npg_fe {
    npg_ctx *ctx = nullptr;
    npg::FeDev d{};
    int64_t n_inv = 0, n_b = 0;
    int64_t n_b_diri = 0;           // entries of the buoyancy Dirichlet value table (tracers keep one of their own per tracer)
    std::vector<void *> allocs;
    double *loc = nullptr;          // [nb][ncell]
    double *loc_inv = nullptr;      // [34][ncell], as iidx addresses it; allocated by the first call that needs it (fe_ensure_loc_inv)
    int64_t *gptr = nullptr;        // inverted index of the buoyancy rows (vector pass 2, matrix rows)
    int32_t *gidx = nullptr;
    int64_t *iptr = nullptr;        // inverted index of the inversion rows [u; p]: (local DoF l) * ncell + cell
    int32_t *iidx = nullptr;
    double *coef[4] = {nullptr, nullptr, nullptr, nullptr};   // nu, kappa_h, kappa_v, f
    double *kv0 = nullptr;          // background kappa_v for the convection closure
    double *hcell = nullptr;
    int *missing = nullptr;
    double *scratch_vec = nullptr;  // n_b doubles
    int precision = NPG_FE_FP64;    // arithmetic of the element-local work (npg_fe_set_precision)
};

namespace npg {
// out[r] = the sum of row r's entries of fe->loc in cell order: fe.hip's k_gather_rows with empty RhsTerms, on the engine's stream
int fe_gather_rows(npg_fe *fe, npg_vec *out);
// the same kernel through any inverted index: out[r] = the sum of loc[idx[k]], ptr[r] <= k < ptr[r + 1], r < n = out->n
int fe_gather_index(npg_fe *fe, const int64_t *ptr, const int32_t *idx, const double *loc, int64_t n, npg_vec *out);
// fe->loc_inv, allocated on first use with its four pressure planes zeroed (tangent_adjoint.hip)
int fe_ensure_loc_inv(npg_fe *fe);
}  // namespace npg
