// The preconditioner handle (npg_precond) and what its three translation units share: dense_inv.hip (the explicit dense inverse),
// mg.hip (the multigrid and block-diagonal kinds, the handle's life and its application) and fgmres.hip (the flexible GMRES
// that applies it).  Internal: not part of the C ABI.
#pragma once
#include <algorithm>
#include <map>

#include "common.h"

// A^-1 of a small system as a dense array in HBM (dense_inv.hip): NPG_PC_DENSE, or the multigrid's exact coarsest-level solve.
// Exactly one storage is held once the build has finished; the build alone writes these fields.
enum DenseStorage { kDenseNone = 0, kDenseF64, kDenseF32, kDenseF16 };
struct DenseInv {
    int64_t n = 0;
    npg::DevBuf<double> M;       // A^-1, column-major (fp64 storage) ...
    npg::DevBuf<float> Mf;       // ... or rounded to fp32 (half the bytes per application; a preconditioner may be inexact),
    int64_t ldf = 0;             //     leading dimension ldf = n rounded up to 4 (16-byte aligned columns)
    npg::DevBuf<_Float16> Mh;    // ... or to fp16, column j divided by cs[j] = its largest magnitude (a quarter of the bytes),
    npg::DevBuf<double> cs;      //     leading dimension ldf = n rounded up to 8
    npg::DevBuf<double> part;    // [nsplit][n] partial products
    int nsplit = 0;
    DenseStorage held = kDenseNone;
    bool ready() const { return held != kDenseNone; }
    DenseStorage storage() const { return held; }
};

struct MgLevel {
    const npg_csr *A = nullptr, *G = nullptr, *D = nullptr, *Dinv = nullptr, *S = nullptr, *P = nullptr, *R = nullptr;
    const npg_csr *Gh = nullptr;                     // Dinv G (npg_precond_mg_set_scaled_gradient): one Dinv product less per step
    int64_t n = 0, nu = 0, np = 0;
    npg::DevBuf<double> sdinv;                       // 1 / diag(S)
    npg::DevBuf<double> r, t, rhs, dp, dp2, res, x, b;
    // distributed level (npg_precond_mg_set_level_dist): this rank's rows of every operator; n, nu, np count OWNED rows, the
    // operators' column spaces are [owned | ghosts] and the vectors that feed them carry the ghost entries behind the owned
    // ones, filled by these plans before each product - hx: whole vectors (A), hu: velocity parts (D), hp: pressure parts (G, S)
    npg_halo *hx = nullptr, *hu = nullptr, *hp = nullptr;
    bool dist = false;
    // transfers between TWO distributed levels (npg_precond_mg_set_transfer_dist; this level being the finer one): P holds this
    // rank's rows over the coarser level's [owned | ghosts of hP] columns, R the coarser level's owned rows over this level's
    // [owned | ghosts of hR] columns; the vectors that feed them are copied into xP / rR, whose ghost segments the plans fill
    npg_halo *hP = nullptr, *hR = nullptr;
    npg::DevBuf<double> xP, rR;
    // fp32 gather-layout copy of the iterate for the residuals r = b - A x of a large level whose A carries windowed tiles
    // (csr.hip: spmv_epi_gather32; mg_prepare)
    npg::DevBuf<float> xg;
    int64_t xg_n = 0;
    bool nb_ok = false;        // t = Dinv r_u may ride in the residual kernel (node-blocked A with Dinv's node counts; mg_prepare)
};

struct BlockPc {
    int64_t off = 0, n = 0;
    const npg_csr *A = nullptr;
    const npg_vec *jac = nullptr;
    npg_cg *cg = nullptr;
    npg_ilu0 *ilu = nullptr;                         // M of the block's CG: these factors instead of the Jacobi vector
    npg_vec *xk = nullptr, *rk = nullptr;            // the block's warm-started solution / right-hand side
    int64_t itmax = 0;
    double atol = 0.0, rtol = 0.0;
};

struct npg_precond {
    npg_ctx *ctx = nullptr;
    int kind = 0;
    int64_t n = 0;
    DenseInv dense;            // NPG_PC_DENSE, or the multigrid's exact coarsest-level solve
    // multigrid
    std::vector<MgLevel> L;
    double omega = 2.5, jw = 0.7;
    int sweeps = 3, nu1 = 2, nu2 = 2, coarse = 20, gamma = 1;
    int mixed = 0;             // the cycle's SpMVs read fp32 copies of the level matrices' values (npg_precond_mg_set_mixed)
    // one instantiated hipGraph of the V-cycle per (input, output) address pair: flexible GMRES applies the preconditioner
    // to the same `memory` basis / Z column pairs in every restart cycle, so a cycle's ~300 launches (most of them
    // latency-bound coarse-level kernels) are enqueued by one hipGraphLaunch
    std::map<std::pair<const double *, double *>, hipGraphExec_t> graphs;
    uint64_t graphs_gen = 0;   // sum of the borrowed level matrices' generation counters when the graphs were captured
    bool use_graphs = true;
    // block diagonal
    std::vector<BlockPc> blocks;
    int64_t inner_iterations = 0, applications = 0;
    int64_t cycle_bytes = 0;   // bytes one application streams as its operators are laid out (counted once: byte_sink, common.h)
};

namespace npg {

static inline int grid_for(int64_t n, int cap = 2048) {
    int64_t g = (n + kBlock - 1) / kBlock;
    return (int)std::max<int64_t>(1, std::min<int64_t>(g, cap));
}

// dense_inv.hip.  The build replaces d by A^-1 of a plain-CSR matrix (fp64 storage; fp32: rounded; fp16: column-scaled fp16 where
// the acceptance check passes, fp32 otherwise) and leaves d empty when it fails; the apply is z = a A^-1 r + b z read from `from`.
int dense_build(npg_ctx *ctx, DenseInv &d, const npg_csr *A, bool fp32, bool fp16 = false);
int dense_apply(npg_ctx *ctx, const DenseInv &d, DenseStorage from, const double *r, double *z, double a, double b);
inline void dense_free(DenseInv &d) { d = DenseInv{}; }

// mg.hip.  z = M^-1 r on raw device pointers (what npg_precond_apply checks is the caller's to have checked), and
// y = a x + b y on the context's stream (b == 0: y is not read; x may be y)
int precond_apply_raw(npg_precond *pc, const double *r, double *z);
void axpby(npg_ctx *c, double *y, double a, const double *x, double b, int64_t n);

}  // namespace npg
