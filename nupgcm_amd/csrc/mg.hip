// General preconditioners for the saddle-point inversion: the multigrid and block-diagonal kinds, and the handle's life and
// application.  (The explicit dense inverse - the NPG_PC_DENSE kind and the multigrid's exact coarsest solve - is dense_inv.hip;
// the flexible GMRES that drives them all is fgmres.hip; the handle and what the three files share is precond.h.)
//
// The reference ships one experimental preconditioner, BlockDiagonalPreconditioner (src/preconditioners.jl:53-125: an inner
// CG per block - friction-only velocity block with ILU(0) / LU, pressure mass matrix / (alpha^2 eps^2) with Jacobi), which its
// author's own log shows to be slower in wall time than Diagonal(1/h^3) (scratch/inversion_log.md:107-191) because the
// friction block still needs O(1/h) inner iterations.  Two kinds live here behind one handle (npg_precond):
//
//   NPG_PC_BLOCKDIAG  the reference's construction: z[block k] = CG(A_k, r[block k]; Jacobi), warm-started from its previous
//                     output exactly as CgPreconditioner does (src/preconditioners.jl:24-37) - the device-resident CG of
//                     cg.hip is the inner solver;
//   NPG_PC_MG         geometric multigrid V-cycle on the WHOLE saddle-point system over the red-refinement hierarchy the big
//                     bowl meshes are made from (new work): rediscretised operators per level, P2 / P1
//                     nodal interpolation, and a Braess-Sarazin smoother built from node blocks:
//                         [ w Dh   G ] [du]   [r_u]      Dh = node-block diagonal of the velocity block (friction on the
//                         [ D      0 ] [dp] = [r_p]           diagonal, Coriolis coupling x and y of the same node),
//                     whose pressure system S dp = D Dh^-1 r_u - w r_p, S = D Dh^-1 G (explicit, assembled at set-up), is
//                     relaxed by a few damped-Jacobi sweeps.  Everything is SpMV + diagonal work: no triangular solves.
//
// Both are applied inexactly, so the outer solver is right-preconditioned FLEXIBLE GMRES(m) (npg_fgmres_*, fgmres.hip).
//
// Setters commit on success: a level, a pair of transfers or a block is built into locals and assigned to the handle only when
// every step has succeeded, so a refused or failed call leaves it unset and a corrected call is accepted.
#include <cmath>

#include "precond.h"
#include "device_utils.h"

namespace npg {

// y = a x + b y (b == 0: y is not read).  x may BE y (in-place scaling by flexible GMRES): no __restrict__ here.
__global__ void k_mg_axpby(double *y, double a, const double *x, double b, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        y[i] = (b == 0.0) ? a * x[i] : a * x[i] + b * y[i];
}

// y = w d x + b y
__global__ void k_mg_daxpby(double *__restrict__ y, double w, const double *__restrict__ d, const double *__restrict__ x,
                            double b, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        y[i] = (b == 0.0) ? w * d[i] * x[i] : w * d[i] * x[i] + b * y[i];
}

__global__ void k_to_float(const double *__restrict__ src, float *__restrict__ dst, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = (float)src[i];
}

void axpby(npg_ctx *c, double *y, double a, const double *x, double b, int64_t n) {
    if (byte_sink) *byte_sink += (b != 0.0 ? 24 : 16) * n;
    hipLaunchKernelGGL(k_mg_axpby, dim3(grid_for(n)), dim3(kBlock), 0, c->stream, y, a, x, b, n);
}

}  // namespace npg

using namespace npg;

static void drop_graphs(npg_precond *pc) {
    for (auto &kv : pc->graphs) hipGraphExecDestroy(kv.second);
    pc->graphs.clear();
}

static inline void daxpby(npg_ctx *c, double *y, double w, const double *d, const double *x, double b, int64_t n) {
    hipLaunchKernelGGL(k_mg_daxpby, dim3(grid_for(n)), dim3(kBlock), 0, c->stream, y, w, d, x, b, n);
}

NPG_API int npg_precond_create(npg_ctx *ctx, int kind, int nparts, npg_precond **out) {
    NPG_REQUIRE(ctx && out, "npg_precond_create: NULL argument");
    NPG_REQUIRE(kind == NPG_PC_MG || kind == NPG_PC_BLOCKDIAG || kind == NPG_PC_DENSE, "npg_precond_create: unknown kind %d",
                kind);
    NPG_REQUIRE(nparts >= 1 && nparts <= 16, "npg_precond_create: need 1..16 levels / blocks");
    std::unique_ptr<npg_precond> pc(new npg_precond());
    pc->ctx = ctx;
    pc->kind = kind;
    // relaunching hipGraphs under rocprofv3's kernel tracer can fault inside the tool (a batch of AQL packets that straddles
    // the end of the queue ring: profiles/r03_rocprofv3_graph_fault.txt): a traced process launches the cycle eagerly unless
    // NPG_MG_EAGER=0 says otherwise
    const bool traced = profiler_attached();
    pc->use_graphs = getenv("NPG_MG_EAGER") ? atoi(getenv("NPG_MG_EAGER")) == 0 : !traced;
    static bool said = false;
    if (traced && !getenv("NPG_MG_EAGER") && !said && (said = true))
        fprintf(stderr, "[npg] rocprofv3 detected: multigrid cycles are launched eagerly instead of replayed from hipGraphs "
                        "(NPG_MG_EAGER=0 overrides)\n");
    if (kind == NPG_PC_MG) pc->L.resize(nparts);
    if (kind == NPG_PC_BLOCKDIAG) pc->blocks.resize(nparts);
    *out = pc.release();
    return NPG_OK;
}

NPG_API int npg_precond_destroy(npg_precond *pc) {
    if (!pc) return NPG_OK;
    hipStreamSynchronize(pc->ctx->stream);
    drop_graphs(pc);
    for (BlockPc &b : pc->blocks) {
        if (b.cg) npg_cg_destroy(b.cg);
        if (b.xk) npg_vec_destroy(b.xk);
        if (b.rk) npg_vec_destroy(b.rk);
    }
    delete pc;
    return NPG_OK;
}

// the multigrid's coarsest level solved exactly by its explicit inverse instead of `coarse_sweeps` smoothing steps; call
// again after npg_precond_mg_update_level(level 0) to rebuild it
NPG_API int npg_precond_mg_set_coarse_dense(npg_precond *pc, int on) {
    NPG_REQUIRE(pc && pc->kind == NPG_PC_MG && !pc->L.empty() && pc->L[0].A, "npg_precond_mg_set_coarse_dense: level 0 is not set");
    NPG_HIP(hipStreamSynchronize(pc->ctx->stream));
    drop_graphs(pc);
    if (!on) {
        dense_free(pc->dense);
        return NPG_OK;
    }
    NPG_REQUIRE(on >= 1 && on <= 3, "npg_precond_mg_set_coarse_dense: mode %d (0 off, 1 fp64, 2 fp32, 3 scaled fp16 storage)", on);
    return dense_build(pc->ctx, pc->dense, pc->L[0].A, on == 2, on == 3);
}

// fp32 copies of one level's operators (mixed mode)
static int mg_refresh_fp32(const MgLevel &l) {
    int rc;
    for (const npg_csr *M : {l.A, l.G, l.D, l.Dinv, l.S, l.P, l.R, l.Gh})
        if (M && (rc = csr_refresh_fp32(M))) return rc;
    return NPG_OK;
}

// a zero-filled vector of a level (at least one entry: a null pointer means "not allocated")
static int mg_alloc(npg_ctx *ctx, DevBuf<double> &v, int64_t n) {
    const size_t len = std::max<size_t>(1, (size_t)n);
    NPG_HIP(v.alloc(len));
    NPG_HIP(hipMemsetAsync(v.p, 0, len * sizeof(double), ctx->stream));
    return NPG_OK;
}

// Set level `level` from operators its entry point has checked: replicated (no plans: D->n = nu, G->n = np, A->n = n) or this
// rank's rows with [owned | ghosts] column spaces and the three plans that fill the ghosts.  The vectors that feed an operator
// have its column count.  The level is built apart and assigned when every step has succeeded: a failure leaves it unset.
static int mg_set_level(npg_precond *pc, int level, const npg_csr *A, int64_t nu, const npg_csr *G, const npg_csr *D,
                        const npg_csr *Dinv, const npg_csr *S, const npg_csr *P, const npg_csr *R, npg_halo *hx, npg_halo *hu,
                        npg_halo *hp) {
    npg_ctx *ctx = pc->ctx;
    const bool finest = level + 1 == (int)pc->L.size();
    MgLevel l;
    l.A = A; l.G = G; l.D = D; l.Dinv = Dinv; l.S = S; l.P = P; l.R = R;
    l.n = A->m; l.nu = nu; l.np = l.n - nu;
    l.hx = hx; l.hu = hu; l.hp = hp;
    l.dist = hx != nullptr;
    int rc;
    if ((rc = mg_alloc(ctx, l.sdinv, l.np))) return rc;
    npg_vec sv;
    sv.ctx = ctx; sv.n = l.np; sv.d = l.sdinv; sv.owns = false;
    if ((rc = npg_csr_inv_diag(S, &sv))) return rc;
    if ((rc = mg_alloc(ctx, l.r, l.n)) || (rc = mg_alloc(ctx, l.t, D->n)) || (rc = mg_alloc(ctx, l.rhs, l.np)) ||
        (rc = mg_alloc(ctx, l.dp, G->n)) || (rc = mg_alloc(ctx, l.dp2, G->n)) || (rc = mg_alloc(ctx, l.res, l.np)))
        return rc;
    // (the iterate of a distributed level is an SpMV input with room for the ghosts: l.x even on the finest level; a level that
    //  is not the finest receives its right-hand side from the level above)
    if ((l.dist || !finest) && (rc = mg_alloc(ctx, l.x, A->n))) return rc;
    if (!finest && (rc = mg_alloc(ctx, l.b, l.n))) return rc;
    if (pc->mixed && (rc = mg_refresh_fp32(l))) return rc;
    pc->L[level] = std::move(l);
    pc->n = A->m;      // the finest level set so far
    if (hx) pc->use_graphs = false;      // host barriers (rehearsal transports) and library collectives sit inside the cycle
    return NPG_OK;
}

NPG_API int npg_precond_mg_set_level(npg_precond *pc, int level, const npg_csr *A, int64_t nu, const npg_csr *G,
                                     const npg_csr *D, const npg_csr *Dinv, const npg_csr *S, const npg_csr *P,
                                     const npg_csr *R) {
    NPG_REQUIRE(pc && pc->kind == NPG_PC_MG, "npg_precond_mg_set_level: not a multigrid preconditioner");
    NPG_REQUIRE(level >= 0 && level < (int)pc->L.size(), "npg_precond_mg_set_level: level %d out of range", level);
    NPG_REQUIRE(A && G && D && Dinv && S, "npg_precond_mg_set_level: NULL operator");
    const int64_t n = A->m, np = n - nu;
    NPG_REQUIRE(A->n == n && nu > 0 && np > 0, "npg_precond_mg_set_level: A must be square with 0 < nu < n");
    NPG_REQUIRE(G->m == nu && G->n == np && D->m == np && D->n == nu && Dinv->m == nu && Dinv->n == nu && S->m == np &&
                    S->n == np,
                "npg_precond_mg_set_level: block shapes do not match (n = %lld, nu = %lld)", (long long)n, (long long)nu);
    NPG_REQUIRE((level == 0) == (P == nullptr) && (P == nullptr) == (R == nullptr),
                "npg_precond_mg_set_level: level 0 takes no transfer operators, every other level needs P and R");
    NPG_REQUIRE(pc->L[level].A == nullptr, "npg_precond_mg_set_level: level %d is already set", level);
    if (P) {
        NPG_REQUIRE(pc->L[level - 1].A, "npg_precond_mg_set_level: set the levels coarse to fine");
        const int64_t nc = pc->L[level - 1].n;
        NPG_REQUIRE(P->m == n && P->n == nc && R->m == nc && R->n == n,
                    "npg_precond_mg_set_level: P must be %lld x %lld and R its transpose", (long long)n, (long long)nc);
    }
    return mg_set_level(pc, level, A, nu, G, D, Dinv, S, P, R, nullptr, nullptr, nullptr);
}

// The finest level of a hierarchy, distributed: this rank's rows of every operator (column spaces [owned | ghosts]) and the
// three halo plans that fill the ghosts of the vectors feeding them; the levels below it are replicated (set with
// npg_precond_mg_set_level on every rank).  P: owned rows x all coarse columns, R: all coarse rows x owned columns.
NPG_API int npg_precond_mg_set_level_dist(npg_precond *pc, int level, const npg_csr *A, int64_t nu, const npg_csr *G,
                                          const npg_csr *D, const npg_csr *Dinv, const npg_csr *S, const npg_csr *P,
                                          const npg_csr *R, npg_halo *hx, npg_halo *hu, npg_halo *hp) {
    NPG_REQUIRE(pc && pc->kind == NPG_PC_MG, "npg_precond_mg_set_level_dist: not a multigrid preconditioner");
    NPG_REQUIRE(level >= 1 && level < (int)pc->L.size(), "npg_precond_mg_set_level_dist: level %d cannot be distributed", level);
    NPG_REQUIRE(A && G && D && Dinv && S && hx && hu && hp, "npg_precond_mg_set_level_dist: NULL argument");
    NPG_REQUIRE(level == (int)pc->L.size() - 1 || level == (int)pc->L.size() - 2,
                "npg_precond_mg_set_level_dist: the distributed levels are the finest one or two");
    const int64_t n = A->m, np = n - nu;
    NPG_REQUIRE(nu > 0 && np > 0 && hx->n_owned == n && A->n == n + hx->n_ghost && hu->n_owned == nu && D->m == np &&
                    D->n == nu + hu->n_ghost && hp->n_owned == np && G->m == nu && G->n == np + hp->n_ghost && S->m == np &&
                    S->n == G->n && Dinv->m == nu && Dinv->n == nu,
                "npg_precond_mg_set_level_dist: operator shapes do not match the halo plans (n = %lld, nu = %lld)", (long long)n,
                (long long)nu);
    NPG_REQUIRE(pc->L[level].A == nullptr && pc->L[level - 1].A, "npg_precond_mg_set_level_dist: set the coarser levels first, this one once");
    if (pc->L[level - 1].dist) {
        // the level below is distributed too: its transfers come with npg_precond_mg_set_transfer_dist
        NPG_REQUIRE(!P && !R, "npg_precond_mg_set_level_dist: above a distributed level P and R are set by npg_precond_mg_set_transfer_dist");
    } else {
        NPG_REQUIRE(P && R, "npg_precond_mg_set_level_dist: NULL transfer operators");
        const int64_t nc = pc->L[level - 1].n;
        NPG_REQUIRE(P->m == n && P->n == nc && R->m == nc && R->n == n, "npg_precond_mg_set_level_dist: P must be %lld x %lld and R its transpose",
                    (long long)n, (long long)nc);
    }
    return mg_set_level(pc, level, A, nu, G, D, Dinv, S, P, R, hx, hu, hp);
}

// Transfers between two DISTRIBUTED levels (`level` and the one below it, both set): P = this rank's rows of the prolongation over
// the coarser level's [owned | ghosts] columns (hP: the plan on the coarser iterate that fills those ghosts), R = the coarser
// level's owned rows of the restriction over this level's [owned | ghosts] columns (hR: the plan on this level's residual).
NPG_API int npg_precond_mg_set_transfer_dist(npg_precond *pc, int level, const npg_csr *P, const npg_csr *R, npg_halo *hP, npg_halo *hR) {
    NPG_REQUIRE(pc && pc->kind == NPG_PC_MG && level >= 1 && level < (int)pc->L.size(), "npg_precond_mg_set_transfer_dist: bad level");
    NPG_REQUIRE(P && R && hP && hR, "npg_precond_mg_set_transfer_dist: NULL argument");
    MgLevel &l = pc->L[level], &lc = pc->L[level - 1];
    NPG_REQUIRE(l.A && lc.A && l.dist && lc.dist && !l.P, "npg_precond_mg_set_transfer_dist: both levels must be distributed, the transfers set once");
    NPG_REQUIRE(hP->n_owned == lc.n && P->m == l.n && P->n == lc.n + hP->n_ghost && hR->n_owned == l.n && R->m == lc.n &&
                    R->n == l.n + hR->n_ghost,
                "npg_precond_mg_set_transfer_dist: operator shapes do not match the halo plans");
    DevBuf<double> xP, rR;
    int rc;
    if ((rc = mg_alloc(pc->ctx, xP, P->n)) || (rc = mg_alloc(pc->ctx, rR, R->n))) return rc;
    l.P = P; l.R = R; l.hP = hP; l.hR = hR;
    l.xP = std::move(xP);
    l.rR = std::move(rR);
    return NPG_OK;
}

// Swap in re-assembled operators of one level (same shapes): what the eddy closure's A refresh needs (src/model.jl:160-170)
NPG_API int npg_precond_mg_set_scaled_gradient(npg_precond *pc, int level, const npg_csr *Gh) {
    NPG_REQUIRE(pc && pc->kind == NPG_PC_MG && level >= 0 && level < (int)pc->L.size() && pc->L[level].A,
                "npg_precond_mg_set_scaled_gradient: the level is not set");
    MgLevel &l = pc->L[level];
    NPG_REQUIRE(!Gh || (Gh->m == l.G->m && Gh->n == l.G->n), "npg_precond_mg_set_scaled_gradient: Dinv G must have the shape of G (%lld x %lld)",
                (long long)l.G->m, (long long)l.G->n);
    NPG_HIP(hipStreamSynchronize(pc->ctx->stream));
    drop_graphs(pc);
    l.Gh = Gh;
    if (Gh && pc->mixed) return csr_refresh_fp32(Gh);
    return NPG_OK;
}

NPG_API int npg_precond_mg_update_level(npg_precond *pc, int level, const npg_csr *A, const npg_csr *G, const npg_csr *D,
                                        const npg_csr *Dinv, const npg_csr *S) {
    NPG_REQUIRE(pc && pc->kind == NPG_PC_MG, "npg_precond_mg_update_level: not a multigrid preconditioner");
    NPG_REQUIRE(level >= 0 && level < (int)pc->L.size() && pc->L[level].A, "npg_precond_mg_update_level: level %d is not set",
                level);
    NPG_REQUIRE(A && G && D && Dinv && S, "npg_precond_mg_update_level: NULL operator");
    MgLevel &l = pc->L[level];
    // (a distributed level's operators are row blocks with [owned | ghost] column spaces: compare with what the level holds)
    NPG_REQUIRE(A->m == l.n && A->n == l.A->n && G->m == l.nu && G->n == l.G->n && D->m == l.np && D->n == l.D->n &&
                    Dinv->m == l.nu && Dinv->n == l.nu && S->m == l.np && S->n == l.S->n,
                "npg_precond_mg_update_level: shapes differ from the level's");
    NPG_HIP(hipStreamSynchronize(pc->ctx->stream));
    drop_graphs(pc);
    l.A = A; l.G = G; l.D = D; l.Dinv = Dinv; l.S = S;
    npg_vec sv;
    sv.ctx = pc->ctx; sv.n = l.np; sv.d = l.sdinv; sv.owns = false;
    int rc = npg_csr_inv_diag(S, &sv);
    if (rc) return rc;
    return pc->mixed ? mg_refresh_fp32(l) : NPG_OK;
}

// Mixed precision: the cycle's SpMVs read fp32 copies of the level operators' values (8 instead of 12 bytes per entry, 12
// instead of 20 per node record); vectors, products and sums stay fp64, and so does the outer flexible GMRES with its
// own SpMV - a preconditioner may be inexact.  The copies are rebuilt by npg_precond_mg_update_level.
NPG_API int npg_precond_mg_set_mixed(npg_precond *pc, int on) {
    NPG_REQUIRE(pc && pc->kind == NPG_PC_MG, "npg_precond_mg_set_mixed: not a multigrid preconditioner");
    NPG_HIP(hipStreamSynchronize(pc->ctx->stream));
    drop_graphs(pc);
    pc->mixed = on ? 1 : 0;
    if (pc->mixed)
        for (const MgLevel &l : pc->L)
            if (l.A) {
                int rc = mg_refresh_fp32(l);
                if (rc) return rc;
            }
    return NPG_OK;
}

NPG_API int npg_precond_mg_set_params(npg_precond *pc, double omega, double jacobi_weight, int schur_sweeps, int nu1,
                                      int nu2, int coarse_sweeps) {
    NPG_REQUIRE(pc && pc->kind == NPG_PC_MG, "npg_precond_mg_set_params: not a multigrid preconditioner");
    NPG_REQUIRE(omega > 0 && jacobi_weight > 0 && schur_sweeps >= 1 && nu1 >= 0 && nu2 >= 0 && nu1 + nu2 >= 1 &&
                    coarse_sweeps >= 1,
                "npg_precond_mg_set_params: bad parameter");
    NPG_HIP(hipStreamSynchronize(pc->ctx->stream));
    drop_graphs(pc);
    pc->omega = omega; pc->jw = jacobi_weight; pc->sweeps = schur_sweeps;
    pc->nu1 = nu1; pc->nu2 = nu2; pc->coarse = coarse_sweeps;
    return NPG_OK;
}

NPG_API int npg_precond_mg_set_cycle(npg_precond *pc, int gamma) {
    NPG_REQUIRE(pc && pc->kind == NPG_PC_MG && (gamma == 1 || gamma == 2), "npg_precond_mg_set_cycle: gamma must be 1 (V) or 2 (W)");
    NPG_HIP(hipStreamSynchronize(pc->ctx->stream));
    drop_graphs(pc);
    pc->gamma = gamma;
    return NPG_OK;
}

// Levels of a million rows and more whose matrix carries a windowed tile set form their residuals from the fp32 gather-layout
// copy of the iterate (one fill kernel + the windowed product: 150 + 8 instead of 190 us at 2.15 M unknowns) - the rounding of x,
// 6e-8 |A| |x|, is far below what a smoothing step or the coarse-grid correction leaves; the outer flexible GMRES forms its own
// product from the fp64 vector.  Called before a cycle is enqueued or captured: buffers follow the matrices' current layouts.
constexpr int64_t kMgGatherMinRows = 1000000;
static int mg_prepare(npg_precond *pc) {
    static const bool on = !getenv("NPG_MG_GATHER32") || atoi(getenv("NPG_MG_GATHER32")) != 0;
    static const bool nb_on = !getenv("NPG_MG_NB_EPILOGUE") || atoi(getenv("NPG_MG_NB_EPILOGUE")) != 0;
    for (MgLevel &l : pc->L) {
        const bool nb = nb_on && l.A && l.Gh && !l.dist && !pc->mixed && nb_epilogue_ok(l.A, l.Dinv, l.nu);
        if (nb != l.nb_ok) {
            NPG_HIP(hipStreamSynchronize(pc->ctx->stream));
            drop_graphs(pc);
            l.nb_ok = nb;
        }
        const int64_t need = (on && l.A && !l.dist && l.n >= kMgGatherMinRows) ? gather32_floats(l.A) : 0;
        if (need == l.xg_n) continue;
        NPG_HIP(hipStreamSynchronize(pc->ctx->stream));
        drop_graphs(pc);
        DevBuf<float> xg;                       // allocated before the old one is released: a failure leaves the level as it was
        if (need) {
            NPG_HIP(xg.alloc((size_t)need));
            NPG_HIP(hipMemsetAsync(xg.p, 0, (size_t)need * sizeof(float), pc->ctx->stream));    // (the pad slots stay zero)
        }
        l.xg = std::move(xg);
        l.xg_n = need;
    }
    return NPG_OK;
}
// y = alpha A x + beta c (+ second output) on level l: the level's matrix in whichever form serves it fastest
static int mg_product(npg_precond *pc, MgLevel &l, const double *x, const SpmvEpi &e, const NbEpi *nb = nullptr) {
    return l.xg ? spmv_epi_gather32(l.A, x, l.xg, e, nb) : spmv_epi(l.A, x, e, nb);
}

// nsteps Braess-Sarazin steps on level l for A x = b.  Eight launches per step (seven with the scaled gradient): the vector updates ride in the epilogues of
// the SpMV kernels (SpmvEpi) - on the coarse levels, where every kernel is latency-bound, the launch count is the cost.
static int mg_smooth(npg_precond *pc, int lev, double *x, const double *b, int nsteps, bool x_is_zero) {
    MgLevel &l = pc->L[lev];
    npg_ctx *c = pc->ctx;
    const int64_t nu = l.nu, np = l.np;
    int rc;
    for (int s = 0; s < nsteps; ++s) {
        const bool zero = x_is_zero && s == 0;
        const double *r = l.r;
        bool have_t = false;                                                         // t (and x_u += t / w) formed by the residual kernel
        if (zero) {
            r = b;                                                                   // r = b - A 0
        } else {
            if (l.hx && (rc = halo_exchange_raw(l.hx, x))) return rc;
            SpmvEpi e{};                                                             // r = b - A x
            e.alpha = -1.0; e.beta = 1.0; e.c = b; e.y = l.r; e.f32 = pc->mixed;
            if (l.nb_ok) {
                // ... and t = Dh^-1 r_u in the same kernel: the node-block epilogue (NbEpi); x_u takes t / w further down, in the
                // kernel that subtracts (Dh^-1 G) dp / w (x is this product's input: it must not change under it)
                const npg_csr *Di = l.Dinv;
                NbEpi nb{Di->rowptr, Di->col, Di->val, (int32_t)nu, l.t, nullptr, 0.0, 0};
                if ((rc = mg_product(pc, l, x, e, &nb))) return rc;
                have_t = true;
            }
            if (!have_t && (rc = mg_product(pc, l, x, e))) return rc;
        }
        if (have_t) {
        } else if (l.Gh) {
            // x_u += Dh^-1 (r_u - G dp) / w  =  t / w - (Dh^-1 G) dp / w: the first part rides in the kernel that forms t
            SpmvEpi e{};                                                             // t = Dh^-1 r_u ; x_u (+)= t / w
            e.alpha = 1.0; e.beta = 0.0; e.y = l.t; e.f32 = pc->mixed;
            e.w = 1.0 / pc->omega; e.zin = zero ? nullptr : x; e.zc = 1.0; e.z = x;
            if ((rc = spmv_epi(l.Dinv, r, e))) return rc;
        } else if ((rc = spmv_raw(l.Dinv, r, l.t, 1.0, 0.0, pc->mixed))) return rc;  // t = Dh^-1 r_u
        double *dp = l.dp, *dq = l.dp2;
        if (l.hu && (rc = halo_exchange_raw(l.hu, l.t))) return rc;
        {
            SpmvEpi e{};                                                             // rhs = D t - w r_p ; dp = jw rhs / diag S
            e.alpha = 1.0; e.beta = -pc->omega; e.c = r + nu; e.y = l.rhs;
            e.w = pc->jw; e.dg = l.sdinv; e.z = dp; e.f32 = pc->mixed;
            if ((rc = spmv_epi(l.D, l.t, e))) return rc;
        }
        for (int k = 1; k < pc->sweeps; ++k) {                                       // damped Jacobi on S dp = rhs
            if (l.hp && (rc = halo_exchange_raw(l.hp, dp))) return rc;
            SpmvEpi e{};                                                             // res = rhs - S dp ; dq = dp + jw res / diag S
            e.alpha = -1.0; e.beta = 1.0; e.c = l.rhs; e.y = l.res;
            e.w = pc->jw; e.dg = l.sdinv; e.zin = dp; e.zc = 1.0; e.z = dq; e.f32 = pc->mixed;
            if ((rc = spmv_epi(l.S, dp, e))) return rc;
            std::swap(dp, dq);
        }
        if (l.hp && (rc = halo_exchange_raw(l.hp, dp))) return rc;
        if (l.Gh && have_t) {
            SpmvEpi e{};                                 // du = (t - (Dh^-1 G) dp) / w  (into t) ; x_u += du  (second output)
            e.alpha = -1.0 / pc->omega; e.beta = 1.0 / pc->omega; e.c = l.t; e.y = l.t; e.f32 = pc->mixed;
            e.w = 1.0; e.zin = x; e.zc = 1.0; e.z = x;
            if ((rc = spmv_epi(l.Gh, dp, e))) return rc;
        } else if (l.Gh) {
            if ((rc = spmv_raw(l.Gh, dp, x, -1.0 / pc->omega, 1.0, pc->mixed))) return rc;   // x_u -= (Dh^-1 G) dp / w
        } else {
            SpmvEpi e{};                                                             // t = r_u - G dp   (t is free again)
            e.alpha = -1.0; e.beta = 1.0; e.c = r; e.y = l.t; e.f32 = pc->mixed;
            if ((rc = spmv_epi(l.G, dp, e))) return rc;
            if ((rc = spmv_raw(l.Dinv, l.t, x, 1.0 / pc->omega, zero ? 0.0 : 1.0, pc->mixed))) return rc;   // x_u += Dh^-1 t / w
        }
        axpby(c, x + nu, 1.0, dp, zero ? 0.0 : 1.0, np);                             // x_p += dp
    }
    return NPG_OK;
}

// One multigrid cycle on level `lev` for A x = b: gamma = 1 is the V-cycle, gamma = 2 the W-cycle (the coarse problem of
// every level is visited gamma times, the second visit continuing from the first one's result).
static int mg_cycle(npg_precond *pc, int lev, double *x, const double *b, bool x_is_zero) {
    int rc;
    if (lev == 0 && pc->dense.ready()) {                                             // direct coarsest-level solve
        const DenseInv &d = pc->dense;
        if (x_is_zero) return dense_apply(pc->ctx, d, d.storage(), b, x, 1.0, 0.0);
        MgLevel &l0 = pc->L[0];
        SpmvEpi e{};
        e.alpha = -1.0; e.beta = 1.0; e.c = b; e.y = l0.r; e.f32 = pc->mixed;
        if ((rc = spmv_epi(l0.A, x, e))) return rc;
        return dense_apply(pc->ctx, d, d.storage(), l0.r, x, 1.0, 1.0);
    }
    if (lev == 0) return mg_smooth(pc, 0, x, b, pc->coarse, x_is_zero);
    MgLevel &l = pc->L[lev], &lc = pc->L[lev - 1];
    if (pc->nu1 > 0 && (rc = mg_smooth(pc, lev, x, b, pc->nu1, x_is_zero))) return rc;
    const bool still_zero = x_is_zero && pc->nu1 == 0;
    const double *rfine = b;                    // what is restricted: b itself while x = 0, else the residual
    if (!still_zero) {
        if (l.hx && (rc = halo_exchange_raw(l.hx, x))) return rc;
        SpmvEpi e{};
        e.alpha = -1.0; e.beta = 1.0; e.c = b; e.y = l.r; e.f32 = pc->mixed;
        if ((rc = mg_product(pc, l, x, e))) return rc;
        rfine = l.r;
    }
    if (l.hR) {
        // both levels distributed: the coarser level's OWNED rows of R reach this level's residual at a few rows of other ranks
        NPG_HIP(hipMemcpyAsync(l.rR, rfine, (size_t)l.n * sizeof(double), hipMemcpyDeviceToDevice, pc->ctx->stream));
        if ((rc = halo_exchange_raw(l.hR, l.rR))) return rc;
        rfine = l.rR;
    }
    if ((rc = spmv_raw(l.R, rfine, lc.b, 1.0, 0.0, pc->mixed))) return rc;
    // a distributed level above replicated ones: R holds this rank's columns of the restriction, the coarse right-hand side is
    // the sum of the ranks' parts - after it every rank runs the coarse levels redundantly on identical data - and the
    // prolongation back needs no communication (P holds this rank's rows)
    if (l.dist && !lc.dist && (rc = allreduce_big_device(pc->ctx, lc.b, lc.n))) return rc;
    for (int g = 0; g < pc->gamma; ++g)
        if ((rc = mg_cycle(pc, lev - 1, lc.x, lc.b, g == 0))) return rc;
    const double *xc = lc.x;
    if (l.hP) {             // both levels distributed: this rank's rows of P reach coarse entries of other ranks
        NPG_HIP(hipMemcpyAsync(l.xP, lc.x, (size_t)lc.n * sizeof(double), hipMemcpyDeviceToDevice, pc->ctx->stream));
        if ((rc = halo_exchange_raw(l.hP, l.xP))) return rc;
        xc = l.xP;
    }
    if ((rc = spmv_raw(l.P, xc, x, 1.0, still_zero ? 0.0 : 1.0, pc->mixed))) return rc;
    return mg_smooth(pc, lev, x, b, pc->nu2, false);
}

static int mg_vcycle(npg_precond *pc, int lev, double *x, const double *b) { return mg_cycle(pc, lev, x, b, true); }

NPG_API int npg_precond_blockdiag_set(npg_precond *pc, int k, int64_t offset, const npg_csr *A, const npg_vec *jacobi,
                                      int64_t itmax, double atol, double rtol) {
    NPG_REQUIRE(pc && pc->kind == NPG_PC_BLOCKDIAG, "npg_precond_blockdiag_set: not a block-diagonal preconditioner");
    NPG_REQUIRE(k >= 0 && k < (int)pc->blocks.size() && A && jacobi, "npg_precond_blockdiag_set: bad argument");
    NPG_REQUIRE(A->m == A->n && jacobi->n == A->m && offset >= 0, "npg_precond_blockdiag_set: block must be square");
    NPG_REQUIRE(!pc->blocks[k].A, "npg_precond_blockdiag_set: block %d is already set", k);
    BlockPc b;
    b.off = offset; b.n = A->m; b.A = A; b.jac = jacobi; b.itmax = itmax; b.atol = atol; b.rtol = rtol;
    int rc;
    if ((rc = npg_cg_create(pc->ctx, b.n, &b.cg)) ||
        (rc = npg_vec_create(pc->ctx, b.n, &b.xk)) ||       // workspace.x .= 0 (src/preconditioners.jl:20)
        (rc = npg_vec_create(pc->ctx, b.n, &b.rk))) {
        npg_cg_destroy(b.cg);                               // (null: nothing to do)
        npg_vec_destroy(b.xk);
        npg_vec_destroy(b.rk);
        return rc;
    }
    pc->blocks[k] = b;
    pc->n = std::max(pc->n, offset + b.n);
    return NPG_OK;
}

NPG_API int npg_precond_blockdiag_set_ilu0(npg_precond *pc, int k, npg_ilu0 *M) {
    NPG_REQUIRE(pc && pc->kind == NPG_PC_BLOCKDIAG, "npg_precond_blockdiag_set_ilu0: not a block-diagonal preconditioner");
    NPG_REQUIRE(k >= 0 && k < (int)pc->blocks.size() && pc->blocks[k].A, "npg_precond_blockdiag_set_ilu0: block %d is not set", k);
    int64_t nnz = 0;
    if (M) {
        int rc = npg_ilu0_info(M, nullptr, nullptr, &nnz);
        if (rc) return rc;
        NPG_REQUIRE(nnz == pc->blocks[k].A->nnz, "npg_precond_blockdiag_set_ilu0: the factors are not of this block's matrix");
    }
    NPG_HIP(hipStreamSynchronize(pc->ctx->stream));
    pc->blocks[k].ilu = M;
    return NPG_OK;
}

// Counts the bytes of the application enqueued while it is alive (byte_sink, common.h) and stores them as the handle's
// cycle_bytes when it goes: once - while cycle_bytes is still 0 - or, where a cycle is captured into a graph, every time.
struct CountBytes {
    npg_precond *pc;
    int64_t count = 0;
    int64_t *const before = byte_sink;
    explicit CountBytes(npg_precond *pc_, bool always = false) : pc(pc_) {
        if (always || pc->cycle_bytes == 0) byte_sink = &count;
    }
    ~CountBytes() {
        byte_sink = before;
        if (count) pc->cycle_bytes = count;
    }
};

static int apply_dense(npg_precond *pc, const double *r, double *z) {
    NPG_REQUIRE(pc->dense.ready(), "npg_precond_apply: the dense inverse has not been set");
    CountBytes counted(pc);
    return dense_apply(pc->ctx, pc->dense, pc->dense.storage(), r, z, 1.0, 0.0);
}

static int apply_mg(npg_precond *pc, const double *r, double *z) {
    NPG_REQUIRE(pc->L.back().A, "npg_precond_apply: multigrid levels are not all set");
    if (int rcp = mg_prepare(pc)) return rcp;
    const int top = (int)pc->L.size() - 1;
    if (pc->L[top].dist) {
        // the iterate is an SpMV input: it lives in the level's own buffer, which has room for the ghost entries
        // (a distributed cycle's bytes are never counted)
        MgLevel &lt = pc->L[top];
        const int rcv = mg_vcycle(pc, top, lt.x, r);
        if (rcv) return rcv;
        NPG_HIP(hipMemcpyAsync(z, lt.x, (size_t)lt.n * sizeof(double), hipMemcpyDeviceToDevice, pc->ctx->stream));
        return NPG_OK;
    }
    if (!pc->use_graphs) {
        CountBytes counted(pc);
        return mg_vcycle(pc, top, z, r);
    }
    hipStream_t st = pc->ctx->stream;
    // the captured cycles bake in the borrowed matrices' tile tables and value arrays: a matrix whose layout was
    // rebuilt since (build_tiles, block_nodes, first fp32 copy) invalidates them.  (A borrowed matrix must outlive the
    // preconditioner or be replaced through the setters, which drop the graphs.)
    uint64_t gsum = 0;
    for (const MgLevel &lv : pc->L)
        for (const npg_csr *M : {lv.A, lv.G, lv.D, lv.Dinv, lv.S, lv.P, lv.R, lv.Gh})
            if (M) gsum += spmv_form(M)->gen;
    if (gsum != pc->graphs_gen) {
        drop_graphs(pc);
        pc->graphs_gen = gsum;
    }
    auto key = std::make_pair(r, z);
    auto it = pc->graphs.find(key);
    if (it == pc->graphs.end()) {
        if (pc->graphs.size() >= 64) drop_graphs(pc);                  // a caller that keeps changing buffers
        hipGraph_t g = nullptr;
        NPG_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        int rcv;
        {
            CountBytes counted(pc, true);
            rcv = mg_vcycle(pc, top, z, r);
        }
        const hipError_t ec = hipStreamEndCapture(st, &g);
        if (rcv || ec != hipSuccess) {
            if (g) hipGraphDestroy(g);
            if (rcv) return rcv;
        }
        NPG_HIP(ec);
        hipGraphExec_t ex = nullptr;
        const hipError_t ei = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
        hipGraphDestroy(g);
        NPG_HIP(ei);
        it = pc->graphs.emplace(key, ex).first;
    }
    NPG_HIP(hipGraphLaunch(it->second, st));
    return NPG_OK;
}

static int apply_blockdiag(npg_precond *pc, const double *r, double *z) {
    for (BlockPc &b : pc->blocks) {
        NPG_REQUIRE(b.A, "npg_precond_apply: a block has not been set");
        // mul!(yb, block.P^-1, xb): CG on the block, warm-started from its previous output (src/preconditioners.jl:24-37,118-125)
        NPG_HIP(hipMemcpyAsync(b.rk->d, r + b.off, (size_t)b.n * sizeof(double), hipMemcpyDeviceToDevice, pc->ctx->stream));
        npg_solve_stats st{};
        int rc = b.ilu ? ilu_pcg_raw(b.ilu, b.A, b.rk->d, b.xk->d, b.atol, b.rtol, b.itmax, &st)
                       : npg_cg_solve(b.cg, b.A, NPG_PRECOND_DIAG, 0.0, b.jac, b.rk, b.xk, b.atol, b.rtol, b.itmax, &st);
        if (rc) return rc;
        pc->inner_iterations += st.niter;
        // (a block solve that broke down - status 3: a non-finite or non-positive curvature, e.g. behind unusable ILU(0) factors - has
        //  NaNs in its iterate: handing them to the outer flexible GMRES would poison its basis)
        NPG_REQUIRE(st.status != 3, "npg_precond_apply: the inner CG of the block at offset %lld broke down after %d iterations; its output is not used",
                    (long long)b.off, st.niter);
        NPG_HIP(hipMemcpyAsync(z + b.off, b.xk->d, (size_t)b.n * sizeof(double), hipMemcpyDeviceToDevice, pc->ctx->stream));
    }
    return NPG_OK;
}

int npg::precond_apply_raw(npg_precond *pc, const double *r, double *z) {
    ++pc->applications;
    return pc->kind == NPG_PC_DENSE ? apply_dense(pc, r, z) : pc->kind == NPG_PC_MG ? apply_mg(pc, r, z) : apply_blockdiag(pc, r, z);
}

NPG_API int npg_precond_apply(npg_precond *pc, const npg_vec *r, npg_vec *z) {
    NPG_REQUIRE(pc && r && z, "npg_precond_apply: NULL argument");
    NPG_REQUIRE(pc->kind != NPG_PC_MG || pc->L.back().A, "npg_precond_apply: multigrid levels are not all set");
    NPG_REQUIRE(pc->kind != NPG_PC_DENSE || pc->dense.ready(),"npg_precond_apply: the dense inverse has not been set");
    NPG_REQUIRE(r->n == pc->n && z->n == pc->n && r->d != z->d, "npg_precond_apply: vectors must have %lld entries and not alias",
                (long long)pc->n);
    return precond_apply_raw(pc, r->d, z->d);
}

NPG_API int npg_precond_cycle_bytes(npg_precond *pc, int64_t *bytes) {
    NPG_REQUIRE(pc && bytes, "npg_precond_cycle_bytes: NULL argument");
    *bytes = pc->cycle_bytes;
    return NPG_OK;
}

NPG_API int npg_precond_counters(npg_precond *pc, int64_t *applications, int64_t *inner_iterations) {
    NPG_REQUIRE(pc, "npg_precond_counters: NULL handle");
    if (applications) *applications = pc->applications;
    if (inner_iterations) *inner_iterations = pc->inner_iterations;
    return NPG_OK;
}

