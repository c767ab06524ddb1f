/* nupgcm_hip.h - C ABI of libnupgcm_hip.so: the MI355X (gfx950) device layer behind nuPGCM's
 * Architecture / IterativeSolverToolkit / InversionToolkit / EvolutionToolkit surface.
 *
 * Each entry point names the reference interface it replaces (file:line under /root/reference/).  The reference reaches
 * its device through Julia dispatch on CuArray / CuSparseMatrixCSR (ext/nuPGCMCUDAExt.jl:24-33) and through Krylov.jl
 * (src/iterative_solvers.jl:58); a Julia package extension binds these symbols with `ccall`, and the
 * Python package `nupgcm_amd` binds the same symbols with ctypes.
 *
 * Conventions: plain C, opaque handles, every call returns NPG_OK (0) or a negative NPG_E* code and leaves a message in
 * npg_last_error().  All indices crossing the boundary are 0-based.  All floating point is fp64; device column indices
 * are int32.  Calls enqueue on the context's HIP stream and are host-synchronous only where they return host data.
 * A context is thread-compatible, not thread-safe.
 */
#ifndef NUPGCM_HIP_H
#define NUPGCM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NPG_OK 0
#define NPG_EINVAL (-1)   /* bad argument / shape mismatch                                    */
#define NPG_EHIP (-2)     /* a HIP runtime call failed                                        */
#define NPG_ENOMEM (-3)   /* device or host allocation failed                                 */
#define NPG_ENODEV (-4)   /* no usable gfx950 device                                          */
#define NPG_ECOMM (-5)    /* RCCL failure                                                     */
#define NPG_EBLOWUP (-6)  /* blow-up guard tripped (src/model.jl:149-153)                     */

typedef struct npg_ctx npg_ctx;
typedef struct npg_vec npg_vec;
typedef struct npg_csr npg_csr;
typedef struct npg_gmres npg_gmres;
typedef struct npg_cg npg_cg;
typedef struct npg_cg_multi npg_cg_multi;
typedef struct npg_fe npg_fe;
typedef struct npg_halo npg_halo;
typedef struct npg_precond npg_precond;
typedef struct npg_ilu0 npg_ilu0;
typedef struct npg_index npg_index;
typedef struct npg_fgmres npg_fgmres;
typedef struct npg_locator npg_locator;
typedef struct npg_located npg_located;
typedef struct npg_integrals npg_integrals;
typedef struct npg_classes npg_classes;
typedef struct npg_particles npg_particles;
typedef struct npg_tracers npg_tracers;

/* ---- context: replaces the implicit CUDA.jl device/stream (ext/nuPGCMCUDAExt.jl:8-16) ------------------------- */
int npg_ctx_create(int device, npg_ctx **out);
int npg_ctx_destroy(npg_ctx *ctx);
const char *npg_last_error(void);
int npg_ctx_sync(npg_ctx *ctx);
/* print_memory_status(::GPU)  (src/architectures.jl:20, ext/nuPGCMCUDAExt.jl:33) */
int npg_mem_status(npg_ctx *ctx, size_t *free_bytes, size_t *total_bytes);
int npg_device_name(npg_ctx *ctx, char *buf, size_t cap);
/* the hipStream_t all work is enqueued on (so a caller can bracket it with HIP events) */
void *npg_ctx_stream(npg_ctx *ctx);
/* HIP-event timer on the context's stream: start ... stop -> elapsed milliseconds (host-synchronous at stop) */
int npg_timer_start(npg_ctx *ctx);
int npg_timer_stop(npg_ctx *ctx, double *ms);

/* ---- dense vectors: on_architecture(::GPU, ::Array) / (::CPU, ::CuArray), vector_type(::GPU, T)
 *      (ext/nuPGCMCUDAExt.jl:24-26,31) and the BLAS-1 / broadcast calls of SURVEY.md section 2a ------------------ */
int npg_vec_create(npg_ctx *ctx, int64_t n, npg_vec **out);              /* zero-filled */
int npg_vec_destroy(npg_vec *v);
/* non-owning window [offset, offset+n) of v (e.g. the velocity part x[1:nu] of [u; p], src/model.jl:314); the parent must
 * outlive the view */
int npg_vec_view(npg_vec *v, int64_t offset, int64_t n, npg_vec **out);
int64_t npg_vec_len(const npg_vec *v);
int npg_vec_upload(npg_vec *v, const double *host);
int npg_vec_download(const npg_vec *v, double *host);
/* v[i] = host[perm[i]]   -- `rhs[perm]` then H2D   (src/model.jl:274-275, src/evolution.jl:91-106) */
int npg_vec_upload_perm(npg_vec *v, const double *host, const int64_t *perm);
/* host[i] = v[perm[i]]   -- `solver.x[inv_perm]` then D2H   (src/model.jl:282,312) */
int npg_vec_download_perm(const npg_vec *v, double *host, const int64_t *perm);
int npg_vec_fill(npg_vec *v, double a);
int npg_vec_copy(npg_vec *dst, const npg_vec *src);
int npg_vec_axpby(npg_vec *y, double a, const npg_vec *x, double b);    /* y = a x + b y */
int npg_vec_dot(const npg_vec *x, const npg_vec *y, double *out);
int npg_vec_nrm2(const npg_vec *x, double *out);
/* max |x_i| and whether any entry is NaN: the blow-up guard's reductions (src/model.jl:149-153) */
int npg_vec_maxabs(const npg_vec *x, double *out, int *has_nan);
/* *is_constant = every entry equals *value (min == max).  Lets a binding recognise `Diagonal(s * ones(n))` - the inversion
 * preconditioner of src/inversion.jl:54 - without indexing a device vector, and pass it as NPG_PRECOND_SCALAR */
int npg_vec_is_constant(const npg_vec *x, double *value, int *is_constant);
/* y = sum_k coef[k] * xs[k]   (k < nterms <= 8): the fused broadcasts at src/inversion.jl:104, src/model.jl:278 */
int npg_vec_lincomb(npg_vec *y, int nterms, const double *coef, const npg_vec *const *xs);
/* y = d .* x   -- mul!(y, ::Diagonal, x) */
int npg_vec_mul(npg_vec *y, const npg_vec *d, const npg_vec *x);

/* ---- CSR matrices: on_architecture(::GPU, ::SparseMatrixCSC) = CuSparseMatrixCSR(a) and its inverse
 *      (ext/nuPGCMCUDAExt.jl:27-29) ------------------------------------------------------------------------------- */
/* CSC (Julia SparseMatrixCSC, made 0-based by the binding) -> device CSR.  drop_zeros != 0 removes entries that are
 * exactly 0.0 (Gridap stores structural zeros; a correct SpMV need not stream them). */
int npg_csr_create_from_csc(npg_ctx *ctx, int64_t m, int64_t n, const int64_t *colptr, const int64_t *rowval,
                            const double *nzval, int drop_zeros, npg_csr **out);
int npg_csr_create(npg_ctx *ctx, int64_t m, int64_t n, const int64_t *rowptr, const int32_t *colind,
                   const double *val, npg_csr **out);
int npg_csr_destroy(npg_csr *A);
int npg_csr_shape(const npg_csr *A, int64_t *m, int64_t *n, int64_t *nnz);
/* device CSR -> host CSC arrays (caller allocates n+1 / nnz / nnz) : on_architecture(::CPU, ::CuSparseMatrixCSR) */
int npg_csr_to_csc(const npg_csr *A, int64_t *colptr, int64_t *rowval, double *nzval);
/* host CSR copy (rowptr m+1 int64, colind nnz int32, val nnz) */
int npg_csr_download(const npg_csr *A, int64_t *rowptr, int32_t *colind, double *val);
/* new matrix with the pattern of A and values copied from it */
int npg_csr_clone(const npg_csr *A, npg_csr **out);
int npg_csr_zero_values(npg_csr *A);
/* out = a*X + b*(Y + Z) on identical patterns: `A = M + theta*(Kh + Kv)` (src/evolution.jl:144,162; src/model.jl:254)
 * done on the device instead of a host SparseMatrixCSC add + re-upload */
int npg_csr_combine(npg_csr *out, double a, const npg_csr *X, double b, const npg_csr *Y, const npg_csr *Z);
/* out += a*X on identical patterns (plain CSR): the restoring term `A += dt*S` of the evolution's left-hand side */
int npg_csr_axpy(npg_csr *out, double a, const npg_csr *X);
/* Store the velocity block of A_inversion node by node.  With constant viscosity node q couples to node c through one
 * friction number K (the x-x, y-y and z-z entries) and one Coriolis number C (x-y entry, -C for y-x)
 * (src/inversion.jl:183-192).  The ordering of nupgcm_amd.fe puts first the n_full nodes with all three components free
 * (rows 3q..3q+2), then the n_surf nodes with free x and y only (w = 0 at the surface; rows 3 n_full + 2 (q - n_full) + {0,1}).
 * Five (four) 12-byte CSR entries and five (four) 8-byte gathers become one 20-byte record {c, K, C} and one gather of the
 * node's contiguous components.  The structure is verified entry by entry (relative tolerance rtol); *blocked = 0 and the
 * matrix is untouched if it does not hold (e.g. function-valued nu).  A node-blocked matrix can be multiplied and solved
 * with, but not downloaded, cloned or re-assembled.
 * Failure paths: whenever the call does not end with *blocked = 1 the handle is the plain matrix it was, bit for bit (it
 * still downloads, clones and multiplies).  That covers (a) a structure that does not hold, (b) a record form that does not
 * fit - the rows of one node exceed an SpMV tile (about 1 900 neighbours of a three-component node): *blocked = 0, NPG_OK,
 * and npg_last_error() names the limit - and (c) an error on the way (out of memory), which is returned.  A matrix that fits
 * the ordinary tiles but not a windowed one - a node beyond a window's caps, or a tile of nodes without any entry in the block
 * columns - is node-blocked without a windowed tile set (npg_csr_window_info: 0 tiles). */
int npg_csr_block_nodes(npg_csr *A, int64_t n_full, int64_t n_surf, double rtol, int *blocked);
/* (round 5; multi-GPU) Ghost NODES of a rank's row block - the matrix's columns [m, n) are the rank's ghosts: node g's (x, y[, z])
 * components are the ghost columns [first_col[g], first_col[g] + ncomp[g]), ncomp = 3 or 2.  Call before npg_csr_block_nodes:
 * the windowed tile set then stores the coupling of an owned node to a ghost node as ONE {c, K, C} node record instead of three
 * column records (a rank's boundary tiles keep their size), the gather-layout copy of the Krylov vector gives
 * ghost nodes 4-float slots behind the owned nodes' and the halo unpack fills them. */
int npg_csr_set_ghost_nodes(npg_csr *A, int64_t n_nodes, const int32_t *first_col, const int32_t *ncomp);
/* The same for a matrix in ANY DoF order - the reference's own RCM of the velocity mass-matrix graph comes out component by
 * component (src/dofs.jl:27-41,70-100), not node by node.  node_of_dof[i] >= 0: DoF i is component comp_of_dof[i] (0, 1, 2) of
 * the velocity node with that label (any non-negative labels: Gridap's node ids); < 0: not a velocity DoF.  The library
 * renumbers internally ([x, y, z of every node with three free components | x, y of every node with those two | other velocity
 * DoFs | the rest], nodes in the order of their first DoF in the caller's numbering), permutes the matrix, blocks it as
 * npg_csr_block_nodes does (windowed tile set included) and KEEPS THE PERMUTATION IN THE HANDLE: npg_spmv and npg_gmres_solve
 * go on taking and returning vectors in the caller's order (right-hand side, warm start / solution and a vector preconditioner
 * are gathered / scattered on the device, four vector passes per solve), so npg_vec_upload_perm / npg_vec_download_perm with
 * the caller's own permutations stay what they were.  Other solvers refuse such a matrix.  *blocked = 0 and the matrix
 * untouched, in the caller's order, on every failure path of npg_csr_block_nodes. */
int npg_csr_block_nodes_dofs(npg_csr *A, const int64_t *node_of_dof, const int32_t *comp_of_dof, double rtol, int *blocked);
/* the two-component special case: npg_csr_block_nodes(A, 0, npairs, ...) */
int npg_csr_pair_xy(npg_csr *A, int64_t npairs, double rtol, int *paired);
/* how the matrix is laid out in HBM: number of block nodes, {c, K, C} records (20 bytes each, standing for 4 or 5 CSR
 * entries) and plain CSR entries (12 bytes each).  Plain matrix: 0, 0, nnz. */
int npg_csr_storage(const npg_csr *A, int64_t *nodes, int64_t *records, int64_t *csr_entries);
/* npg_csr_block_nodes also packs (a) what the rows BEHIND the block rows (the divergence rows of A_inversion, the last block row
 * of src/inversion.jl:183-192) hold in the block columns: one 28-byte record {c, d_x, d_y, d_z} per (row, column node) in
 * place of three (two) CSR entries (NPG_SPMV_COUPLING=0 keeps them as CSR entries); (b) what the block rows hold OUTSIDE the
 * block columns (the gradient entries, a rank's ghost columns): one 28-byte record {m, a_x, a_y, a_z} per (node, column) - the
 * coefficients of column m in the node's x, y, z rows - whenever that is fewer bytes than the entries (NPG_SPMV_COLUMN_RECORDS=0:
 * never).  *records = how many 28-byte records of both kinds (0: none). */
int npg_csr_coupling_records(const npg_csr *A, int64_t *records);
/* Record form for a matrix whose velocity block has NO {K, C} structure - function-valued viscosity, where the full-stress form
 * (src/inversion.jl:172-181) couples all nine component pairs of a node pair, and the eddy closure re-assembles the values
 * (src/model.jl:160-170).  The plain matrix A stays what it is (assembly target, download, clone ...); a companion in record form
 * is attached to it: FULL node records {c, a_00 .. a_22} (76 bytes and one gather of node c's components for nine entries of
 * 12 bytes and nine gathers), coupling records and column records as npg_csr_block_nodes builds them.  The companion knows where
 * in A's value array each of its values comes from and follows every change of A on the device (npg_fe_assemble_matrix,
 * npg_csr_combine, npg_csr_gather_values, npg_csr_zero_values); npg_spmv, npg_gmres_solve and the preconditioners read it.
 * *packed = 0 and nothing attached if the rows of some node would not fit an SpMV tile. */
int npg_csr_pack_nodes(npg_csr *A, int64_t n_full, int64_t n_surf, int *packed);
/* bytes of the matrix arrays one SpMV streams from HBM in the form the kernels read (records and their offset arrays, remaining
 * CSR entries, row offsets): plain CSR 12 nnz + 8 (m + 1); record forms as laid out by npg_csr_block_nodes / npg_csr_pack_nodes */
int npg_csr_spmv_bytes(const npg_csr *A, int64_t *matrix_bytes);
/* npg_csr_block_nodes also builds (NPG_SPMV_WINDOW=0: not) a WINDOWED tile set of the block rows for the Krylov kernels that
 * gather their SpMV input from its fp32 gather-layout copy (npg_gmres_set_gather): every tile lists its distinct column nodes
 * and distinct other columns, gathers each of them ONCE into an LDS window, and the node / column records address the window by
 * 16-bit indices; a node's record list is padded to an even count with a zero record so that two adjacent records of one row
 * node are summed before they reach LDS (csrc/spmv_window.h).  *tiles = tiles in that set (0: none), *block_tiles = how many of
 * them are windowed block tiles, *distinct = entries of both window lists (= gathers of the input one product issues in the
 * block rows), *matrix_bytes = what one product streams from HBM in that form (records with 2-byte indices, window lists,
 * offsets, descriptors, and the coupling records / CSR entries of the rows behind the block rows). */
int npg_csr_window_info(const npg_csr *A, int64_t *tiles, int64_t *block_tiles, int64_t *distinct, int64_t *matrix_bytes);
/* lanes per row in the tiled SpMV's segmented sums (4, 8, 16 or 32; 0 returns to the rule of thumb from the mean row length that
 * every matrix starts with).  A tuning knob: results change only in the order of a row's partial sums. */
int npg_csr_set_lanes(npg_csr *A, int lanes);
/* y = A fl32(x): the product of the Krylov kernels' gather-layout instance as a call of its own - x is copied, rounded to fp32,
 * into the gather layout (a node's components padded to 16 bytes) and multiplied in fp64 (synchronous).  windowed != 0: on the
 * windowed tile set (an error without one), 0: on the ordinary tiles.  reps > 1 repeats the product (timing).  Only for matrices
 * stored by {c, K, C} node blocks (npg_csr_block_nodes). */
int npg_spmv_gather32(const npg_csr *A, const npg_vec *x, npg_vec *y, int windowed, int reps);
/* dst.val[k] = src.val[map[k]]: a matrix whose entries are a fixed subset / rearrangement of another's - a rank's row block
 * of a replicated, re-assembled matrix (closure refreshes of K_v and A, src/model.jl:160-170,229-261, when the solve is
 * distributed).  npg_index = a device-resident int64 index array, every entry checked against `bound` at creation. */
int npg_index_create(npg_ctx *ctx, int64_t n, const int64_t *host, int64_t bound, npg_index **out);
int npg_index_destroy(npg_index *ix);
int npg_csr_gather_values(npg_csr *dst, const npg_csr *src, const npg_index *map);
/* Device-side pieces of the multigrid set-up / refresh (csrc/mg.hip), all on FIXED patterns supplied by the host:
 * Dinv <- inverse of the node-block diagonal of A[0:nu, 0:nu] (3 x 3 blocks for the first n_full nodes, 2 x 2 for the next
 * n_surf, 1 x 1 for the rest; Dinv's pattern holds exactly these blocks), and S <- D Dinv G (products outside S's pattern
 * are an error).  With npg_csr_gather_values for G = A[u, p] and D = A[p, u] a re-assembled A (eddy closure) refreshes a
 * level's smoother without leaving the device. */
int npg_csr_node_block_inverse(npg_csr *Dinv, const npg_csr *A, int64_t n_full, int64_t n_surf);
/* Dinv = inverse of a block diagonal of A[0:nu, 0:nu] with arbitrary blocks: block b = block_dofs[block_ptr[b] .. block_ptr[b+1])
 * (ascending; the blocks partition [0, nu); at most 136 unknowns each), Dinv's pattern = exactly the blocks.  The z-line smoother
 * of the multigrid cycle: a block = the velocity unknowns of the nodes above one another (new work, csrc/mg.hip). */
int npg_csr_line_block_inverse(npg_csr *Dinv, const npg_csr *A, const npg_index *block_ptr, const npg_index *block_dofs);
/* S = D Dinv G for a line-block Dinv (npg_csr_line_block_inverse) without the generic triple product's n_line-fold work: per
 * line l the dense W_l = B_l G[l, :] over the line's distinct pressure columns wcols[wptr[l] .. wptr[l+1]) (ascending), stored at
 * woff[l] (n_l x m_l, row-major; woff's bound = total + 1); then row p of S sums D[p, l] W_l over the lines it touches.  dperm:
 * D's entry positions sorted by (row, line, column); dpos: the position of each such entry's column inside its line; segment s =
 * entries [seg_start[s], seg_start[s+1]) of that order = one (row, line) pair, line seg_line[s]; row p owns segments
 * [seg_ptr[p], seg_ptr[p+1]).  All index arrays are the caller's (host logic on patterns: nupgcm_amd/multigrid.py). */
int npg_csr_line_schur(npg_csr *S, const npg_csr *D, const npg_csr *Dinv, const npg_csr *G, const npg_index *wptr,
                       const npg_index *wcols, const npg_index *woff, const npg_index *dperm, const npg_index *dpos,
                       const npg_index *seg_ptr, const npg_index *seg_line, const npg_index *seg_start);
/* the stored values of a plain-CSR matrix into the head of a vector, and values[k] = v[map[k]] back: with an ordinary halo plan on
 * such a vector, matrix VALUES travel between ranks (distributed multigrid: the rows of Dinv G that belong to a neighbour's ghost
 * unknowns are refreshed without leaving the device) */
int npg_csr_values_to_vec(const npg_csr *A, npg_vec *v);
int npg_csr_values_from_vec(npg_csr *A, const npg_vec *v, const npg_index *map);
/* C = A B on C's FIXED pattern (plain CSR; an error if a product falls outside it) */
int npg_csr_product(npg_csr *C, const npg_csr *A, const npg_csr *B);
int npg_csr_triple_product(npg_csr *S, const npg_csr *D, const npg_csr *Dinv, const npg_csr *G);
/* d[i] = 1 / A[i,i]   -- `Diagonal(1 ./ diag(A))` (src/evolution.jl:149,167; src/model.jl:256) */
int npg_csr_inv_diag(const npg_csr *A, npg_vec *d);
/* y = alpha * A x + beta * y   -- mul!(y, A, x) / A*x  (cuSPARSE SpMV in the reference) */
int npg_spmv(const npg_csr *A, const npg_vec *x, npg_vec *y, double alpha, double beta);

/* ---- Krylov solvers: Krylov.krylov_solve!(workspace, A, y, x; M=P, kwargs...) (src/iterative_solvers.jl:58) ---- */
#define NPG_PRECOND_NONE 0
#define NPG_PRECOND_SCALAR 1   /* P = Diagonal(s * ones(n))   (src/inversion.jl:54)          */
#define NPG_PRECOND_DIAG 2     /* P = Diagonal(d)             (src/evolution.jl:149,167)     */

typedef struct npg_solve_stats {
    int32_t solved;       /* workspace.stats.solved                                             */
    int32_t niter;        /* workspace.stats.niter (cumulative inner iterations)                */
    int32_t npass;        /* GMRES restart cycles started                                       */
    int32_t status;       /* 1 solved, 2 itmax reached, 3 breakdown, 4 zero residual at start.  CG: 3 = the start's r'z is NaN or
                             Inf (0 iterations), or p'Ap is not positive (zero, negative, NaN): that step is not taken, and x, niter,
                             rnorm and the history are those of the last completed iteration; or r'z turned NaN  */
    int32_t nreorth;      /* GMRES: second Gram-Schmidt passes taken                            */
    int32_t nflagged;   /* GMRES: Arnoldi steps flagged by the device - a Pythagorean norm that lost > 4 digits (distributed), or a
                         * column that was due a second Gram-Schmidt pass while the fast kernels ran (the next solves use the
                         * full kernels); 0 for CG */
    double rnorm0;        /* || M r0 ||                                                         */
    double rnorm;         /* last residual estimate                                             */
    double seconds;       /* host wall time of the call                                         */
} npg_solve_stats;

/* GmresWorkspace(n, n, VT; memory)  (src/inversion.jl:84) */
int npg_gmres_create(npg_ctx *ctx, int64_t n, int memory, npg_gmres **out);
int npg_gmres_destroy(npg_gmres *ws);
/* Left-preconditioned restarted GMRES(memory).  x is in/out: the incoming x is the warm start (x aliases workspace.x in
 * the reference, src/iterative_solvers.jl:26-29).  itmax == 0 means 2 n.  Orthogonalisation is classical Gram-Schmidt
 * with a selective second pass (reorth_eta: take it when ||w'|| < eta ||w||; eta <= 0 never, eta >= 1 always) instead
 * of Krylov.jl's sequential modified Gram-Schmidt: one reduction per pass instead of j. */
int npg_gmres_solve(npg_gmres *ws, const npg_csr *A, int precond_kind, double precond_scalar,
                    const npg_vec *precond_diag, const npg_vec *y, npg_vec *x, double atol, double rtol,
                    int64_t itmax, double reorth_eta, npg_solve_stats *stats);
/* Profile mode: the next solves launch eagerly (no hipGraph) with HIP events on the context's stream around every
 * Arnoldi kernel - the fused SpMV + Gram-Schmidt-dots kernel that dominates the solve - and accumulate their durations
 * over complete restart cycles.  npg_gmres_get_profile returns the accumulated milliseconds and launch count. */
int npg_gmres_set_profile(npg_gmres *ws, int on);
/* kernel organisation of the Arnoldi step: 0 = fused (SpMV + Gram-Schmidt dots in one kernel, group-interleaved basis:
 * latency-bound sizes), 1 = split (SpMV kernel + row-streaming dots/orthogonalisation kernels, column-major basis:
 * bandwidth-bound sizes), -1 = by size (split from 8192 rows; default).  Same arithmetic either way. */
/* Stored Krylov basis of the split kernel organisation (n >= 8192): 64 = fp64, 32 = fp32 ("compressed basis": only the
 * stored copy used by the Gram-Schmidt sums and x += V y is rounded; sums, products and the restart residual stay fp64, and so
 * does the SpMV input unless its fp32 gather-layout copy is in use - npg_gmres_set_gather below, the default wherever it applies),
 * 0 = by tolerance (fp32 when rtol >= 1e-7, the reference's 1e-6 included).  NPG_GMRES_BASIS=32|64 overrides the default. */
int npg_gmres_set_basis(npg_gmres *ws, int bits);
/* Where the basis is stored in fp32 (above), with a node-blocked matrix, the Arnoldi kernel gathers its SpMV input
 * from an fp32 copy of the Krylov vector laid out for gathering - a node's components padded to 16 bytes: one gather per node
 * record instead of two (the kernel is bound by its gather instructions).  The copy carries the rounding the
 * stored basis column has anyway; products and sums stay fp64.  mode: -1 = default (on where it applies; NPG_GMRES_XG=0 turns
 * the default off), 0 = off, 1 = on where it applies, 2 = on, but on the matrix's ordinary tiles even when it has a windowed
 * tile set (npg_csr_window_info; NPG_GMRES_WINDOW=0 makes that the default). */
int npg_gmres_set_gather(npg_gmres *ws, int mode);
int npg_gmres_set_split(npg_gmres *ws, int mode);
int npg_gmres_get_profile(npg_gmres *ws, double *ms_total, int64_t *launches);
/* residual history of the last solve (workspace.stats.residuals with history=true): returns entries written */
int64_t npg_gmres_history(npg_gmres *ws, double *buf, int64_t cap);
/* The kernel instances the last solve launched, as up to n int32 entries in this order: split organisation, stored basis bits
 * (64 / 32), fast orthogonalisation kernels, SpMV input from the fp32 gather copy (0 = off, 1 = node records, 2 = plain CSR),
 * windowed tile set, lanes per node of the windowed segmented sums, windowed set with ordinary tiles, lanes per row of the
 * tiled SpMV, full node records, distributed (halo attached), Pythagorean norm, tiles of the Arnoldi launch, workgroups of the
 * Arnoldi launch, workgroups of the row / orthogonalisation kernels, rows, memory, lazy second-pass sums.  Returns the number of
 * entries written (0 before the first solve and after a solve that failed). */
int npg_gmres_last_config(const npg_gmres *ws, int32_t *cfg, int n);
/* The widest step, in basis columns, that the last solve's plan gave to the resident fused row launch: 20 (every instance), 16
 * (NPG_GMRES_FUSED_COLS=16, or a row grid admitted for the one-pass instances only) or 0 (the separate launches; no solve yet). */
int npg_gmres_fused_cols(const npg_gmres *ws);

/* CgWorkspace(n, n, VT)  (src/evolution.jl:120) */
int npg_cg_create(npg_ctx *ctx, int64_t n, npg_cg **out);
int npg_cg_destroy(npg_cg *ws);
int npg_cg_solve(npg_cg *ws, const npg_csr *A, int precond_kind, double precond_scalar, const npg_vec *precond_diag,
                 const npg_vec *y, npg_vec *x, double atol, double rtol, int64_t itmax, npg_solve_stats *stats);
int64_t npg_cg_history(npg_cg *ws, double *buf, int64_t cap);

/* CG for several right-hand sides against one matrix: every column has the bits of npg_cg_solve on that column;
 * the matrix is streamed once per iteration for up to eight columns.  y, x: stacked vectors of ncol * n (column k at k * n); x is
 * the warm start and the result.  stats: ncol entries (may be NULL); `seconds` is the whole call's, in every entry.  A: plain CSR
 * (no node blocks, records or internal renumbering).  Single device: there is no halo variant. */
#define NPG_CG_MULTI_MAX 32
int npg_cg_multi_create(npg_ctx *ctx, int64_t n, int ncol_max, npg_cg_multi **out);
int npg_cg_multi_destroy(npg_cg_multi *ws);
int npg_cg_multi_solve(npg_cg_multi *ws, const npg_csr *A, int precond_kind, double precond_scalar, const npg_vec *precond_diag,
                       int ncol, const npg_vec *y, npg_vec *x, double atol, double rtol, int64_t itmax, npg_solve_stats *stats);
/* residual history of column `col` of the last solve: returns entries written */
int64_t npg_cg_multi_history(npg_cg_multi *ws, int col, double *buf, int64_t cap);

/* ---- general preconditioners + flexible GMRES: src/preconditioners.jl:1-125 and SURVEY 8f rank 1 --------------------------
 * `P` of the IterativeSolverToolkit is a tagged union: NPG_PRECOND_NONE / _SCALAR / _DIAG are linear diagonal actions that
 * npg_gmres_solve / npg_cg_solve fold into their SpMV epilogue; an npg_precond is an INEXACT operator application
 * (inner iterations), which only a flexible Krylov method may use - iterative_solve! hands such a P to npg_fgmres_solve. */
#define NPG_PC_BLOCKDIAG 1   /* BlockDiagonalPreconditioner([Block(CgPreconditioner(A_k, Diagonal), indices_k)...])
                                (src/preconditioners.jl:53-125): nparts blocks                                        */
#define NPG_PC_MG 2          /* geometric multigrid V-cycle on the saddle-point system (new work): nparts levels      */
#define NPG_PC_DENSE 3       /* explicit dense inverse in HBM (new work; small systems, <= 46 340 unknowns: rocSOLVER indexes n x n with 32 bits): nparts = 1 */
int npg_precond_create(npg_ctx *ctx, int kind, int nparts, npg_precond **out);
int npg_precond_destroy(npg_precond *pc);
/* Block k acts on x[offset, offset + n_k): CG on A_k with M = Diagonal(jacobi) (ldiv = false), itmax / atol / rtol as given
 * (itmax 0 = 2 n_k), warm-started from the block's previous output - CgPreconditioner, src/preconditioners.jl:5-37.  The
 * matrices and vectors are borrowed and must outlive the preconditioner. */
int npg_precond_blockdiag_set(npg_precond *pc, int k, int64_t offset, const npg_csr *A_k, const npg_vec *jacobi,
                              int64_t itmax, double atol, double rtol);
/* ILU(0) of a plain-CSR square matrix with a full diagonal and ascending columns - KrylovPreconditioners.kp_ilu0(P) of the
 * reference's GPU P-block (src/preconditioners.jl:101-107; csrilu02 + two csrsv2 there): level-scheduled IKJ factorisation in
 * A's pattern and level-scheduled triangular solves, csrc/ilu.hip.  The handle keeps its own copy of the pattern. */
int npg_ilu0_create(npg_ctx *ctx, const npg_csr *A, npg_ilu0 **out);
int npg_ilu0_destroy(npg_ilu0 *M);
int npg_ilu0_refactor(npg_ilu0 *M, const npg_csr *A);                 /* A's values changed, same pattern */
int npg_ilu0_apply(npg_ilu0 *M, const npg_vec *r, npg_vec *z);        /* z = U^-1 L^-1 r  (ldiv!) */
int npg_ilu0_info(const npg_ilu0 *M, int64_t *levels_lower, int64_t *levels_upper, int64_t *nnz);
int npg_ilu0_factors(const npg_ilu0 *M, double *host_values);         /* L (strictly lower, unit diagonal implied) and U, A's pattern */
/* CG on A x = b with M = the factors, ldiv = true, warm start x: what the reference's CgPreconditioner runs for the P-block
 * (src/preconditioners.jl:24-37; Krylov.jl cg: gamma = r'z, stop at sqrt(gamma) <= atol + rtol sqrt(gamma_0); itmax 0 = 2 n) */
int npg_cg_ilu0_solve(npg_ilu0 *M, const npg_csr *A, const npg_vec *b, npg_vec *x, double atol, double rtol, int64_t itmax,
                      npg_solve_stats *stats);
/* block k of a block-diagonal preconditioner (already set with npg_precond_blockdiag_set) runs its CG with M = these factors
 * instead of the Jacobi vector (NULL: back to Jacobi).  Borrowed. */
int npg_precond_blockdiag_set_ilu0(npg_precond *pc, int k, npg_ilu0 *M);
/* Multigrid level `level` (0 = coarsest; set them coarse to fine).  A = the level's saddle-point matrix ordered [u; p]
 * with nu velocity unknowns, G = A[0:nu, nu:], D = A[nu:, 0:nu], Dinv = inverse of the node-block diagonal of A[0:nu, 0:nu]
 * (a node's components are adjacent; <= 3 entries per row), S = D Dinv G.  P (n_level x n_{level-1}) interpolates from the
 * next coarser level, R = P' restricts; both NULL at level 0.  All handles are borrowed. */
int npg_precond_mg_set_level(npg_precond *pc, int level, const npg_csr *A, int64_t nu, const npg_csr *G, const npg_csr *D,
                             const npg_csr *Dinv, const npg_csr *S, const npg_csr *P, const npg_csr *R);
/* replace the operators of a level by re-assembled ones of the same shapes (the eddy closure's refresh of A,
 * src/model.jl:160-170); the previous handles are no longer referenced afterwards */
/* Gh = Dinv G (same shape as G; borrowed, values kept current by the caller: npg_csr_product after every change of Dinv / G).
 * With it a smoothing step applies Dinv once instead of twice: x_u += Dinv (r_u - G dp) / w is formed as t / w (in the kernel that
 * forms t = Dinv r_u) minus (Dinv G) dp / w.  NULL returns to the two-product form. */
int npg_precond_mg_set_scaled_gradient(npg_precond *pc, int level, const npg_csr *Gh);
int npg_precond_mg_update_level(npg_precond *pc, int level, const npg_csr *A, const npg_csr *G, const npg_csr *D,
                                const npg_csr *Dinv, const npg_csr *S);
/* omega: scaling of the node-block diagonal in the Braess-Sarazin smoother (> largest eigenvalue of Dinv F; default 2.5),
 * jacobi_weight / schur_sweeps: damped-Jacobi relaxation of the pressure system (0.7, 3), nu1 / nu2: pre- / post-smoothing
 * steps (2, 2), coarse_sweeps: smoothing steps that stand in for the coarsest-level solve (20). */
int npg_precond_mg_set_params(npg_precond *pc, double omega, double jacobi_weight, int schur_sweeps, int nu1, int nu2,
                              int coarse_sweeps);
/* gamma = 1: V-cycle (default); gamma = 2: W-cycle - every level's coarse problem is visited twice, which keeps the
 * convergence independent of the number of levels where the V-cycle's degrades (4 levels: DESIGN.md section 4.5) */
int npg_precond_mg_set_cycle(npg_precond *pc, int gamma);
/* Mixed precision inside the cycle: its SpMVs read fp32 copies of the level operators' values (8 instead of 12 bytes per
 * CSR entry, 12 instead of 20 per node record); vectors, products, sums and the outer flexible GMRES (with its own fp64
 * SpMV) stay fp64.  npg_precond_mg_update_level rebuilds the copies. */
int npg_precond_mg_set_mixed(npg_precond *pc, int on);
/* NPG_PC_DENSE: A^-1 as n^2 doubles in HBM (2 GB at 16 k unknowns, 8 GB at 31 k: what 288 GB buy) - densified, factorised
 * and inverted once by rocSOLVER (getrf + getrs against the identity, set-up), applied per solve by a hand-written split-column GEMV at HBM speed.
 * For the reference's small meshes, where the scalar-preconditioned GMRES is bound by kernel latency (19 us x 600 iterations),
 * this is the device counterpart of its CPU() path's `lu(A)` + `ldiv!` (src/inversion.jl:55-58, src/iterative_solvers.jl:42-47);
 * behind flexible GMRES it needs 1-2 iterations.  A must be plain CSR.  Call again to follow a re-assembled A. */
int npg_precond_dense_set(npg_precond *pc, const npg_csr *A, int fp32_storage);
/* fp32_storage != 0 keeps the inverse rounded to fp32 (half the bytes per application; products still accumulate in fp64):
 * one application then carries ~1e-7 relative error and flexible GMRES takes 2-3 iterations at tight tolerances.
 * multigrid: solve the coarsest level with its dense inverse instead of smoothing steps; on = 1: fp64 storage, on = 2: fp32
 * (a coarse-grid correction inside a preconditioner does not need more), on = 3: fp16 storage, every column divided by its
 * largest magnitude (a quarter of the bytes; products and chunk sums in fp32), on = 0: back to smoothing steps */
int npg_precond_mg_set_coarse_dense(npg_precond *pc, int on);
/* z = M^-1 r (one application: one V-cycle / one round of inner CG solves) */
int npg_precond_apply(npg_precond *pc, const npg_vec *r, npg_vec *z);
int npg_precond_counters(npg_precond *pc, int64_t *applications, int64_t *inner_iterations);
/* Bytes ONE application of the preconditioner streams as its operators are laid out in HBM (multigrid: every product of the
 * V-cycle with the matrix in the form its kernel reads - records, windowed tiles, fp32 / fp16 value copies - plus its vectors;
 * dense inverse: n^2 values in their storage type).  Counted on the host when the cycle is first enqueued (0 before that); the
 * numerator of the multigrid roofline in bench.py.  Distributed levels are not counted (0). */
int npg_precond_cycle_bytes(npg_precond *pc, int64_t *bytes);

/* Right-preconditioned flexible GMRES(memory), restarted.  x in/out (warm start, as npg_gmres_solve).  pc may be NULL.
 * Stopping rule of the reference with its Diagonal(scale) preconditioner made explicit: scale ||y - A x|| <= atol + rtol
 * scale ||y - A x0||  (src/inversion.jl:42-54,76; Krylov.jl gmres!).  stats->rnorm0 / rnorm are scaled residual norms; the
 * returned rnorm is the TRUE residual recomputed after the last pass.  itmax == 0 means 2 n. */
int npg_fgmres_create(npg_ctx *ctx, int64_t n, int memory, npg_fgmres **out);
int npg_fgmres_destroy(npg_fgmres *ws);
/* Distributed flexible GMRES: A = this rank's rows (columns [owned | ghosts]), x = [owned | ghosts]; SpMV inputs get their
 * ghosts through `h`, reductions are summed over the ranks.  With npg_precond_mg_set_level_dist: the multigrid whose finest
 * level is row-partitioned like the system and whose coarser levels are replicated (one coarse-vector all-reduce per cycle). */
int npg_fgmres_set_halo(npg_fgmres *ws, npg_halo *h);
int npg_precond_mg_set_level_dist(npg_precond *pc, int level, const npg_csr *A, int64_t nu_owned, const npg_csr *G,
                                  const npg_csr *D, const npg_csr *Dinv, const npg_csr *S, const npg_csr *P, const npg_csr *R,
                                  npg_halo *hx, npg_halo *hu, npg_halo *hp);
/* Two distributed levels: the level below a distributed level may be distributed as well (the finest one or two levels of a
 * hierarchy).  Set the coarser one first - npg_precond_mg_set_level_dist with its transfers to the replicated level below it -,
 * then the finer one with P = R = NULL, then the transfers between the two: P = this rank's rows of the prolongation over the
 * coarser level's [owned | ghosts of hP] columns, R = the coarser level's owned rows of the restriction over the finer level's
 * [owned | ghosts of hR] columns; hP / hR are halo plans on the coarser iterate / the finer residual. */
int npg_precond_mg_set_transfer_dist(npg_precond *pc, int level, const npg_csr *P, const npg_csr *R, npg_halo *hP, npg_halo *hR);
int npg_fgmres_solve(npg_fgmres *ws, const npg_csr *A, npg_precond *pc, const npg_vec *y, npg_vec *x, double scale,
                     double atol, double rtol, int64_t itmax, npg_solve_stats *stats);
int64_t npg_fgmres_history(npg_fgmres *ws, double *buf, int64_t cap);

/* ---- element-local finite-element kernels: Gridap.assemble_vector / assemble_matrix call sites ------------------
 * The host supplies what Gridap holds: cell geometry, per-cell DoF tables and the quadrature / shape tables, so the
 * device uses the same rule as `Measure(Omega, 4)` (src/meshes.jl:33).  A DoF table entry >= 0 is an index into the
 * *device vector the field lives in* (i.e. already composed with the RCM permutation the solvers use,
 * src/dofs.jl:27-41); an entry < 0 is Dirichlet value number (-1 - entry) of the `diri` array. */
typedef struct npg_fe_desc {
    int64_t ncell;
    int32_t nq;               /* quadrature points per cell                                                    */
    int32_t nloc_b;           /* buoyancy nodes per cell: 10 (P2) or 4 (P1)                                    */
    const double *grad_lambda;/* [ncell][4][3] physical gradients of the barycentric coordinates              */
    const double *wdet;       /* [ncell] |det J|                                                               */
    const double *qw;         /* [nq] quadrature weights on the reference cell                                 */
    const double *N2;         /* [nq][10] P2 shape values                                                      */
    const double *dN2;        /* [nq][10][4] P2 shape derivatives w.r.t. barycentric coordinates               */
    const double *Nb;         /* [nq][nloc_b] buoyancy shape values (== N2 when nloc_b == 10)                  */
    const double *dNb;        /* [nq][nloc_b][4]                                                               */
    const double *N1;         /* [nq][4] P1 shape values (pressure)                                            */
    const int32_t *cell_u;    /* [ncell][10][3] velocity DoF table (into the inversion solution vector)        */
    const int32_t *cell_p;    /* [ncell][4] pressure DoF table (into the inversion solution vector)            */
    const int32_t *cell_b;    /* [ncell][nloc_b] buoyancy DoF table (into the evolution solution vector)       */
    const double *u_diri;     /* Dirichlet values referenced by cell_u                                          */
    int64_t n_u_diri;
    const double *b_diri;     /* Dirichlet values referenced by cell_b                                          */
    int64_t n_b_diri;
    int64_t n_inv;            /* length of the inversion vector [u; p]                                          */
    int64_t n_b;              /* length of the buoyancy vector                                                  */
} npg_fe_desc;

int npg_fe_create(npg_ctx *ctx, const npg_fe_desc *desc, npg_fe **out);
int npg_fe_destroy(npg_fe *fe);
/* per-cell, per-quadrature-point coefficient tables [ncell][nq], pre-evaluated by the host from the user's closures
 * (nu, kappa_h, kappa_v, f): the device never runs user code.  name in {"nu","kappa_h","kappa_v","f"} */
int npg_fe_set_coeff(npg_fe *fe, const char *name, const double *values);

/* Arithmetic of the element-LOCAL work of every assembly kernel below (shape tables, geometry, nodal values, the integrand
 * at a quadrature point).  NPG_FE_FP64 (default) matches Gridap.  NPG_FE_FP32 is the mixed mode of BASELINE.json configs[4]
 * ("mixed fp32 assembly / fp64 solve"; new work - the reference assembles in Float64 only): local products in fp32, every
 * sum over quadrature points / cells, all stored matrices and vectors, and the solvers in fp64.  Entries then carry a
 * relative error of a few 1e-7 of the largest local entry. */
#define NPG_FE_FP64 0
#define NPG_FE_FP32 1
int npg_fe_set_precision(npg_fe *fe, int precision);
int npg_fe_get_precision(const npg_fe *fe);

#define NPG_BDF1 1
#define NPG_BDF2 2
/* y = assemble_vector(d -> advection_lform(d, b, b_prev, u, u_prev, ...), B_test)[perm]
 *       + theta*rhs_diff + dt*rhs_flux - (rhs_M + theta*(rhs_h + rhs_v))
 * i.e. src/model.jl:269-278 in one call, entirely on the device.  x_inv / x_inv_prev are the inversion solution vectors
 * [u; p] (current and previous step), b / b_prev the evolution solution vectors.  Any of the five rhs_* may be NULL. */
int npg_fe_evolution_rhs(npg_fe *fe, int scheme, double dt, double N2, double theta, const npg_vec *b,
                         const npg_vec *b_prev, const npg_vec *x_inv, const npg_vec *x_inv_prev,
                         const npg_vec *rhs_diff, const npg_vec *rhs_flux, const npg_vec *rhs_M, const npg_vec *rhs_h,
                         const npg_vec *rhs_v, npg_vec *y);
/* advection part alone (for parity tests of src/model.jl:292-300) */
int npg_fe_advection_rhs(npg_fe *fe, int scheme, double dt, double N2, const npg_vec *b, const npg_vec *b_prev,
                         const npg_vec *x_inv, const npg_vec *x_inv_prev, npg_vec *out);
/* The tangent of the advection load:
 * out_i = int ( u_base . grad db + du . grad b_base + du_z N2 ) phi_i over the free buoyancy DoFs.  b_base / x_base are read
 * through the engine's Dirichlet tables (as npg_fe_advection_rhs reads b / x_inv); db / dx are perturbations: a negative
 * table entry reads 0.  Always fp64, whatever npg_fe_set_precision says. */
int npg_fe_tangent_rhs(npg_fe *fe, double N2, const npg_vec *b_base, const npg_vec *x_base,
                       const npg_vec *db, const npg_vec *dx, npg_vec *out);
/* The adjoint of the tangent load: for a multiplier lam on the free buoyancy DoFs (a Dirichlet DoF reads 0)
 * out_b_j = int lam_h u_base . grad phi_j and out_x_(j,a) = int lam_h (d_a b_base + N2 delta_az) phi^u_j (pressure rows: 0), so that
 * <lam, npg_fe_tangent_rhs(db, dx)> = <out_b, db> + <out_x, dx> at the same base state.  out_b holds n_b, out_x n_inv entries;
 * neither may be an input.  Always fp64. */
int npg_fe_tangent_adjoint(npg_fe *fe, double N2, const npg_vec *b_base, const npg_vec *x_base,
                           const npg_vec *lam, npg_vec *out_b, npg_vec *out_x);
/* The derivatives of the convection and eddy closures.  With s = alpha (N2 + d_z b_base) at a quadrature point
 * (b_base through the Dirichlet table, the expression of the two closure updates below):
 *   tangent_diffusion     out_i = int kappa_eff d_z db d_z phi_i,  kappa_eff = kappa_v(s) + s kappa_v'(s),
 *                         kappa_v(s) = kappa_v0 + kappa_c (1 + tanh(-s / N2min)) / 2 over the BACKGROUND table (the one npg_fe_set_coeff
 *                         "kappa_v" last stored); kappa_c = 0 gives the product with the background K_v
 *   tangent_eddy          out_x_(i,a) = -a2e2 int nu'(s) alpha d_z db ( grad u_a . grad phi_i [+ sum_c d_a u_c d_c phi_i if full_stress] )
 *                         with u = x_base's velocity: -(dA/dnu)[dnu] x_base on the rows of NPG_MAT_A; the pressure rows are 0
 *   tangent_eddy_adjoint  out_b with <mu, tangent_eddy(db)> = <out_b, db> for a multiplier mu of n_inv entries
 * nu(s) = LogSumExp(nu_min, f^2 / sqrt(N2min^2 + s^2)) as npg_fe_update_nu_eddy forms it.  db and mu are perturbations: a Dirichlet DoF
 * reads 0.  The closure derivatives are evaluated on the fly; no coefficient table is written, and of the tables only the background
 * kappa_v and f are read.  tanh and exp are evaluated by arithmetic of the library's own, the same bits in both libraries.  An output
 * must not be an input; N2min > 0 (and smoothing > 0).  Always fp64. */
int npg_fe_tangent_diffusion(npg_fe *fe, double kappa_c, double N2min, double alpha, double N2, const npg_vec *b_base,
                             const npg_vec *db, npg_vec *out);
int npg_fe_tangent_eddy(npg_fe *fe, double a2e2, int full_stress, double N2min, double alpha, double N2, double smoothing,
                        double nu_min, const npg_vec *b_base, const npg_vec *x_base, const npg_vec *db, npg_vec *out_x);
int npg_fe_tangent_eddy_adjoint(npg_fe *fe, double a2e2, int full_stress, double N2min, double alpha, double N2, double smoothing,
                                double nu_min, const npg_vec *b_base, const npg_vec *x_base, const npg_vec *mu, npg_vec *out_b);
/* the read-back of npg_fe_set_coeff: host_out[ncell][nq] <- the table as it stands (after a closure update: the updated values) */
int npg_fe_get_coeff(npg_fe *fe, const char *name, double *host_out);

/* Matrix (re)assembly into an existing CSR pattern (values are overwritten).
 * which: */
#define NPG_MAT_M 1        /* build_M        src/evolution.jl:209-212 ; lift = rhs_M                         */
#define NPG_MAT_KH 2       /* build_Kh       src/evolution.jl:225-228 ; coefficient "kappa_h" ; lift = rhs_h */
#define NPG_MAT_KV 3       /* build_Kv       src/evolution.jl:240-246 ; coefficient "kappa_v" ; lift = rhs_v */
#define NPG_MAT_A 4        /* build_A_inversion(!) src/inversion.jl:133-192, coefficients "nu", "f"          */
#define NPG_MAT_B 5        /* build_B_inversion    src/inversion.jl:199-219 ; lift = Dirichlet part of b0    */
/* a2e2 = alpha^2 eps^2 (A), scale = 1/alpha (B); full_stress != 0 selects the sigma(u):sigma(v) form used when nu is
 * a function (src/inversion.jl:172-181).  lift (may be NULL) receives sum_j a(phi_j^D, phi_i) b_D,j, the Dirichlet
 * correction vector of build_matrix_vector (src/evolution.jl:256-260) / build_b_inversion (src/inversion.jl:241). */
int npg_fe_assemble_matrix(npg_fe *fe, int which, double scale, int full_stress, npg_csr *A, npg_vec *lift);
/* rhs_diff = -N2 int kappa_v d_z(d)   (src/evolution.jl:269-278) */
int npg_fe_assemble_rhs_diff(npg_fe *fe, double N2, npg_vec *out);
/* kappa_v <- kappa_v0 + kappa_c (1 + tanh(-alpha (N2 + d_z b) / N2min)) / 2 at every quadrature point
 * (kappa_v_convection, src/inputs.jl:87-91, called at src/model.jl:229-232) */
int npg_fe_update_kappa_convection(npg_fe *fe, const double *kappa_v0_host_or_null, double kappa_c, double N2min,
                                   double alpha, double N2, const npg_vec *b);
/* nu <- LogSumExp(nu_min, f^2 / sqrt(N2min^2 + (alpha (N2 + d_z b))^2)) (nu_eddy, src/inputs.jl:130-137) */
int npg_fe_update_nu_eddy(npg_fe *fe, double N2min, double alpha, double N2, double smoothing, double nu_min,
                          const npg_vec *b);
/* Coefficient `name` of `coarse` <- the volume-weighted average, over each coarse cell's eight children (cells 8c .. 8c+7 of the
 * uniformly refined mesh `fine` lives on), of the quadrature mean of `fine`'s table: the multigrid hierarchy's coarse levels follow
 * a closure (nu_eddy, src/inputs.jl:130-137; refreshed at src/model.jl:160-170) through the FINE level's viscosity instead of
 * re-evaluating the non-linear closure on an injected buoyancy.  No counterpart in the reference (it has no multigrid). */
int npg_fe_restrict_coeff(npg_fe *coarse, const npg_fe *fine, const char *name);
/* out[c] = quadrature mean of coefficient `name` over cell c (out: one entry per cell of the engine's mesh): what a rank of a
 * partitioned multigrid level contributes to that average - its cells' children live on other ranks too, so the sums over children
 * are formed on the host from the ranks' cell means (nupgcm_amd/partition.py). */
int npg_fe_coeff_cell_mean(const npg_fe *fe, const char *name, npg_vec *out);
/* CFL:  min_K h_K / max(max_q |u|, u_min)   (update_dt!, src/timesteppers.jl:108-119) */
int npg_fe_cfl_ratio(npg_fe *fe, const double *h_cells_host, double u_min, const npg_vec *x_inv, double *out);

/* ---- point sampling of the device-resident state: nan_eval / plot_slice / plot_profiles (src/plotting.jl:9-90) ------
 * The reference evaluates FEFunctions at points through Gridap's point search and returns NaN outside the domain
 * (src/plotting.jl:13-24); its `cache` argument (plot_slice(cache, u, b)) is the split kept here: a set of points is
 * LOCATED once (npg_locator_find -> npg_located: cell id and barycentric coordinates per point, device-resident) and
 * EVALUATED as often as the state changes (npg_fe_sample).
 * Locator: anchor = [ncell][3] host doubles, the coordinates of each cell's OWN local vertex 0 (cells across a periodic seam
 * are located where they lie); with the engine's grad_lambda, lambda_i(x) = G_i . (x - x0) (i = 1..3), lambda_0 = 1 - sum.
 * A uniform bin grid over the mesh's bounding box lists per bin the cells whose bounding box overlaps it; nbins = 0 picks
 * about one bin per cell.  A point belongs to the candidate of its bin with the largest min lambda, ties to the lowest cell
 * id, if that min lambda >= -1e-10; otherwise cell = -1 and lambda = NaN. */
int npg_locator_create(npg_fe *fe, const double *anchor, int64_t nbins, npg_locator **out);
/* The locator of ONE RANK of a partitioned mesh, from explicit cell records instead of the engine's cells: the cells the rank OWNS
 * plus their witness layer - every cell sharing a geometric vertex with an owned cell (nupgcm_amd/partition.py,
 * RankLayout.locator_cells).  geo12[ncell_loc][12] = {x0, G1, G2, G3} of each cell, engine_cell = its index in the
 * rank's npg_fe cell tables (-1: a witness cell the engine does not hold), gid = its global cell id, distinct - the tie key: the
 * election among the records is the serial one (largest min lambda, equal min lambda to the lowest GLOBAL id), owned = 1 where this
 * rank reports the cell's points.  box6 = {lo[3], hi[3]}, the bounding box of the WHOLE mesh as npg_locator_box gives it (the one
 * npg_locator_info of the one-device locator of that mesh reports); the bins cover it, those away from the rank's cells stay empty;
 * nbins = 0: one bin per record.  npg_locator_find then stores the ENGINE cell index of a point whose winner is owned, and -1 / NaN
 * both for a point outside the mesh and for one whose winner another rank owns; npg_fe_grid_integrals accumulates the owned points
 * only.  Over the ranks every point is reported exactly once; the sum over ranks (npg_comm_allreduce_long) completes the result. */
int npg_locator_create_cells(npg_ctx *ctx, const double *geo12, const int32_t *engine_cell, const int64_t *gid,
                             const uint8_t *owned, int64_t ncell_loc, const double *box6, int64_t nbins, npg_locator **out);
/* box6 = the bounding box npg_locator_create gives the mesh with grad_lambda[ncell][12] and anchor[ncell][3] (host arrays; no device) */
int npg_locator_box(const double *grad_lambda, const double *anchor, int64_t ncell, double *box6);
/* cell records held, how many of them are owned (all of them on a one-device locator), device bytes of records and bins (any may be NULL) */
int npg_locator_cells(const npg_locator *loc, int64_t *nrecords, int64_t *nowned, int64_t *bytes);
int npg_locator_destroy(npg_locator *loc);
/* dims[3] bins per axis, box[6] = {lo[3], hi[3]}, total bin entries, longest candidate list (any may be NULL) */
int npg_locator_info(const npg_locator *loc, int64_t *dims, double *box, int64_t *nentries, int64_t *max_per_bin);
/* n located points: int32 cell ids [n] and fp64 barycentric coordinates [n][4] on the device.  upload takes them from the
 * caller instead of a locator (npg_fe_sample checks every cell id against the engine's cell count before using it). */
int npg_located_create(npg_ctx *ctx, int64_t n, npg_located **out);
int npg_located_destroy(npg_located *pts);
int npg_located_upload(npg_located *pts, const int32_t *cell, const double *lambda);
int npg_located_download(const npg_located *pts, int32_t *cell, double *lambda);
/* points: [n][3] coordinates (a vector of 3 n doubles); out: created for n points */
int npg_locator_find(npg_locator *loc, const npg_vec *points, int64_t n, npg_located *out);
#define NPG_SAMPLE_U 1        /* velocity, 3 values: P2 through cell_u and the Dirichlet table; vec = [u; p]            */
#define NPG_SAMPLE_P 2        /* pressure, 1 value: P1 through cell_p, the pinned vertex reads 0; vec = [u; p]          */
#define NPG_SAMPLE_B 3        /* buoyancy perturbation b', 1 value: P2 or P1 by nloc_b; vec = the buoyancy vector       */
#define NPG_SAMPLE_GRAD_B 4   /* grad b', 3 values: shape derivatives in lambda contracted with the cell's grad_lambda  */
/* out[n][ncomp] (a vector of ncomp n doubles) = the field at the located points; NaN in every component where cell = -1
 * (or a cell id outside the engine's cells).  Shape functions in closed form from lambda, local ordering of the DoF tables. */
int npg_fe_sample(npg_fe *fe, int field, const npg_vec *vec, const npg_located *pts, npg_vec *out);
/* Merging the point samples of the ranks of a partitioned model.  buf = [n][ncomp] values (npg_fe_sample wrote them) followed by n
 * counts, ncomp = 0 .. 3.  mask: where pts holds cell = -1 the values become 0, and count = 1 where this rank reports the point, else
 * 0.  After the sum over ranks (npg_comm_allreduce_long: one rank's value plus zeros - exact) unmask turns the values of the points
 * with count 0 into NaN. */
int npg_sample_mask(const npg_located *pts, int ncomp, npg_vec *buf);
int npg_sample_unmask(int64_t n, int ncomp, npg_vec *buf);
/* The reductions of the reference's post-processing (postprocess/utils.py:81-94, streamfunctions.py:14-80,
 * stratification.py:45-62) over the tensor grid x[nx] (x) y[ny] (x) z[nz], in one pass over the device-resident state: every
 * grid point is generated, located and evaluated (as npg_locator_find / npg_fe_sample would) and added to the trapezoid of its
 * column and of its zonal line; the nx ny nz samples are never stored.  axes = [x; y; z] (nx + ny + nz doubles, each axis
 * strictly increasing, n >= 2); the trapezoid weights come from the axes (w_0 = (a_1 - a_0) / 2, w_i = (a_{i+1} - a_{i-1}) / 2).
 *   col[4][nx][ny], reduced over z: count of valid points, H = int mask dz, int u_x dz, int u_y dz
 *   zon[6][ny][nz], reduced over x: count, width = int mask dx, int u_y dx, int u_z dx, int b dx with b = N2 z + b',
 *                                   int max(d_z b, 0) dx with d_z b = N2 + d_z b'
 * x_inv = [u; p], b = the buoyancy vector.  A point outside the mesh adds 0 to every entry.  No atomics: one fixed summation
 * order per entry, the same bits on every call.  The locator keeps the working memory (ceil(nx / 16) partial zon arrays). */
int npg_fe_grid_integrals(npg_fe *fe, npg_locator *loc, const npg_vec *x_inv, const npg_vec *b, double N2, const npg_vec *axes,
                          int64_t nx, int64_t ny, int64_t nz, npg_vec *col, npg_vec *zon);

/* ---- quadrature integrals of the state over the mesh (new work: the reference logs maxima only) ------------------------------
 * The exact integrals of the finite-element fields with the engine's own rule, NPG_NINT channels (csrc/integrals_core.h):
 *    0  1 (volume; area on the embedded 2-D meshes)     1  b'               2  b'^2
 *    3  (u_x^2 + u_y^2) / 2                             4  u_z^2 / 2        5  u_z b'
 *    6  nu grad u : grad u  (0 without a nu table)      7  2 nu sigma : sigma, sigma = (grad u + grad u') / 2 (full_stress = 1; else 0)
 *    8  z b'                                            9  u . grad b'     10  u_z
 *   11  kappa_h (d_x b'^2 + d_y b'^2) + kappa_v d_z b'^2                   12  kappa_v d_z b'      13  kappa_v      14  (div u)^2
 * RAW integrals: the model's prefactors (alpha^2 eps^2, 1 / alpha, N2) are the caller's.  Always fp64 - npg_fe_set_precision does
 * not apply.  Dirichlet nodes count with their values.  No atomics, a grid that depends on the cell count alone, one summation order:
 * the same bits on every call.  The handle owns the partial sums, the z table and the mask; the engine must outlive it. */
#define NPG_NINT 15
/* cell_z[ncell][4]: z of each cell's OWN vertices (Mesh.geo_coords[Mesh.cell_geo], as the locator's anchor);
   cell_mask[ncell] or NULL: 1 = this cell counts (a rank's owned cells) */
int npg_integrals_create(npg_fe *fe, const double *cell_z, const uint8_t *cell_mask, npg_integrals **out);
int npg_integrals_destroy(npg_integrals *I);
/* out: NPG_NINT doubles on the device. x_inv = [u; p], b = buoyancy vector. */
int npg_integrals_compute(npg_integrals *I, const npg_vec *x_inv, const npg_vec *b, int full_stress, npg_vec *out);

/* ---- quadrature integrals of the state over the mesh's BOUNDARY faces (new work: the reference has no boundary diagnostics) -----
 * Where the model is forced and where it dissipates: wind work, buoyancy flux, drag, pressure against the bottom.  A face is (cell,
 * local face k = the side lambda_k = 0 of that cell, a group 0 .. ngroup - 1); the fields and their gradients are the CELL's, the
 * rule is the 9-point face rule of the project's surface load vectors (weights summing to 1/2) lifted into the cell, the measure
 * qw area2, n the outward unit normal (csrc/boundary_core.h).  NPG_NBND channels per group:
 *    0  1 (area)          1..3  n (closed boundary: 0)         4  z n_z (closed boundary: the volume)       5  u . n
 *    6  b'                7  b' u . n                          8  p                9..11  p n                12  p u . n
 *   13..15  t = nu (grad u) n, or 2 nu sigma n with full_stress = 1               16  u . t
 *   17  kappa_h (d_x b' n_x + d_y b' n_y) + kappa_v d_z b' n_z                     18  kappa_v n_z
 *   19  tau_x u_x + tau_y u_y                                  20  F               21  d_z b'                22, 23  u_x, u_y
 * RAW integrals: the model's prefactors are the caller's.  Always fp64.  Dirichlet nodes count with their values.  nu, kappa_h,
 * kappa_v (the BACKGROUND value), tau_x, tau_y, F are the caller's values at the face points, tables [9][nface] set by
 * npg_boundary_set_coeff (copied; NULL removes one; every value finite); a missing table contributes 0.  npg_boundary_set_closure adds
 * the convection closure of npg_classes_mixing to kappa_v, evaluated from the point's own d_z b' (kappa_c = 0, the default: off, tanh is
 * not evaluated).
 * face_xyz[9][nface]: the face's own three nodes, (3 node + axis) major, in the order of the face's sorted vertices;
 * face_normal[3][nface]; face_area2[nface] = twice the area; face_mask[nface] or NULL: 1 = this face counts.
 * One lane per face, the faces that count sorted by group (stably: the caller's order within a group) into rows of 256 that hold ONE
 * group each, one partial row per workgroup, one workgroup per group folds its rows: no atomics, rows that depend on the face counts
 * alone, one summation order - the same bits on every call.  out[ngroup][NPG_NBND]; faces_out (or NULL) [NPG_NBND][nface]: every
 * face's own integrals in the caller's order, zeros for a face that does not count.
 * Validation (NPG_EINVAL + message) happens before anything is launched: NULL arguments, vector lengths, face_cell out of range,
 * face_local > 3, face_group >= ngroup, ngroup outside 1 .. 8, non-finite geometry, full_stress not 0 or 1, an embedded 2-D engine.
 * nface = 0, a mask that leaves nothing or an empty group give zeros for that group.  The engine must outlive the handle. */
typedef struct npg_boundary npg_boundary;
#define NPG_NBND 24
#define NPG_BND_NU 0
#define NPG_BND_KH 1
#define NPG_BND_KV 2
#define NPG_BND_TAUX 3
#define NPG_BND_TAUY 4
#define NPG_BND_FLUX 5
int npg_boundary_create(npg_fe *fe, int64_t nface, const int32_t *face_cell, const uint8_t *face_local, const uint8_t *face_group,
                        int ngroup, const double *face_xyz, const double *face_normal, const double *face_area2,
                        const uint8_t *face_mask, npg_boundary **out);
int npg_boundary_set_coeff(npg_boundary *B, int which, const double *table);
int npg_boundary_set_closure(npg_boundary *B, double kappa_c, double N2min, double alpha, double N2c);
int npg_boundary_compute(npg_boundary *B, const npg_vec *x_inv, const npg_vec *b, int full_stress, npg_vec *out, npg_vec *faces_out);
int npg_boundary_destroy(npg_boundary *B);

/* ---- time-dependent surface forcing and a restoring buoyancy condition (new work: the reference's forcings are set-up constants) --
 * The wind part of the inversion's right-hand side and the flux vector of the evolution, recomputed on the device for the time level
 * being solved, and the surface mass matrix of a restoring condition flux = gamma (b* - b) (csrc/forcing_core.h).
 * The handle holds the forced faces (cell, local face, twice the area from the face's own nodes - as npg_boundary_create takes
 * them), keyframe tables [nkey][9][nface] per series (NPG_FRC_TAUX, _TAUY, _FLUX, _TARGET) at the nine points of the face rule of
 * npg_boundary_compute, and a static table gamma [9][nface] (>= 0).  Tables are copied; NULL removes one; every value is finite.
 *   npg_forcing_apply: the value of series c at a point is (1 - w[c]) table[key[c]] + w[c] table[key[c] + 1] (behind the last
 *   keyframe: table[0]); w[c] = 0 reads one keyframe and returns its bits.  key and w have NPG_FRC_NSERIES entries; those of a
 *   series that is not set are ignored.  Then
 *       b_inv_out[r]    = b_inv_base[r] + alpha int (tau_x | tau_y) phi_r dGamma     on the u_x | u_y rows the faces touch, else b_inv_base[r]
 *       rhs_flux_out[r] = alpha int (F + gamma b*) phi_r dGamma                      on the buoyancy rows the faces touch, else 0
 *   with the face functions of the space (P2 velocity; P2 or P1 buoyancy) and Dirichlet DoFs skipped.  Two launches, sums in one
 *   fixed order, no atomics: the same bits on every call.  nface = 0 is legal: the outputs are the base and zeros.
 *   npg_forcing_surface_matrix: S = scale int gamma phi_i phi_j dGamma on the pattern given at create (entries no face touches: 0);
 *   S is symmetric to the bits.  A position missing in the pattern is an error of create.
 * Validation (NPG_EINVAL + message) happens before anything is launched.  The engine must outlive the handle; an embedded 2-D
 * engine is refused. */
typedef struct npg_forcing npg_forcing;
#define NPG_FRC_NSERIES 4
#define NPG_FRC_TAUX 0
#define NPG_FRC_TAUY 1
#define NPG_FRC_FLUX 2
#define NPG_FRC_TARGET 3
int npg_forcing_create(npg_fe *fe, int64_t nface, const int32_t *face_cell, const uint8_t *face_local, const double *face_area2,
                       const npg_csr *pattern, npg_forcing **out);
int npg_forcing_set_series(npg_forcing *F, int which, int nkey, const double *tables);
int npg_forcing_set_gamma(npg_forcing *F, const double *table);
int npg_forcing_apply(npg_forcing *F, const int32_t *key, const double *w, double alpha, const npg_vec *b_inv_base, npg_vec *b_inv_out,
                      npg_vec *rhs_flux_out);
int npg_forcing_surface_matrix(npg_forcing *F, double scale, npg_csr *S);
int npg_forcing_info(const npg_forcing *F, int64_t *nface, int64_t *wind_slots, int64_t *flux_slots, int64_t *matrix_entries,
                     int64_t *matrix_slots);
int npg_forcing_destroy(npg_forcing *F);

/* ---- interior buoyancy forcing: a volume source and a sponge (new work: the reference forces the buoyancy at the boundary only) -------
 * The volume load of d_t b' = ... + Q(x, t) + gamma(x) (b*(x, t) - b'), recomputed on the device for the time level being solved, the
 * gamma-weighted mass matrix R of the sponge and the integrals of its budget (csrc/interior_core.h).  The handle holds
 * the nkept KEPT cells (strictly ascending cell ids of the engine), keyframe tables [nkey][nq][nkept] per series (NPG_ITR_SOURCE: Q,
 * NPG_ITR_TARGET: b*) at the points of the engine's own volume rule - the rule NPG_MAT_M is assembled with - and a static table gamma
 * [nq][nkept] (>= 0).  Tables are copied; NULL removes one; every value is finite.
 *   npg_interior_apply: the value of series c at a point is (1 - w[c]) table[key[c]] + w[c] table[key[c] + 1] (behind the last
 *   keyframe: table[0]); w[c] = 0 reads one keyframe and returns its bits.  key and w have NPG_ITR_NSERIES entries; those of a series
 *   that is not set are ignored.  Then
 *       rhs_src_out[r] = int (Q + gamma (b* - b_D)) phi_r dV     on the buoyancy rows the kept cells touch, else 0
 *   with b_D the finite-element function of the cell's Dirichlet nodal values (the Dirichlet columns of R, lifted) and Dirichlet rows
 *   skipped.  Two launches, sums in one fixed order, no atomics: the same bits on every call.  nkept = 0 is legal: zeros.
 *   npg_interior_matrix: R = int gamma phi_i phi_j dV on the pattern given at create (entries no kept cell touches: 0).  A position
 *   missing in the pattern is an error of create.
 *   npg_interior_budget: out[0 .. NPG_ITR_NBUDGET) = int dV, int Q dV, int gamma (b* - b) dV over the kept cells for the state b
 *   (Dirichlet values included); a per-workgroup partial row and a fold in fixed order.
 * Validation (NPG_EINVAL + message) happens before anything is launched.  The engine must outlive the handle. */
typedef struct npg_interior npg_interior;
#define NPG_ITR_NSERIES 2
#define NPG_ITR_SOURCE 0
#define NPG_ITR_TARGET 1
#define NPG_ITR_NBUDGET 3
int npg_interior_create(npg_fe *fe, int64_t nkept, const int32_t *cells, const npg_csr *pattern, npg_interior **out);
int npg_interior_set_series(npg_interior *F, int which, int nkey, const double *tables);
int npg_interior_set_gamma(npg_interior *F, const double *table);
int npg_interior_apply(npg_interior *F, const int32_t *key, const double *w, npg_vec *rhs_src_out);
int npg_interior_matrix(npg_interior *F, npg_csr *R);
int npg_interior_budget(npg_interior *F, const int32_t *key, const double *w, const npg_vec *b, npg_vec *out);
int npg_interior_info(const npg_interior *F, int64_t *nkept, int64_t *load_slots, int64_t *matrix_entries, int64_t *matrix_slots);
int npg_interior_destroy(npg_interior *F);

/* ---- time means and eddy co-moments of the running state (new work: the reference has no time averaging) ------------------------------
 * A weighted running mean of [u; p] and b and the ten co-moments uu uv uw vv vw ww ub vb wb bb of the mesh nodes, updated once per
 * time step on the device (csrc/tavg_core.h).  The handle owns the node table only: iu[3][nnode] the position of each
 * velocity component of a node in x_inv, ib[2][nnode] two positions in b - equal for a P2 node or a vertex, the edge's two vertices
 * for a mid-node of a P1 buoyancy (its delta is half their sum); -1 is a Dirichlet DoF (delta = 0).  The accumulators are the caller's
 * vectors, zero before the first sample.
 *   npg_tavg_accumulate: for a sample of weight w the caller forms W' = W + w, r = w / W', q = w (W / W') and the call does, with the
 *   OLD means and exactly this association (add, subtract, multiply; no contraction, no division),
 *       delta_a = a - mu_a;   comom[pair][node] += (q delta_a) delta_b;   mu_a += r delta_a
 *   comom = NULL: the means only.  Two launches on the context's stream (co-moments first), no atomics: the bits of the host library.
 * Validation (NPG_EINVAL + message: vector lengths, r in (0, 1], q >= 0, both finite, index ranges at create) happens before anything
 * is launched: a failed call leaves the accumulators untouched. */
typedef struct npg_tavg npg_tavg;
int npg_tavg_create(npg_ctx *ctx, int64_t n_inv, int64_t n_b, int64_t nnode, const int32_t *iu, const int32_t *ib, npg_tavg **out);
int npg_tavg_accumulate(npg_tavg *T, double r, double q, const npg_vec *x_inv, const npg_vec *b, npg_vec *mean_x, npg_vec *mean_b,
                        npg_vec *comom);
int npg_tavg_info(const npg_tavg *T, int64_t *nnode, int64_t *n_inv, int64_t *n_b);
int npg_tavg_destroy(npg_tavg *T);

/* ---- gradients of the state recovered at the mesh's P2 nodes (new work: the reference's save_vtk hands Gridap cell fields) -------------
 * d_j u_a, grad b', grad p as NODAL fields: what vorticity, divergence, N^2 + d_z b' and the planetary PV are made of
 * (csrc/nodal_core.h).  Tetrahedral engines only.  Selected node j has the incidences inc[inc_ptr[j] .. inc_ptr[j + 1]),
 * each 16 cell + local with local = 0 .. 9 the node's place in that cell (vertices, then the edges (0,1) (0,2) (1,2) (0,3) (1,3) (2,3)),
 * in ascending cell order.  Per cell and field the gradient at the cell's four vertices is formed as npg_fe_sample forms it there; a
 * mid-node of the edge (a, b) takes 0.5 (g_a + g_b); per node S = sum_c w_c g_c and W = sum_c w_c from 0.0 in incidence order and the
 * result is S / W, with w_c = the cell's wdet (weight_mode 0) or 1.0 (weight_mode 1).  Boundary nodes get one-sided averages.
 * out[channel][nsel], the channels of the groups of fields_mask in this order: NPG_NODAL_U d_j u_a at 3 a + j (9), NPG_NODAL_B grad b' (3),
 * NPG_NODAL_P grad p (3), then W and the valence - NPG_NODAL_NCH = 17 with every group.  Two launches on the context's stream (cells
 * into a scratch of [ncell][<= 51] doubles owned by the handle, then nodes), no atomics: the bits of the host library on every call.
 * Validation (NPG_EINVAL + message) happens before anything is launched: NULL arguments, inc_ptr not starting at 0 or decreasing, a
 * selected node without incidence, cell >= ncell, local >= 10, cells not ascending, ncell >= 2^27, weight_mode, fields_mask, vector
 * lengths, an embedded 2-D engine.  nsel = 0 is legal.  The engine must outlive the handle. */
typedef struct npg_nodal npg_nodal;
#define NPG_NODAL_U 1
#define NPG_NODAL_B 2
#define NPG_NODAL_P 4
#define NPG_NODAL_NCH 17
int npg_nodal_create(npg_fe *fe, int64_t nsel, const int64_t *inc_ptr, const int32_t *inc, int weight_mode, npg_nodal **out);
int npg_nodal_compute(npg_nodal *N, const npg_vec *x_inv, const npg_vec *b, int fields_mask, npg_vec *out);
int npg_nodal_info(const npg_nodal *N, int64_t *nsel, int64_t *ninc, int64_t *max_valence, int64_t *scratch_doubles);
int npg_nodal_destroy(npg_nodal *N);

/* ---- transports through sections: exact quadrature on the polygons a plane cuts out of the cells (new work: the reference samples
 * slices of a .vtu file) ------------------------------------------------------------------------------------------------------------
 * A section is a frame {o, n, e1, e2} (orthonormal to 1e-12) and two strictly increasing edge arrays (first / last may be -inf / +inf);
 * bin (i, j) of section s is edges1[i] <= (x - o) . e1 < edges1[i + 1], edges2[j] <= (x - o) . e2 < edges2[j + 1], numbered section by
 * section, (i, j) row-major (csrc/sections_core.h).  Integrated over every bin, with the degree-4 six-point triangle rule
 * on every piece (exact for the P2 / P1 fields): NPG_NSEC = 14 raw channels - 1, u.n, b', b' u.n, z u.n, p, u_x, u_y, u_z, grad b'.n,
 * kappa_h (d_x b' n_x + d_y b' n_y) + kappa_v d_z b' n_z, kappa_v n_z, z, d_z b'.
 * The cut rule: d = ((x0 - o0) n0 + (x1 - o1) n1) + (x2 - o2) n2 at a cell's own vertices, below iff d < 0 (d == 0 is above); the corners
 * lie on the edges with d_a < 0 <= d_b at t = d_a / (d_a - d_b).  So a mesh face in the plane is counted by exactly one of its two
 * cells, and the polygons are clipped at the bin edges with the same half-open rule and fan-triangulated into pieces of area > 0.
 * Pieces are ordered by (bin, cell, index); out[bin][ch] adds a bin's pieces in one fixed order - 64 accumulators filled round-robin in
 * piece order from 0.0, then a fixed pairwise tree (section_fold of csrc/sections_core.h); an empty bin gives zeros; pieces_out
 * [ch][npiece] holds the pieces' own terms.  Two launches on the context's stream, no atomics: the bits of the host library on every
 * call (the convection closure's tanh apart).  set_coeff: kappa_h / kappa_v at the 6 points of every piece, [6][npiece] in piece order
 * (NULL removes the table; a missing table contributes 0); set_closure adds the convection closure to kappa_v at the point's own d_z b'.
 * Validation (NPG_EINVAL + message) happens before anything is launched: NULL arguments, non-finite frames or vertices, axes that are
 * not orthonormal, edges that do not increase or are infinite inside, nsec outside 1 .. 64, more than 2^20 bins, more than 2^31 - 1
 * pieces, non-finite coefficients (the handle keeps the table it had), vector lengths, an embedded 2-D engine.  The engine must outlive
 * the handle. */
typedef struct npg_sections npg_sections;
#define NPG_NSEC 14
#define NPG_SEC_KH 0
#define NPG_SEC_KV 1
int npg_sections_create(npg_fe *fe, const double *cell_xyz /* [ncell][4][3], the cells' own vertices */, int nsec,
                        const double *frames /* [nsec][12]: o, n, e1, e2 */, const int32_t *n1, const int32_t *n2,
                        const double *edges1 /* concatenated, n1[s] + 1 each */, const double *edges2,
                        const uint8_t *cell_mask /* or NULL */, npg_sections **out);
int npg_sections_info(const npg_sections *S, int64_t *npiece, int64_t *nbin, int64_t *ncut_cells, int64_t *max_per_bin);
int npg_sections_pieces(const npg_sections *S, int32_t *cell, int32_t *bin, double *lam /* [npiece][3][4] */, double *area);
int npg_sections_set_coeff(npg_sections *S, int which, const double *table /* [6][npiece] or NULL */);
int npg_sections_set_closure(npg_sections *S, double kappa_c, double N2min, double alpha, double N2c);
int npg_sections_compute(npg_sections *S, const npg_vec *x_inv, const npg_vec *b, npg_vec *out /* [nbin][NPG_NSEC] */,
                         npg_vec *pieces_out /* or NULL: [NPG_NSEC][npiece] */);
int npg_sections_destroy(npg_sections *S);

/* ---- the state binned into (latitude band, buoyancy class) (new work: the reference overlays isopycnals on a z-coordinate psi) --
 * A joint table [ny + 1][nb + 1][NPG_NCLS] over the cells of the mesh (csrc/classes_core.h).
 * Sample rule - NOT the engine's quadrature (Keast's rule has a negative weight): ns barycentric points rule_lam[ns][4] with weights
 * rule_w[ns], every weight > 0, sum = 1 (checked to 1e-12, as every lam row).  A sample of cell c carries the measure
 * w[s] wdet(c) sum_q qw[q] (the last factor from the engine's own table).  Exact for functions linear in the cell, otherwise a
 * positive Riemann sum.  At a sample, all from one lambda (closed-form P2 / P1 shape functions, Dirichlet nodes count):
 *    y = sum lambda_i y_i, z = sum lambda_i z_i (the cell's own vertices),  B = N2 z + b',  u,  grad B = grad b' + N2 e_z.
 * Bins: b_edges[nb], y_edges[ny] finite and strictly increasing, nb >= 0, ny >= 0.  Class = the number of b_edges <= B
 * (searchsorted(b_edges, B, side = "right"), 0 .. nb); band = the same of y_edges and y: the end bins are open, every finite sample is
 * counted exactly once.  A sample whose B or y is not finite goes to no bin and is counted in `dropped`.
 * Channels (term = measure x integrand; RAW integrals, prefactors are the caller's):
 *    0  1 (volume census)       1  u_x       2  u_y (residual overturning)       3  u_z
 *    4  z                       5  B         6  d_z B                            7  u . grad B
 * The same bits on every call, whatever the arrival order: pass 1 sums S_c = sum |term_c| (fixed order, as npg_integrals_compute) and
 * counts the dropped samples; with frexp(S_c) = (m, e) the channel's scale is 2^(61 - e) (1 when S_c = 0); pass 2 adds
 * llrint(term scale_c) as signed 64-bit integers with relaxed device-scope atomics (integer addition is associative); pass 3 divides
 * by the scale.  Quantisation: at most half a unit per sample, n_bin 2^-61 S_c per bin.  A channel whose S_c is not finite comes back
 * NaN.  Always fp64.  Validation (NPG_EINVAL + message) happens before anything is launched.  A mask that leaves no cell gives a zero
 * table.  The handle owns the integer table (zeroed at the start of every compute, on the stream), the partial rows, the rule and the
 * edges; the engine must outlive it. */
#define NPG_NCLS 8
/* cell_y / cell_z [ncell][4]: y and z of each cell's OWN vertices; cell_mask[ncell] or NULL: 1 = this cell counts;
   1 <= ns <= 4096; (ny + 1)(nb + 1) <= 2^22 */
int npg_classes_create(npg_fe *fe, const double *cell_y, const double *cell_z, const uint8_t *cell_mask, const double *rule_lam,
                       const double *rule_w, int ns, const double *y_edges, int64_t ny, const double *b_edges, int64_t nb,
                       npg_classes **out);
/* table: (ny + 1)(nb + 1) NPG_NCLS doubles, entry ((band (nb + 1)) + class) NPG_NCLS + channel; info: >= 1 + NPG_NCLS doubles:
   dropped, S_c.  N2 = 0 bins the perturbation b'. */
int npg_classes_compute(npg_classes *K, const npg_vec *x_inv, const npg_vec *b, double N2, npg_vec *table, npg_vec *info);
int npg_classes_destroy(npg_classes *K);

/* ---- water-mass transformation by mixing: the diffusivity-weighted table of the same handle (csrc/mixing_core.h) ----
 * For FE fields div(kappa grad B) is a distribution, so the transformation is built from the quantity that is a function in every cell:
 *    D(B0) = int_{B < B0} kappa_h (d_x B^2 + d_y B^2) + kappa_v (d_z B)^2 dV,      Phi(B0) = dD / dB0 >= 0,      E(B0) = dPhi / dB0
 * Phi is the down-gradient diffusive buoyancy flux through the surface B = B0, E the diapycnal volume transport towards higher
 * buoyancy.  Boundary terms (a surface flux) are not part of it.  Binned with the sample rule, the measure, the edges, the mask and the
 * bin search of the handle; B = N2 z + b', grad B = grad b' + N2 e_z as in npg_classes_compute.  At a sample
 *    kappa_h = kappa_h[cell][s] (or the scalar),
 *    kappa_v = kappa_v0 + kappa_c (1 + tanh(-a / N2min)) / 2,   a = alpha (N2c + d_z b'),   kappa_v0 = kappa_v0[cell][s] (or the scalar):
 * the BACKGROUND diffusivity plus the convection closure of npg_fe_update_kappa_convection evaluated from the sample's own d_z b'.
 * N2c and alpha are the closure's, separate from the binning N2.  kappa_c = 0: closure off (tanh is not evaluated).
 * Channels (term = measure x integrand, raw integrals), table [ny + 1][nb + 1][NPG_NMIX]:
 *    0  1 (the census: bit-identical to channel 0 of npg_classes_compute)      4  kappa_v
 *    1  kappa_h (d_x B^2 + d_y B^2)                                            5  kappa_h
 *    2  kappa_v (d_z B)^2                                                      6  |grad B|^2
 *    3  kappa_v d_z B                                                          7  kappa_v - kappa_v0 (the closure's part)
 * The same order-independent 64-bit integer sums, scales and info vector as npg_classes_compute; both calls zero the handle's integer
 * table on the stream at their start, so they may be interleaved on one handle.
 * npg_classes_set_diffusivity: tables [ncell][ns] (copied) or NULL = the scalar holds everywhere; every value finite and >= 0; a
 * second call replaces the first.  npg_classes_mixing refuses (NPG_EINVAL + message, before any launch): NULL arguments, no
 * diffusivities set, a non-finite or negative kappa_c, alpha, N2 or N2c, kappa_c > 0 with N2min not > 0, wrong lengths, vectors of
 * another context. */
#define NPG_NMIX 8
int npg_classes_set_diffusivity(npg_classes *K, const double *kappa_h /* [ncell][ns] or NULL */, double kappa_h_scalar,
                                const double *kappa_v0 /* [ncell][ns] or NULL */, double kappa_v0_scalar);
int npg_classes_mixing(npg_classes *K, const npg_vec *b, double N2, double kappa_c, double N2min, double alpha, double N2c,
                       npg_vec *table, npg_vec *info);   /* table, info: as npg_classes_compute */

/* ---- Lagrangian particles advected through the device-resident flow (new work: offline tracking needs u saved every step) -----
 * n particles on the device: position [n][3], the cell each was last located in, status (0 alive, 1 lost, 2 stuck), wind [n][3] and t_lost.
 * npg_particles_advance carries every live particle through nsub classical RK4 steps of dx/dt = u(x, t), h = dt / nsub, in ONE kernel
 * (csrc/particles_core.h): per stage locate -> evaluate u (closed-form P2 through the DoF tables, as npg_fe_sample(NPG_SAMPLE_U)) ->
 * next stage point; the remembered cell is accepted without reading the bins when the point's min lambda there is >= 1e-8, otherwise
 * the full election of npg_locator_find runs - either way the cell and lambda of npg_locator_find, bit for bit.
 * Velocity in time: u = (1 - s) u(x_a) + s u(x_b), s = s0 + (s1 - s0) (tau / dt), tau = the time since the start of the call; x_a and
 * x_b the same vector (the same device memory): frozen flow, one evaluation, s unused.  Model time is the particles' clock.
 * Periodic axes (npg_particles_set_period): L[a] > 0 = the period of axis a, 0 = not periodic; the lower bound is the locator's box.
 * Stage points are wrapped into [lo, lo + L) for their location only, the stored position after the step; wind counts the crossings:
 * the unwrapped position is x + wind L.
 * Leaving the mesh: a step with a stage point or an end point outside the mesh is not taken - the particle keeps its position of the
 * start of that step, status = 1, t_lost = the time at the start of that step, and no later call moves it.  A seed that is NaN or
 * outside the mesh is lost at the start of the first call.  No reflection, no projection onto the boundary.
 * Always fp64.  Validation (NPG_EINVAL + message) happens before anything is launched.  A partitioned locator
 * (npg_locator_create_cells) is refused: migration between ranks is not implemented; an embedded 2-D engine has no locator. */
int npg_particles_create(npg_ctx *ctx, int64_t n, npg_particles **out);       /* n = 0 is legal; positions 0, t = 0 until set */
int npg_particles_destroy(npg_particles *P);
/* xyz[n][3] (host) at time t0; resets status, wind, t_lost (NaN) and the remembered cells */
int npg_particles_set(npg_particles *P, const double *xyz, double t0);
int npg_particles_set_period(npg_particles *P, const double *L3);
int npg_particles_advance(npg_particles *P, npg_fe *fe, npg_locator *loc, const npg_vec *x_a, const npg_vec *x_b, double s0, double s1,
                          double dt, int64_t nsub);
/* host copies: xyz[n][3], cell[n], status[n], wind[n][3] (int32), t_lost[n] (NaN while alive); any may be NULL */
int npg_particles_download(const npg_particles *P, double *xyz, int32_t *cell, int32_t *status, int32_t *wind, double *t_lost);
/* device copy of the positions into a vector of 3 n doubles: what npg_locator_find / npg_fe_sample take (b along a path) */
int npg_particles_positions(const npg_particles *P, npg_vec *out);

/* ---- diffusing particles and reflecting walls (csrc/particles_walk_core.h; opt-in: npg_particles_advance keeps its bits) -----------
 * npg_particles_walk is npg_particles_advance - the same arguments, the same clock, the same RK4 step - with every move of a particle
 * (the three stage points, the RK4 end point, the random displacement) walked from cell to cell through a neighbour table: across an
 * interior face into the neighbour, across a periodic seam with the face's translation, off a boundary face by reflection of the
 * remainder (r <- r - 2 (r . n) n), which the particle's reflection counter counts for the moves that move the particle (the end
 * point and the random displacement; a stage point's reflections and crossings are its own).  More than 64 face events in one move,
 * or an end point that npg_locator_find would refuse: the step is not taken and the particle is STUCK - status 2, otherwise the rule
 * of a lost one.  A seed that is NaN or outside the mesh is lost (status 1), as before.
 *   nbr[ncell][4]       the cell across the face opposite local vertex i (the locator's vertex order), -1 = a boundary face
 *   shift[ncell][4][3]  the translation in periods (-1, 0, 1) a point takes on each axis when it crosses that face: x += shift L,
 *                       wind -= shift (unwrapped = x + wind L stays where it was); nonzero only across a periodic seam.  On an axis
 *                       with a period the table must carry the seam (a walked point is not wrapped), on any other it must not.
 * Diffusion (optional; without it: reflecting advection): kappa_h[ncell][4], kappa_v[ncell][4] at each cell's own vertices, piecewise
 * linear (kappa = sum lambda_i kappa_i, grad kappa constant in the cell), finite and >= 0.  After each RK4 step of length h, in the
 * cell of its end point (Visser's scheme with uniform increments):
 *   delta = c_d h (d_x kappa_h, d_y kappa_h, d_z kappa_v);   kappa* = max(kappa + delta . grad kappa / 2, 0) for kappa_h and kappa_v;
 *   Delta_a = delta_a + R_a sqrt(6 c_d kappa*_a h),          R = the generator's three uniforms in (-1, 1): variance 2 c_d kappa* h.
 * Generator: Philox4x32-10, key = seed (low, high word), counter = (particle index low, high, step number low, high), R_a =
 * (2 w_a + 1) 2^-32 - 1 from words 0..2.  The step number counts the steps of npg_particles_walk since npg_particles_set (nsub per
 * call).  A second npg_particles_set_diffusion replaces the first; kappa_h = kappa_v = NULL switches diffusion off. */
int npg_particles_set_walls(npg_particles *P, const int32_t *nbr, const int8_t *shift, int64_t ncell);
int npg_particles_set_diffusion(npg_particles *P, const double *kappa_h, const double *kappa_v, int64_t ncell, double c_d, uint64_t seed);
int npg_particles_walk(npg_particles *P, npg_fe *fe, npg_locator *loc, const npg_vec *x_a, const npg_vec *x_b, double s0, double s1,
                       double dt, int64_t nsub);
/* nreflect[n] (host; zeros before any walls were set) and the step number; either may be NULL */
int npg_particles_download_walk(const npg_particles *P, int32_t *nreflect, uint64_t *step);
/* the generator alone: R of n consecutive particle indices from first_index at one step number, out = 3 n doubles */
int npg_particles_uniforms(npg_ctx *ctx, uint64_t seed, uint64_t first_index, int64_t n, uint64_t step, npg_vec *out);

/* ---- maps on buoyancy surfaces (new work: the reference overlays contour lines of b on slices) ----------------------------------
 * Where the surfaces B = B_k of the full buoyancy B = N2 z + b' lie over fixed columns (x_j, y_j), and the flow on them
 * (csrc/surfaces_core.h).  npg_surfaces_create tiles every column into the cells the vertical line passes through,
 * top to bottom: segments (cell, z_top, z_bot) that abut bit for bit, from the locator's cell records.  A cell's interval is
 * {z : lambda_i >= 0 for all i}; a constraint that does not depend on z (|d_z lambda_i| <= 1e-12 |grad lambda_i|) is met iff
 * lambda_i >= -1e-10; intervals no longer than 1e-12 of the box's z extent are dropped; the sweep starts at the highest interval
 * top and takes, among the intervals that contain the point just below, the one that reaches deepest (ties: the lowest cell id).
 * It stops at the first gap: a column is its uppermost connected piece.  A column without an interval, or with NaN coordinates, is
 * dry.  xy[ncol][2] is host memory (copied); the engine and the locator must outlive the handle (one context; a partitioned locator and a
 * locator of another mesh - an embedded 2-D engine has none - are refused).
 * npg_surfaces_compute: one thread per column walks its segments once.  Along a segment B is a quadratic in z through its values at
 * the top (carried from the segment above), the midpoint and the bottom - exact for P2 b', linear for P1 - and "above" means
 * B - B_k >= 0.  Ends that differ: one crossing; ends that agree: two where the vertex of the parabola lies inside and on the other
 * side.  out[9][nlev][ncol]: z of the uppermost crossing, z of the lowermost, the number of crossings, and at the uppermost one u_x,
 * u_y, u_z, d_x B, d_y B, d_z B (evaluated as npg_fe_sample does; N2 added to d_z).  cols[4][ncol]: z_top, z_bot, B at the top, B at
 * the bottom.  No crossing, or a dry column: NaN (the count is 0).  The same bits on every call.  levels[nlev] is host memory,
 * finite and strictly increasing.  Validation (NPG_EINVAL + message) happens before anything is launched or written. */
typedef struct npg_surfaces npg_surfaces;
#define NPG_NSURF 9
int npg_surfaces_create(npg_fe *fe, npg_locator *loc, const double *xy, int64_t ncol, npg_surfaces **out);
int npg_surfaces_destroy(npg_surfaces *S);
/* the number of segments, the most of one column and the number of dry columns; any may be NULL */
int npg_surfaces_info(const npg_surfaces *S, int64_t *nseg, int64_t *max_per_col, int64_t *ndry);
/* per column (host arrays, any may be NULL): z_top, z_bot (NaN where dry) and the number of segments */
int npg_surfaces_columns(const npg_surfaces *S, double *z_top, double *z_bot, int32_t *nseg);
/* the segments themselves, column after column (host arrays of npg_surfaces_info's nseg entries, any may be NULL) */
int npg_surfaces_segments(const npg_surfaces *S, int32_t *cell, double *z_top, double *z_bot);
int npg_surfaces_compute(npg_surfaces *S, const npg_vec *x_inv, const npg_vec *b, double N2, const double *levels, int nlev,
                         npg_vec *out, npg_vec *cols);

/* ---- column integrals (the reference: scratch/postprocess.jl, compute_U_V / compute_gamma / compute_JEBAR on sampled grids) ---
 * The exact vertical integrals of the state over fixed columns (x_j, y_j), and the state at the columns' ends (csrc/columns_core.h,
 * DESIGN.md 32).  npg_columns_create tiles the columns exactly as npg_surfaces_create does (the same segments, bit for bit; the same
 * rules for a dry column), and npg_columns_info / _columns / _segments read the tiling as their npg_surfaces_* namesakes do.  xy[ncol][2]
 * is host memory (copied); the engine and the locator must outlive the handle.  Refused: NULL arguments, ncol < 1, arguments of
 * different contexts, a partitioned locator, a locator of another mesh (an embedded 2-D engine has none), 2^31 segments or more.
 * npg_columns_compute: along a segment every integrand is a polynomial in z of degree <= 5, integrated exactly by the 3-point
 * Gauss-Legendre rule at z_bot + s (z_top - z_bot), s = 1/2 (1 - sqrt(3/5)), 1/2, 1/2 (1 + sqrt(3/5)), weights 5/18, 8/18, 5/18; the
 * terms of a column's segments are added top to bottom from 0.0.  out[NPG_NCOLI + NPG_NCOLE][ncol]:
 *    0 thickness | 1-3 int u_x, u_y, u_z | 4 int b' | 5 int z b' | 6 int p | 7, 8 int d_x p, d_y p | 9, 10 int d_x b', d_y b' |
 *    11, 12 int z d_x b', z d_y b' | 13 int (u_x^2 + u_y^2) / 2 | 14-16 int u_x b', u_y b', u_z b' |
 *    17-24 at the bottom (the last segment's cell, z_bot): p, b', d_z b', d_x p, d_y p, d_z p, d_x z_bot, d_y z_bot |
 *    25-30 at the top (the first segment's cell, z_top): p, b', u_x, u_y, d_x z_top, d_y z_top.
 * The slopes of z_bot and z_top are those of the cell's face the column leaves through: - G_ix / G_iz of the constraint lambda_i >= 0
 * that bounds the column's interval in the cell (at a tie the lowest i).  The fields are evaluated as npg_fe_sample evaluates them.
 * A dry column: NaN in every channel.  segments_out (may be NULL): the terms themselves, [NPG_NCOLI][nseg].  The same bits on every
 * call, and the same bits from both libraries.  Validation (NPG_EINVAL + message) happens before anything is launched or written. */
typedef struct npg_columns npg_columns;
#define NPG_NCOLI 17
#define NPG_NCOLE 14
int npg_columns_create(npg_fe *fe, npg_locator *loc, const double *xy, int64_t ncol, npg_columns **out);
int npg_columns_destroy(npg_columns *C);
/* the number of segments, the most of one column and the number of dry columns; any may be NULL */
int npg_columns_info(const npg_columns *C, int64_t *nseg, int64_t *max_per_col, int64_t *ndry);
/* per column (host arrays, any may be NULL): z_top, z_bot (NaN where dry) and the number of segments */
int npg_columns_columns(const npg_columns *C, double *z_top, double *z_bot, int32_t *nseg);
/* the segments themselves, column after column (host arrays of npg_columns_info's nseg entries, any may be NULL) */
int npg_columns_segments(const npg_columns *C, int32_t *cell, double *z_top, double *z_bot);
int npg_columns_compute(npg_columns *C, const npg_vec *x_inv, const npg_vec *b, npg_vec *out, npg_vec *segments_out);

/* ---- passive tracers carried by the flow (new work: the reference evolves b' alone) -------------------------------------------
 * K scalars stepped with the model's own advection-diffusion operator: the same BDF scheme, the same matrix M + theta (Kh + Kv) and the
 * same velocity extrapolation as b' (csrc/tracers_core.h).  Tracer k has nodal values c (free DoFs in the buoyancy
 * numbering; Dirichlet nodes take the tracer's OWN values, not b_diri), a background gradient gamma (the full tracer is gamma z + c)
 * and a uniform source.  npg_tracers_rhs writes, for every tracer and every row i,
 *    y_k[i] = int ( c1 c + c2 c_prev - cdt ( u~ . grad c~ + u~_z gamma_k - source_k ) ) phi_i
 *           - int ( c_D phi_i + theta ( kappa_h grad_h c_D . grad_h phi_i + kappa_v d_z c_D d_z phi_i ) )
 *           + theta gamma_k rhs_diff1[i] + dt flux_k[i]
 * with the scheme constants of npg_fe_evolution_rhs, c_D = the tracer's Dirichlet part, kappa_h / kappa_v the engine's CURRENT tables
 * (the tracers follow the convection closure), rhs_diff1 = npg_fe_assemble_rhs_diff(fe, 1.0, .), shared by all tracers.
 * One launch evaluates u~ at the quadrature points once per cell and loops over the tracers; a second one gathers the rows in cell
 * order: no atomics, the same bits on every call, and tracer k's output does not depend on the other tracers of the call.  The
 * arithmetic follows npg_fe_set_precision.  The handle owns the local vectors (ntracer * nloc_b * ncell doubles); the engine must
 * outlive it.  Validation (NPG_EINVAL + message) happens before anything is launched. */
int npg_tracers_create(npg_fe *fe, int ntracer, npg_tracers **out);
int npg_tracers_destroy(npg_tracers *T);
/* diri_or_null[n_b_diri]: the tracer's values at the Dirichlet nodes in the order of npg_fe_desc.b_diri (NULL = zeros) */
int npg_tracers_set(npg_tracers *T, int k, const double *diri_or_null, double gamma, double source);
/* c, c_prev, flux, y: [ntracer * n_b], tracer k at k * n_b.  rhs_diff1 may be NULL only if every gamma is 0; flux may be NULL. */
int npg_tracers_rhs(npg_tracers *T, int scheme, double dt, double theta, const npg_vec *c, const npg_vec *c_prev,
                    const npg_vec *x_inv, const npg_vec *x_inv_prev, const npg_vec *rhs_diff1_or_null,
                    const npg_vec *flux_or_null, npg_vec *y);

/* ---- isoneutral mixing of the passive tracers: the rotated diffusion tensor of the running buoyancy --------------------------------
 * (csrc/redi_core.h).  With B = N2 z + b' in mesh coordinates, at a quadrature point
 *    Bz+ = max(d_z B, bz_min),   S = -grad_h B / Bz+,   S <- S min(1, slope_max / |S|),
 *    K = kappa_iso [1 0 S_x; 0 1 S_y; S_x S_y |S|^2] + kappa_v z z'.
 * npg_tracers_set_isoneutral copies kappa_iso[nq][ncell] (the engine's [q][cell] layout; NULL switches the mode off) and allocates the
 * three tensor tables kxz = kappa_iso S_x, kyz = kappa_iso S_y, kzz = kappa_iso |S|^2 in the same layout.
 * npg_tracers_isoneutral_update rebuilds them from b (one launch, one lane per cell) and counts the points floored by bz_min and
 * clipped by slope_max (per-workgroup partial counts folded in workgroup order; no atomics).
 * npg_tracers_isoneutral_matrix assembles on the buoyancy pattern (one launch, sixteen lanes per CSR row, no atomics, the same bits on
 * every call)
 *    K[i][j] = sum_q w_q ( kappa_iso (g_ix g_jx + g_iy g_jy) + kxz (g_ix g_jz + g_iz g_jx) + kyz (g_iy g_jz + g_iz g_jy) + kzz g_iz g_jz ),
 * free columns only: the Dirichlet lift is per tracer and goes through npg_tracers_rhs.  With S = 0 it adds exact zeros to the
 * NPG_MAT_KH form.  Tables and matrix are fp64 whatever npg_fe_set_precision says.
 * With the mode on, the second integral of npg_tracers_rhs becomes  int ( c_D phi_i + theta ( K (grad c_D + gamma_k z) ) . grad phi_i ),
 * K with kzz + kappa_v, in every cell where the tracer has a non-zero Dirichlet value or gamma_k != 0, and theta gamma_k rhs_diff1 is
 * NOT added (rhs_diff1 may be NULL).  npg_tracers_rhs after npg_tracers_set_isoneutral and before an update is NPG_EINVAL.
 * Refused (NPG_EINVAL + message, before anything is launched): a non-finite or negative kappa_iso, slope_max < 0 or non-finite,
 * bz_min <= 0 or non-finite, an embedded 2-D engine, a matrix that is not on the buoyancy pattern, a vector of the wrong length.
 * npg_tracers_isoneutral_info: the counts of the last update, the number of points, state 0 = off, 1 = set, 2 = updated.
 * npg_tracers_isoneutral_tables downloads the three tables ([nq][ncell] each) of the last update. */
int npg_tracers_set_isoneutral(npg_tracers *T, const double *kappa_iso_or_null, double slope_max, double bz_min);
int npg_tracers_isoneutral_update(npg_tracers *T, double N2, const npg_vec *b);
int npg_tracers_isoneutral_matrix(npg_tracers *T, npg_csr *K);
int npg_tracers_isoneutral_info(npg_tracers *T, int64_t *nfloored, int64_t *nclipped, int64_t *npoints, int *state);
int npg_tracers_isoneutral_tables(npg_tracers *T, double *kxz, double *kyz, double *kzz);

/* ---- the tracers' transport operator as a matrix: equilibria and implicit-advection steps with a frozen flow ----------------------
 * (csrc/transport_core.h).  With W = w_q |J| and u(q) = scale sum_a N2[q][a] u_a,
 *    C[i][j] = sum_{cells, q} W phi_i(q) ( u(q) . grad phi_j(q) ),
 *    g_k[i]  = int ( S_k - u_z gamma_k - u . grad c_D,k - lambda_k c_D,k ) phi_i
 *              - kappa_hat int ( kappa_h grad_h c_D,k . grad_h phi_i + kappa_v d_z c_D,k d_z phi_i ) + kappa_hat gamma_k rhs_diff1[i] + flux_k[i],
 * c_D,k the tracer's Dirichlet values (npg_tracers_set), so that for any c, any dt and lambda = 0
 *    npg_tracers_rhs(NPG_BDF1, dt, dt kappa_hat, c, c, x, x) = M c + dt (g - C c)          over the free rows, to summation rounding.
 * npg_tracers_transport_update writes the three velocity tables ux, uy, uz [nq][ncell] from x_inv = [u; p] (one launch, one lane per
 * cell).  npg_tracers_transport_matrix assembles C on the buoyancy pattern (one launch, sixteen lanes per CSR row, no atomics, the
 * same bits on every call; free columns only: the Dirichlet lift is in the load; scale = 0 gives exact zeros).
 * npg_tracers_transport_load writes the K loads (one fused element launch that reads the velocity tables once per cell, and the
 * gather of npg_tracers_rhs); decay = lambda[K] on the host or NULL, rhs_diff1 is needed when a tracer has gamma != 0, the engine's
 * kappa_h / kappa_v tables when one has a non-zero Dirichlet value.  All fp64 whatever npg_fe_set_precision says.
 * Refused (NPG_EINVAL + message, before anything is launched, outputs untouched): a non-finite scale, an x_inv of the wrong length, a
 * matrix that is not on the buoyancy pattern, a negative or non-finite decay rate or kappa_hat, a matrix / load / tables call before an
 * update, an embedded 2-D engine, handles of different contexts.
 * npg_tracers_transport_info: state 0 = no tables, 1 = updated; umax = the largest |u| over the points of the last update.
 * npg_tracers_transport_tables downloads the three tables ([nq][ncell] each). */
int npg_tracers_transport_update(npg_tracers *T, const npg_vec *x_inv, double scale);
int npg_tracers_transport_matrix(npg_tracers *T, npg_csr *C);
int npg_tracers_transport_load(npg_tracers *T, double kappa_hat, const double *decay_or_null, const npg_vec *rhs_diff1_or_null,
                               const npg_vec *flux_or_null, npg_vec *out);
int npg_tracers_transport_info(npg_tracers *T, int *state, double *umax);
int npg_tracers_transport_tables(npg_tracers *T, double *ux, double *uy, double *uz);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI (new work: the reference is single-device) ----------------- */
#define NPG_UNIQUE_ID_BYTES 128
int npg_comm_unique_id(void *id128);                                  /* rank 0 makes it, the launcher broadcasts it */
int npg_comm_init(npg_ctx *ctx, const void *id128, int rank, int nranks);
/* one line of JSON about the communicator: rank, nranks, rccl_ranks (ncclCommCount), device, in_cycle_transport */
int npg_comm_info(npg_ctx *ctx, char *buf, size_t cap);
/* auto transport only: drop the peer windows, RCCL carries the in-cycle traffic from here on (no live halo plans) */
int npg_comm_disable_peer(npg_ctx *ctx);
int npg_comm_allreduce_sum(npg_ctx *ctx, double *host_inout, int n);  /* tiny host-side helper for tests/bench */
int npg_comm_allreduce_vec(npg_ctx *ctx, npg_vec *v);                 /* <= 32 doubles, in place, on the context's stream */
/* any length, in place; in pieces of what the transport's window takes.  peer and shm windows: summed in rank order (the same bits
 * on every rank, every call and both transports), synchronises with the host */
int npg_comm_allreduce_long(npg_ctx *ctx, npg_vec *v);
/* Replicate a row-block distributed vector on every rank: segment s of `full` ([global_off, global_off + len)) is owned
 * by rank seg_rank[s], who holds it at local[local_off ..].  One grouped ncclBroadcast per segment over xGMI. */
int npg_comm_allgather_segments(npg_ctx *ctx, const npg_vec *local, int nseg, const int32_t *seg_rank,
                                const int64_t *seg_local_off, const int64_t *seg_global_off, const int64_t *seg_len,
                                npg_vec *full);
/* Halo plan for a row-block distributed CSR: this rank owns n_owned rows; columns >= n_owned of the local matrix are
 * ghosts filled from neighbours.  send_idx lists owned entries to ship to each peer, recv goes to consecutive ghost
 * slots. */
int npg_halo_create(npg_ctx *ctx, int64_t n_owned, int64_t n_ghost, int npeers, const int32_t *peer_rank,
                    const int64_t *send_ptr, const int32_t *send_idx, const int64_t *recv_ptr, npg_halo **out);
int npg_halo_destroy(npg_halo *h);
int npg_halo_exchange(npg_halo *h, npg_vec *x_with_ghosts);
/* Attach a plan to a workspace created for n = n_owned: npg_gmres_solve / npg_cg_solve then take A as the rank's
 * n_owned x (n_owned + n_ghost) row block, y with n_owned and x with n_owned + n_ghost entries, exchange the interface
 * before every SpMV and all-reduce the inner products (two 32-double messages per GMRES iteration). */
int npg_gmres_set_halo(npg_gmres *ws, npg_halo *h);
/* Distributed cycles (new work, no reference counterpart).  overlap (default 1): the split cycle (>= 8192 rows per rank)
 * runs the tiles of the row block that read no ghost column while the halo exchange of the Arnoldi vector is in flight
 * on the plan's own stream, the others behind it; 0 exchanges first.  graph (default 0): replay the cycle - RCCL calls
 * included - from a hipGraph instead of launching it eagerly (RCCL transport only; exercised on a one-rank communicator
 * so far).  Same iterates in every combination (tests/rccl_selftest_worker.py). */
int npg_gmres_set_dist_options(npg_gmres *ws, int overlap, int graph);
int npg_cg_set_halo(npg_cg *ws, npg_halo *h);

#ifdef __cplusplus
}
#endif
#endif /* NUPGCM_HIP_H */
