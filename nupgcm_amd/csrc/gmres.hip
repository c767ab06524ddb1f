// Device-resident restarted GMRES(m): replaces Krylov.krylov_solve!(::GmresWorkspace, A, y, x; M=P, ...) as configured at
// /root/reference/src/inversion.jl:74-94 and driven from /root/reference/src/iterative_solvers.jl:58.
//
// MI355X design.  On the reference's GPU path one inner iteration is ~23 library calls and ~11 host-blocking scalar
// reductions (modified Gram-Schmidt: j dependent dot->axpy pairs).  Measured on MI355X, a dependent kernel boundary that
// carries a small reduction costs ~4.5 us, so the iteration is organised to need exactly TWO of them, and no scalar ever
// visits the host inside a restart cycle (one hipGraph = 2 m + 2 kernels):
//
//   K1(j)  finalise Hessenberg column j-1 from the previous kernel's partial sums (Givens, residual estimate, stopping
//          test - redundantly in every workgroup, fixed summation order), v_j = wt/beta, w = P A v_j with the CSR-stream
//          SpMV of spmv_device.h, partial h1 = V_{0..j}' w and ||w||^2                                        -> P1
//   K2(j)  h1 = sum P1 ; wt = w - V h1 ; partial h2 = V' wt and ||wt||^2                                      -> P2
//   XU     finalise the last column, back-substitute R y = z, x += V y
//   R1     wt = P (b - A x), ||wt||^2   (true residual that starts the next cycle)                            -> PR
//
// Orthogonalisation = classical Gram-Schmidt (one reduction for all j+1 coefficients instead of MGS's j sequential
// ones) with a SELECTIVE second pass folded into the next K1: h2 = V' wt is always available from K2's reduction; when
// ||wt|| < eta ||w|| (cancellation, DGKS test) K1 uses wt - V h2 instead of wt - correcting its SpMV gather on the fly -
// the Hessenberg column becomes h1 + h2 and ||wt - V h2||^2 = ||wt||^2 - ||h2||^2.  No third kernel, no extra reduction.
// Results agree with Krylov.jl's MGS to rounding, not bitwise; partial sums are combined in a fixed order, so a solve is
// bit-reproducible run to run.
//
// Basis layout: V is stored GROUP-INTERLEAVED, Vi[k/8][row][k%8] (64 B per row and group of 8 basis vectors).  Every kernel
// that needs "all basis vectors at one row" maps 32 consecutive lanes to one row (lane = basis index): the first j+1
// entries of consecutive rows are ceil((j+1)/8) contiguous, fully used streams, there is ONE accumulator per
// thread (its basis index, summed over the rows the thread visits), and the block reduction is a 32 x 32 LDS transpose
// instead of 22 shuffle trees.  The SpMV never reads Vi: its input is the contiguous vector wt.
//
// State hand-off between kernels goes through write-once snapshot slots T[j] ("state after j finalised columns"): a slot
// is written by workgroup 0 of one kernel and only read by LATER kernels, so no workgroup ever reads a location another
// workgroup of the same launch writes.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <type_traits>

#include <hip/hip_ext.h>

#include "common.h"
#include "spmv_device.h"
#include "spmv_window.h"

namespace npg {

constexpr int kKB = 512;                  // threads per Krylov workgroup: 8 waves, three workgroups per CU (<= 80 VGPRs)
constexpr int kKP = kPartStride;          // 32: lanes per row group = padded basis size = doubles per partial row
constexpr int kNS = kKB / kKP;            // 32 row slots per workgroup pass / slices of the partial reduction
constexpr int kMaxG = 768;                // max workgroups (= partial rows): three per CU
constexpr int kMaxI = kMaxG / kNS;        // loads per thread in the partial reduction (8)
constexpr int kNormSlot = kKP - 1;        // partial rows carry the squared norm in their last entry
constexpr int kMaxRows = 2048;            // capacity of the partial-row buffers

struct Snap {
    double eps, rnorm0, rnorm, beta, zeta;
    int iter, inner, done, npass, first, nreorth, pad0, pad1;
};

struct GParams {
    double atol, rtol, eta2, btol;
    long long itmax;
};

struct GDev {
    CsrDev A;
    const TileDesc *tile_ptr;
    int ntiles, n, mem;
    int nt_int;           // tiles [0, nt_int) read no ghost column (distributed row blocks; = ntiles otherwise)
    const WTileDesc *wt_ptr;  // windowed tile set (spmv_window.h) for the Arnoldi kernel's gather-layout instance; null: none
    WinDev W;
    int nwt, nwt_int, wl; // wl: lanes per node in a windowed tile's segmented sums (4 or 8)
    int word;             // the windowed set also holds ordinary tiles
    int wpre;             // request the first tile's window before the prologue (tuning switch NPG_WIN_PRE)
    int pkind;
    double pscalar;
    const double *pdiag;
    const double *b;
    double *x, *Vi, *w, *wt;
    double *P1, *P2, *PR;
    int G1, G2, GP1, GP2; // GP1/GP2 = partial rows in P1/P2: G1/G2 in fused mode, GR in split mode
    int GR;               // grid of the row-streaming kernels (split mode)
    int split;
    int64_t ldv;          // split mode stores the basis column-major, Vi[k * ldv + row] (0: group-interleaved layout)
    float *Vf;            // split mode, compressed basis: the SAME columns stored in fp32 (null: fp64 in Vi).  Only stored
                          // copies are rounded (the basis columns; with `xg` below also the SpMV's gather copy of the
                          // Krylov vector) - every product and sum stays fp64; see npg_gmres_set_basis
    int pyth;             // distributed runs: ||w - V h||^2 = ||w||^2 - ||h||^2 instead of a second all-reduce
    int lazy2;            // one GPU: the same identity decides whether the second-pass sums need reducing at all
    int rev;              // split mode: the orthogonalisation kernel walks the row blocks downwards, the dots kernel upwards -
                          // what one sweep read last is what the next reads first (Infinity Cache reuse of the basis)
    GatherMap xg;         // fp32-stored basis, fast mode, node-blocked A: wt ALSO in fp32 gather layout (spmv_device.h),
                          // written by the kernels that write wt, gathered by the Arnoldi kernel (p = null: off)
    const int32_t *gslot; // distributed, ghost nodes as record columns: float position of every ghost column's node slot in xg (-1: none)
    int fast;             // one GPU, split mode: the orthogonalisation kernel does not form the second-pass sums at all; a
                          // column that would have needed them is counted (pad1) and later solves run the full kernels
    // what the CONSUMER prologues reduce: the producers' partial rows on one GPU, or the single all-reduced row when
    // the system is distributed over several GPUs
    const double *Q1, *Q2, *QR;
    int nQ1, nQ2, nQR;
    int onefold;          // one GPU, split mode, fast instances: the dots kernel's partial rows are summed ONCE (k_gmres_fold_first)
                          // into the row Q1 points at, which also takes hcol1 / wnorm2 out of the orthogonalisation kernel
    int vdots;            // ... and, with the fp32-stored basis, column j is formed where it is first read: the dots kernel of
                          // step j computes it from wt and T[j].beta and stores it, the Arnoldi kernel's epilogue stores w only
    int fusedrows;        // ... and steps of up to GmresPlan::fused_cols columns run dots, fold and update as ONE resident launch
                          // (k_gmres_rows_fused), which keeps a thread's last trips on chip across a grid-wide hand-off
    struct RowsHandOff *ho;   // that hand-off's counters, generation and status word (monotonic: nothing is reset between launches)
    Snap *C, *T;
    double *c, *s, *z, *R, *hcol1, *wnorm2;
    double *hist;
    int hist_cap;
    const GParams *prm;
};

__device__ __forceinline__ void sym_givens(double a, double b, double &c, double &s, double &rho) {
    if (b == 0.0) {
        c = (a == 0.0) ? 1.0 : copysign(1.0, a);
        s = 0.0;
        rho = fabs(a);
    } else if (a == 0.0) {
        c = 0.0;
        s = copysign(1.0, b);
        rho = fabs(b);
    } else if (fabs(b) > fabs(a)) {
        const double t = a / b;
        s = copysign(1.0, b) / sqrt(1.0 + t * t);
        c = s * t;
        rho = b / s;
    } else {
        const double t = b / a;
        c = copysign(1.0, a) / sqrt(1.0 + t * t);
        s = c * t;
        rho = a / c;
    }
}

struct KShared {
    double red[kKP];
    double h[kKP], h2[kKP], cc[kKP], ss[kKP], y[kKP];
    Snap T;
    double rho, zcol;     // diagonal entry of R and rotated z of the column finalised in THIS launch
    int fin;              // 1 if finalize_column really finalised a column in this launch
    int reorth;           // 1 if that column took the second Gram-Schmidt pass (the new vector is wt - V h2)
};

// All threads: acc holds this thread's accumulator for (slot = tid / 32, k = tid % 32).  Sums the 32 slots in a fixed
// order and stores the block's partial row.
__device__ __forceinline__ void store_partial_row(double acc, double *tmp, double *part) {
    __syncthreads();
    tmp[threadIdx.x] = acc;                   // [slot][k]
    __syncthreads();
    if (threadIdx.x < kKP) {
        double s = 0.0;
#pragma unroll
        for (int sl = 0; sl < kNS; ++sl) s += tmp[sl * kKP + threadIdx.x];
        part[(size_t)blockIdx.x * kKP + threadIdx.x] = s;
    }
}

// Finalise Hessenberg column `colj` from K2(colj)'s partial sums (all threads call; thread 0 does the serial part).
// Every global load is issued before the first barrier: one memory round trip.  Leaves the new snapshot in sh.T.
__device__ void finalize_column(const GDev &d, int colj, KShared &sh, double *tmp) {
    const int t32 = threadIdx.x & (kKP - 1);
    const double h1 = d.hcol1[colj * kKP + t32];
    const double cv = d.c[t32], sv = d.s[t32];
    const Snap prev = d.T[colj];
    const double wnorm2 = d.wnorm2[colj];
    // ||w - V h||^2 by Pythagoras from the first-pass sums (every 32-lane group computes the same number).  While it is
    // far from cancellation (and from the second-pass threshold) the orthogonalisation kernel's own partial sums - the
    // exact norm and h2 = V'(w - V h) - are not needed and their reduction over <= 768 rows is skipped.
    const double q1 = group_sum_dpp<kKP>(t32 <= colj ? h1 * h1 : 0.0);
    const double n2f = wnorm2 - q1;
    // (fast mode: the rows then hold the exactly summed norm only, h2 = 0 - no second pass, but no cancellation either)
    const bool need2 = !d.pyth && (!d.lazy2 || !(n2f >= fmax(d.prm->eta2, 1e-4) * wnorm2));
    if (need2) reduce_partials<kNS, kMaxI>(d.Q2, d.nQ2, kKP, tmp, sh.red);        // [0..colj] = h2, [31] = ||wt||^2
    if (threadIdx.x < kKP) {
        sh.h[threadIdx.x] = h1;
        sh.h2[threadIdx.x] = (need2 && !d.fast && (int)threadIdx.x <= colj) ? sh.red[threadIdx.x] : 0.0;
        sh.cc[threadIdx.x] = cv;
        sh.ss[threadIdx.x] = sv;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        Snap t = prev;
        sh.fin = (t.done == 0) ? 1 : 0;
        sh.reorth = 0;
        if (t.done == 0) {
            double n2;
            if (d.pyth) {
                // V orthonormal, h = V'w  =>  ||w - V h||^2 = ||w||^2 - ||h||^2: both already summed over the ranks by
                // the first all-reduce of this step.  Close to cancellation the difference is worthless: the pass is
                // interrupted BEFORE this column (done = 5; the update kernel applies the columns finalised so far) and
                // the host carries on with explicitly reduced norms.
                n2 = fmax(n2f, 0.0);
                if (n2f < 1e-4 * wnorm2) {
                    t.pad0 += 1;
                    t.done = 5;
                    sh.fin = 0;
                }
            } else if (!need2) {
                n2 = fmax(n2f, 0.0);
            } else {
                n2 = sh.red[kNormSlot];
            }
          if (t.done == 0) {
            const bool due = need2 && n2 < d.prm->eta2 * wnorm2;
            if (due && d.fast) t.pad1 += 1;              // a second pass was due; the fast kernels have no h2 for it
            const bool reorth = due && !d.fast;
            if (reorth) {
                double q = 0.0;
                for (int i = 0; i <= colj; ++i) {
                    q += sh.h2[i] * sh.h2[i];
                    sh.h[i] += sh.h2[i];
                }
                n2 = fmax(n2 - q, 0.0);
                sh.reorth = 1;
            }
            const double hbis = sqrt(n2);
            // apply the previous rotations; the running entry is carried in a register so that the LDS reads of step
            // i+1 do not depend on the arithmetic of step i
            double hi = sh.h[0];
#pragma unroll 4
            for (int i = 0; i < colj; ++i) {
                const double ci = sh.cc[i], si = sh.ss[i], hn = sh.h[i + 1];
                sh.h[i] = ci * hi + si * hn;
                hi = si * hi - ci * hn;
            }
            sh.h[colj] = hi;
            double cj, sj, rho;
            sym_givens(hi, hbis, cj, sj, rho);
            const double zeta_next = sj * t.zeta;
            const double zcol = cj * t.zeta;
            t.rnorm = fabs(zeta_next);
            t.iter += 1;
            t.inner += 1;
            t.nreorth += reorth ? 1 : 0;
            const bool solved = (t.rnorm <= t.eps) || (t.rnorm + 1.0 <= 1.0);
            t.done = solved ? 1 : ((long long)t.iter >= d.prm->itmax ? 2 : (hbis <= d.prm->btol ? 3 : 0));
            t.beta = hbis;
            t.zeta = zeta_next;
            sh.rho = rho;
            sh.zcol = zcol;
            if (blockIdx.x == 0) {
                d.c[colj] = cj;
                d.s[colj] = sj;
                d.z[colj] = zcol;
                const int base = colj * (colj + 1) / 2;
                for (int i = 0; i < colj; ++i) d.R[base + i] = sh.h[i];
                d.R[base + colj] = rho;
                if (t.iter < d.hist_cap) d.hist[t.iter] = t.rnorm;
            }
          }
        }
        sh.T = t;
        if (blockIdx.x == 0) d.T[colj + 1] = t;
    }
    __syncthreads();
}

// Basis storage: four groups of eight basis vectors, each group a dense [row][8] array (64 B per row and group), so that
// reading the first j+1 entries of consecutive rows touches ceil((j+1)/8) fully used, fully contiguous streams.
//
// Large systems (split mode) use plain column-major storage instead, Vi[k * ldv + row] (ldv = n rounded up to 32): every
// kernel there is a thread-per-row stream, so column k is read by consecutive lanes contiguously, exactly the j+1 columns
// in use are read (the grouped layout always moves whole groups of 8), and the new column is written without partial lines.
__device__ __forceinline__ size_t vidx(int64_t row, int k, int64_t n, int64_t ldv) {
    return ldv ? (size_t)k * (size_t)ldv + (size_t)row
               : ((size_t)(k >> 3) * (size_t)n + (size_t)row) * 8 + (size_t)(k & 7);
}

__device__ __forceinline__ double precond_row(const GDev &d, int row) {
    return d.pkind == NPG_PRECOND_SCALAR ? d.pscalar : (d.pkind == NPG_PRECOND_DIAG ? d.pdiag[row] : 1.0);
}

// second Gram-Schmidt pass applied on the fly to the SpMV input: (wt - V h2)[c]  (rare path, see the header comment)
struct CorrectedX {
    const double *wt, *Vi, *h2;
    int nb;
    int64_t n, ldv;
    const float *Vf;
    __device__ __forceinline__ double operator()(int c) const {
        double v = wt[c];
        for (int k = 0; k < nb; ++k) v -= h2[k] * (Vf ? (double)Vf[vidx(c, k, n, ldv)] : Vi[vidx(c, k, n, ldv)]);
        return v;
    }
    __device__ __forceinline__ double2 two(int i) const { return make_double2((*this)(i), (*this)(i + 1)); }
    __device__ __forceinline__ double third(int i) const { return (*this)(i); }
};

// ---- R1: wt = P (b - A x), partial ||wt||^2 ---------------------------------------------------------------------------
template <int L, bool N9 = false>
__global__ void __launch_bounds__(kKB, 6) k_gmres_residual(GDev d) {
    __shared__ TileLds tl;
    __shared__ double sw[kTileRows];
    double *tmp = tl.prod;                // scratch for the final block reduction (the tile loop is over by then)
    const Snap c = *d.C;
    double acc = 0.0;
    if (c.done == 0) {
        TileDesc nd = d.tile_ptr[blockIdx.x < (unsigned)d.ntiles ? blockIdx.x : 0];
        for (int t = blockIdx.x; t < d.ntiles; t += gridDim.x) {
            const TileDesc td = nd;
            if (t + (int)gridDim.x < d.ntiles) nd = d.tile_ptr[t + gridDim.x];      // in flight during this tile
            const int r0 = td.r0, r1 = td.r0 + td.nrows;
            spmv_tile<kKB, L, PlainX, kTileNnz, 4, NoProf, false, false, N9>(d.A, PlainX{d.x}, td, tl, sw);
            const int r = threadIdx.x;
            if (r < r1 - r0) {
                const int row = r0 + r;
                const double res = precond_row(d, row) * (d.b[row] - sw[r]);
                d.wt[row] = res;
                if (d.xg.p) d.xg.p[d.xg.pos(row)] = (float)res;
                acc += res * res;
            }
        }
    }
    // every thread contributes to entry 0 of the partial row: fold the 32 lanes of a slot first
    acc = group_sum_dpp<kKP>(acc);
    store_partial_row((threadIdx.x & (kKP - 1)) == 0 ? acc : 0.0, tmp, d.PR);
}

// ---- K1 ---------------------------------------------------------------------------------------------------------------
// (the fused form serves small, latency-bound systems: it may take 128 registers, two workgroups per CU)
// Tiles [t0, t1).  The distributed split cycle launches it twice per step - the tiles without ghost columns while the halo
// exchange is in flight, the others behind it; the prologue is a pure function of state neither launch changes, so
// running it twice writes the same values twice.
// XG: the SpMV input is gathered from the fp32 gather-layout copy of wt (GDev::xg; no second Gram-Schmidt pass in that mode):
// 1 = node-blocked matrix (records), 2 = plain CSR matrix (the copy is then simply the vector in fp32: 4-byte gathers).
// N9: the matrix may hold FULL node records (spmv_device.h).
// WL > 0: the tiles come from the matrix's WINDOWED set (spmv_window.h; XG = 1 only): block tiles gather every distinct column
// once into LDS, WL lanes per node in their segmented sums; the tiles of the other rows are the ordinary ones.
// ORD: that set also holds ordinary tiles (rows behind the block rows with CSR entries, e.g. a rank's ghost columns); the instance
// without them carries less code through its register budget.
template <int L, bool FUSED, int XG = 0, bool N9 = false, int WL = 0, bool ORD = true>
__global__ void __launch_bounds__(kKB, FUSED ? 4 : 6) k_gmres_arnoldi(GDev d, int j, int t0, int t1) {
    static_assert(WL == 0 || (XG == 1 && !N9 && !FUSED), "windowed tiles serve the gather-layout instance of the split organisation");
    __shared__ KShared sh;
    __shared__ TileLds tl;
    __shared__ double sw[kTileRows];
    double *tmp = tl.prod;                // scratch of the prologue / final block reduction, outside the tile loop
    // (WL) the first tile's window is requested before the prologue: its two dependent round trips pass behind the Givens work
    using TD = std::conditional_t<WL != 0, WTileDesc, TileDesc>;
    const TD *__restrict__ tiles;
    if constexpr (WL != 0) tiles = d.wt_ptr; else tiles = d.tile_ptr;
    TD nd = tiles[t0 + (int)blockIdx.x < t1 ? t0 + (int)blockIdx.x : 0];
    WinPre pre;                  // (WL) a windowed tile's window, gathered during the tile before it
    bool have = false;
    if constexpr (WL != 0) {
        if (d.wpre && t0 + (int)blockIdx.x < t1 && nd.nw) {
            win_first<kKB>(d.W, PaddedX{d.xg}, nd, pre);
            have = true;
        }
    }
    if (j == 0) {
        const Snap c = *d.C;
        reduce_partials<kNS, kMaxI>(d.QR, d.nQR, 1, tmp, sh.red);
        if (threadIdx.x == 0) {
            Snap t = c;
            if (t.done == 0) {
                const double beta = sqrt(sh.red[0]);
                if (t.first) {
                    t.rnorm0 = beta;
                    t.rnorm = beta;
                    t.eps = d.prm->atol + d.prm->rtol * beta;
                    t.first = 0;
                    if (blockIdx.x == 0) d.hist[0] = beta;
                    if (beta == 0.0) t.done = 4;
                }
                t.beta = beta;
                t.zeta = beta;
                t.npass += 1;
            }
            t.inner = 0;
            sh.T = t;
            sh.reorth = 0;
            if (blockIdx.x == 0) d.T[0] = t;
        }
        __syncthreads();
    } else {
        finalize_column(d, j - 1, sh, tmp);
    }
    const Snap T = sh.T;
    if (T.done != 0) return;

    const int k = threadIdx.x & (kKP - 1), slot = threadIdx.x >> 5;
    const double inv_beta = 1.0 / T.beta;
    const bool ro = XG == 0 && sh.reorth != 0;        // (the gather-layout instance runs in fast mode: never a second pass)
    const double h2k = (ro && k < j) ? sh.h2[k] : 0.0;
    double acc = 0.0;
    for (int t = t0 + blockIdx.x; t < t1; t += gridDim.x) {
        const TD td = nd;
        if (t + (int)gridDim.x < t1) nd = tiles[t + gridDim.x];      // in flight during this tile
        const int r0 = td.r0, r1 = td.r0 + td.nrows;
        // split mode: this thread's row of wt for the epilogue, fetched now so that its latency hides behind the tile
        // (a tile has at most kTileRows <= kKB rows: one row per thread)
        static_assert(kTileRows <= kKB, "one epilogue row per thread");
        double wt_row = 0.0;
        // (vdots: the basis column is formed by the dots kernel - neither this load nor the column's store below)
        if (!FUSED && !d.vdots && (int)threadIdx.x < td.nrows) wt_row = d.wt[td.r0 + threadIdx.x];
        // one instantiation for both cases: without a second pass the correction loop has no trips
        if constexpr (WL != 0) {
            if (td.nw) {
                if (!have) win_first<kKB>(d.W, PaddedX{d.xg}, td, pre);
                have = t + (int)gridDim.x < t1 && nd.nw != 0;
                if (td.r0 < block_rows(d.A))
                    spmv_tile_win<kKB, WL>(d.A, d.W, PaddedX{d.xg}, td, nd, have, pre, tl, sw);
                else
                    spmv_tile_winrows<kKB, L>(d.A, d.W, PaddedX{d.xg}, td, nd, have, pre, tl, sw);
            } else if constexpr (ORD) {
                have = false;
                spmv_tile<kKB, L, PaddedX, kTileNnz, 2, NoProf, false, true, false>(d.A, PaddedX{d.xg}, ordinary(td), tl, sw);
                pre = WinPre{};          // (dead across the call above: nothing to keep in registers)
            }
        } else if constexpr (XG == 2)
            spmv_tile<kKB, L>(d.A, PaddedX{d.xg}, td, tl, sw);
        else if constexpr (XG == 1)
            // (node-blocked by definition: hardly any CSR entries - two pairs per lane there keep the records' loops inside the
            //  register budget)
            spmv_tile<kKB, L, PaddedX, kTileNnz, 2, NoProf, false, true, N9>(d.A, PaddedX{d.xg}, td, tl, sw);
        else
            spmv_tile<kKB, L, CorrectedX, kTileNnz, 4, NoProf, false, false, N9>(
                d.A, CorrectedX{d.wt, d.Vi, sh.h2, ro ? j : 0, d.n, d.ldv, d.Vf}, td, tl, sw);
        const int nr = r1 - r0;
        if (!FUSED) {
            // split mode (large systems): only what depends on the SpMV result; the dots stream in k_gmres_dots_rows
            const int r = threadIdx.x;
            if (r < nr) {
                const int row = r0 + r;
                d.w[row] = sw[r] * inv_beta * precond_row(d, row);
                if (!d.vdots) {
                    double tv = wt_row;
                    if (ro)
                        for (int q = 0; q < j; ++q)
                            tv -= sh.h2[q] * (d.Vf ? (double)d.Vf[vidx(row, q, d.n, d.ldv)] : d.Vi[vidx(row, q, d.n, d.ldv)]);
                    if (d.Vf)
                        d.Vf[vidx(row, j, d.n, d.ldv)] = (float)(tv * inv_beta);
                    else
                        d.Vi[vidx(row, j, d.n, d.ldv)] = tv * inv_beta;
                }
            }
            continue;
        }
        // 32 lanes per row (lane = basis index): new basis entry, w, and the partial dot products
        // (two rows per trip so that their independent loads overlap)
        for (int r = slot; r < nr; r += 2 * kNS) {
            const int rb = r + kNS;
            const bool hb = rb < nr;
            const int rowa = r0 + r, rowb = r0 + (hb ? rb : r);
            double va = (k < j) ? d.Vi[vidx(rowa, k, d.n, d.ldv)] : 0.0;
            double vb = (hb && k < j) ? d.Vi[vidx(rowb, k, d.n, d.ldv)] : 0.0;
            double ta = d.wt[rowa], tb = d.wt[rowb];
            const double wa = sw[r] * inv_beta * precond_row(d, rowa);
            const double wb = hb ? sw[rb] * inv_beta * precond_row(d, rowb) : 0.0;
            if (ro) {
                ta -= group_sum_dpp<kKP>(h2k * va);
                tb -= group_sum_dpp<kKP>(h2k * vb);
            }
            if (k == j) {
                va = ta * inv_beta;
                d.Vi[vidx(rowa, j, d.n, d.ldv)] = va;
                if (hb) {
                    vb = tb * inv_beta;
                    d.Vi[vidx(rowb, j, d.n, d.ldv)] = vb;
                }
            }
            if (k == 0) {
                d.w[rowa] = wa;
                if (hb) d.w[rowb] = wb;
            }
            acc += (k == kNormSlot) ? wa * wa + wb * wb : va * wa + vb * wb;
        }
    }
    if (FUSED) store_partial_row(acc, tmp, d.P1);
}

// ---- row-streaming kernels (split mode) -----------------------------------------------------------------------------------
// One thread per row, consecutive lanes = consecutive rows: every basis column in use is one coalesced 8-byte stream and
// every thread keeps 8*NG accumulators (NG = groups of eight columns, a template parameter).  On one GPU the fast instances' first-pass rows
// are folded to one row by k_gmres_fold_first and every other consumer reduces the partial rows itself (at most kMaxG rows);
// distributed runs fold them to one row first (k_reduce_rows) for the all-reduce.
constexpr int kRB = 256;
constexpr int kMaxRowsI = kMaxG / (kRB / 32);      // chunks of reduce_partials over at most kMaxG partial rows

// column-major layout: the j+1 columns in use, one coalesced 8-byte stream each (k <= j is wave-uniform)
template <int NG, typename BT>
__device__ __forceinline__ void load_row_cols(const BT *__restrict__ Vi, int64_t row, int64_t ldv, int j,
                                              double (&v)[8 * NG]) {
#pragma unroll
    for (int k = 0; k < 8 * NG; ++k) v[k] = (k <= j) ? (double)Vi[(size_t)k * (size_t)ldv + (size_t)row] : 0.0;
}
template <typename BT>
__device__ __forceinline__ const BT *basis_ptr(const GDev &d);
template <>
__device__ __forceinline__ const double *basis_ptr<double>(const GDev &d) { return d.Vi; }
template <>
__device__ __forceinline__ const float *basis_ptr<float>(const GDev &d) { return d.Vf; }

template <int NG>
__device__ __forceinline__ void store_partial_row_rows(const double (&acc)[8 * NG], double nrm, double *tmp, double *part) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane < kKP) tmp[wave * kKP + lane] = 0.0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8 * NG; ++k) {
        const double s = group_sum_dpp<64>(acc[k]);
        if (lane == 0 && k < kNormSlot) tmp[wave * kKP + k] = s;
    }
    const double sn = group_sum_dpp<64>(nrm);
    if (lane == 0) tmp[wave * kKP + kNormSlot] = sn;
    __syncthreads();
    if (threadIdx.x < kKP) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < kRB / 64; ++w) s += tmp[w * kKP + threadIdx.x];
        part[(size_t)blockIdx.x * kKP + threadIdx.x] = s;
    }
}

// (fp32-stored basis: two adjacent rows per thread, so that a lane still moves 8 bytes per column - with one row the loads
//  are 4-byte ones and the kernel is bound by their number, not by the bytes: measured slower than the fp64 basis)
template <int NG>
__device__ __forceinline__ void load_row_pair_cols(const float *__restrict__ Vf, int64_t r0, bool two, int64_t ldv, int j,
                                                   float2 (&v)[8 * NG]) {
    // straight-line 8-byte loads (k <= j is wave-uniform and the loop is unrolled; a lane-varying branch around the loads
    // would make hipcc wait for every one of them in turn).  r0 + 1 <= ldv - 1 always: the second element of the last pair of
    // an odd n lies in the column's padding and is zeroed after the load.
#pragma unroll
    for (int k = 0; k < 8 * NG; ++k) {
        float2 f = make_float2(0.f, 0.f);
        if (k <= j) f = *reinterpret_cast<const float2 *>(Vf + (size_t)k * (size_t)ldv + (size_t)r0);   // 8-byte aligned
        if (!two) f.y = 0.f;
        v[k] = f;                                                              // kept in fp32 registers, widened at use
    }
}
// One trip of the row-pair kernels: rows (r0, r0 + 1) of block `blk`, their basis entries and w.  A lane past the last row
// loads row 0 instead (no lane-varying branch around the loads) and gets zero weights.  The kernels issue trip t + 1's loads
// BEFORE trip t's arithmetic: with three waves per SIMD and one dependent round trip per loop trip the plain loop streamed at
// 3.9 TB/s, the software-pipelined one at 5.5-6.9 TB/s (tools/rows_bench.hip, profiles/r03_rows_bench.txt).
// VD (the dots kernel with GDev::vdots): column j does not exist yet - the trip loads the rows' wt pair instead (one more 16-byte
// load) and the kernel forms the column's entries from it.
template <int NG, bool VD = false>
struct RowPair {
    float2 v[8 * NG];
    double w0, w1;
    double2 t;            // (VD) wt of the two rows
    int64_t r0;
    bool valid, two;
    __device__ __forceinline__ void load(const GDev &d, int64_t blk, int j) {
        r0 = 2 * (blk * kRB + threadIdx.x);
        valid = r0 < d.n;
        two = r0 + 1 < d.n;
        const int64_t rc = valid ? r0 : 0;
        load_row_pair_cols<NG>(d.Vf, rc, two, d.ldv, VD ? j - 1 : j, v);
        const double2 ww = *reinterpret_cast<const double2 *>(d.w + rc);    // (w is padded: the pair of an odd n's last row)
        if constexpr (VD) t = *reinterpret_cast<const double2 *>(d.wt + rc);    // (so is wt)
        w0 = valid ? ww.x : 0.0;
        w1 = (valid && two) ? ww.y : 0.0;
    }
};

// VD: this launch also FORMS column j, v_j = (float)(wt / beta) - the expression and the rounding point of the Arnoldi kernel's
// epilogue, which then leaves the column alone (GDev::vdots) - stores it and takes its own j-th sum from the registers.
template <int NG, typename BT, bool VD = false>
__global__ void __launch_bounds__(kRB) k_gmres_dots_rows(GDev d, int j) {
    static_assert(!VD || sizeof(BT) == 4, "the column is formed by the row-pair kernel of the fp32-stored basis");
    __shared__ double tmp[(kRB / 64) * kKP];
    double acc[8 * NG];
#pragma unroll
    for (int k = 0; k < 8 * NG; ++k) acc[k] = 0.0;
    double nrm = 0.0;
    const Snap *Tj = d.T + j;
    if (Tj->done == 0) {
        if constexpr (sizeof(BT) == 4) {
            const int64_t nblk = ((int64_t)d.n + 2 * kRB - 1) / (2 * kRB);
            RowPair<NG, VD> cur, nxt;
            int64_t blk = blockIdx.x;
            if (blk < nblk) cur.load(d, blk, j);
            double inv_beta = 0.0;
            if constexpr (VD) inv_beta = 1.0 / Tj->beta;                     // (T[j]: written by the Arnoldi launch before this one)
            for (; blk < nblk; blk += gridDim.x) {
                const bool more = blk + gridDim.x < nblk;
                if (more) nxt.load(d, blk + gridDim.x, j);                   // in flight during this trip's arithmetic
                if constexpr (VD) {
                    float2 vj = make_float2((float)(cur.t.x * inv_beta), (float)(cur.t.y * inv_beta));
                    if (cur.valid) {
                        float *col = d.Vf + (size_t)j * (size_t)d.ldv + (size_t)cur.r0;
                        if (cur.two)
                            *reinterpret_cast<float2 *>(col) = vj;
                        else
                            *col = vj.x;
                    }
                    if (!cur.two) vj.y = 0.f;                                // (as load_row_pair_cols returns the other columns)
#pragma unroll
                    for (int k = 0; k < 8 * NG; ++k)
                        if (k == j) cur.v[k] = vj;                           // (wave-uniform)
                }
#pragma unroll
                for (int k = 0; k < 8 * NG; ++k) acc[k] += (double)cur.v[k].x * cur.w0 + (double)cur.v[k].y * cur.w1;
                nrm += cur.w0 * cur.w0 + cur.w1 * cur.w1;
                if (more) cur = nxt;
            }
        } else {
            for (int64_t row = blockIdx.x * (int64_t)kRB + threadIdx.x; row < d.n; row += (int64_t)gridDim.x * kRB) {
                double v[8 * NG];
                load_row_cols<NG, BT>(basis_ptr<BT>(d), row, d.ldv, j, v);          // split mode: the basis is column-major
                const double wv = d.w[row];
#pragma unroll
                for (int k = 0; k < 8 * NG; ++k) acc[k] += v[k] * wv;
                nrm += wv * wv;
            }
        }
    }
    store_partial_row_rows<NG>(acc, nrm, tmp, d.P1);
}

// FAST: wt = w - V h and ||wt||^2 (one pass over the columns, nothing kept).  Otherwise also h2 = V'wt for the selective
// second Gram-Schmidt pass.  The next Arnoldi kernel takes ||wt||^2 from Pythagoras and falls back on the sum formed here
// when that is close to cancellation.
template <int NG, bool FAST, typename BT>
__global__ void __launch_bounds__(kRB, (NG < 4 || FAST) ? 3 : 2) k_gmres_orth_rows(GDev d, int j) {
    __shared__ double tmp[(kRB / 32) * kKP];
    __shared__ double red[kKP];
    const Snap T = d.T[j];
    if (T.done != 0) {
        // the solve has ended: nothing to reduce and nothing to stream - the partial row reads as zeros, as it always did
        if (threadIdx.x < kKP) d.P2[(size_t)blockIdx.x * kKP + threadIdx.x] = 0.0;
        return;
    }
    // (fp32 basis, fast instance) the first trip's rows do not depend on h: their loads go out before the reduction below
    constexpr bool kPipe = sizeof(BT) == 4 && FAST;
    const int64_t nblk2 = ((int64_t)d.n + 2 * kRB - 1) / (2 * kRB);
    RowPair<kPipe ? NG : 1> cur;
    if constexpr (kPipe) {
        if ((int64_t)blockIdx.x < nblk2) cur.load(d, d.rev ? nblk2 - 1 - blockIdx.x : blockIdx.x, j);
    }
    // h1 = the dots kernel's partial rows summed in a fixed order by every workgroup (one GPU, full kernels), or a single row:
    // the one k_gmres_fold_first summed in that same order (one GPU, fast kernels) or the all-reduced one (several GPUs)
    reduce_partials<kRB / 32, kMaxRowsI>(d.Q1, d.nQ1, kKP, tmp, red);
    // h is wave-uniform: keep it in scalar registers (the kernel needs 16 NG vector registers for v and as many for acc)
    double h[8 * NG], acc[8 * NG];
#pragma unroll
    for (int k = 0; k < 8 * NG; ++k) {
        const double hv = (k <= j) ? red[k] : 0.0;
        const unsigned long long b = __double_as_longlong(hv);
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
        h[k] = __longlong_as_double(((unsigned long long)hi << 32) | lo);
        acc[k] = 0.0;
    }
    double nrm = 0.0;
    if (!d.onefold && blockIdx.x == 0 && threadIdx.x < kKP) {            // (onefold: the fold kernel has stored them)
        d.hcol1[j * kKP + threadIdx.x] = ((int)threadIdx.x <= j) ? red[threadIdx.x] : 0.0;
        if (threadIdx.x == 0) d.wnorm2[j] = red[kNormSlot];
    }
    if constexpr (kPipe) {
        const int64_t nblk = nblk2;
        RowPair<NG> nxt;
        for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
            const int64_t nb = blk + gridDim.x;
            const bool more = nb < nblk;
            if (more) nxt.load(d, d.rev ? nblk - 1 - nb : nb, j);        // in flight during this trip's arithmetic
            double p0 = cur.w0, p1 = cur.w1;
#pragma unroll
            for (int k = 0; k < 8 * NG; ++k) {
                p0 -= h[k] * (double)cur.v[k].x;
                p1 -= h[k] * (double)cur.v[k].y;
            }
            if (cur.valid) {
                if (cur.two)
                    *reinterpret_cast<double2 *>(d.wt + cur.r0) = make_double2(p0, p1);
                else
                    d.wt[cur.r0] = p0;
                if (d.xg.p) {
                    d.xg.p[d.xg.pos((int)cur.r0)] = (float)p0;
                    if (cur.two) d.xg.p[d.xg.pos((int)cur.r0 + 1)] = (float)p1;
                }
            } else {
                p0 = 0.0;                                               // (a clamped lane read row 0's basis entries)
                p1 = 0.0;
            }
            if (!cur.two) p1 = 0.0;
            nrm += p0 * p0 + p1 * p1;
            if (more) cur = nxt;
        }
    } else if constexpr (sizeof(BT) == 4) {       // full kernels: the second-pass sums leave no registers for a second trip
        const int64_t nblk = ((int64_t)d.n + 2 * kRB - 1) / (2 * kRB);
        for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
            const int64_t r0 = 2 * ((d.rev ? nblk - 1 - blk : blk) * kRB + threadIdx.x);
            if (r0 >= d.n) continue;
            const bool two = r0 + 1 < d.n;
            float2 v[8 * NG];
            load_row_pair_cols<NG>(d.Vf, r0, two, d.ldv, j, v);
            const double2 ww = *reinterpret_cast<const double2 *>(d.w + r0);
            double p0 = ww.x, p1 = two ? ww.y : 0.0;
#pragma unroll
            for (int k = 0; k < 8 * NG; ++k) {
                p0 -= h[k] * (double)v[k].x;
                p1 -= h[k] * (double)v[k].y;
            }
            if (two)
                *reinterpret_cast<double2 *>(d.wt + r0) = make_double2(p0, p1);
            else
                d.wt[r0] = p0;
            if (!FAST) {
#pragma unroll
                for (int k = 0; k < 8 * NG; ++k) acc[k] += (double)v[k].x * p0 + (double)v[k].y * p1;
            }
            nrm += p0 * p0 + p1 * p1;
        }
    } else {
    const int64_t nblk = ((int64_t)d.n + kRB - 1) / kRB;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t row = (d.rev ? nblk - 1 - blk : blk) * kRB + threadIdx.x;
        if (row >= d.n) continue;
        double v[8 * NG];
        load_row_cols<NG, BT>(basis_ptr<BT>(d), row, d.ldv, j, v);          // split mode: the basis is column-major
        double wp = d.w[row];
#pragma unroll
        for (int k = 0; k < 8 * NG; ++k) wp -= h[k] * v[k];
        d.wt[row] = wp;
        if (!FAST) {
#pragma unroll
            for (int k = 0; k < 8 * NG; ++k) acc[k] += v[k] * wp;
        }
        nrm += wp * wp;
    }
    }
    if (!FAST) {
        store_partial_row_rows<NG>(acc, nrm, tmp, d.P2);
    } else {
        // the exactly summed norm only: one wave reduction, zeros in the h2 slots
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        const double sn = group_sum_dpp<64>(nrm);
        __syncthreads();
        if (lane == 0) tmp[wave] = sn;
        __syncthreads();
        if (threadIdx.x < kKP) {
            double t = 0.0;
            if (threadIdx.x == kNormSlot)
                for (int w = 0; w < kRB / 64; ++w) t += tmp[w];
            d.P2[(size_t)blockIdx.x * kKP + threadIdx.x] = t;
        }
    }
}

// One GPU, fast kernels: the dots kernel's GP1 partial rows summed ONCE, by one workgroup between the two row kernels, instead of
// by every workgroup of the orthogonalisation kernel (768 x 196 KB of L2 reads and twelve dependent round trips per launch).
// The ORDER is that of reduce_partials<kRB / 32, kMaxRowsI>: slice s of 8 adds rows s, s + 8, ... upwards from 0.0, then the 8
// slice sums are added upwards from 0.0 - and the consumer's own pass over the one row adds exact zeros (a sum that starts at
// +0.0 is never -0.0) - so h, ||w||^2 and everything after them keep their bits.  Every load is issued before the first add.
__global__ void __launch_bounds__(kRB) k_gmres_fold_first(GDev d, int j, double *out) {
    constexpr int NS = kRB / 32;
    __shared__ double tmp[NS * kKP];
    const int done = d.T[j].done;
    const int k = threadIdx.x & (kKP - 1), slice = threadIdx.x >> 5;
    const int nrows = d.GP1;                                      // (1 <= GP1 <= kMaxG = NS * kMaxRowsI)
    double v[kMaxRowsI];
#pragma unroll
    for (int i = 0; i < kMaxRowsI; ++i) {
        const int b = slice + NS * i;
        v[i] = d.P1[(size_t)(b < nrows ? b : 0) * kKP + k];       // (clamped, not branched around: straight-line loads)
    }
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < kMaxRowsI; ++i) s += (slice + NS * i < nrows) ? v[i] : 0.0;
    tmp[slice * kKP + k] = s;
    __syncthreads();
    if (threadIdx.x < kKP && done == 0) {
        double t = 0.0;
#pragma unroll
        for (int sl = 0; sl < NS; ++sl) t += tmp[sl * kKP + threadIdx.x];
        out[threadIdx.x] = t;
        d.hcol1[j * kKP + threadIdx.x] = ((int)threadIdx.x <= j) ? t : 0.0;
        if (threadIdx.x == kNormSlot) d.wnorm2[j] = t;
    }
}

// ---- one resident launch for the Gram-Schmidt sums, their fold and the update (one GPU, fast kernels, fp32-stored basis) ----
// k_gmres_rows_fused<C> does, for a step of at most C <= kFusedMaxCols columns, the work of k_gmres_dots_rows<., float, true>,
// k_gmres_fold_first and k_gmres_orth_rows<., true, float> - same grid, same rows per thread, same partial rows, same orders of
// summation, so no bit of any result changes - and keeps what the update would read a second time on chip:
//   phase 1  the dots pass.  A thread's trips rotate through B register buffers (trip t lives in buffer t % B; trip t + B - 1 is
//            requested before trip t's arithmetic), so when the pass ends the registers still hold the thread's LAST B trips - the
//            basis entries, the freshly formed v_j among them, and the w pair.  The (up to) L trips before those are copied to
//            LDS as they leave their buffer.
//   hand-off the workgroup stores its partial row write-through and takes a ticket on the counter of its shard (blockIdx % 8).
//            The last arriver of shard s adds the rows s, s + 8, ... upwards from 0.0 - slice s of reduce_partials<kRB / 32,
//            kMaxRowsI> - and takes a ticket on the top counter; the last of those adds the eight slice sums upwards from 0.0,
//            stores the folded row, hcol1[j] and wnorm2[j], and publishes the generation.  One lane per workgroup polls it.
//   phase 2  the update, trips in ascending order: the early ones are read again from memory, then those in LDS, then the registers.
// Counters and generation only ever grow (a launch reads the generation E it starts from; its targets are (E + 1) x the number of
// arrivals), so a replayed graph needs no memset node.  Every workgroup must be resident: the host launches this kernel only on a
// grid the occupancy query admits (rows_fused_blocks_per_cu).  The poll is bounded by the wall clock: on expiry the workgroup sets
// the status word and leaves; a launch that finds it set does nothing; npg_gmres_solve reports it as an error.
// The instances of up to kFusedOnePassCols columns stream a trip's columns at once.  Two register buffers of 20 columns spill (168
// registers + 164 B of scratch), so the widest instance splits phase 1 by COLUMNS, not by trips:
//   pass a   streams columns [0, H) and w for all trips in ascending order and copies those entries of the last B trips to LDS;
//   pass b   streams columns [H, C), w and wt for all trips in ascending order, forms v_j (j >= H) as the one-pass loop does and
//            ends with the last B trips' entries of those columns and their w pair in registers.
// Every sum still takes its trips in ascending order and ||w||^2 is summed once (pass b), so the partial row keeps its bits; phase 2
// subtracts the columns of a kept trip in ascending order, [0, H) from LDS and [H, C) from the registers.  w is read once more.
constexpr int kFusedMaxCols = 20;
constexpr int kFusedOnePassCols = 16;
constexpr int kHoLine = 16;                      // 8-byte words per 128-byte line: every polled word has a line of its own
constexpr int kHoShards = kRB / 32;              // = the slices of reduce_partials<kRB / 32, kMaxRowsI>
struct RowsHandOff {
    unsigned long long gen[kHoLine];
    unsigned long long top[kHoLine];
    unsigned long long shard[kHoShards][kHoLine];
    unsigned long long status[kHoLine];
    double slice[kHoShards][kKP];
};
constexpr long long kHandOffTicks = 200000000;   // wall_clock64() counts at 100 MHz: two seconds, against a launch of ~50 us

// register buffers B and LDS trips L of the instance for C columns: B (2C + 8) + 2C registers in phase 1, L (8C + 16) bytes of LDS
// per thread (three workgroups per CU: 168 registers and ~53 KB).  H > 0: two passes, columns [0, H) in pass a - then the L = B trips
// in LDS are the SAME trips as those in registers (B (2 (C - H) + 8) + 2C registers in pass b, 8 L H bytes of LDS per thread)
template <int C> struct FusedGeom {
    static constexpr int B = C <= 8 ? 4 : C <= 12 ? 3 : 2, L = C <= 8 ? 2 : C <= kFusedOnePassCols ? 1 : 2;
    static constexpr int H = C <= kFusedOnePassCols ? 0 : C / 2;
};
constexpr int kFusedPassADepth = 3;              // register buffers of pass a (it keeps nothing in registers)
static_assert(kFusedMaxCols % 4 == 0, "instances come in steps of four columns");

#define NPG_LD_AGENT(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define NPG_ST_AGENT(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

template <int C, int K0 = 0>
struct RowTrip {
    float2 v[C];
    double w0, w1;
    // the loads of RowPair<., VD>::load, for the C columns from K0 on (VD: t = wt of the two rows, column j is not read)
    template <bool VD>
    __device__ __forceinline__ void load(const GDev &d, int64_t blk, int j, double2 &t) {
        const int64_t r0 = 2 * (blk * kRB + threadIdx.x);
        const bool valid = r0 < d.n, two = r0 + 1 < d.n;
        const int64_t rc = valid ? r0 : 0;
        const int jl = VD ? j - 1 : j;
#pragma unroll
        for (int k = 0; k < C; ++k) {
            float2 f = make_float2(0.f, 0.f);
            if (K0 + k <= jl) f = *reinterpret_cast<const float2 *>(d.Vf + (size_t)(K0 + k) * (size_t)d.ldv + (size_t)rc);
            if (!two) f.y = 0.f;
            v[k] = f;
        }
        const double2 ww = *reinterpret_cast<const double2 *>(d.w + rc);
        if constexpr (VD) t = *reinterpret_cast<const double2 *>(d.wt + rc);
        w0 = valid ? ww.x : 0.0;
        w1 = (valid && two) ? ww.y : 0.0;
    }
};

template <int C>
__global__ void __launch_bounds__(kRB, 3) k_gmres_rows_fused(GDev d, int j) {
    constexpr int B = FusedGeom<C>::B, L = FusedGeom<C>::L, H = FusedGeom<C>::H;
    constexpr bool kTwo = H > 0;                               // phase 1 in two passes over the columns
    constexpr int CB = C - H;                                  // columns [H, C) go through the register buffers
    static_assert(kMaxG == kHoShards * kMaxRowsI && kMaxRowsI % kHoShards == 0, "a shard is one slice of the fold");
    static_assert(!kTwo || L == B, "two passes: a kept trip has one half in LDS and the other in registers");
    __shared__ float2 lds_v[L * (kTwo ? H : C) * kRB];
    __shared__ double lds_w[kTwo ? 1 : L * 2 * kRB];           // (two passes: the w pair of a kept trip is in registers)
    __shared__ double tmp[(kRB / 32) * kKP];
    __shared__ double red[kKP];
    __shared__ int sh_role, sh_ok;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const Snap *Tj = d.T + j;
    if (Tj->done != 0) {
        // the solve has ended: both partial rows read as zeros, as the separate kernels leave them, and nobody waits
        if (tid < kKP) {
            d.P1[(size_t)blockIdx.x * kKP + tid] = 0.0;
            d.P2[(size_t)blockIdx.x * kKP + tid] = 0.0;
        }
        return;
    }
    RowsHandOff *ho = d.ho;
    if (NPG_LD_AGENT(&ho->status[0]) != 0) return;            // an earlier hand-off gave up: the host is about to report it
    unsigned long long E = 0;
    if (tid == 0) E = NPG_LD_AGENT(&ho->gen[0]);                // hand-offs completed so far (nobody adds to it before every
                                                                // workgroup of this launch has arrived, i.e. has read it)
    const int G = gridDim.x;
    const int64_t nblk = ((int64_t)d.n + 2 * kRB - 1) / (2 * kRB);
    const int nt = (int64_t)blockIdx.x < nblk ? (int)((nblk - 1 - blockIdx.x) / G) + 1 : 0;      // this workgroup's trips
    const int nreg = nt < B ? nt : B;                          // trips [nt - nreg, nt) end the pass in registers,
    const int nlds = kTwo ? 0 : (nt - nreg < L ? nt - nreg : L);      // [ne, ne + nlds) in LDS (two passes: half of the last nreg),
    const int ne = nt - nreg - nlds;                           // [0, ne) are read again
    auto blk_of = [&](int t) { return (int64_t)blockIdx.x + (int64_t)t * G; };

    // ---- phase 1: v_j, the sums and ||w||^2 ----
    RowTrip<CB, H> buf[B];
    double2 unused;
    double nrm = 0.0;
    {
        double acc[C];
#pragma unroll
        for (int k = 0; k < C; ++k) acc[k] = 0.0;
        if constexpr (kTwo) {
            // pass a: the sums of columns [0, H) (all of them stored: H <= j), trip after trip; the last nreg trips' entries to LDS
            constexpr int PA = kFusedPassADepth;
            RowTrip<H> ba[PA];
#pragma unroll
            for (int s = 0; s < PA - 1; ++s)
                if (s < nt) ba[s].template load<false>(d, blk_of(s), j, unused);
            for (int base = 0; base < nt; base += PA) {
#pragma unroll
                for (int s = 0; s < PA; ++s) {
                    const int t = base + s;
                    if (t < nt) {
                        if (t + PA - 1 < nt) ba[(s + PA - 1) % PA].template load<false>(d, blk_of(t + PA - 1), j, unused);
                        const RowTrip<H> &cur = ba[s];
#pragma unroll
                        for (int k = 0; k < H; ++k) acc[k] += (double)cur.v[k].x * cur.w0 + (double)cur.v[k].y * cur.w1;
                        if (t >= ne) {
#pragma unroll
                            for (int k = 0; k < H; ++k) lds_v[((t - ne) * H + k) * kRB + tid] = cur.v[k];
                        }
                    }
                }
            }
        }
        double2 tq[B];
        const double inv_beta = 1.0 / Tj->beta;                // (T[j]: written by the Arnoldi launch before this one)
#pragma unroll
        for (int s = 0; s < B - 1; ++s)
            if (s < nt) buf[s].template load<true>(d, blk_of(s), j, tq[s]);
        for (int base = 0; base < nt; base += B) {
#pragma unroll
            for (int s = 0; s < B; ++s) {
                const int t = base + s;
                if (t < nt) {
                    const int sp = (s + B - 1) % B;            // the buffer of trip t - 1, whose arithmetic is done
                    if (t + B - 1 < nt) {
                        if (!kTwo && t - 1 >= ne) {            // (then t - 1 < ne + nlds: trip t - 1 is not among the last B)
                            const int sl = t - 1 - ne;
#pragma unroll
                            for (int k = 0; k < C; ++k) lds_v[(sl * C + k) * kRB + tid] = buf[sp].v[k];
                            lds_w[(sl * 2 + 0) * kRB + tid] = buf[sp].w0;
                            lds_w[(sl * 2 + 1) * kRB + tid] = buf[sp].w1;
                        }
                        buf[sp].template load<true>(d, blk_of(t + B - 1), j, tq[sp]);      // in flight during this trip's arithmetic
                    }
                    RowTrip<CB, H> &cur = buf[s];
                    const int64_t r0 = 2 * (blk_of(t) * kRB + tid);
                    const bool valid = r0 < d.n, two = r0 + 1 < d.n;
                    float2 vj = make_float2((float)(tq[s].x * inv_beta), (float)(tq[s].y * inv_beta));
                    if (valid) {
                        float *col = d.Vf + (size_t)j * (size_t)d.ldv + (size_t)r0;
                        if (two)
                            *reinterpret_cast<float2 *>(col) = vj;
                        else
                            *col = vj.x;
                    }
                    if (!two) vj.y = 0.f;
#pragma unroll
                    for (int k = 0; k < CB; ++k)
                        if (H + k == j) cur.v[k] = vj;         // (wave-uniform)
#pragma unroll
                    for (int k = 0; k < CB; ++k) acc[H + k] += (double)cur.v[k].x * cur.w0 + (double)cur.v[k].y * cur.w1;
                    nrm += cur.w0 * cur.w0 + cur.w1 * cur.w1;
                }
            }
        }
        // the partial row of store_partial_row_rows (columns >= C sum to 0.0 there too), stored write-through
        __syncthreads();
        if (lane < kKP) tmp[wave * kKP + lane] = 0.0;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const double s = group_sum_dpp<64>(acc[k]);
            if (lane == 0) tmp[wave * kKP + k] = s;
        }
        const double sn = group_sum_dpp<64>(nrm);
        if (lane == 0) tmp[wave * kKP + kNormSlot] = sn;
        __syncthreads();
        if (tid < kKP) {
            double s = 0.0;
#pragma unroll
            for (int w = 0; w < kRB / 64; ++w) s += tmp[w * kKP + tid];
            NPG_ST_AGENT(d.P1 + (size_t)blockIdx.x * kKP + tid, s);
        }
    }

    // ---- hand-off ----
    // (the rows are stored by wave 0, which also signals: its own wait is all the ordering the ticket needs)
    const int shard = blockIdx.x % kHoShards;
    const int cnt = (G - shard + kHoShards - 1) / kHoShards;   // workgroups (= partial rows) of this shard
    const int nsh = G < kHoShards ? G : kHoShards;             // shards that have any
    if (wave == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (tid == 0) {
        const unsigned long long old = __hip_atomic_fetch_add(&ho->shard[shard][0], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sh_role = (old + 1 == (E + 1) * (unsigned long long)cnt) ? 1 : 0;
    }
    __syncthreads();
    if (sh_role == 1) {
        // last arriver of the shard: slice `shard` of the fold.  Thread (i, k) loads rows shard + 8 (8 m + i), m = 0 .. 11, all at
        // once; the 96 adds are made in row order by the threads k of the first group, eight rows per round through LDS
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        constexpr int M = kMaxRowsI / kHoShards;
        const int k = tid & (kKP - 1), i = tid >> 5;
        double v[M];
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const int q = m * kHoShards + i;
            const unsigned long long bits = NPG_LD_AGENT(reinterpret_cast<const unsigned long long *>(d.P1) +
                                                         (size_t)(q < cnt ? shard + kHoShards * q : shard) * kKP + k);
            v[m] = q < cnt ? __longlong_as_double(bits) : 0.0;
        }
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            __syncthreads();
            tmp[i * kKP + k] = v[m];
            __syncthreads();
            if (tid < kKP) {
#pragma unroll
                for (int ii = 0; ii < kHoShards; ++ii) s += tmp[ii * kKP + tid];
            }
        }
        if (tid < kKP) NPG_ST_AGENT(&ho->slice[shard][tid], s);
        if (wave == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (tid == 0) {
            const unsigned long long old = __hip_atomic_fetch_add(&ho->top[0], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (old + 1 == (E + 1) * (unsigned long long)nsh) sh_role = 2;
        }
        __syncthreads();
        if (sh_role == 2) {
            // last arriver of all: the eight slice sums upwards from 0.0, then the generation
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            if (tid < kKP) {
                double sv[kHoShards];
#pragma unroll
                for (int sl = 0; sl < kHoShards; ++sl) {
                    const unsigned long long bits = NPG_LD_AGENT(reinterpret_cast<const unsigned long long *>(&ho->slice[sl][tid]));
                    sv[sl] = sl < nsh ? __longlong_as_double(bits) : 0.0;
                }
                double tsum = 0.0;
#pragma unroll
                for (int sl = 0; sl < kHoShards; ++sl) tsum += sv[sl];
                NPG_ST_AGENT(const_cast<double *>(d.Q1) + tid, tsum);
                d.hcol1[j * kKP + tid] = (tid <= j) ? tsum : 0.0;
                if (tid == kNormSlot) d.wnorm2[j] = tsum;
            }
            if (wave == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (tid == 0) NPG_ST_AGENT(&ho->gen[0], E + 1);
        }
    }
    // the first early trip's rows do not depend on h: their loads go out before the wait
    RowTrip<C> early;
    if (ne > 0) early.template load<false>(d, blk_of(0), j, unused);
    if (tid == 0) {
        int ok = 1;
        const long long t0 = wall_clock64();
        while (NPG_LD_AGENT(&ho->gen[0]) < E + 1) {
            __builtin_amdgcn_s_sleep(8);
            if (wall_clock64() - t0 > kHandOffTicks) {
                NPG_ST_AGENT(&ho->status[0], 1ull);
                ok = 0;
                break;
            }
        }
        sh_ok = ok;
    }
    if (wave == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    if (!sh_ok) return;                                        // gave up: no update, the status word says so
    if (tid < kKP) {
        const unsigned long long bits = NPG_LD_AGENT(reinterpret_cast<const unsigned long long *>(d.Q1) + tid);
        red[tid] = __longlong_as_double(bits);
    }
    __syncthreads();

    // ---- phase 2: wt = w - V h, the gather copy and ||wt||^2 ----
    double h[C];
#pragma unroll
    for (int k = 0; k < C; ++k) {
        const double hv = (k <= j) ? red[k] : 0.0;
        const unsigned long long b = __double_as_longlong(hv);
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
        h[k] = __longlong_as_double(((unsigned long long)hi << 32) | lo);
    }
    nrm = 0.0;
    auto update = [&](const RowTrip<C> &cur, int t) {
        const int64_t r0 = 2 * (blk_of(t) * kRB + tid);
        const bool valid = r0 < d.n, two = r0 + 1 < d.n;
        double p0 = cur.w0, p1 = cur.w1;
#pragma unroll
        for (int k = 0; k < C; ++k) {
            // (opaque to the optimiser: it would otherwise keep phase 1's widened copies of the kept entries alive across the
            //  hand-off, twice the registers)
            float vx = cur.v[k].x, vy = cur.v[k].y;
            asm("" : "+v"(vx), "+v"(vy));
            p0 -= h[k] * (double)vx;
            p1 -= h[k] * (double)vy;
        }
        if (valid) {
            if (two)
                *reinterpret_cast<double2 *>(d.wt + r0) = make_double2(p0, p1);
            else
                d.wt[r0] = p0;
            if (d.xg.p) {
                d.xg.p[d.xg.pos((int)r0)] = (float)p0;
                if (two) d.xg.p[d.xg.pos((int)r0 + 1)] = (float)p1;
            }
        } else {
            p0 = 0.0;                                           // (a clamped lane read row 0's basis entries)
            p1 = 0.0;
        }
        if (!two) p1 = 0.0;
        nrm += p0 * p0 + p1 * p1;
    };
    for (int t = 0; t < ne; ++t) {
        update(early, t);                                       // (one buffer: the registers hold the last trips)
        if (t + 1 < ne) early.template load<false>(d, blk_of(t + 1), j, unused);
    }
#pragma unroll
    for (int sl = 0; sl < L; ++sl) {
        if (!kTwo && sl < nlds) {
#pragma unroll
            for (int k = 0; k < C; ++k) early.v[k] = lds_v[(sl * C + k) * kRB + tid];
            early.w0 = lds_w[(sl * 2 + 0) * kRB + tid];
            early.w1 = lds_w[(sl * 2 + 1) * kRB + tid];
            update(early, ne + sl);
        }
    }
    {
        const int tr = nt - nreg, rot = tr % B;                // the oldest trip in registers and its buffer
#pragma unroll
        for (int ro = 0; ro < B; ++ro) {
            if (ro == rot) {
#pragma unroll
                for (int r = 0; r < B; ++r) {
                    if (r >= nreg) continue;
                    if constexpr (kTwo) {                       // columns [0, H) as pass a left them in LDS slot r, then the registers
                        const RowTrip<CB, H> &kept = buf[(ro + r) % B];
#pragma unroll
                        for (int k = 0; k < H; ++k) early.v[k] = lds_v[(r * H + k) * kRB + tid];
#pragma unroll
                        for (int k = 0; k < CB; ++k) early.v[H + k] = kept.v[k];
                        early.w0 = kept.w0;
                        early.w1 = kept.w1;
                        update(early, tr + r);
                    } else {
                        update(buf[(ro + r) % B], tr + r);
                    }
                }
            }
        }
    }
    // the exactly summed norm only: one wave reduction, zeros in the h2 slots
    const double sn2 = group_sum_dpp<64>(nrm);
    __syncthreads();
    if (lane == 0) tmp[wave] = sn2;
    __syncthreads();
    if (tid < kKP) {
        double tt = 0.0;
        if (tid == kNormSlot)
            for (int w = 0; w < kRB / 64; ++w) tt += tmp[w];
        d.P2[(size_t)blockIdx.x * kKP + tid] = tt;
    }
}

// ---- K2 ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kKB, 6) k_gmres_orth(GDev d, int j) {
    __shared__ KShared sh;
    __shared__ double tmp[kNS * kKP];
    const Snap T = d.T[j];
    reduce_partials<kNS, kMaxI>(d.Q1, d.nQ1, kKP, tmp, sh.red);      // [0..j] = h1, [31] = ||w||^2
    if (T.done != 0) return;
    const int k = threadIdx.x & (kKP - 1), slot = threadIdx.x >> 5;
    if (blockIdx.x == 0 && threadIdx.x < kKP) {
        d.hcol1[j * kKP + threadIdx.x] = ((int)threadIdx.x <= j) ? sh.red[threadIdx.x] : 0.0;
        if (threadIdx.x == 0) d.wnorm2[j] = sh.red[kNormSlot];
    }
    const double hk = (k <= j) ? sh.red[k] : 0.0;
    double acc = 0.0;
    // two rows per trip: their loads are independent, so both are in flight before the first DPP sum
    const int64_t stride = (int64_t)gridDim.x * kNS;
    for (int64_t row = (int64_t)blockIdx.x * kNS + slot; row < d.n; row += 2 * stride) {
        const int64_t rowb = row + stride;
        const bool hb = rowb < d.n;
        const double va = (k <= j) ? d.Vi[vidx(row, k, d.n, d.ldv)] : 0.0;
        const double vb = (hb && k <= j) ? d.Vi[vidx(rowb, k, d.n, d.ldv)] : 0.0;
        const double wa = d.w[row];
        const double wb = hb ? d.w[rowb] : 0.0;
        const double pa = wa - group_sum_dpp<kKP>(hk * va);
        const double pb = wb - group_sum_dpp<kKP>(hk * vb);
        if (k == 0) {
            d.wt[row] = pa;
            if (hb) d.wt[rowb] = pb;
        }
        acc += (k == kNormSlot) ? pa * pa + pb * pb : va * pa + vb * pb;
    }
    store_partial_row(acc, tmp, d.P2);
}

// ---- XU ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kKB, 6) k_gmres_update(GDev d) {
    __shared__ KShared sh;
    __shared__ double tmp[kNS * kKP];
    __shared__ double Rl[kKP * (kKP + 1) / 2];
    const double zv = d.z[threadIdx.x & (kKP - 1)];
    finalize_column(d, d.mem - 1, sh, tmp);     // no-op copy if the pass already ended
    const Snap T = sh.T;
    const int kk = T.inner;
    // The last column (R entries, rotated z) was finalised inside THIS launch by every workgroup redundantly: take it
    // from shared memory, never from the global copies workgroup 0 is writing concurrently.
    const bool fin = sh.fin != 0;
    const int last = d.mem - 1;
    // stage the packed upper-triangular R (column c starts at c(c+1)/2) in LDS with one parallel load
    for (int t = threadIdx.x; t < kk * (kk + 1) / 2; t += kKB) Rl[t] = d.R[t];
    __syncthreads();
    if (fin && threadIdx.x <= (unsigned)last && kk == d.mem)
        Rl[last * (last + 1) / 2 + threadIdx.x] = ((int)threadIdx.x == last) ? sh.rho : sh.h[threadIdx.x];
    __syncthreads();
    if (threadIdx.x < 64) {
        // column-oriented back substitution in wave 0: lane r owns y_r; step c broadcasts y_c and updates the rows above
        const int lane = threadIdx.x;
        double y = (lane < kk) ? ((fin && lane == last) ? sh.zcol : zv) : 0.0;
        const double btol = d.prm->btol;
        for (int c = kk - 1; c >= 0; --c) {
            const double rcc = Rl[c * (c + 1) / 2 + c];
            double yc = __shfl(y, c, 64);
            yc = (fabs(rcc) <= btol) ? 0.0 : yc / rcc;
            if (lane == c) y = yc;
            if (lane < c) y -= Rl[c * (c + 1) / 2 + lane] * yc;
        }
        if (lane < kKP) sh.y[lane] = (lane < kk) ? y : 0.0;
        if (blockIdx.x == 0 && lane == 0) {
            *d.C = sh.T;            // (no local Snap copy: it would live in scratch)
            d.C->inner = 0;
        }
    }
    __syncthreads();
    if (kk == 0) return;
    if (d.ldv && d.Vf) {
        // column-major fp32 basis: two adjacent rows per thread (8-byte loads, as the other row kernels), every column in use
        // requested before the first is needed; kk <= kKP - 1 is wave-uniform
        const int64_t nblk = ((int64_t)d.n + 2 * kKB - 1) / (2 * kKB);
        for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
            const int64_t r0 = 2 * (blk * kKB + threadIdx.x);
            if (r0 >= d.n) continue;
            const bool two = r0 + 1 < d.n;
            double2 xx = make_double2(d.x[r0], two ? d.x[r0 + 1] : 0.0);
            for (int q0 = 0; q0 < kk; q0 += 16) {          // sixteen columns requested at a time (register budget: 80)
                float2 f[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    f[q] = make_float2(0.f, 0.f);
                    if (q0 + q < kk) f[q] = *reinterpret_cast<const float2 *>(d.Vf + (size_t)(q0 + q) * (size_t)d.ldv + (size_t)r0);
                }
#pragma unroll
                for (int q = 0; q < 16; ++q)
                    if (q0 + q < kk) {
                        xx.x += sh.y[q0 + q] * (double)f[q].x;
                        xx.y += sh.y[q0 + q] * (double)f[q].y;
                    }
            }
            d.x[r0] = xx.x;
            if (two) d.x[r0 + 1] = xx.y;
        }
        return;
    }
    if (d.ldv) {
        // column-major basis: one thread per row, kk coalesced column streams
        for (int64_t row = (int64_t)blockIdx.x * kKB + threadIdx.x; row < d.n; row += (int64_t)gridDim.x * kKB) {
            double s = 0.0;
#pragma unroll 4
            for (int q = 0; q < kk; ++q)
                s += sh.y[q] * (d.Vf ? (double)d.Vf[(size_t)q * (size_t)d.ldv + (size_t)row] : d.Vi[(size_t)q * (size_t)d.ldv + (size_t)row]);
            d.x[row] += s;
        }
        return;
    }
    const int k = threadIdx.x & (kKP - 1), slot = threadIdx.x >> 5;
    const double yk = sh.y[k];             // zero for k >= kk
    for (int64_t row = (int64_t)blockIdx.x * kNS + slot; row < d.n; row += (int64_t)gridDim.x * kNS) {
        const double vk = (k < kk) ? d.Vi[vidx(row, k, d.n, d.ldv)] : 0.0;
        const double s = group_sum_dpp<kKP>(yk * vk);
        if (k == 0) d.x[row] += s;
    }
}

// distributed mode: fold this rank's partial rows into one row, which RCCL then sums over the ranks
__global__ void __launch_bounds__(1024) k_reduce_rows(const double *__restrict__ part, int nrows, double *out) {
    __shared__ double tmp[32 * kKP];
    const int k = threadIdx.x & (kKP - 1), slice = threadIdx.x >> 5;      // 32 slices of 32 lanes
    double s = 0.0;
    for (int b0 = slice; b0 < nrows; b0 += 32 * 8) {
        double v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int b = b0 + 32 * i;
            v[i] = b < nrows ? part[(size_t)b * kKP + k] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) s += v[i];
    }
    tmp[slice * kKP + k] = s;
    __syncthreads();
    if (threadIdx.x < kKP) {
        double t = 0.0;
#pragma unroll
        for (int sl = 0; sl < 32; ++sl) t += tmp[sl * kKP + threadIdx.x];
        out[threadIdx.x] = t;
    }
}

}  // namespace npg

using namespace npg;

// npg_gmres_last_config: entries of the report, in this order (nupgcm_amd/iterative_solvers.py names them)
constexpr int kCfgLen = 18;

// The environment switches that are read ONCE per process, by the first solve (DESIGN.md 4.2 lists every switch; NPG_GMRES_ONEFOLD,
// NPG_GMRES_FUSEDROWS, NPG_GMRES_FUSED_COLS and NPG_HALO_OVERLAP_VERBOSE are read at every solve, where they are used)
struct GmresKnobs {
    int split = env_int("NPG_GMRES_SPLIT", -1);
    int basis = env_int("NPG_GMRES_BASIS", 0);
    int pyth = env_int("NPG_GMRES_PYTH", 1);
    int lazy2 = env_int("NPG_GMRES_LAZY2", 1);
    int fast = env_int("NPG_GMRES_FAST", 1);
    int rev = env_int("NPG_ORTH_REVERSE", 0);
    int rows_wg = std::max(64, env_int("NPG_GMRES_ROWS_WG", kMaxG));      // (tuning: fewer partial rows for the next prologue to fold)
    int xg = env_int("NPG_GMRES_XG", 1);
    int xg_csr = env_int("NPG_GMRES_XG_CSR", -1);
    int window = env_int("NPG_GMRES_WINDOW", 1);
    int win_ord = env_int("NPG_WIN_ORD", 0);
    int win_pre = env_int("NPG_WIN_PRE", 1);
    // a traced process launches eagerly unless told otherwise (profiler_attached(), common.h: why); =0 forces graph replay there
    int eager = env_int("NPG_GMRES_EAGER", profiler_attached());
    int trace = env_int("NPG_GMRES_TRACE", 0);
    int dist_graph = env_int("NPG_DIST_GRAPH", -1);
    int overlap = env_int("NPG_HALO_OVERLAP", -1);
    int overlap_unverified = env_int("NPG_HALO_OVERLAP_UNVERIFIED", 0);
    int64_t overlap_min_ghosts = env_int64("NPG_HALO_OVERLAP_MIN_GHOSTS", 200000);
    int reserve_cus = env_int("NPG_HALO_RESERVE_CUS", 4);
    GmresKnobs() {
        if (eager && profiler_attached() && !getenv("NPG_GMRES_EAGER"))
            fprintf(stderr, "[npg] rocprofv3 detected: GMRES restart cycles are launched eagerly instead of replayed from hipGraphs "
                            "(rocprofiler-sdk faults on graph launches that wrap the AQL ring; NPG_GMRES_EAGER=0 overrides)\n");
    }
};

// What one solve launches: the kernels' argument block and everything else the launches of a cycle depend on.  Host only.  The captured
// cycle graphs bake all of it in, so the whole plan is their cache key - compared with memcmp: gmres_plan zeroes it with memset first.
struct GmresPlan {
    GDev d;
    int lanes;                  // lane instance of the products with the matrix (npg_csr::lanes - npg_csr_set_lanes changes it)
    int dist;                   // distributed cycle: halo exchanges, partial rows folded to one row and summed over the ranks
    int kernel_only;            // ... on a transport whose in-cycle calls only launch kernels (the peer windows)
    int use_graph;              // the cycles replay from the captured graphs (0: every cycle is launched eagerly)
    int a_nt, a_int;            // tiles of the Arnoldi launches / those of them without ghost columns, which come first
    int grid;                   // workgroups of a step's one Arnoldi launch
    int overlap;                // distributed split cycle: the interior tiles run beside the halo exchange, the others behind it
    int reserve;                // ... CUs that the interior launch leaves free (RCCL)
    int grid_int, grid_bnd;     // ... workgroups of the interior and of the boundary launch
    int64_t xg_floats;          // floats of the gather-layout copy GDev::xg (0: the copy is not used)
    int fused_cols;             // steps of up to this many columns (j < fused_cols) take the fused row launch (0: none does)
};

struct npg_gmres {
    npg_ctx *ctx = nullptr;
    int64_t n = 0;
    int mem = 20;
    double *Vi = nullptr, *w = nullptr, *wt = nullptr;
    double *P1 = nullptr, *P2 = nullptr, *PR = nullptr;
    Snap *C = nullptr, *T = nullptr;
    double *c = nullptr, *s = nullptr, *z = nullptr, *R = nullptr, *hcol1 = nullptr, *wnorm2 = nullptr;
    double *hist = nullptr;
    int hist_cap = 0;
    GParams *prm = nullptr;
    Snap *h_C = nullptr;          // pinned, two slots (one per graph of the ping-pong pair)
    GParams *h_prm = nullptr;     // pinned
    int64_t hist_len = 0;
    // graph cache: two instances of the cycle graph that differ only in where the carried state is copied for the host,
    // so that cycle c+1 can be enqueued before the host has looked at the outcome of cycle c
    hipGraph_t graph[2] = {nullptr, nullptr};
    hipGraphExec_t exec[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    GmresPlan key;                // the plan those graphs were captured for
    bool have_graph = false;
    // profile mode: eager launches with HIP events around every Arnoldi (SpMV) kernel
    bool profile = false;
    bool explicit_norm = false;   // distributed: a solve met cancellation in the Pythagorean norm
    bool safe_mode = false;       // one GPU: a solve in fast mode met a column that was due a second Gram-Schmidt pass
    int split_mode = -1;
    int basis_bits = 0;           // stored Krylov basis of the split organisation: 64, 32, or 0 = by tolerance (npg_gmres_set_basis)
    int halo_overlap = -1;        // distributed split cycle: interior tiles beside the halo exchange: -1 = default (on with the
                                  // peer windows, off with RCCL), 0 / 1 = npg_gmres_set_dist_options
    int dist_graph = -1;          // distributed cycles replayed from a hipGraph: -1 = default (on for the kernel-only peer
                                  // transport, off with RCCL calls in the cycle), 0 = off, 1 = on
    std::vector<hipEvent_t> pev;
    double prof_ms = 0.0;
    int64_t prof_launches = 0;
    int gather32 = -1;            // SpMV input of the Arnoldi kernel from the fp32 gather-layout copy: -1 = default (on where it
                                  // applies), 0 = off, 1 = on where it applies (npg_gmres_set_gather)
    float *xg = nullptr;          // wt in fp32 gather layout (GDev::xg), allocated on first use
    int64_t xg_len = 0;
    int xg_key[3] = {-1, -1, -1}; // (nfull, nsurf, columns) the pads of xg were zeroed for
    npg_halo *halo = nullptr;
    double *Rg = nullptr;         // 3 x 32 doubles: all-reduced rows (distributed mode)
    int64_t n_ghost = 0;
    RowsHandOff *ho = nullptr;    // hand-off state of k_gmres_rows_fused (allocated and zeroed on first use)
    unsigned long long *h_ho = nullptr;   // pinned, two slots: its status word as each cycle left it
    int fused_blocks[2] = {-1, -1};   // workgroups of that kernel per CU (rows_fused_blocks_per_cu), -1: not asked yet:
                                  // [0] over the one-pass instances, [1] over all of them
    int fused_cols = 0;           // GmresPlan::fused_cols of the last solve's plan (npg_gmres_fused_cols)
    bool fused_off = false;       // a hand-off has timed out: the workspace keeps to the separate launches
    int32_t cfg[kCfgLen] = {};    // the kernel instances the last solve launched (npg_gmres_last_config)
    bool have_cfg = false;
};

// distributed cycle: fold one set of partial rows into a single row and sum it over the ranks (peer transport: fold + exchange in ONE kernel)
static int fold_rows(npg_gmres *ws, const double *part, int nrows, int slot, hipStream_t st) {
    return fold_allreduce_rows(ws->ctx, part, nrows, ws->Rg + slot * kKP, st);
}

template <int NG, typename BT>
static void launch_rows_bt(const GDev &d, int j, hipStream_t st, bool orth) {
    if (orth && d.fast)
        hipLaunchKernelGGL((k_gmres_orth_rows<NG, true, BT>), dim3(d.GR), dim3(kRB), 0, st, d, j);
    else if (orth)
        hipLaunchKernelGGL((k_gmres_orth_rows<NG, false, BT>), dim3(d.GR), dim3(kRB), 0, st, d, j);
    else
        hipLaunchKernelGGL((k_gmres_dots_rows<NG, BT>), dim3(d.GR), dim3(kRB), 0, st, d, j);
}
template <int NG>
static void launch_rows(const GDev &d, int j, hipStream_t st, bool orth) {
    if (d.Vf && d.vdots && !orth)
        hipLaunchKernelGGL((k_gmres_dots_rows<NG, float, true>), dim3(d.GR), dim3(kRB), 0, st, d, j);
    else if (d.Vf)
        launch_rows_bt<NG, float>(d, j, st, orth);
    else
        launch_rows_bt<NG, double>(d, j, st, orth);
}

static void launch_rows_kernel(const GDev &d, int j, hipStream_t st, bool orth) {
    switch ((j + 8) / 8) {       // groups of 8 basis vectors needed for j+1 vectors
        case 1: launch_rows<1>(d, j, st, orth); break;
        case 2: launch_rows<2>(d, j, st, orth); break;
        case 3: launch_rows<3>(d, j, st, orth); break;
        default: launch_rows<4>(d, j, st, orth); break;
    }
}

static void launch_rows_fused(const GDev &d, int j, hipStream_t st) {
    switch ((j + 4) / 4) {       // instances for 4, 8, ... kFusedMaxCols columns
        case 1: hipLaunchKernelGGL(k_gmres_rows_fused<4>, dim3(d.GR), dim3(kRB), 0, st, d, j); break;
        case 2: hipLaunchKernelGGL(k_gmres_rows_fused<8>, dim3(d.GR), dim3(kRB), 0, st, d, j); break;
        case 3: hipLaunchKernelGGL(k_gmres_rows_fused<12>, dim3(d.GR), dim3(kRB), 0, st, d, j); break;
        case 4: hipLaunchKernelGGL(k_gmres_rows_fused<16>, dim3(d.GR), dim3(kRB), 0, st, d, j); break;
        default: hipLaunchKernelGGL(k_gmres_rows_fused<20>, dim3(d.GR), dim3(kRB), 0, st, d, j); break;
    }
}
// Workgroups of k_gmres_rows_fused that one CU holds at a time, over the instances: the occupancy query's answer, corrected as it
// has to be for 256-thread workgroups on gfx950 - min(API, 8, floor(800 / (ceil(sgpr / 16) 16 + 16))) - with the largest scalar
// register count a kernel can have (every instance is reported at 106, profiles/gmres_fusedrows_ab.txt), so the bound errs low.  0: unknown.
template <int C>
static int rows_fused_blocks() {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_gmres_rows_fused<C>, kRB, 0) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return nb;
}
// `cols`: the widest instance a cycle will launch (kFusedOnePassCols or kFusedMaxCols) - the minimum is over the instances up to it.
static int rows_fused_blocks_per_cu(int cols) {
    constexpr int kSgprMax = 112;
    int api = std::min({rows_fused_blocks<4>(), rows_fused_blocks<8>(), rows_fused_blocks<12>(), rows_fused_blocks<16>()});
    if (cols > kFusedOnePassCols) api = std::min(api, rows_fused_blocks<20>());
    return std::min({api, 8, 800 / ((kSgprMax + 15) / 16 * 16 + 16)});
}

// the Arnoldi kernel instance for this matrix / input form: tiles [t0, t1) on `grid` workgroups
template <int L>
static void launch_arnoldi_split(const GDev &d, int grid, int j, int t0, int t1, hipStream_t st, hipEvent_t e0 = nullptr,
                                 hipEvent_t e1 = nullptr) {
    const dim3 g(std::max(1, grid)), b(kKB);
    // profile mode: e0 / e1 are the LAUNCH'S OWN start and stop events (hipExtLaunchKernelGGL: the dispatch packet's timestamps, what
    // rocprofv3's kernel trace reports) - events recorded before and after the launch also time the two marker packets, 4-6 us
#define NPG_ARNOLDI(...)                                                                          \
    do {                                                                                          \
        if (e0) hipExtLaunchKernelGGL((__VA_ARGS__), g, b, 0, st, e0, e1, 0, d, j, t0, t1);       \
        else hipLaunchKernelGGL((__VA_ARGS__), g, b, 0, st, d, j, t0, t1);                        \
    } while (0)
    if (d.A.pk9) {
        if (d.xg.p)
            NPG_ARNOLDI(k_gmres_arnoldi<L, false, 1, true>);
        else
            NPG_ARNOLDI(k_gmres_arnoldi<L, false, 0, true>);
    } else if (d.xg.p && d.xg.nbr == 0) {
        NPG_ARNOLDI(k_gmres_arnoldi<L, false, 2>);
    } else if (d.xg.p && d.wt_ptr) {
        if (d.wl == 8 && !d.word)
            NPG_ARNOLDI(k_gmres_arnoldi<L, false, 1, false, 8, false>);
        else if (d.wl == 8)
            NPG_ARNOLDI(k_gmres_arnoldi<L, false, 1, false, 8, true>);
        else if (!d.word)
            NPG_ARNOLDI(k_gmres_arnoldi<L, false, 1, false, 4, false>);
        else
            NPG_ARNOLDI(k_gmres_arnoldi<L, false, 1, false, 4, true>);
    } else if (d.xg.p) {
        NPG_ARNOLDI(k_gmres_arnoldi<L, false, 1>);
    } else {
        NPG_ARNOLDI(k_gmres_arnoldi<L, false>);
    }
#undef NPG_ARNOLDI
}
template <int L>
static void launch_residual_L(const GDev &d, hipStream_t st) {
    if (d.A.pk9)
        hipLaunchKernelGGL((k_gmres_residual<L, true>), dim3(d.G1), dim3(kKB), 0, st, d);
    else
        hipLaunchKernelGGL((k_gmres_residual<L>), dim3(d.G1), dim3(kKB), 0, st, d);
}

// the lane instance (npg_csr::lanes: 4, 8, 16, otherwise 32) as a type: f(std::integral_constant<int, L>())
template <class F>
static auto with_lanes(int lanes, F f) {
    switch (lanes) {
        case 4: return f(std::integral_constant<int, 4>());
        case 8: return f(std::integral_constant<int, 8>());
        case 16: return f(std::integral_constant<int, 16>());
        default: return f(std::integral_constant<int, 32>());
    }
}

// One restart cycle as the plan has it and, behind it, its outcome for the host into result slot `slot`: the carried state and,
// with the fused row kernel, the status word of its hand-off.
template <int L>
static int launch_cycle_L(const GmresPlan &p, hipStream_t st, hipEvent_t *pev, npg_gmres *ws, int slot) {
    const GDev &d = p.d;
    const bool dist = p.dist;
    int rc = NPG_OK;
    // distributed + gather-layout input: the ghosts of wt are also stored as floats behind the owned part of the copy
    float *g32 = (dist && d.xg.p) ? d.xg.p + d.xg.pos(d.n) : nullptr;
    for (int j = 0; j < d.mem; ++j) {
        if (p.overlap) {
            if ((rc = halo_exchange_async(ws->halo, d.wt, g32, d.gslot, d.xg.p))) return rc;
            if (pev) hipEventRecord(pev[2 * j], st);
            launch_arnoldi_split<L>(d, p.grid_int, j, 0, p.a_int, st);
            if ((rc = halo_exchange_wait(ws->halo))) return rc;
            launch_arnoldi_split<L>(d, p.grid_bnd, j, p.a_int, p.a_nt, st);
            if (pev) hipEventRecord(pev[2 * j + 1], st);
            launch_rows_kernel(d, j, st, false);
        } else {
        if (dist && (rc = halo_exchange_raw(ws->halo, d.wt, g32, d.gslot, d.xg.p))) return rc;
        if (d.split) {
            launch_arnoldi_split<L>(d, p.grid, j, 0, p.a_nt, st, pev ? pev[2 * j] : nullptr, pev ? pev[2 * j + 1] : nullptr);
            if (j < p.fused_cols) {
                launch_rows_fused(d, j, st);     // sums, fold and update in one resident launch
                continue;
            }
            launch_rows_kernel(d, j, st, false);
            if (d.onefold) hipLaunchKernelGGL(k_gmres_fold_first, dim3(1), dim3(kRB), 0, st, d, j, const_cast<double *>(d.Q1));
        } else {
            if (pev) hipEventRecord(pev[2 * j], st);
            hipLaunchKernelGGL((k_gmres_arnoldi<L, true>), dim3(p.grid), dim3(kKB), 0, st, d, j, 0, d.ntiles);
            if (pev) hipEventRecord(pev[2 * j + 1], st);
        }
        }
        if (dist && (rc = fold_rows(ws, d.P1, d.GP1, 0, st))) return rc;
        if (d.split)
            launch_rows_kernel(d, j, st, true);
        else
            hipLaunchKernelGGL(k_gmres_orth, dim3(d.G2), dim3(kKB), 0, st, d, j);
        if (dist && !d.pyth && (rc = fold_rows(ws, d.P2, d.GP2, 1, st))) return rc;
    }
    hipLaunchKernelGGL(k_gmres_update, dim3(d.G2), dim3(kKB), 0, st, d);
    if (dist && (rc = halo_exchange_raw(ws->halo, d.x))) return rc;
    launch_residual_L<L>(d, st);
    if (dist && (rc = fold_rows(ws, d.PR, d.G1, 2, st))) return rc;
    NPG_HIP(hipMemcpyAsync(ws->h_C + slot, ws->C, sizeof(Snap), hipMemcpyDeviceToHost, st));
    if (d.fusedrows) NPG_HIP(hipMemcpyAsync(ws->h_ho + slot, d.ho->status, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    return rc;
}

static int launch_cycle(const GmresPlan &p, hipStream_t st, hipEvent_t *pev, npg_gmres *ws, int slot) {
    return with_lanes(p.lanes, [&](auto lanes) { return launch_cycle_L<decltype(lanes)::value>(p, st, pev, ws, slot); });
}

NPG_API int npg_gmres_create(npg_ctx *ctx, int64_t n, int memory, npg_gmres **out) {
    NPG_REQUIRE(ctx && out && n > 0, "npg_gmres_create: bad argument");
    NPG_REQUIRE(memory >= 1 && memory <= kMaxMem, "npg_gmres_create: memory must be in [1,%d]", kMaxMem);
    NPG_REQUIRE(n < INT32_MAX / kKP, "npg_gmres_create: n exceeds the int32 indexing of the interleaved basis");
    npg_gmres *ws = new npg_gmres();
    ws->ctx = ctx;
    ws->n = n;
    ws->mem = memory;
    NPG_HIP(hipSetDevice(ctx->device));
    const size_t vb = ((size_t)n + 2) * sizeof(double);          // (+2: the row kernels of the fp32-stored basis read rows in pairs)
    const size_t vbytes = ((size_t)n + 32) * sizeof(double) * kKP;     // either layout: 32 columns of n (+ padding) doubles
    NPG_HIP(hipMalloc((void **)&ws->Vi, vbytes));
    NPG_HIP(hipMalloc((void **)&ws->w, vb));
    NPG_HIP(hipMalloc((void **)&ws->wt, vb));
    const size_t pb = (size_t)kMaxRows * kKP * sizeof(double);
    NPG_HIP(hipMalloc((void **)&ws->P1, pb));
    NPG_HIP(hipMalloc((void **)&ws->P2, pb));
    NPG_HIP(hipMalloc((void **)&ws->PR, pb));
    NPG_HIP(hipMalloc((void **)&ws->C, sizeof(Snap)));
    NPG_HIP(hipMalloc((void **)&ws->T, sizeof(Snap) * (memory + 1)));
    NPG_HIP(hipMalloc((void **)&ws->c, sizeof(double) * kKP));
    NPG_HIP(hipMalloc((void **)&ws->s, sizeof(double) * kKP));
    NPG_HIP(hipMalloc((void **)&ws->z, sizeof(double) * kKP));
    NPG_HIP(hipMalloc((void **)&ws->R, sizeof(double) * kKP * (kKP + 1) / 2));
    NPG_HIP(hipMalloc((void **)&ws->hcol1, sizeof(double) * kKP * kKP));
    NPG_HIP(hipMalloc((void **)&ws->wnorm2, sizeof(double) * kKP));
    ws->hist_cap = (int)std::min<int64_t>(2 * n + 2, 1 << 22);
    NPG_HIP(hipMalloc((void **)&ws->hist, sizeof(double) * ws->hist_cap));
    NPG_HIP(hipMalloc((void **)&ws->prm, sizeof(GParams)));
    NPG_HIP(hipMalloc((void **)&ws->Rg, 3 * kKP * sizeof(double)));
    NPG_HIP(hipMemsetAsync(ws->Rg, 0, 3 * kKP * sizeof(double), ctx->stream));
    NPG_HIP(hipHostMalloc((void **)&ws->h_C, 2 * sizeof(Snap), hipHostMallocDefault));
    NPG_HIP(hipEventCreateWithFlags(&ws->ev[0], hipEventDisableTiming));
    NPG_HIP(hipEventCreateWithFlags(&ws->ev[1], hipEventDisableTiming));
    NPG_HIP(hipHostMalloc((void **)&ws->h_prm, sizeof(GParams), hipHostMallocDefault));
    NPG_HIP(hipMemsetAsync(ws->Vi, 0, vbytes, ctx->stream));
    NPG_HIP(hipMemsetAsync(ws->w, 0, vb, ctx->stream));
    NPG_HIP(hipMemsetAsync(ws->wt, 0, vb, ctx->stream));
    NPG_HIP(hipMemsetAsync(ws->P1, 0, pb, ctx->stream));
    NPG_HIP(hipMemsetAsync(ws->P2, 0, pb, ctx->stream));
    NPG_HIP(hipMemsetAsync(ws->PR, 0, pb, ctx->stream));
    NPG_HIP(hipMemsetAsync(ws->c, 0, sizeof(double) * kKP, ctx->stream));
    NPG_HIP(hipMemsetAsync(ws->s, 0, sizeof(double) * kKP, ctx->stream));
    NPG_HIP(hipMemsetAsync(ws->z, 0, sizeof(double) * kKP, ctx->stream));
    NPG_HIP(hipMemsetAsync(ws->hcol1, 0, sizeof(double) * kKP * kKP, ctx->stream));
    NPG_HIP(hipMemsetAsync(ws->wnorm2, 0, sizeof(double) * kKP, ctx->stream));
    NPG_HIP(hipStreamSynchronize(ctx->stream));
    *out = ws;
    return NPG_OK;
}

NPG_API int npg_gmres_destroy(npg_gmres *ws) {
    if (!ws) return NPG_OK;
    hipStreamSynchronize(ws->ctx->stream);
    for (int k = 0; k < 2; ++k) {
        if (ws->exec[k]) hipGraphExecDestroy(ws->exec[k]);
        if (ws->graph[k]) hipGraphDestroy(ws->graph[k]);
        if (ws->ev[k]) hipEventDestroy(ws->ev[k]);
    }
    for (hipEvent_t e : ws->pev) hipEventDestroy(e);
    void *ptrs[] = {ws->Vi, ws->w, ws->wt, ws->P1, ws->P2, ws->PR, ws->C, ws->T, ws->c, ws->s,
                    ws->z, ws->R, ws->hcol1, ws->wnorm2, ws->hist, ws->prm, ws->Rg, ws->xg, ws->ho};
    for (void *p : ptrs)
        if (p) hipFree(p);
    if (ws->h_C) hipHostFree(ws->h_C);
    if (ws->h_prm) hipHostFree(ws->h_prm);
    if (ws->h_ho) hipHostFree(ws->h_ho);
    delete ws;
    return NPG_OK;
}

NPG_API int npg_gmres_set_halo(npg_gmres *ws, npg_halo *h) {
    NPG_REQUIRE(ws, "npg_gmres_set_halo: NULL workspace");
    NPG_REQUIRE(!h || h->n_owned == ws->n, "npg_gmres_set_halo: the plan owns %lld rows, the workspace %lld",
                h ? (long long)h->n_owned : 0LL, (long long)ws->n);
    NPG_HIP(hipStreamSynchronize(ws->ctx->stream));
    ws->halo = h;
    ws->have_graph = false;
    ws->n_ghost = h ? h->n_ghost : 0;
    // the SpMV input wt needs room for the ghost entries
    NPG_HIP(hipFree(ws->wt));
    const size_t nb = (size_t)(ws->n + ws->n_ghost) * sizeof(double);
    NPG_HIP(hipMalloc((void **)&ws->wt, nb));
    NPG_HIP(hipMemset(ws->wt, 0, nb));
    return NPG_OK;
}

// Which kernel instances, on which grids, a solve launches: EVERY selection rule is here.  Fills the plan except for the pointers of
// the buffers that exist only once the selection says they are needed (gmres_plan_buffers).  `reorth_eta`: as the kernels get it.
static void gmres_plan(GmresPlan &p, npg_gmres *ws, const npg_csr *A, int precond_kind, double precond_scalar, const npg_vec *precond_diag,
                       const npg_vec *y, npg_vec *x, double rtol, double reorth_eta, const GmresKnobs &k) {
    npg_ctx *ctx = ws->ctx;
    const bool dist = ws->halo != nullptr;
    const int maxg = std::min(kMaxG, 3 * ctx->num_cu);
    memset(&p, 0, sizeof p);
    p.lanes = A->lanes;
    p.dist = dist;
    p.kernel_only = dist && comm_is_kernel_only(ctx);
    GDev &d = p.d;
    d.A = csr_view(A);
    d.tile_ptr = A->tile_ptr;
    d.ntiles = A->ntiles;
    d.nt_int = A->ntiles_interior;
    d.n = (int)ws->n;
    d.mem = ws->mem;
    d.pkind = precond_kind;
    d.pscalar = precond_scalar;
    d.pdiag = precond_kind == NPG_PRECOND_DIAG ? precond_diag->d : nullptr;
    d.b = y->d;
    d.x = x->d;
    d.Vi = ws->Vi;
    d.w = ws->w;
    d.wt = ws->wt;
    d.P1 = ws->P1;
    d.P2 = ws->P2;
    d.PR = ws->PR;
    d.G1 = std::max(1, std::min<int>(A->ntiles, maxg));
    d.G2 = (int)std::max<int64_t>(1, std::min<int64_t>((ws->n + kNS - 1) / kNS, maxg));
    const int split_req = ws->split_mode >= 0 ? ws->split_mode : k.split;
    // measured on MI355X (bowl3D h = 0.1 / 0.08 / 0.05: 23.7 vs 26.0, 27.0 vs 32.0, 50.5 vs 72.6 us per iteration): the
    // split organisation wins from the smallest mesh of interest on; the fused kernels remain for tiny systems
    d.split = split_req >= 0 ? (split_req != 0) : (ws->n >= 8192 ? 1 : 0);
    if (A->pk9) d.split = 1;        // (full node records are served by the split kernels only)
    // distributed: one all-reduce per Arnoldi step (norm of the orthogonalised vector by Pythagoras); NPG_GMRES_PYTH=0
    // or a cancellation flagged by an earlier cycle selects the explicitly reduced norm (a second all-reduce)
    d.pyth = (dist && k.pyth && !ws->explicit_norm) ? 1 : 0;
    d.lazy2 = (!dist && k.lazy2) ? 1 : 0;
    // one GPU, split mode: no second-pass sums until a solve reports that a column needed them (NPG_GMRES_FAST=0: never)
    // (only at the default threshold or below, where a second pass is a rare event; a caller asking for eta > 0.1 wants them)
    // distributed runs take no second pass at all (reorth_eta = 0 for them): they always use the fast instance, whose exactly
    // summed norm is what the explicit-norm fallback reduces over the ranks
    d.fast = (d.split && k.fast && reorth_eta <= 0.1 + 1e-12 && (dist || (d.lazy2 && !ws->safe_mode))) ? 1 : 0;
    d.rev = k.rev;
    d.ldv = d.split ? (int64_t)((ws->n + 31) / 32) * 32 : 0;
    // Compressed basis (split organisation only): the stored columns in fp32.  They serve the Gram-Schmidt sums and the
    // update x += V y; the vector that enters the next SpMV is formed from wt in fp64, the true residual is recomputed in
    // fp64 at every restart, and all arithmetic is fp64 - what the stored copy limits is the accuracy a SINGLE cycle can
    // add (~1e-7 of the residual it starts from), so it is the default only for tolerances a cycle never exceeds.
    const int basis_req = ws->basis_bits ? ws->basis_bits : k.basis;
    const bool basis32 = d.split && (basis_req == 32 || (basis_req == 0 && rtol >= 1e-7));
    d.Vf = basis32 ? reinterpret_cast<float *>(ws->Vi) : nullptr;
    // grid of the row kernels.  distributed: ONE workgroup folds their partial rows before they travel (k_peer_fold_allreduce) -
    // a rank's share of the rows is latency-bound in these kernels anyway, so fewer, longer workgroups cost nothing and the fold
    // reads 256 rows in one trip instead of 768 in three.  fp32-stored basis: they take two rows per thread (and NPG_GMRES_ROWS_WG).
    const int64_t rows_per_wg = basis32 ? 2 * kRB : kRB;
    const int rows_cap = std::min(dist ? 256 : (basis32 ? std::min(kMaxG, k.rows_wg) : kMaxG), 3 * ctx->num_cu);
    d.GR = (int)std::max<int64_t>(1, std::min<int64_t>((ws->n + rows_per_wg - 1) / rows_per_wg, rows_cap));
    d.GP1 = d.split ? d.GR : d.G1;
    d.GP2 = d.split ? d.GR : d.G2;
    // Gather-layout fp32 copy of the SpMV input (one GPU, fp32-stored basis, fast mode, node-blocked matrix): the Arnoldi kernel
    // is bound by its gather instructions and a node's three components then come with ONE 16-byte gather.
    // The rounding is the one the stored basis column has anyway.  NPG_GMRES_XG=0 turns it off.
    // plain-CSR matrices (function-valued viscosity: the full-stress form has no node records): the copy is then the vector in
    // fp32, every gather 4 bytes instead of 8 - measured on the channel basin at 4.1 M unknowns: Arnoldi kernel 1 019 against
    // 1 075 us; from 100 000 rows on (below that the solve is latency-bound and the extra stores buy nothing);
    // NPG_GMRES_XG_CSR=0 / 1 forces it off / on at any size
    const bool xg_csr = k.xg_csr >= 0 ? k.xg_csr != 0 : ws->n >= 100000;
    if ((ws->gather32 >= 0 ? ws->gather32 : k.xg) && basis32 && d.fast && (A->nnode() > 0 || xg_csr) && (dist ? A->n == A->m + ws->n_ghost : A->n == A->m)) {
        // node slots: the owned block nodes and, behind them, the ghost nodes the windowed tiles use as record columns
        // (NOT gather32_floats(A): that is the stand-alone product's question and answers 0 for a rank's row block - round 5's first
        //  version sized the copy without the ghost slots through it and the unpack wrote 4 ngn floats past the end)
        const int64_t nslots = A->win.wtile_ptr ? gather32_nodes(A) : A->nnode();
        const int64_t nbr = A->block_rows();
        p.xg_floats = 4 * nslots + (A->n - nbr) + 8;
        d.xg = GatherMap{nullptr, 3 * A->nfull, A->nfull, (int)nbr, (int)(4 * nslots - nbr)};
        d.gslot = A->win.wtile_ptr ? A->win.gslot : nullptr;
        // windowed tile set of the block rows (spmv_window.h; NPG_GMRES_WINDOW=0: the ordinary tiles)
        if (k.window && ws->gather32 != 2 && d.split && A->win.wtile_ptr && !A->pk9 && nbr > 0) {
            d.wt_ptr = A->win.wtile_ptr;
            d.W = win_view(A);
            d.nwt = A->win.nwtiles;
            d.nwt_int = A->win.nwtiles_interior;
            d.wl = A->win.wlanes;
            d.word = k.win_ord || (A->win.nwrow_tiles == 0 && A->m > A->block_rows());
            d.wpre = k.win_pre;
        }
    }
    // One GPU, split organisation, fast kernels: the first-pass sums are folded once and the basis column is formed by the dots
    // kernel (NPG_GMRES_ONEFOLD=0: every orthogonalisation workgroup folds them, the Arnoldi epilogue stores the column).  Same
    // sums in the same order, same expression for the column: the switch changes no bit of any result.
    d.onefold = (!dist && d.split && d.fast && env_int("NPG_GMRES_ONEFOLD", 1) != 0) ? 1 : 0;
    d.vdots = (d.onefold && d.Vf) ? 1 : 0;
    // ... and, with the fp32-stored basis, the three row launches of a step as one resident launch (k_gmres_rows_fused;
    // NPG_GMRES_FUSEDROWS=0: the separate launches).  It is the onefold arrangement in one kernel, so it selects that arrangement
    // for the cycle's other steps too; NPG_GMRES_ONEFOLD=0 chooses among the separate launches, i.e. with NPG_GMRES_FUSEDROWS=0 or
    // where the fused kernel does not apply.  Only on a grid that is resident as a whole: the hand-off waits for every workgroup.
    // NPG_GMRES_FUSED_COLS: the widest fused step - 20 (the default: every instance) or 16 (the one-pass instances only; steps of
    // 17-20 columns then take the separate launches, as they do where the grid is admitted for the one-pass instances alone).
    if (!dist && d.split && d.fast && d.Vf && !d.rev && !ws->fused_off && env_int("NPG_GMRES_FUSEDROWS", 1) != 0) {
        if (ws->fused_blocks[0] < 0) {
            ws->fused_blocks[0] = rows_fused_blocks_per_cu(kFusedOnePassCols);
            ws->fused_blocks[1] = rows_fused_blocks_per_cu(kFusedMaxCols);
        }
        const bool wide = env_int("NPG_GMRES_FUSED_COLS", kFusedMaxCols) > kFusedOnePassCols && d.GR <= ctx->num_cu * ws->fused_blocks[1];
        if (wide || d.GR <= ctx->num_cu * ws->fused_blocks[0]) {
            d.fusedrows = d.onefold = d.vdots = 1;
            p.fused_cols = wide ? kFusedMaxCols : kFusedOnePassCols;
        }
    }
    const bool one1 = dist || d.onefold;        // (slot 0 of the all-reduced rows is free on one GPU)
    d.Q1 = one1 ? ws->Rg : d.P1;
    d.Q2 = dist ? ws->Rg + kKP : d.P2;
    d.QR = dist ? ws->Rg + 2 * kKP : d.PR;
    d.nQ1 = one1 ? 1 : d.GP1;
    d.nQ2 = dist ? 1 : d.GP2;
    d.nQR = dist ? 1 : d.G1;
    d.C = ws->C;
    d.T = ws->T;
    d.c = ws->c;
    d.s = ws->s;
    d.z = ws->z;
    d.R = ws->R;
    d.hcol1 = ws->hcol1;
    d.wnorm2 = ws->wnorm2;
    d.hist = ws->hist;
    d.hist_cap = ws->hist_cap;
    d.prm = ws->prm;

    // Distributed cycles.  On the peer transport (comm.hip) every communication step is a kernel on a HIP stream, so the
    // cycle replays from one hipGraph exactly like the single-GPU cycle - the default there (NPG_DIST_GRAPH=0 turns it off).
    // With RCCL in the cycle the calls can be captured too (the exchange stream forks from and joins the captured stream
    // through the plan's events), but a captured collective costs more than an eager one and has only
    // run on a one-rank communicator: opt-in (NPG_DIST_GRAPH=1 / npg_gmres_set_dist_options).  The host-driven shm
    // rehearsal transport cannot be captured.
    const bool graph_dist = dist && !ctx->shm &&
                            (p.kernel_only ? (k.dist_graph != 0 && ws->dist_graph != 0) : ((ws->dist_graph > 0 || k.dist_graph > 0) && ctx->comm));
    p.use_graph = (!dist || graph_dist) && !k.eager && !ws->profile;

    // tile range of the Arnoldi launches: the windowed set where the gather-layout instance has one
    p.a_nt = d.wt_ptr ? d.nwt : d.ntiles;
    p.a_int = d.wt_ptr ? d.nwt_int : d.nt_int;
    p.grid = d.split ? std::min(d.G1, std::max(1, p.a_nt)) : d.G1;
    if (!dist) return;
    // distributed split cycle: the tiles that read no ghost column run while the exchange of wt's ghost segment is in
    // flight on the plan's own stream (NPG_HALO_OVERLAP=0: exchange first, one launch)
    // default: on with the peer windows (two kernels on one stream around the interior tiles); with RCCL (a second stream and
    // two events, never run between two physical GPUs) only when asked for - NPG_HALO_OVERLAP=1 / npg_gmres_set_dist_options
    int want = ws->halo_overlap >= 0 ? ws->halo_overlap : (k.overlap >= 0 ? k.overlap : (p.kernel_only || ctx->shm ? 1 : 0));
    // RCCL's two-stream overlap has never run between two physical GPUs: REFUSED (not merely off by default) unless the caller
    // states that it knows - NPG_HALO_OVERLAP_UNVERIFIED=1.  (The two-event arrangement itself is sound: rerun with the peer
    // kernel on a second stream after the epoch fix, profiles/r04_overlap_rerun.txt.)
    if (want && !p.kernel_only && !ctx->shm && !k.overlap_unverified) {
        static bool told = false;
        if (!told && (told = true))
            fprintf(stderr, "[npg] halo overlap on the RCCL transport was asked for but has never been verified on two physical GPUs: "
                            "running the exchange before the Arnoldi launch instead (NPG_HALO_OVERLAP_UNVERIFIED=1 overrides)\n");
        want = 0;
    }
    // By DEFAULT the two-launch form is taken only when at least half of the tiles read no ghost column: splitting costs a second
    // launch with its prologue and a second partly filled round of workgroups, and with hardly any interior tiles there is nothing to
    // run beside the exchange (rank 4 of 8 of bowl3D h = 0.02 before the interior-first numbering of partition.py: 106 of 2 606 tiles
    // interior, 81.8 us per iteration split against 73.5 us exchanged first - profiles/r05_dist_cycle.txt) AND the exchange is large
    // enough for its wire time to exceed what the split costs: the END ranks of the 8-rank partition of that system have 1 000 of
    // 1 783 tiles interior and 19 k ghost entries (150 KB: ~1 us on an xGMI link) - split, they took 67 us per iteration where the
    // inner ranks took 59, and the slowest rank sets the pace (section 5 there).  NPG_HALO_OVERLAP_MIN_GHOSTS: 200 000 entries
    // = 1.6 MB ~ 10 us on one link.  An explicit request (NPG_HALO_OVERLAP=1 / npg_gmres_set_dist_options) splits whenever both
    // parts are non-empty.
    const bool asked = ws->halo_overlap >= 0 || k.overlap >= 0;
    const bool big = ws->halo->n_ghost >= k.overlap_min_ghosts;
    p.overlap = d.split && want && p.a_int > 0 && p.a_int < p.a_nt && (asked || (2 * p.a_int >= p.a_nt && big));
    if (p.overlap) {
        // RCCL: the interior launch leaves a few CUs free - its workgroups are persistent (they hold their CU until the last
        // tile) and RCCL's send/recv kernels on the other stream could otherwise not start before they are all done.  Peer
        // windows: nothing of ours runs beside it (the neighbours' stores need no CU here): full grid.
        p.reserve = p.kernel_only ? 0 : std::max(0, std::min(k.reserve_cus, maxg / 6));
        p.grid_int = std::min(p.a_int, maxg - 3 * p.reserve);
        p.grid_bnd = std::min(p.a_nt - p.a_int, maxg);
    }
    if (getenv("NPG_HALO_OVERLAP_VERBOSE")) {
        static int last = -1;
        const int now = (p.overlap ? 2 : 0) + (d.split ? 1 : 0);
        if (now != last && (last = now, true))
            fprintf(stderr, "halo overlap %s: %d interior / %d boundary tiles per Arnoldi step (split %d)\n", p.overlap ? "on" : "off",
                    p.a_int, p.a_nt - p.a_int, d.split);
    }
}

// The buffers that only some plans need, made (or grown) on first use, and their pointers entered into the plan: the gather-layout
// copy of the SpMV input with its pads zeroed, the hand-off state of the fused row kernel.
static int gmres_plan_buffers(GmresPlan &p, npg_gmres *ws, const npg_csr *A, hipStream_t st) {
    if (p.xg_floats) {
        if (ws->xg_len < p.xg_floats) {
            if (ws->xg) NPG_HIP(hipFree(ws->xg));
            ws->xg = nullptr;
            NPG_HIP(hipMalloc((void **)&ws->xg, (size_t)p.xg_floats * sizeof(float)));
            ws->xg_len = p.xg_floats;
            ws->xg_key[0] = -1;
        }
        if (ws->xg_key[0] != A->nfull || ws->xg_key[1] != A->nsurf || ws->xg_key[2] != (int)A->n) {
            NPG_HIP(hipMemsetAsync(ws->xg, 0, (size_t)ws->xg_len * sizeof(float), st));      // the pads must read as zero
            ws->xg_key[0] = A->nfull;
            ws->xg_key[1] = A->nsurf;
            ws->xg_key[2] = (int)A->n;
        }
        p.d.xg.p = ws->xg;
    }
    if (p.d.fusedrows) {
        if (!ws->ho) {
            NPG_HIP(hipMalloc((void **)&ws->ho, sizeof(RowsHandOff)));
            NPG_HIP(hipMemsetAsync(ws->ho, 0, sizeof(RowsHandOff), st));
            NPG_HIP(hipHostMalloc((void **)&ws->h_ho, 2 * sizeof(unsigned long long), hipHostMallocDefault));
            ws->h_ho[0] = ws->h_ho[1] = 0;
        }
        p.d.ho = ws->ho;
    }
    return NPG_OK;
}

// (re)capture the per-cycle graphs when anything they bake in - the plan - has changed
static int ensure_graphs(npg_gmres *ws, const GmresPlan &p, hipStream_t st) {
    if (!p.use_graph || (ws->have_graph && memcmp(&ws->key, &p, sizeof p) == 0)) return NPG_OK;
    for (int k = 0; k < 2; ++k) {
        if (ws->exec[k]) hipGraphExecDestroy(ws->exec[k]);
        if (ws->graph[k]) hipGraphDestroy(ws->graph[k]);
        ws->exec[k] = nullptr;
        ws->graph[k] = nullptr;
        ws->have_graph = false;
        NPG_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        int rc = launch_cycle(p, st, nullptr, ws, k);
        if (rc) {
            hipGraph_t broken = nullptr;
            hipStreamEndCapture(st, &broken);
            if (broken) hipGraphDestroy(broken);
            return rc;
        }
        NPG_HIP(hipStreamEndCapture(st, &ws->graph[k]));
        NPG_HIP(hipGraphInstantiate(&ws->exec[k], ws->graph[k], nullptr, nullptr, 0));
    }
    memcpy(&ws->key, &p, sizeof p);
    ws->have_graph = true;
    return NPG_OK;
}

// the true residual that starts a cycle, of the iterate as it stands: wt = P (b - A x) and its squared norm
static int launch_first_residual(npg_gmres *ws, const GmresPlan &p, hipStream_t st) {
    if (int rc = p.dist ? halo_exchange_raw(ws->halo, p.d.x) : NPG_OK) return rc;
    with_lanes(p.lanes, [&](auto lanes) { launch_residual_L<decltype(lanes)::value>(p.d, st); });
    NPG_HIP(hipGetLastError());
    return p.dist ? fold_rows(ws, p.d.PR, p.d.G1, 2, st) : NPG_OK;
}

// done == 5, distributed: ||w||^2 - ||h||^2 met cancellation and the device interrupted the pass before that column.  Carry on
// from the current iterate with explicitly reduced norms (a second all-reduce per step), for this and all later solves of the
// workspace.  `last` = the state read from result slot `slot`; returns with the stream idle and the slot a result slot again.
static int restart_with_explicit_norms(npg_gmres *ws, GmresPlan &p, Snap &last, int slot, hipStream_t st) {
    NPG_HIP(hipStreamSynchronize(st));           // (pipelined: the cycle enqueued ahead has exited at once)
    p.d.pyth = 0;
    ws->explicit_norm = true;
    // the captured cycles have pyth = 1 baked into their kernel arguments: replaying them would flag the same cancellation for
    // ever - capture the explicit-norm cycle
    if (int rc = ensure_graphs(ws, p, st)) return rc;
    last.done = 0;
    last.inner = 0;
    ws->h_C[slot] = last;
    NPG_HIP(hipMemcpyAsync(ws->C, ws->h_C + slot, sizeof(Snap), hipMemcpyHostToDevice, st));
    if (int rc = launch_first_residual(ws, p, st)) return rc;
    NPG_HIP(hipStreamSynchronize(st));
    return NPG_OK;
}

// A hand-off of k_gmres_rows_fused that ran out of time has set the status word: that launch and every later one skipped the
// update, so the iterate is not to be trusted.  Report it, re-zero the hand-off state and keep to the separate launches.
static int fused_gave_up(npg_gmres *ws, hipStream_t st) {
    hipStreamSynchronize(st);
    hipMemset(ws->ho, 0, sizeof(RowsHandOff));
    ws->h_ho[0] = ws->h_ho[1] = 0;
    ws->fused_off = true;
    ws->have_graph = false;
    npg::set_error("npg_gmres_solve: the grid-wide hand-off of the fused row kernel timed out (a workgroup was not resident); "
                   "the iterate is not valid - this workspace uses the separate row launches from now on");
    return NPG_EHIP;
}

// Cycles until the carried state says done, at most max_cycles.  Cycle c+1 is enqueued before the host reads the outcome of
// cycle c: the device never idles waiting for the host, and a cycle launched after convergence costs only its early-exit kernels.
// Profile mode: eager launches with HIP events around every Arnoldi (SpMV) kernel, one cycle at a time - the events are read between two cycles.
static int run_cycles(npg_gmres *ws, GmresPlan &p, int64_t max_cycles, Snap &last, hipStream_t st, std::chrono::steady_clock::time_point t0, int trace) {
    if (ws->profile && ws->pev.empty()) {
        ws->pev.resize(2 * ws->mem);
        for (auto &e : ws->pev) NPG_HIP(hipEventCreate(&e));
    }
    double t_launch = 0.0;
    int64_t n_launch = 0;
    auto enqueue_cycle = [&](int slot) -> int {
        const auto l0 = std::chrono::steady_clock::now();
        if (p.use_graph)
            NPG_HIP(hipGraphLaunch(ws->exec[slot], st));
        else if (int rc = launch_cycle(p, st, ws->profile ? ws->pev.data() : nullptr, ws, slot))
            return rc;
        NPG_HIP(hipEventRecord(ws->ev[slot], st));
        t_launch += std::chrono::duration<double>(std::chrono::steady_clock::now() - l0).count();
        ++n_launch;
        return NPG_OK;
    };
    int rc = enqueue_cycle(0);
    if (rc) return rc;
    for (int64_t cyc = 0;; ++cyc) {
        const int cur = (int)(cyc & 1), nxt = cur ^ 1;
        const bool more = cyc + 1 < max_cycles;
        if (more && !ws->profile && (rc = enqueue_cycle(nxt))) return rc;
        NPG_HIP(hipEventSynchronize(ws->ev[cur]));
        last = ws->h_C[cur];
        if (p.d.fusedrows && ws->h_ho[cur] != 0) return fused_gave_up(ws, st);
        if (last.done == 5) {
            if ((rc = restart_with_explicit_norms(ws, p, last, cur, st))) return rc;
            if ((rc = enqueue_cycle(cur))) return rc;
            cyc = -1 + (cur == 0 ? 0 : 1);               // keep the slot parity of the ping-pong
            continue;
        }
        if (last.done != 0) break;      // (profile mode: the last (partial) cycle is not counted: some of its kernels exit early)
        if (ws->profile)
            for (int j = 0; j < ws->mem; ++j) {
                float ms = 0.f;
                NPG_HIP(hipEventElapsedTime(&ms, ws->pev[2 * j], ws->pev[2 * j + 1]));
                ws->prof_ms += ms;
                ws->prof_launches += 1;
            }
        if (!more) break;
        if (ws->profile && (rc = enqueue_cycle(nxt))) return rc;
    }
    NPG_HIP(hipStreamSynchronize(st));
    if (trace)
        fprintf(stderr,
                "[npg gmres] %s: %lld cycle launches, %.1f us host time per launch, %d iterations, %.1f us wall per "
                "iteration, %d second GS passes, fused rows %d up to %d columns (row grid %d, %d workgroups per CU admitted)\n",
                p.use_graph ? "graph" : "eager", (long long)n_launch, 1e6 * t_launch / (double)n_launch, last.iter,
                1e6 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() /
                    std::max(1, last.iter),
                last.nreorth, p.d.fusedrows, p.fused_cols, p.d.GR, ws->fused_blocks[p.fused_cols > kFusedOnePassCols ? 1 : 0]);
    return NPG_OK;
}

// what the solve launched (npg_gmres_last_config; gmres_plan reroutes on size, tolerance, matrix form and safe_mode) and how it ended
static int gmres_report(npg_gmres *ws, const GmresPlan &p, const Snap &last, std::chrono::steady_clock::time_point t0, npg_solve_stats *stats) {
    const GDev &d = p.d;
    ws->hist_len = std::min<int64_t>((int64_t)last.iter + 1, ws->hist_cap);
    const int32_t cfg[kCfgLen] = {d.split, d.Vf ? 32 : 64, d.fast, d.xg.p ? (d.xg.nbr == 0 ? 2 : 1) : 0, d.wt_ptr ? 1 : 0,
                                  d.wt_ptr ? d.wl : 0, d.wt_ptr ? d.word : 0, p.lanes, d.A.pk9 ? 1 : 0, p.dist, d.pyth,
                                  p.a_nt, p.grid, d.split ? d.GR : d.G2, d.n, d.mem, d.lazy2, d.fusedrows};
    memcpy(ws->cfg, cfg, sizeof cfg);
    ws->have_cfg = true;
    ws->fused_cols = p.fused_cols;
    // a replayed cycle reports communication timeouts through the status word only
    if (int rc = p.dist ? comm_check(ws->ctx) : NPG_OK) return rc;
    if (stats) {
        stats->solved = (last.done == 1 || last.done == 4) ? 1 : 0;
        stats->niter = last.iter;
        stats->npass = last.npass;
        stats->status = last.done;
        stats->nreorth = last.nreorth;
        // distributed: Arnoldi steps whose Pythagorean norm lost > 4 digits; one GPU, fast mode: columns that were due a
        // second Gram-Schmidt pass and did not get it (the following solves then run the full kernels)
        stats->nflagged = last.pad0 + last.pad1;
        if (d.fast && last.pad1 > 0) ws->safe_mode = true;
        stats->rnorm0 = last.rnorm0;
        stats->rnorm = last.rnorm;
        stats->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    return NPG_OK;
}

// npg_csr_block_nodes_dofs: right-hand side, iterate (warm start in, solution out) and a vector preconditioner come and go
// in the CALLER's DoF order - three gather passes in, one scatter pass out, then the solve proper on the library's order
static int solve_in_caller_order(npg_gmres *ws, const npg_csr *A_in, int precond_kind, double precond_scalar, const npg_vec *precond_diag,
                                 const npg_vec *y, npg_vec *x, double atol, double rtol, int64_t itmax, double reorth_eta,
                                 npg_solve_stats *stats) {
    NPG_REQUIRE(!ws->halo, "npg_gmres_solve: a matrix with an internal renumbering cannot be a distributed row block");
    NPG_REQUIRE(y->n == A_in->m && x->n == A_in->m, "npg_gmres_solve: vector lengths do not match the matrix");
    npg_csr *Am = const_cast<npg_csr *>(A_in);
    npg_vec yi = *y, xi = *x, di;
    yi.d = Am->uvec[0];
    xi.d = Am->uvec[1];
    yi.owns = xi.owns = false;
    perm_gather(A_in, yi.d, y->d);
    perm_gather(A_in, xi.d, x->d);
    const npg_vec *dp = precond_diag;
    if (precond_kind == NPG_PRECOND_DIAG && precond_diag) {
        NPG_REQUIRE(precond_diag->n == A_in->m, "npg_gmres_solve: bad preconditioner");
        di = *precond_diag;
        di.d = Am->uvec[2];
        di.owns = false;
        perm_gather(A_in, di.d, precond_diag->d);
        dp = &di;
    }
    Am->uperm_active = true;
    const int rc = npg_gmres_solve(ws, A_in, precond_kind, precond_scalar, dp, &yi, &xi, atol, rtol, itmax, reorth_eta, stats);
    Am->uperm_active = false;
    if (rc) return rc;
    perm_scatter(A_in, x->d, xi.d);
    NPG_HIP(hipStreamSynchronize(ws->ctx->stream));
    return NPG_OK;
}

NPG_API int npg_gmres_solve(npg_gmres *ws, const npg_csr *A_in, int precond_kind, double precond_scalar,
                            const npg_vec *precond_diag, const npg_vec *y, npg_vec *x, double atol, double rtol,
                            int64_t itmax, double reorth_eta, npg_solve_stats *stats) {
    NPG_REQUIRE(ws && A_in && y && x, "npg_gmres_solve: NULL argument");
    ws->have_cfg = false;         // (npg_gmres_last_config reports nothing for a solve that fails)
    if (A_in->uperm && !A_in->uperm_active)
        return solve_in_caller_order(ws, A_in, precond_kind, precond_scalar, precond_diag, y, x, atol, rtol, itmax, reorth_eta, stats);
    const npg_csr *A = spmv_form(A_in);           // (the record-form companion of a plain matrix, if it has one)
    if (int rc = check_record_view(A, true, "npg_gmres_solve")) return rc;     // (full node records: the split kernels, forced in gmres_plan)
    const int64_t nloc = ws->n + ws->n_ghost;     // distributed: vectors the SpMV reads hold [owned | ghosts]
    NPG_REQUIRE(A->m == ws->n && A->n == nloc && y->n == ws->n && x->n == nloc,
                "npg_gmres_solve: workspace is for n=%lld (+%lld ghosts) but A is %lldx%lld, y has %lld, x has %lld",
                (long long)ws->n, (long long)ws->n_ghost, (long long)A->m, (long long)A->n, (long long)y->n,
                (long long)x->n);
    NPG_REQUIRE(precond_kind == NPG_PRECOND_NONE || precond_kind == NPG_PRECOND_SCALAR ||
                    (precond_kind == NPG_PRECOND_DIAG && precond_diag && precond_diag->n == ws->n),
                "npg_gmres_solve: bad preconditioner");
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t st = ws->ctx->stream;
    static const GmresKnobs knobs;
    if (ws->halo) reorth_eta = 0.0;     // distributed: the on-the-fly second pass would need basis rows of ghost columns

    // the plan: selection decides instances, grids and buffer sizes; the buffers are made; their pointers complete the plan
    GmresPlan p;
    gmres_plan(p, ws, A, precond_kind, precond_scalar, precond_diag, y, x, rtol, reorth_eta, knobs);
    if (int rc = gmres_plan_buffers(p, ws, A, st)) return rc;

    if (itmax <= 0) itmax = 2 * ws->n;
    ws->h_prm->atol = atol;
    ws->h_prm->rtol = rtol;
    ws->h_prm->eta2 = reorth_eta <= 0.0 ? -1.0 : reorth_eta * reorth_eta;
    ws->h_prm->btol = std::pow(2.220446049250313e-16, 0.75);
    ws->h_prm->itmax = itmax;
    NPG_HIP(hipMemcpyAsync(ws->prm, ws->h_prm, sizeof(GParams), hipMemcpyHostToDevice, st));
    Snap c0{};
    c0.first = 1;
    ws->h_C[0] = c0;
    NPG_HIP(hipMemcpyAsync(ws->C, ws->h_C, sizeof(Snap), hipMemcpyHostToDevice, st));
    NPG_HIP(hipStreamSynchronize(st));      // h_C[0] is reused below as a result slot

    if (int rc = ensure_graphs(ws, p, st)) return rc;

    // first true residual, then cycles until the carried state says done
    if (int rc = launch_first_residual(ws, p, st)) return rc;
    const int64_t max_cycles = (itmax + ws->mem - 1) / ws->mem + 1;
    Snap last{};
    if (int rc = run_cycles(ws, p, max_cycles, last, st, t0, knobs.trace)) return rc;
    return gmres_report(ws, p, last, t0, stats);
}

NPG_API int npg_gmres_set_dist_options(npg_gmres *ws, int overlap, int graph) {
    NPG_REQUIRE(ws, "npg_gmres_set_dist_options: NULL workspace");
    ws->halo_overlap = overlap < 0 ? -1 : (overlap ? 1 : 0);
    ws->dist_graph = graph < 0 ? -1 : (graph ? 1 : 0);
    ws->have_graph = false;
    return NPG_OK;
}

NPG_API int npg_gmres_set_basis(npg_gmres *ws, int bits) {
    NPG_REQUIRE(ws && (bits == 0 || bits == 32 || bits == 64), "npg_gmres_set_basis: bits must be 0 (by tolerance), 32 or 64");
    ws->basis_bits = bits;
    ws->have_graph = false;
    return NPG_OK;
}

NPG_API int npg_gmres_set_gather(npg_gmres *ws, int mode) {
    NPG_REQUIRE(ws && mode >= -1 && mode <= 2, "npg_gmres_set_gather: mode must be -1 (default), 0, 1 or 2");
    ws->gather32 = mode;
    ws->have_graph = false;
    return NPG_OK;
}

NPG_API int npg_gmres_set_split(npg_gmres *ws, int mode) {
    NPG_REQUIRE(ws && mode >= -1 && mode <= 1, "npg_gmres_set_split: bad argument");
    ws->split_mode = mode;
    return NPG_OK;
}

NPG_API int npg_gmres_set_profile(npg_gmres *ws, int on) {
    NPG_REQUIRE(ws, "npg_gmres_set_profile: NULL workspace");
    ws->profile = on != 0;
    ws->prof_ms = 0.0;
    ws->prof_launches = 0;
    return NPG_OK;
}

NPG_API int npg_gmres_get_profile(npg_gmres *ws, double *ms_total, int64_t *launches) {
    NPG_REQUIRE(ws && ms_total && launches, "npg_gmres_get_profile: NULL argument");
    *ms_total = ws->prof_ms;
    *launches = ws->prof_launches;
    return NPG_OK;
}

NPG_API int npg_gmres_last_config(const npg_gmres *ws, int32_t *cfg, int n) {
    if (!ws || !cfg || n <= 0 || !ws->have_cfg) return 0;
    const int k = std::min(n, kCfgLen);
    memcpy(cfg, ws->cfg, (size_t)k * sizeof(int32_t));
    return k;
}

NPG_API int npg_gmres_fused_cols(const npg_gmres *ws) { return (ws && ws->have_cfg) ? ws->fused_cols : 0; }

NPG_API int64_t npg_gmres_history(npg_gmres *ws, double *buf, int64_t cap) {
    if (!ws || !buf || cap <= 0) return 0;
    const int64_t k = std::min<int64_t>(cap, ws->hist_len);
    if (hipMemcpy(buf, ws->hist, (size_t)k * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return k;
}
