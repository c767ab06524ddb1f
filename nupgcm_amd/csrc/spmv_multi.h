// Multi-column form of spmv_tile's plain-CSR path (spmv_device.h): one tile of a matrix WITHOUT records times up to C input
// columns.  The tile's (col, val) pairs are read from HBM once - at NT = 1024 and U2 = 4 one trip's registers hold a whole tile
// (8192 >= kTileNnz + 2 slots) - and reused for every column; per column the work is spmv_tile's own: gather, products into the same
// slots of `prod`, barrier, the same L-lane pair sums and group_sum_dpp<L>, so a column's row sums carry the bits of the
// single-column product.  One `out[kTileRows]` serves all columns: `epi(j)` runs behind the barrier that follows column j's sums
// and before the next column's.
//
// Input column j of matrix column c is xb[c * cs + j * js]: (cs, js) = (1, n) for stacked vectors, (K, 1) for row-major ones.
// active: bit j set = column j takes part (a clear bit costs nothing and touches nothing).
#pragma once
#include "spmv_device.h"

namespace npg {

template <int NT, int L, int C, class EPI>
__device__ __forceinline__ void spmv_tile_multi(const CsrDev &A, const double *__restrict__ xb, int64_t cs, int64_t js, unsigned active,
                                                const TileDesc &td, TileLds &t, double *__restrict__ out, EPI epi) {
    constexpr int U2 = 4;
    static_assert(2 * NT * U2 >= kTileNnz + 2, "one trip must cover a tile");
    const int r0 = td.r0, nrows = td.nrows;
    const int64_t base = td.base;
    const int n = td.n;
    const int tid = threadIdx.x;
    const int64_t abase = base & ~1LL;
    const int off = (int)(base - abase);
    const int total = n + off;
    for (int r = tid; r <= nrows; r += NT) t.rp[r] = (int32_t)(A.rowptr[r0 + r] - base) + off;
    if (total <= kTileNnz + 2) {
        // ---- the tile's entries: U2 pairs per lane, kept for all columns
        const int k0 = 2 * tid;
        int2 c[U2];
        double2 v[U2];
#pragma unroll
        for (int u = 0; u < U2; ++u) {
            const int k = k0 + u * 2 * NT;
            if (k < total && abase + k + 1 < A.nnz) {
                const long long cc = __builtin_nontemporal_load(reinterpret_cast<const long long *>(A.col + abase + k));
                c[u] = make_int2((int)(cc & 0xffffffffLL), (int)(cc >> 32));
                v[u].x = __builtin_nontemporal_load(A.val + abase + k);
                v[u].y = __builtin_nontemporal_load(A.val + abase + k + 1);
            } else if (k < total && abase + k < A.nnz) {
                c[u] = make_int2(A.col[abase + k], 0);
                v[u] = make_double2(A.val[abase + k], 0.0);
            } else {
                c[u] = make_int2(0, 0);
                v[u] = make_double2(0.0, 0.0);
            }
        }
        const int g = tid / L, l = tid % L;
#pragma unroll
        for (int j = 0; j < C; ++j) {
            if (!((active >> j) & 1u)) continue;        // uniform
            const double *__restrict__ xj = xb + j * js;
            double xa[U2], xc[U2];
#pragma unroll
            for (int u = 0; u < U2; ++u) {
                xa[u] = xj[c[u].x * cs];
                xc[u] = xj[c[u].y * cs];
            }
#pragma unroll
            for (int u = 0; u < U2; ++u) {
                const int k = k0 + u * 2 * NT;
                if (k < total) t.prod[k] = (k >= off) ? v[u].x * xa[u] : 0.0;
                if (k + 1 < total) t.prod[k + 1] = v[u].y * xc[u];
            }
            __syncthreads();
            for (int r = g; r < nrows; r += NT / L) {
                double s = 0.0;
                const int e = t.rp[r + 1];
                for (int k = t.rp[r] + 2 * l; k < e; k += 2 * L) {
                    const double a = t.prod[k], b = t.prod[k + 1];
                    s += a + (k + 1 < e ? b : 0.0);
                }
                s = group_sum_dpp<L>(s);
                if (l == 0) out[r] = s;
            }
            __syncthreads();
            epi(j);
        }
    } else {
        // one very long row: the whole workgroup strides over it, column by column (the row is re-read per column: such rows are rare)
#pragma unroll
        for (int j = 0; j < C; ++j) {
            if (!((active >> j) & 1u)) continue;
            const double *__restrict__ xj = xb + j * js;
            double s = 0.0;
            for (int k = tid; k < n; k += NT) s += A.val[base + k] * xj[A.col[base + k] * cs];
            s = wave_sum(s);
            __syncthreads();
            if ((tid & 63) == 0) t.prod[tid >> 6] = s;
            __syncthreads();
            if (tid == 0) {
                double tot = 0.0;
                for (int w = 0; w < NT / 64; ++w) tot += t.prod[w];
                out[0] = tot;
            }
            __syncthreads();
            epi(j);
        }
    }
}

}  // namespace npg
