// Time-dependent surface forcing (npg_forcing_*): the load vectors of the wind stress and of the surface buoyancy flux,
// recomputed for the time level being solved, and the surface mass matrix of a restoring condition.  The arithmetic shared by the
// device kernels (forcing.hip) and the host library (csrc_host/nupgcm_host.cpp), with the plan both build at create and the argument
// checks of the entry points: GPU() and CPU() evaluate the same expressions in the same order.  Always fp64.
//
// A face is (cell c, local face kf) as in boundary_core.h: the side lambda_kf = 0 of that cell, its vertices in ascending local index
// taking the face's (mu_0, mu_1, mu_2) - the order of Mesh.surface_load.  The face functions are the SPACE's own restricted to the face:
//   P2 (velocity, P2 buoyancy)   k = 0 .. 2: mu_k (2 mu_k - 1) at the face's vertex k;  k = 3, 4, 5: 4 mu_a mu_b on the edges (0,1) (0,2) (1,2)
//   P1 buoyancy                  k = 0 .. 2: mu_k
// at the nine points of fe.tri_quadrature_degree4 (kBndMu, kBndW), tabulated at compile time (kFrcBasis).  frc_local_node maps k to
// the cell's local node, hence to the DoF codes of the engine's tables; codes < 0 (Dirichlet) take no part.
//
// Tables are component-major [key][point][face]: a wave of consecutive faces reads unit stride.  The value of a series at a point is
//   v = a                          (w == 0: the second keyframe is not read)
//   v = (1 - w) a + w b            a = keyframe key, b = keyframe key + 1 (or 0 behind the last: the periodic wrap); w from the host
// Channels: 0 tau_x, 1 tau_y, 2 F, 3 b* (with the static gamma [point][face]).  The flux integrand is F + gamma b*, formed point by point.
//   pass 1   loc[c][k][f] = sum_q (w_q area2_f v_q) N_k(q)           c = 0 wind x, 1 wind y, 2 flux; one face per lane
//   pass 2   out[r] = base[r] + alpha sum_{slots of r} loc[slot]      (flux rows: alpha sum; rows without slots: base[r] / 0)
//            the slots of a row in (face, k) order - one order, no atomics, the same bits on every call
//   matrix   S[e] = scale sum_{slots (f, i, j) of e} sum_q (w_q area2_f gamma_q) (N_i(q) N_j(q))     e over the entries some face touches,
//            slots in (face, i, j) order; N_i N_j commutes, so S is symmetric to the bits
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "boundary_core.h"

namespace npg {

constexpr int kFrcNSeries = 4;      // tau_x, tau_y, F, b*
constexpr int kFrcNLoad = 3;        // wind x, wind y, flux
constexpr int kFrcK = 6;            // face functions of the P2 space (rows of loc per load; P1 uses the first three)
#ifndef NPG_FRC_BLOCK
#define NPG_FRC_BLOCK 256
#endif

// the face functions at the face points: N2[q][k] (P2), N1[q][k] = mu_k (P1)
struct FrcBasis {
    double N2[kBndQ][kFrcK], N1[kBndQ][3];
};
constexpr FrcBasis frc_basis() {
    FrcBasis b{};
    const int ea[3] = {0, 0, 1}, eb[3] = {1, 2, 2};
    for (int q = 0; q < kBndQ; ++q) {
        for (int j = 0; j < 3; ++j) {
            b.N1[q][j] = kBndMu[q][j];
            b.N2[q][j] = kBndMu[q][j] * (2.0 * kBndMu[q][j] - 1.0);
        }
        for (int e = 0; e < 3; ++e) b.N2[q][3 + e] = 4.0 * kBndMu[q][ea[e]] * kBndMu[q][eb[e]];
    }
    return b;
}
constexpr FrcBasis kFrcBasis = frc_basis();

template <int KB>
NPG_HD double frc_N(int q, int k) {
    if constexpr (KB == 6) return kFrcBasis.N2[q][k];
    else return kFrcBasis.N1[q][k];
}

// the cell's local node (0 .. 9, the order of fe.p2_tables) behind face function k of local face kf
NPG_HD int frc_local_node(int kf, int k) {
    const int v0 = kf == 0 ? 1 : 0, v1 = kf <= 1 ? 2 : 1, v2 = kf == 3 ? 2 : 3;          // the face's vertices, ascending
    if (k == 0) return v0;
    if (k == 1) return v1;
    if (k == 2) return v2;
    const int a = k == 5 ? v1 : v0, b = k == 3 ? v1 : v2;                                  // edges (0,1) (0,2) (1,2) of the face
    return b == 3 ? 7 + a : (a == 0 ? 3 + b : 6);                                          // (0,1) (0,2) (1,2) (0,3) (1,3) (2,3) -> 4 .. 9
}

// what pass 1 and the matrix kernel read ([key][point][face] tables; device pointers in the device library)
struct FrcFaces {
    int64_t nface;
    const double *area2;                  // [nface]
    const double *ser[kFrcNSeries];       // [nkey][9][nface] or null
    const double *gamma;                  // [9][nface] or null
    int32_t nkey[kFrcNSeries], key[kFrcNSeries];
    double w[kFrcNSeries];
    NPG_HD bool has(int c) const { return ser[c] != nullptr; }
    NPG_HD double at(int c, int q, int64_t f) const {
        const size_t nf = (size_t)nface;
        const double a = ser[c][((size_t)key[c] * kBndQ + q) * nf + f];
        if (w[c] == 0.0) return a;
        const int32_t k1 = key[c] + 1 < nkey[c] ? key[c] + 1 : 0;
        const double b = ser[c][((size_t)k1 * kBndQ + q) * nf + f];
        return (1.0 - w[c]) * a + w[c] * b;
    }
    NPG_HD double g(int q, int64_t f) const { return gamma[(size_t)q * (size_t)nface + f]; }
    NPG_HD bool has_flux() const { return has(2) || (has(3) && gamma != nullptr); }
};

// out[k] = sum_q (w_q area2) v[q] N_k(q)
template <int KB>
NPG_HD void frc_contract(double area2, const double v[kBndQ], double out[KB]) {
    double wv[kBndQ];
NPG_UNROLL
    for (int q = 0; q < kBndQ; ++q) wv[q] = (kBndW[q] * area2) * v[q];
NPG_UNROLL
    for (int k = 0; k < KB; ++k) {
        double s = 0.0;
NPG_UNROLL
        for (int q = 0; q < kBndQ; ++q) s += wv[q] * frc_N<KB>(q, k);
        out[k] = s;
    }
}

// pass 1 of face f: loc[(c kFrcK + k) nface + f]; a load without tables gets zeros.  KB: the buoyancy's face functions (6 or 3)
template <int KB>
NPG_HD void frc_face_loads(const FrcFaces &t, int64_t f, double *loc) {
    const size_t nf = (size_t)t.nface;
    const double area2 = t.area2[f];
    double v[kBndQ], out[kFrcK];
    for (int c = 0; c < 2; ++c) {
        if (t.has(c)) {
NPG_UNROLL
            for (int q = 0; q < kBndQ; ++q) v[q] = t.at(c, q, f);
            frc_contract<kFrcK>(area2, v, out);
        } else {
NPG_UNROLL
            for (int k = 0; k < kFrcK; ++k) out[k] = 0.0;
        }
NPG_UNROLL
        for (int k = 0; k < kFrcK; ++k) loc[((size_t)c * kFrcK + k) * nf + f] = out[k];
    }
NPG_UNROLL
    for (int k = 0; k < kFrcK; ++k) out[k] = 0.0;
    if (t.has_flux()) {
        const bool hf = t.has(2), hr = t.has(3) && t.gamma != nullptr;
NPG_UNROLL
        for (int q = 0; q < kBndQ; ++q) {
            double x = hf ? t.at(2, q, f) : 0.0;
            if (hr) x = x + t.g(q, f) * t.at(3, q, f);
            v[q] = x;
        }
        frc_contract<KB>(area2, v, out);
    }
NPG_UNROLL
    for (int k = 0; k < KB; ++k) loc[((size_t)2 * kFrcK + k) * nf + f] = out[k];
}

// pass 2 of row r of [the n_inv inversion rows | the n_b buoyancy rows]
NPG_HD void frc_gather_row(int64_t r, int64_t n_inv, const int32_t *ptr, const int32_t *slot, const double *loc, double alpha,
                           const double *base, double *inv_out, double *flux_out) {
    const int32_t lo = ptr[r], hi = ptr[r + 1];
    double s = 0.0;
    for (int32_t i = lo; i < hi; ++i) s += loc[slot[i]];
    if (r < n_inv) inv_out[r] = hi > lo ? base[r] + alpha * s : base[r];
    else flux_out[r - n_inv] = hi > lo ? alpha * s : 0.0;
}

// entry e of the surface matrix: its slots (face, code = i KB + j) added in order
template <int KB>
NPG_HD double frc_matrix_entry(const FrcFaces &t, const int32_t *eptr, const int32_t *eface, const uint8_t *ecode, int64_t e) {
    double s = 0.0;
    for (int32_t i = eptr[e]; i < eptr[e + 1]; ++i) {
        const int64_t f = eface[i];
        const int a = ecode[i] / KB, b = ecode[i] % KB;
        const double area2 = t.area2[f];
        double m = 0.0;
        for (int q = 0; q < kBndQ; ++q) m += ((kBndW[q] * area2) * t.g(q, f)) * (frc_N<KB>(q, a) * frc_N<KB>(q, b));
        s += m;
    }
    return s;
}

// The plan of a handle, built on the host at create by both libraries: the slots of pass 2 and of the matrix.
struct FrcPlan {
    int kb = 6;                           // the buoyancy's face functions
    std::vector<int32_t> gptr, gslot;     // [n_inv + n_b + 1], [nslot]: positions in loc
    std::vector<int32_t> eptr, eface;     // [nent + 1], [nmslot]
    std::vector<uint8_t> ecode;           // [nmslot]
    std::vector<int64_t> epos;            // [nent]: the entry's position in the values of a matrix with the pattern
    bool has_pattern = false;
    int64_t pat_m = 0, pat_nnz = 0;
    int64_t wind_slots = 0, flux_slots = 0;
};

// npg_forcing_create's validation and plan, for both libraries: "" or what is wrong (nothing has been allocated or launched yet).
// V: the engine's DoF codes (a CellView over HOST memory); rowptr / col: the "b" pattern on the host, or null (no surface matrix).
template <class V>
inline std::string frc_build_plan(const V &view, int64_t n_inv, int64_t n_b, int64_t nface, const int32_t *face_cell, const uint8_t *face_local,
                                  const double *face_area2, int64_t pat_m, const int64_t *rowptr, const int32_t *col, FrcPlan &pl) {
    if (nface < 0 || (int64_t)kFrcNLoad * kFrcK * nface > INT32_MAX) return "npg_forcing_create: nface must be 0 .. (2^31 - 1) / 18";
    if (nface > 0 && !(face_cell && face_local && face_area2)) return "npg_forcing_create: NULL face table";
    if (n_inv + n_b + 1 > INT32_MAX) return "npg_forcing_create: more than 2^31 - 2 rows";
    for (int64_t f = 0; f < nface; ++f) {
        const char *what = nullptr;
        if (face_cell[f] < 0 || face_cell[f] >= view.ncell) what = "face_cell is out of range";
        else if (face_local[f] > 3) what = "face_local must be 0 .. 3";
        else if (!std::isfinite(face_area2[f]) || face_area2[f] < 0.0) what = "face_area2 must be finite and >= 0";
        if (what) return msgf("npg_forcing_create: face %lld: %s", (long long)f, what);
    }
    if (rowptr && pat_m != n_b) return msgf("npg_forcing_create: the pattern has %lld rows, the buoyancy has %lld unknowns", (long long)pat_m, (long long)n_b);
    const int kb = pl.kb = view.nb == 10 ? 6 : 3;
    // pass 2: count, offsets, fill - faces ascending, k ascending: a row's slots are sorted by (face, k)
    const int64_t R = n_inv + n_b;
    pl.gptr.assign((size_t)R + 1, 0);
    auto row_of = [&](int64_t f, int c, int k) -> int64_t {
        const int ln = frc_local_node(face_local[f], k);
        if (c < 2) {
            const int32_t code = view.cu(3 * ln + c, face_cell[f]);
            return code >= 0 ? (int64_t)code : -1;
        }
        if (k >= kb) return -1;
        const int32_t code = view.cb(ln, face_cell[f]);
        return code >= 0 ? n_inv + code : -1;
    };
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<int32_t> next;
        if (pass) {
            for (int64_t r = 0; r < R; ++r) pl.gptr[(size_t)r + 1] += pl.gptr[(size_t)r];
            pl.gslot.assign((size_t)pl.gptr[(size_t)R], 0);
            next.assign(pl.gptr.begin(), pl.gptr.end() - 1);
        }
        for (int64_t f = 0; f < nface; ++f)
            for (int k = 0; k < kFrcK; ++k)
                for (int c = 0; c < kFrcNLoad; ++c) {
                    const int64_t r = row_of(f, c, k);
                    if (r < 0) continue;
                    if (r >= R) return msgf("npg_forcing_create: face %lld: a DoF code is out of range", (long long)f);
                    if (!pass) ++pl.gptr[(size_t)r + 1];
                    else pl.gslot[(size_t)next[(size_t)r]++] = (int32_t)(((int64_t)c * kFrcK + k) * nface + f);
                }
    }
    pl.wind_slots = pl.gptr[(size_t)n_inv];
    pl.flux_slots = pl.gptr[(size_t)R] - pl.gptr[(size_t)n_inv];
    // the matrix: (position, face, code) of every pair of free face functions, sorted by (position, face, code)
    pl.has_pattern = rowptr != nullptr;
    pl.eptr.assign(1, 0);
    pl.eface.clear(), pl.ecode.clear(), pl.epos.clear();
    if (!rowptr) return "";
    pl.pat_m = pat_m, pl.pat_nnz = rowptr[pat_m];
    struct Slot {
        int64_t pos;
        int32_t face;
        uint8_t code;
    };
    std::vector<Slot> slots;
    for (int64_t f = 0; f < nface; ++f)
        for (int i = 0; i < kb; ++i) {
            const int32_t ri = view.cb(frc_local_node(face_local[f], i), face_cell[f]);
            if (ri < 0) continue;
            for (int j = 0; j < kb; ++j) {
                const int32_t cj = view.cb(frc_local_node(face_local[f], j), face_cell[f]);
                if (cj < 0) continue;
                const int32_t *b = col + rowptr[ri], *e = col + rowptr[ri + 1];
                const int32_t *p = std::lower_bound(b, e, cj);
                if (p == e || *p != cj)
                    return msgf("npg_forcing_create: face %lld: entry (%d, %d) is not in the pattern", (long long)f, ri, cj);
                slots.push_back(Slot{(int64_t)(p - col), (int32_t)f, (uint8_t)(i * kb + j)});
            }
        }
    if (slots.size() > (size_t)INT32_MAX) return "npg_forcing_create: more than 2^31 - 1 matrix slots";
    std::sort(slots.begin(), slots.end(), [](const Slot &a, const Slot &b) {
        return a.pos != b.pos ? a.pos < b.pos : (a.face != b.face ? a.face < b.face : a.code < b.code);
    });
    for (size_t i = 0; i < slots.size(); ++i) {
        if (i == 0 || slots[i].pos != slots[i - 1].pos) {
            if (i) pl.eptr.push_back((int32_t)i);
            pl.epos.push_back(slots[i].pos);
        }
        pl.eface.push_back(slots[i].face), pl.ecode.push_back(slots[i].code);
    }
    if (!slots.empty()) pl.eptr.push_back((int32_t)slots.size());
    return "";
}

// a table [n][9][nface] of npg_forcing_set_series / set_gamma: finite, gamma >= 0
inline std::string frc_check_table(const char *who, const double *table, int64_t n, int64_t nface, bool nonneg) {
    for (int64_t i = 0; i < n * kBndQ * nface; ++i) {
        if (!std::isfinite(table[i]) || (nonneg && table[i] < 0.0))
            return msgf("%s: the table is %s at keyframe %lld, point %d of face %lld", who, std::isfinite(table[i]) ? "negative" : "not finite",
                        (long long)(i / (kBndQ * nface)), (int)((i / nface) % kBndQ), (long long)(i % nface));
    }
    return "";
}

// npg_forcing_apply's arguments, for both libraries
inline std::string frc_check_apply(const int32_t *key, const double *w, double alpha, const int32_t nkey[kFrcNSeries], int64_t n_inv, int64_t n_b,
                                   bool have_all, int64_t base_n, int64_t inv_n, int64_t flux_n, bool aliased, bool one_ctx) {
    if (!have_all || !key || !w) return "npg_forcing_apply: NULL argument";
    if (!std::isfinite(alpha)) return "npg_forcing_apply: alpha is not finite";
    for (int c = 0; c < kFrcNSeries; ++c) {
        if (nkey[c] == 0) continue;
        if (key[c] < 0 || key[c] >= nkey[c]) return msgf("npg_forcing_apply: series %d: key %d is outside its %d keyframes", c, key[c], nkey[c]);
        if (!(w[c] >= 0.0 && w[c] <= 1.0)) return msgf("npg_forcing_apply: series %d: the weight must be in [0, 1], got %g", c, w[c]);
    }
    if (base_n != n_inv || inv_n != n_inv)
        return msgf("npg_forcing_apply: b_inv_base and b_inv_out have %lld and %lld entries, expected %lld", (long long)base_n, (long long)inv_n, (long long)n_inv);
    if (flux_n != n_b) return msgf("npg_forcing_apply: rhs_flux_out has %lld entries, expected %lld", (long long)flux_n, (long long)n_b);
    if (aliased) return "npg_forcing_apply: b_inv_out must not be b_inv_base";
    if (!one_ctx) return "npg_forcing_apply: arguments of different contexts";
    return "";
}

}  // namespace npg
