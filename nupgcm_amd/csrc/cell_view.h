// The element engine's cell tables as every diagnostic reads them, cell by cell: ONE accessor template for the device library
// (tables [component][cell], built from FeDev: cell_view() of fe_dev.h) and the host library (tables [cell][component], built from the
// host npg_fe: csrc_host/nupgcm_host.cpp).  The two differ in the index map alone.  The *_core.h templates take it as their `T`; what a
// diagnostic reads beside the engine's tables (y / z of the cells' vertices, the tracers' slot index, the sorted face tables) is a small
// struct DERIVED from the view next to the arithmetic that reads it.  Also the checks of the state vectors that the entry points of
// both libraries share (check_state_vectors).
#pragma once
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>

#if defined(__HIPCC__)
#define NPG_HD __host__ __device__ __forceinline__
#define NPG_UNROLL _Pragma("unroll")
#else
#define NPG_HD inline
#define NPG_UNROLL
#endif

namespace npg {

// the value of DoF code idx: an unknown of x, or (idx < 0) entry -1 - idx of the Dirichlet value table
NPG_HD double field_val(const double *x, const double *diri, int32_t idx) { return idx >= 0 ? x[idx] : diri[-1 - idx]; }

// where component k (of n) of cell c (of ncell) lives in a table
struct CompMajor {       // [component][cell]: unit stride across the lanes of a wave
    static NPG_HD size_t at(int k, int, int64_t c, int64_t ncell) { return (size_t)k * ncell + c; }
};
struct CellMajor {       // [cell][component]
    static NPG_HD size_t at(int k, int n, int64_t c, int64_t) { return (size_t)c * n + k; }
};

template <class Map>
struct CellView {
    const int32_t *cu_, *cp_, *cb_;          // DoF codes: 30 velocity, 4 pressure, nb buoyancy per cell
    const double *G_, *udiri, *bdiri;        // grad lambda (component 3 vertex + axis); the Dirichlet value tables
    int64_t ncell;
    int nb;                                  // buoyancy nodes per cell (10 or 4)
    const double *wdet_;
    const double *nu_, *kh_, *kv_;           // [nq] per cell, or null
    int nq;
    NPG_HD size_t at(int k, int n, int64_t c) const { return Map::at(k, n, c, ncell); }
    NPG_HD int32_t cu(int l, int64_t c) const { return cu_[at(l, 30, c)]; }
    NPG_HD int32_t cp(int m, int64_t c) const { return cp_[at(m, 4, c)]; }
    NPG_HD int32_t cb(int i, int64_t c) const { return cb_[at(i, nb, c)]; }
    NPG_HD double G(int k, int64_t c) const { return G_[at(k, 12, c)]; }
    NPG_HD double wdet(int64_t c) const { return wdet_[c]; }
    NPG_HD double u(const double *x, int l, int64_t c) const { return field_val(x, udiri, cu(l, c)); }
    NPG_HD double p(const double *x, int m, int64_t c) const {
        const int32_t i = cp(m, c);
        return i >= 0 ? x[i] : 0.0;          // the pinned vertex of the zero-mean space
    }
    NPG_HD double b(const double *x, int i, int64_t c) const { return field_val(x, bdiri, cb(i, c)); }
    NPG_HD bool has_nu() const { return nu_ != nullptr; }
    NPG_HD bool has_kh() const { return kh_ != nullptr; }
    NPG_HD bool has_kv() const { return kv_ != nullptr; }
    NPG_HD double nu(int q, int64_t c) const { return nu_[at(q, nq, c)]; }
    NPG_HD double kh(int q, int64_t c) const { return kh_[at(q, nq, c)]; }
    NPG_HD double kv(int q, int64_t c) const { return kv_[at(q, nq, c)]; }
};

// the view and y / z of the cells' own vertices, 4 per cell in the view's layout (integrals: cz alone; classes: both)
template <class View>
struct CellsYZ : View {
    const double *cy, *cz;
    NPG_HD double y(int i, int64_t c) const { return cy[this->at(i, 4, c)]; }
    NPG_HD double z(int i, int64_t c) const { return cz[this->at(i, 4, c)]; }
};

// printf into a message
inline std::string msgf(const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return buf;
}

// the sizes of the state vectors of an entry point `who` (empty: fine)
inline std::string check_state_vectors(const char *who, int64_t n_inv, int64_t n_b, int64_t x_inv_n, int64_t b_n) {
    if (x_inv_n != n_inv) return msgf("%s: the flow vector has %lld entries, expected %lld", who, (long long)x_inv_n, (long long)n_inv);
    if (b_n != n_b) return msgf("%s: the buoyancy vector has %lld entries, expected %lld", who, (long long)b_n, (long long)n_b);
    return "";
}

}  // namespace npg
