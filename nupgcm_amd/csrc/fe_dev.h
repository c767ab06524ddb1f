// The element engine's device tables and handle, shared by the translation units that read them (fe.hip: assembly; sample.hip:
// point evaluation of the state).
#pragma once
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

}  // namespace npg

struct npg_fe {
    npg_ctx *ctx = nullptr;
    npg::FeDev d{};
    int64_t n_inv = 0, n_b = 0;
    std::vector<void *> allocs;
    double *loc = nullptr;          // [nb][ncell]
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
