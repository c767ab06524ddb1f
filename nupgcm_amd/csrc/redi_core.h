// Isoneutral mixing of the passive tracers (npg_tracers_isoneutral_*): the small-slope rotated diffusion tensor of the
// running buoyancy.  The arithmetic shared by the device kernels (tracers.hip) and the host library (csrc_host/nupgcm_host.cpp), as
// tracers_core.h is for the right-hand side: both evaluate the same expressions, point by point.  The reference has no counterpart.
//
// With B = N2 z + b' in mesh coordinates, at a quadrature point
//
//    Bz+ = max(d_z B, bz_min),     S = -grad_h B / Bz+,     S <- S min(1, slope_max / |S|)
//
//    K = kappa_iso [ 1    0    S_x  ]  + kappa_v z z'          v' K_iso v = kappa_iso ((v_x + S_x v_z)^2 + (v_y + S_y v_z)^2) >= 0
//                  [ 0    1    S_y  ]
//                  [ S_x  S_y  |S|^2 ]
//
// cell_redi_update   the three tables kxz = kappa_iso S_x, kyz = kappa_iso S_y, kzz = kappa_iso |S|^2 of ONE cell and how many of its
//                    points were floored (d_z B < bz_min) and clipped (|S| > slope_max)
// redi_entry         what one quadrature point adds to entry (i, j) of K_iso: with S = 0 the three slope products are exact zeros
//                    added to the kappa_h form of npg_fe_assemble_matrix(NPG_MAT_KH)
// check_redi         every argument check of the entry points, for both libraries
//
// Everything here is fp64 whatever npg_fe_set_precision says: the slope divides by a floored small number.
//
// S: the shape tables - dNb[4 (NB q + i) + k].  T: the cell tables (cell_view.h) - G(k, c), b(x, i, c) (nodal buoyancy, Dirichlet
// nodes included), at(q, nq, c) (where point q of cell c lives in a [nq] per cell table).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "cell_view.h"

namespace npg {

enum { kRediOff = 0, kRediSet = 1, kRediUpdated = 2 };      // the state npg_tracers_isoneutral_info reports

// the tracers' view of the cell tables with the mode on: the engine's tables, kappa_iso and the three tensor tables ([nq] per cell in
// the view's layout)
template <class View>
struct RediCells : View {
    const double *kiso_, *kxz_, *kyz_, *kzz_;
    NPG_HD size_t loc(int i, int64_t c) const { return this->at(i, this->nb, c); }
    NPG_HD double kiso(int q, int64_t c) const { return kiso_[this->at(q, this->nq, c)]; }
    NPG_HD double kxz(int q, int64_t c) const { return kxz_[this->at(q, this->nq, c)]; }
    NPG_HD double kyz(int q, int64_t c) const { return kyz_[this->at(q, this->nq, c)]; }
    NPG_HD double kzz(int q, int64_t c) const { return kzz_[this->at(q, this->nq, c)]; }
};

template <int NB, class S, class T>
NPG_HD void cell_redi_update(const S &s, const T &t, int nq, double N2, const double *b, const double *kiso, double slope_max, double bz_min,
                             int64_t c, double *kxz, double *kyz, double *kzz, int &nfloor, int &nclip) {
    double G[12], bn[NB];
NPG_UNROLL
    for (int k = 0; k < 12; ++k) G[k] = t.G(k, c);
NPG_UNROLL
    for (int i = 0; i < NB; ++i) bn[i] = t.b(b, i, c);
    for (int q = 0; q < nq; ++q) {
        double gl0 = 0, gl1 = 0, gl2 = 0, gl3 = 0;
NPG_UNROLL
        for (int i = 0; i < NB; ++i) {
            const double *dn = &s.dNb[(q * NB + i) * 4];
            gl0 += dn[0] * bn[i];
            gl1 += dn[1] * bn[i];
            gl2 += dn[2] * bn[i];
            gl3 += dn[3] * bn[i];
        }
        const double gx = gl0 * G[0] + gl1 * G[3] + gl2 * G[6] + gl3 * G[9];
        const double gy = gl0 * G[1] + gl1 * G[4] + gl2 * G[7] + gl3 * G[10];
        const double gz = gl0 * G[2] + gl1 * G[5] + gl2 * G[8] + gl3 * G[11];
        const double Bz = N2 + gz;
        const bool floored = Bz < bz_min;
        const double Bzp = floored ? bz_min : Bz;
        double sx = -gx / Bzp, sy = -gy / Bzp;
        const double smag = sqrt(sx * sx + sy * sy);
        const bool clipped = smag > slope_max;
        if (clipped) {
            const double f = slope_max / smag;
            sx *= f;
            sy *= f;
        }
        nfloor += floored;
        nclip += clipped;
        const size_t o = t.at(q, nq, c);
        const double k = kiso[o];
        kxz[o] = k * sx;
        kyz[o] = k * sy;
        kzz[o] = k * (sx * sx + sy * sy);
    }
}

// w = qw wdet; gi, gj: the physical gradients of the row's and the column's basis function at the point
NPG_HD double redi_entry(double w, double kiso, double kxz, double kyz, double kzz, double gix, double giy, double giz, double gjx,
                         double gjy, double gjz) {
    const double wk = w * kiso;
    return wk * (gix * gjx + giy * gjy) + w * (kxz * (gix * gjz + giz * gjx) + kyz * (giy * gjz + giz * gjy) + kzz * (giz * gjz));
}

// ---- the argument checks of npg_tracers_isoneutral_set / _update / _matrix and of npg_tracers_rhs with the mode on ("" = fine) ----
struct RediCheck {
    const char *who;
    // set: the table (may be null = switch off), its length, the thresholds, whether the engine is an embedded 2-D one
    bool set = false;
    const double *kiso = nullptr;
    int64_t npts = 0;
    double slope_max = 0.0, bz_min = 1.0;
    bool flat = false;
    // update / matrix / rhs: the state the call needs (kRediSet or kRediUpdated) and the one the handle is in
    int need = kRediOff, state = kRediOff;
    // update: the buoyancy vector and N2
    int64_t n_b = 0, vec_n = -1;
    double N2 = 0.0;
    // matrix: its shape and whether it is a plain CSR matrix
    int64_t mat_m = -1, mat_n = -1;
    bool mat_plain = true;
};

inline std::string check_redi(const RediCheck &a) {
    if (a.set) {
        if (a.flat) return msgf("%s: an embedded 2-D engine is refused (its buoyancy surfaces are lines; the tensor is written for tetrahedra)", a.who);
        if (!a.kiso) return "";
        if (!std::isfinite(a.slope_max) || a.slope_max < 0.0) return msgf("%s: slope_max must be finite and >= 0, got %g", a.who, a.slope_max);
        if (!std::isfinite(a.bz_min) || a.bz_min <= 0.0) return msgf("%s: bz_min must be finite and > 0, got %g", a.who, a.bz_min);
        for (int64_t k = 0; k < a.npts; ++k)
            if (!std::isfinite(a.kiso[k]) || a.kiso[k] < 0.0)
                return msgf("%s: kappa_iso must be finite and >= 0, entry %lld is %g", a.who, (long long)k, a.kiso[k]);
        return "";
    }
    if (a.need == kRediSet && a.state == kRediOff) return msgf("%s: isoneutral mixing is off (npg_tracers_set_isoneutral has not been called)", a.who);
    if (a.need == kRediUpdated && a.state != kRediUpdated)
        return msgf("%s: the tensor has not been updated since npg_tracers_set_isoneutral (call npg_tracers_isoneutral_update first)", a.who);
    if (a.vec_n >= 0) {
        if (a.vec_n != a.n_b) return msgf("%s: the buoyancy vector has %lld entries, expected n_b = %lld", a.who, (long long)a.vec_n, (long long)a.n_b);
        if (!std::isfinite(a.N2)) return msgf("%s: N2 must be finite", a.who);
    }
    if (a.mat_m >= 0) {
        if (!a.mat_plain) return msgf("%s: the matrix is not a plain CSR matrix on the buoyancy pattern", a.who);
        if (a.mat_m != a.n_b || a.mat_n != a.n_b)
            return msgf("%s: the matrix is %lld x %lld, not the buoyancy pattern (n_b = %lld)", a.who, (long long)a.mat_m, (long long)a.mat_n,
                        (long long)a.n_b);
    }
    return "";
}

}  // namespace npg
