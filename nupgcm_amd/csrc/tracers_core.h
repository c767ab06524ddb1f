// Passive tracers carried by the flow (npg_tracers_rhs): what ONE cell adds to the local vectors of K tracers.  The arithmetic shared
// by the device kernel (tracers.hip) and the host library (csrc_host/nupgcm_host.cpp), as integrals_core.h is for the mesh integrals:
// GPU() and CPU() evaluate the same expressions in the same order, cell by cell.
//
// For tracer k with nodal values c, c_prev (Dirichlet nodes take the tracer's OWN Dirichlet values), background gradient Gamma_k (the
// full tracer is Gamma_k z + c) and uniform source S_k, with the scheme constants of k_advection_local (fe.hip):
//
//    loc_k[i] = int ( c1 c + c2 c_prev - cdt ( u~ . grad c~ + u~_z Gamma_k - S_k ) ) phi_i
//             - int ( c_D phi_i + theta ( kappa_h grad_h c_D . grad_h phi_i + kappa_v d_z c_D d_z phi_i ) ),   c_D = sum_{j Dirichlet} c_D,j phi_j
//
// u~ = e1 u + e2 u_prev at the quadrature points is evaluated ONCE per cell, before the loop over the tracers: the 30 scattered
// velocity values, the geometry and the velocity shape functions are not touched again.  The loop over the tracers reloads the nodal
// values per tracer; only G, wdet and the nq x 3 velocities live across it.  The velocities are indexed by the quadrature point, a
// run-time index: the caller supplies their storage U (uq(j), j = 3 q + a) - on the device a per-lane column of LDS, because a
// register array indexed at run time goes to scratch and the fully unrolled loop spills; on the host a local array.
//
// The second integral is the Dirichlet lift, -(rhs_M + theta (rhs_h + rhs_v)) of src/evolution.jl:256-260 evaluated per cell: a
// Dirichlet node's basis function is supported on the cells that carry the node, so the lift of a row is a sum over the row's own
// cells and rides on the same gather.  It is evaluated only in cells that have a Dirichlet node with a non-zero value of the tracer.
//
// R = the type of the element-local arithmetic (double, or float under npg_fe_set_precision); the BDF combinations of the fp64 state
// are formed before rounding and the sums over quadrature points are fp64, as in k_advection_local.
//
// S: the shape tables - qw[q], N2[10 q + i], Nb[NB q + i], dNb[4 (NB q + i) + k].  T: the cell tables - G(k, c), wdet(c),
// u(x, l, c) (nodal velocity, Dirichlet nodes included), cb(i, c) (the DoF code of local node i: a row, or -1 - j for Dirichlet value
// j), kh / kv (q, c), loc(i, c) (where local entry i of cell c lives within one tracer's local block).
#pragma once
#include <cstddef>
#include <cstdint>

#include "cell_view.h"

namespace npg {

constexpr int kTrMaxQ = 16;        // = kMaxQ of the element engine

// the K tracers of one call: tracer k's vectors start at k * n_b, its Dirichlet values at k * n_diri, its local block at k * loc_stride
struct TracerSet {
    int ntracer;
    int64_t n_b, n_diri, loc_stride;
    const double *c, *c_prev;          // [ntracer][n_b]
    const double *diri;                // [ntracer][n_diri]
    const double *gamma, *source;      // [ntracer]
    double *loc;                       // [ntracer][loc_stride]
};

// the cell tables and where local entry i of cell c lives within one tracer's local block (the view's layout, nb entries per cell)
template <class View>
struct TracerCells : View {
    NPG_HD size_t loc(int i, int64_t c) const { return this->at(i, this->nb, c); }
};

// ISO (npg_tracers_set_isoneutral, redi_core.h): T is a RediCells view and the second integral becomes
//    int ( c_D phi_i + theta ( K (grad c_D + Gamma_k z) ) . grad phi_i ),      K = the rotated tensor with kzz + kappa_v,
// evaluated in every cell where the tracer has a non-zero Dirichlet value or Gamma_k != 0.  ISO = false: the instances are what they
// were before the flag existed.
template <typename R, int NB, bool ISO = false, class S, class T, class U>
NPG_HD void cell_tracers(const S &s, const T &t, U &uq, int nq, bool bdf2, double dt, double theta, const double *xi, const double *xip,
                         const TracerSet &ts, int64_t c) {
    const double c1 = bdf2 ? 4.0 / 3.0 : 1.0, c2 = bdf2 ? -1.0 / 3.0 : 0.0, e1 = bdf2 ? 2.0 : 1.0, e2 = bdf2 ? -1.0 : 0.0;
    const R cdt = (R)(bdf2 ? 2.0 / 3.0 * dt : dt), rth = (R)theta;
    R G[12];
NPG_UNROLL
    for (int k = 0; k < 12; ++k) G[k] = (R)t.G(k, c);
    const R wdet = (R)t.wdet(c);
    // u~ at the quadrature points, once
    {
        R ut[30];
NPG_UNROLL
        for (int l = 0; l < 30; ++l) ut[l] = (R)(e1 * t.u(xi, l, c) + e2 * t.u(xip, l, c));
        for (int q = 0; q < nq; ++q) {
            R ux = 0, uy = 0, uz = 0;
NPG_UNROLL
            for (int i = 0; i < 10; ++i) {
                const R n = s.N2[q * 10 + i];
                ux += n * ut[3 * i];
                uy += n * ut[3 * i + 1];
                uz += n * ut[3 * i + 2];
            }
            uq(3 * q) = ux, uq(3 * q + 1) = uy, uq(3 * q + 2) = uz;
        }
    }
    for (int k = 0; k < ts.ntracer; ++k) {
        const double *ck = ts.c + (size_t)k * ts.n_b, *cpk = ts.c_prev + (size_t)k * ts.n_b, *dk = ts.diri + (size_t)k * ts.n_diri;
        const R gam = (R)ts.gamma[k], src = (R)ts.source[k];
        R bm[NB], bt[NB];
        bool lift = false;
NPG_UNROLL
        for (int i = 0; i < NB; ++i) {
            const int32_t idx = t.cb(i, c);
            const double v = field_val(ck, dk, idx), vp = field_val(cpk, dk, idx);
            bm[i] = (R)(c1 * v + c2 * vp);
            bt[i] = (R)(e1 * v + e2 * vp);
            lift = lift || (idx < 0 && dk[-1 - idx] != 0.0);
        }
        double acc[NB];
NPG_UNROLL
        for (int i = 0; i < NB; ++i) acc[i] = 0.0;
        for (int q = 0; q < nq; ++q) {
            R bq = 0, gl0 = 0, gl1 = 0, gl2 = 0, gl3 = 0;
NPG_UNROLL
            for (int i = 0; i < NB; ++i) {
                bq += s.Nb[q * NB + i] * bm[i];
                const R *dn = &s.dNb[(q * NB + i) * 4];
                gl0 += dn[0] * bt[i];
                gl1 += dn[1] * bt[i];
                gl2 += dn[2] * bt[i];
                gl3 += dn[3] * bt[i];
            }
            const R ux = uq(3 * q), uy = uq(3 * q + 1), uz = uq(3 * q + 2);
            const R gx = gl0 * G[0] + gl1 * G[3] + gl2 * G[6] + gl3 * G[9];
            const R gy = gl0 * G[1] + gl1 * G[4] + gl2 * G[7] + gl3 * G[10];
            const R gz = gl0 * G[2] + gl1 * G[5] + gl2 * G[8] + gl3 * G[11];
            const R integrand = bq - cdt * ((ux * gx + uy * gy + uz * gz + uz * gam) - src);
            const R wq = s.qw[q] * wdet * integrand;
NPG_UNROLL
            for (int i = 0; i < NB; ++i) acc[i] += (double)(wq * s.Nb[q * NB + i]);
        }
        if (lift || (ISO && gam != (R)0)) {
            R cd[NB];
NPG_UNROLL
            for (int i = 0; i < NB; ++i) {
                const int32_t idx = t.cb(i, c);
                cd[i] = idx < 0 ? (R)dk[-1 - idx] : (R)0;
            }
            for (int q = 0; q < nq; ++q) {
                R cq = 0, gl0 = 0, gl1 = 0, gl2 = 0, gl3 = 0;
NPG_UNROLL
                for (int i = 0; i < NB; ++i) {
                    cq += s.Nb[q * NB + i] * cd[i];
                    const R *dn = &s.dNb[(q * NB + i) * 4];
                    gl0 += dn[0] * cd[i];
                    gl1 += dn[1] * cd[i];
                    gl2 += dn[2] * cd[i];
                    gl3 += dn[3] * cd[i];
                }
                const R w = s.qw[q] * wdet;
                R ax, ay, az;
                if constexpr (ISO) {
                    const R ki = (R)t.kiso(q, c), kxz = (R)t.kxz(q, c), kyz = (R)t.kyz(q, c), kzz = (R)t.kzz(q, c) + (R)t.kv(q, c);
                    const R gx = gl0 * G[0] + gl1 * G[3] + gl2 * G[6] + gl3 * G[9];
                    const R gy = gl0 * G[1] + gl1 * G[4] + gl2 * G[7] + gl3 * G[10];
                    const R gz = (gl0 * G[2] + gl1 * G[5] + gl2 * G[8] + gl3 * G[11]) + gam;
                    ax = rth * (ki * gx + kxz * gz);
                    ay = rth * (ki * gy + kyz * gz);
                    az = rth * ((kxz * gx + kyz * gy) + kzz * gz);
                } else {
                    const R kh = rth * (R)t.kh(q, c), kv = rth * (R)t.kv(q, c);
                    ax = kh * (gl0 * G[0] + gl1 * G[3] + gl2 * G[6] + gl3 * G[9]);
                    ay = kh * (gl0 * G[1] + gl1 * G[4] + gl2 * G[7] + gl3 * G[10]);
                    az = kv * (gl0 * G[2] + gl1 * G[5] + gl2 * G[8] + gl3 * G[11]);
                }
NPG_UNROLL
                for (int i = 0; i < NB; ++i) {
                    const R *dn = &s.dNb[(q * NB + i) * 4];
                    const R px = dn[0] * G[0] + dn[1] * G[3] + dn[2] * G[6] + dn[3] * G[9];
                    const R py = dn[0] * G[1] + dn[1] * G[4] + dn[2] * G[7] + dn[3] * G[10];
                    const R pz = dn[0] * G[2] + dn[1] * G[5] + dn[2] * G[8] + dn[3] * G[11];
                    acc[i] -= (double)(w * (cq * s.Nb[q * NB + i] + (ax * px + ay * py + az * pz)));
                }
            }
        }
        double *lk = ts.loc + (size_t)k * ts.loc_stride;
NPG_UNROLL
        for (int i = 0; i < NB; ++i) lk[t.loc(i, c)] = acc[i];
    }
}

// one destination row of tracer k: its cells' local entries in cell order (the engine's inverted index), then the shared diffusion
// of the background gradient and the tracer's surface flux
template <class I>
NPG_HD double tracer_row(const int64_t *gptr, const I *gidx, const double *lock, int64_t r, double theta_gamma, double dt,
                         const double *rhs_diff1, const double *fluxk) {
    double sum = 0.0;
    for (int64_t j = gptr[r]; j < gptr[r + 1]; ++j) sum += lock[gidx[j]];
    if (rhs_diff1) sum += theta_gamma * rhs_diff1[r];
    if (fluxk) sum += dt * fluxk[r];
    return sum;
}

}  // namespace npg
