// Lagrangian particles in the device-resident flow: the arithmetic of one classical RK4 step of dx/dt = u(x, t), shared by the device
// kernel (particles.hip) and the host library (csrc_host/nupgcm_host.cpp), as sample_core.h and integrals_core.h are.  A step is
// locate -> evaluate -> next stage, four times, plus the location of the end point; the cell of the last located point is remembered
// and tried first (locate_cached), so a particle that stays in its cell never looks at the bins.
//
// Time: the velocity is the blend (1 - s) u_a + s u_b of two vectors [u; p], s linear in model time over the call - model time is the
// particle's clock, since the nondimensional buoyancy equation carries the same factor in front of d_t b and u . grad b.
// Always fp64 (npg_fe_set_precision does not apply).
//
// Periodic axes: L[a] > 0 is the period of axis a (0 = not periodic), the lower bound is the locator's box.  A stage point is wrapped
// into [lo, lo + L) for its location only; the stored position is wrapped after the step and wind[a] counts the crossings, so that the
// unwrapped position is x + wind L.
//
// Leaving the mesh: a step in which a stage point or the end point is not located does not happen - the particle keeps the state it had
// at the start of that step and is LOST (status 1, t_lost = the time at the start of that step).  No reflection, no projection.
#pragma once
#include "sample_core.h"

namespace npg {

constexpr double kCacheTol = 1e-8;      // the remembered cell is taken without an election when the point's min lambda there is >= this
constexpr double kMaxWind = 1073741824.0;   // a point further than 2^30 periods away is not wrapped: it is not located

// what a step reads of the locator and the period
struct ParticleMesh {
    BinGrid g;
    const int32_t *bin_ptr, *bin_cells;
    const double *geo;
    double L[3];
};

// one call of npg_particles_advance: nsub steps of h = dt / nsub from time t, s = s0 + ds * (tau / dt), tau from the start of the call
struct ParticleCall {
    double t, h, s0, ds, dt;
};

// a live particle between two steps: x in [lo, lo + L) on the periodic axes, c and lam its location
struct ParticleState {
    double x[3], lam[4];
    int32_t c, wind[3];
};

// locate_point with a first guess: lambda in cell c by the expressions of locate_point, in their order; min lambda >= kCacheTol means
// strictly interior, and since the cells do not overlap the election would choose c with these very lambda - the bins are not read.
// Any other point (and c < 0) goes through locate_point<false>: the result has the bits of locate_point for every point.
NPG_HD void locate_cached(const ParticleMesh &m, int32_t c, const double p[3], int32_t *cell, double lam[4]) {
    if (c >= 0) {
        const double *q = m.geo + (size_t)c * kGeoStride;
        const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
        const double l1 = q[3] * dx + q[4] * dy + q[5] * dz;
        const double l2 = q[6] * dx + q[7] * dy + q[8] * dz;
        const double l3 = q[9] * dx + q[10] * dy + q[11] * dz;
        const double l0 = 1.0 - (l1 + l2 + l3);
        if (fmin(fmin(l0, l1), fmin(l2, l3)) >= kCacheTol) {      // NaN: false
            *cell = c;
            lam[0] = l0, lam[1] = l1, lam[2] = l2, lam[3] = l3;
            return;
        }
    }
    locate_point<false>(m.g, m.bin_ptr, m.bin_cells, m.geo, p, cell, lam);
}

// p wrapped into [lo, lo + L) on the periodic axes, k[a] = the periods taken off (p = w + k L).  false: not finite or out of range.
NPG_HD bool wrap_point(const ParticleMesh &m, const double p[3], double w[3], int32_t k[3]) {
    bool ok = true;
NPG_UNROLL
    for (int a = 0; a < 3; ++a) {
        w[a] = p[a], k[a] = 0;
        if (m.L[a] > 0.0) {
            const double lo = m.g.lo[a], L = m.L[a];
            double kk = floor((p[a] - lo) / L);
            if (!(fabs(kk) <= kMaxWind)) {     // NaN, infinite or absurdly far: left as it is, locate_point refuses it
                ok = false;
                continue;
            }
            double x = p[a] - kk * L;
            if (x < lo) x += L, kk -= 1.0;                 // the rounding of the quotient at a multiple of L
            else if (x >= lo + L) x -= L, kk += 1.0;
            w[a] = x, k[a] = (int32_t)kk;
        }
    }
    return ok;
}

// the location of point p (wrapped for this purpose only), starting from cell c; false = outside the mesh
NPG_HD bool locate_stage(const ParticleMesh &m, int32_t c, const double p[3], int32_t *cell, double lam[4]) {
    double w[3];
    int32_t k[3];
    if (!wrap_point(m, p, w, k)) return false;
    locate_cached(m, c, w, cell, lam);
    return *cell >= 0;
}

// u at a located point and stage parameter s: u_a and u_b evaluated one after the other from the same lambda (the 30 nodal values are
// live once), blended; BLEND = false (x_a and x_b are the same vector): one evaluation, no arithmetic on it
template <bool BLEND, class T>
NPG_HD void stage_velocity(const T &t, const double *xa, const double *xb, double s, int64_t c, const double l[4], double u[3]) {
    sample_point(t, NPG_SAMPLE_U, xa, c, l, u);
    if (BLEND) {
        double ub[3];
        sample_point(t, NPG_SAMPLE_U, xb, c, l, ub);
NPG_UNROLL
        for (int a = 0; a < 3; ++a) u[a] = (1.0 - s) * u[a] + s * ub[a];
    }
}

NPG_HD double stage_parameter(const ParticleCall &k, double tau) { return k.s0 + k.ds * (k.dt != 0.0 ? tau / k.dt : 0.0); }

// A particle enters a call: its stored position wrapped (a fresh seed may lie periods away) and located from its remembered cell.
// false = lost at the start of the call; p is then untouched.
NPG_HD bool particle_enter(const ParticleMesh &m, ParticleState &p) {
    double w[3], lam[4];
    int32_t k[3], c;
    if (!wrap_point(m, p.x, w, k)) return false;
    locate_cached(m, p.c, w, &c, lam);
    if (c < 0) return false;
NPG_UNROLL
    for (int a = 0; a < 3; ++a) p.x[a] = w[a], p.wind[a] += k[a];
NPG_UNROLL
    for (int i = 0; i < 4; ++i) p.lam[i] = lam[i];
    p.c = c;
    return true;
}

// Step j of the call: stage points x, x + h/2 k1, x + h/2 k2, x + h k3 at s(tau), s(tau + h/2), s(tau + h/2), s(tau + h) with
// tau = j h; x+ = x + h/6 (k1 + 2 k2 + 2 k3 + k4), wrapped and located.  false = a point was not located: p is untouched.
template <bool BLEND, class T>
NPG_HD bool rk4_step(const ParticleMesh &m, const T &t, const double *xa, const double *xb, const ParticleCall &call, int64_t j,
                     ParticleState &p) {
    const double h = call.h;
    const double s1 = BLEND ? stage_parameter(call, (double)j * h) : 0.0;
    const double s2 = BLEND ? stage_parameter(call, ((double)j + 0.5) * h) : 0.0;
    const double s4 = BLEND ? stage_parameter(call, ((double)j + 1.0) * h) : 0.0;
    double k[3], acc[3], y[3], lam[4];
    int32_t c = p.c;
    stage_velocity<BLEND>(t, xa, xb, s1, c, p.lam, k);
NPG_UNROLL
    for (int a = 0; a < 3; ++a) acc[a] = k[a], y[a] = p.x[a] + (0.5 * h) * k[a];
    if (!locate_stage(m, c, y, &c, lam)) return false;
    stage_velocity<BLEND>(t, xa, xb, s2, c, lam, k);
NPG_UNROLL
    for (int a = 0; a < 3; ++a) acc[a] += 2.0 * k[a], y[a] = p.x[a] + (0.5 * h) * k[a];
    if (!locate_stage(m, c, y, &c, lam)) return false;
    stage_velocity<BLEND>(t, xa, xb, s2, c, lam, k);
NPG_UNROLL
    for (int a = 0; a < 3; ++a) acc[a] += 2.0 * k[a], y[a] = p.x[a] + h * k[a];
    if (!locate_stage(m, c, y, &c, lam)) return false;
    stage_velocity<BLEND>(t, xa, xb, s4, c, lam, k);
NPG_UNROLL
    for (int a = 0; a < 3; ++a) y[a] = p.x[a] + (h / 6.0) * (acc[a] + k[a]);
    double w[3];
    int32_t kw[3];
    if (!wrap_point(m, y, w, kw)) return false;
    locate_cached(m, c, w, &c, lam);
    if (c < 0) return false;
NPG_UNROLL
    for (int a = 0; a < 3; ++a) p.x[a] = w[a], p.wind[a] += kw[a];
NPG_UNROLL
    for (int i = 0; i < 4; ++i) p.lam[i] = lam[i];
    p.c = c;
    return true;
}

// One particle through a call: nsub steps.  Returns the number of steps taken; fewer than nsub = lost at the start of that step, -1 =
// lost where the call found it (a seed that is NaN or outside the mesh).  p then holds the state at the start of the step that failed.
template <bool BLEND, class T>
NPG_HD int64_t particle_advance(const ParticleMesh &m, const T &t, const double *xa, const double *xb, const ParticleCall &call,
                                int64_t nsub, ParticleState &p) {
    if (!particle_enter(m, p)) return -1;
    for (int64_t j = 0; j < nsub; ++j)
        if (!rk4_step<BLEND>(m, t, xa, xb, call, j, p)) return j;
    return nsub;
}

// nullptr if the arguments of npg_particles_advance that are numbers are usable
inline const char *check_particle_call(double s0, double s1, double dt, int64_t nsub) {
    if (!(nsub >= 1 && nsub <= ((int64_t)1 << 20))) return "nsub must be 1 .. 2^20";
    if (!std::isfinite(dt)) return "dt is not finite";
    if (!std::isfinite(s0) || !std::isfinite(s1)) return "s0 and s1 must be finite";
    return nullptr;
}

inline ParticleCall make_particle_call(double t, double s0, double s1, double dt, int64_t nsub) {
    return ParticleCall{t, dt / (double)nsub, s0, s1 - s0, dt};
}

}  // namespace npg
