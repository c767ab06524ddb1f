// Diffusing particles and reflecting walls (npg_particles_walk): the arithmetic of one step of
//     dx = u dt + c_d (d_x kappa_h, d_y kappa_h, d_z kappa_v) dt + sqrt(2 c_d kappa*) dW
// shared by the device kernel (particles.hip) and the host library (csrc_host/nupgcm_host.cpp), as particles_core.h is.  A step is
// the RK4 step of particles_core.h followed by Visser's random displacement, and EVERY move of the particle - the three stage points,
// the RK4 end point, the random displacement - is a segment walked from cell to cell through the neighbour table: across an interior
// face into the neighbour (across a periodic seam with the face's translation), off a boundary face by reflection.
//
// Generator: Philox4x32-10, key = the 64-bit seed (low, high), counter = (particle index low, high, step number low, high); words 0..2
// give R_a = (2 w_a + 1) 2^-32 - 1 in (-1, 1), exact in fp64.  One counter per particle and step, nothing consumed by a reflection: a
// path does not depend on the number or the order of the particles, nor on how an interval is cut into calls of equal h.
//
// Tables (per cell, in the locator's local vertex order): nbr[c][i] = the cell across the face opposite local vertex i, -1 = boundary;
// shift[c][i][a] = the translation in periods on axis a that a point takes when it crosses that face (x += shift L), so that wind,
// which counts the periods taken OFF (unwrapped = x + wind L, particles_core.h), changes by -shift; kappa_h[c][i], kappa_v[c][i] =
// the diffusivities at the cell's own vertices: kappa = sum lambda_i kappa_i, grad kappa = sum kappa_i grad lambda_i, constant in the
// cell.  Both are formed from the differences kappa_i - kappa_0 (grad lambda_0 = -(grad lambda_1 + .. + grad lambda_3), lambda_0 = 1 -
// ..), so that a constant kappa has gradient 0 and value kappa exactly.
//
// A step that cannot be finished - more than kMaxFaceEvents face events in one move, a neighbour table that does not lead back, an
// end point the election refuses - is not taken: the particle is STUCK (status 2), with the rule of a lost one.
#pragma once
#include "particles_core.h"

namespace npg {

constexpr int kMaxFaceEvents = 64;

struct WalkTables {
    const int32_t *nbr;          // [ncell][4]
    const int8_t *shift;         // [ncell][4][3]
    const double *kh, *kv;       // [ncell][4] each; unused without diffusion
    double cd;
    uint32_t key0, key1;         // the seed, low and high word
};

NPG_HD uint32_t mulhi32(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32); }

NPG_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
NPG_UNROLL
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = mulhi32(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = mulhi32(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0, c1 = l1, c2 = h0 ^ c3 ^ k1, c3 = l0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

// the three uniforms of particle `index` at step number `step`
NPG_HD void particle_uniforms(uint32_t key0, uint32_t key1, uint64_t index, uint64_t step, double R[3]) {
    uint32_t w[4];
    philox4x32_10((uint32_t)index, (uint32_t)(index >> 32), (uint32_t)step, (uint32_t)(step >> 32), key0, key1, w);
NPG_UNROLL
    for (int a = 0; a < 3; ++a) R[a] = (2.0 * (double)w[a] + 1.0) * 0x1p-32 - 1.0;
}

// Visser's displacement over h at a located point: drift delta = c_d h grad kappa (horizontal: kappa_h, vertical: kappa_v), the
// diffusivities taken half a drift away by the cell's own linear extension, clipped at 0, and R sqrt(6 c_d kappa* h)
NPG_HD void walk_displacement(const ParticleMesh &m, const WalkTables &w, int32_t c, const double lam[4], double h, const double R[3],
                              double d[3]) {
    const double *q = m.geo + (size_t)c * kGeoStride;
    const double *kh = w.kh + (size_t)c * 4, *kv = w.kv + (size_t)c * 4;
    const double h1 = kh[1] - kh[0], h2 = kh[2] - kh[0], h3 = kh[3] - kh[0];
    const double v1 = kv[1] - kv[0], v2 = kv[2] - kv[0], v3 = kv[3] - kv[0];
    double gh[3], gv[3], dl[3];
NPG_UNROLL
    for (int a = 0; a < 3; ++a) {
        gh[a] = h1 * q[3 + a] + h2 * q[6 + a] + h3 * q[9 + a];
        gv[a] = v1 * q[3 + a] + v2 * q[6 + a] + v3 * q[9 + a];
    }
    const double ch = w.cd * h;
    dl[0] = ch * gh[0], dl[1] = ch * gh[1], dl[2] = ch * gv[2];
    const double kap_h = kh[0] + (lam[1] * h1 + lam[2] * h2 + lam[3] * h3);
    const double kap_v = kv[0] + (lam[1] * v1 + lam[2] * v2 + lam[3] * v3);
    const double sh = fmax(kap_h + 0.5 * (dl[0] * gh[0] + dl[1] * gh[1] + dl[2] * gh[2]), 0.0);
    const double sv = fmax(kap_v + 0.5 * (dl[0] * gv[0] + dl[1] * gv[1] + dl[2] * gv[2]), 0.0);
    const double ah = sqrt(6.0 * ch * sh), av = sqrt(6.0 * ch * sv);
    d[0] = dl[0] + R[0] * ah, d[1] = dl[1] + R[1] * ah, d[2] = dl[2] + R[2] * av;
}

// move(c, lambda, x, d): the segment from p.x to p.x + d walked through the cells.  In the current cell lambda_i(x + d) = lambda_i(x)
// + grad lambda_i . d; all four >= 0: the move ends there.  Otherwise the face with lambda_i(x + d) < 0 and the smallest
// t = lambda_i(x) / (lambda_i(x) - lambda_i(x + d)), clamped to [0, 1], is crossed (ties: the lowest i) at q = x + t d with the
// remainder (1 - t) d: into the neighbour, q translated across a seam, or - a boundary face - the remainder reflected about the
// face, ++nrefl.  lambda of that face is exactly 0 at q.  The end point is located from the walk's last cell (locate_cached: the bits
// of npg_locator_find).  false = not finished (see the head of the file); p and nrefl are then meaningless.
// The faces are chosen by select chains over named values: no register array is indexed with a run-time index.
NPG_HD bool walk_move(const ParticleMesh &m, const WalkTables &w, ParticleState &p, int32_t &nrefl, const double d[3]) {
    double x0 = p.x[0], x1 = p.x[1], x2 = p.x[2];
    double r0 = d[0], r1 = d[1], r2 = d[2];
    double l0 = p.lam[0], l1 = p.lam[1], l2 = p.lam[2], l3 = p.lam[3];
    int32_t c = p.c;
    for (int ev = 0;; ++ev) {
        const double *q = m.geo + (size_t)c * kGeoStride;
        const double d1 = q[3] * r0 + q[4] * r1 + q[5] * r2;
        const double d2 = q[6] * r0 + q[7] * r1 + q[8] * r2;
        const double d3 = q[9] * r0 + q[10] * r1 + q[11] * r2;
        const double d0 = -(d1 + d2 + d3);
        const double e0 = l0 + d0, e1 = l1 + d1, e2 = l2 + d2, e3 = l3 + d3;
        if (e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0 && e3 >= 0.0) break;
        if (ev == kMaxFaceEvents) return false;
        int f = -1;
        double t = 2.0;
        if (e0 < 0.0) {
            const double s = fmin(fmax(l0 / (l0 - e0), 0.0), 1.0);
            if (s < t) t = s, f = 0;
        }
        if (e1 < 0.0) {
            const double s = fmin(fmax(l1 / (l1 - e1), 0.0), 1.0);
            if (s < t) t = s, f = 1;
        }
        if (e2 < 0.0) {
            const double s = fmin(fmax(l2 / (l2 - e2), 0.0), 1.0);
            if (s < t) t = s, f = 2;
        }
        if (e3 < 0.0) {
            const double s = fmin(fmax(l3 / (l3 - e3), 0.0), 1.0);
            if (s < t) t = s, f = 3;
        }
        if (f < 0) return false;                     // NaN
        x0 += t * r0, x1 += t * r1, x2 += t * r2;
        const double u = 1.0 - t;
        r0 *= u, r1 *= u, r2 *= u;
        const int32_t nb = w.nbr[(size_t)c * 4 + f];
        if (nb >= 0) {
            const int8_t *sh = w.shift + ((size_t)c * 4 + f) * 3;
            const int32_t s0 = sh[0], s1 = sh[1], s2 = sh[2];
            x0 += (double)s0 * m.L[0], x1 += (double)s1 * m.L[1], x2 += (double)s2 * m.L[2];
            p.wind[0] -= s0, p.wind[1] -= s1, p.wind[2] -= s2;
            const double *qn = m.geo + (size_t)nb * kGeoStride;
            const double dx = x0 - qn[0], dy = x1 - qn[1], dz = x2 - qn[2];
            l1 = qn[3] * dx + qn[4] * dy + qn[5] * dz;
            l2 = qn[6] * dx + qn[7] * dy + qn[8] * dz;
            l3 = qn[9] * dx + qn[10] * dy + qn[11] * dz;
            l0 = 1.0 - (l1 + l2 + l3);
            // the face of nb that leads back: the lowest j with nbr[nb][j] = c and the opposite translation
            const int32_t *bn = w.nbr + (size_t)nb * 4;
            const int8_t *bs = w.shift + (size_t)nb * 12;
            int back = -1;
NPG_UNROLL
            for (int j = 3; j >= 0; --j)
                if (bn[j] == c && bs[3 * j] == -s0 && bs[3 * j + 1] == -s1 && bs[3 * j + 2] == -s2) back = j;
            if (back < 0) return false;
            l0 = back == 0 ? 0.0 : l0, l1 = back == 1 ? 0.0 : l1, l2 = back == 2 ? 0.0 : l2, l3 = back == 3 ? 0.0 : l3;
            c = nb;
        } else {
            l0 = f == 0 ? 0.0 : l0 + t * d0, l1 = f == 1 ? 0.0 : l1 + t * d1;
            l2 = f == 2 ? 0.0 : l2 + t * d2, l3 = f == 3 ? 0.0 : l3 + t * d3;
            // grad lambda of the face, n = g / |g|: r <- r - 2 (r . n) n
            const double a0 = -(q[3] + q[6] + q[9]), a1 = -(q[4] + q[7] + q[10]), a2 = -(q[5] + q[8] + q[11]);
            const double g0 = f == 0 ? a0 : f == 1 ? q[3] : f == 2 ? q[6] : q[9];
            const double g1 = f == 0 ? a1 : f == 1 ? q[4] : f == 2 ? q[7] : q[10];
            const double g2 = f == 0 ? a2 : f == 1 ? q[5] : f == 2 ? q[8] : q[11];
            const double k = 2.0 * ((r0 * g0 + r1 * g1 + r2 * g2) / (g0 * g0 + g1 * g1 + g2 * g2));
            r0 -= k * g0, r1 -= k * g1, r2 -= k * g2;
            ++nrefl;
        }
    }
    const double y[3] = {x0 + r0, x1 + r1, x2 + r2};
    int32_t cell;
    double lam[4];
    locate_cached(m, c, y, &cell, lam);
    if (cell < 0) return false;
NPG_UNROLL
    for (int a = 0; a < 3; ++a) p.x[a] = y[a];
NPG_UNROLL
    for (int i = 0; i < 4; ++i) p.lam[i] = lam[i];
    p.c = cell;
    return true;
}

// a stage point: the state's own copy walked by d; wind and reflections of a stage point are not the particle's
NPG_HD bool walk_stage(const ParticleMesh &m, const WalkTables &w, const ParticleState &p, const double d[3], ParticleState &y) {
    y = p;
    int32_t unused = 0;
    return walk_move(m, w, y, unused, d);
}

// Step j of the call, step number `step` of particle `index`: the RK4 step of rk4_step with every point walked, then (DIFFUSE) the
// random displacement from the cell of the RK4 end point.  Only the RK4 end point and the random displacement move the particle:
// their crossings go into wind, their hits into nrefl.  false = the step cannot be finished: p and nrefl are untouched.
template <bool BLEND, bool DIFFUSE, class T>
NPG_HD bool walk_step(const ParticleMesh &m, const WalkTables &w, const T &t, const double *xa, const double *xb,
                      const ParticleCall &call, int64_t j, uint64_t index, uint64_t step, ParticleState &p, int32_t &nrefl) {
    const double h = call.h;
    const double s1 = BLEND ? stage_parameter(call, (double)j * h) : 0.0;
    const double s2 = BLEND ? stage_parameter(call, ((double)j + 0.5) * h) : 0.0;
    const double s4 = BLEND ? stage_parameter(call, ((double)j + 1.0) * h) : 0.0;
    double k[3], acc[3], d[3];
    ParticleState y;
    stage_velocity<BLEND>(t, xa, xb, s1, p.c, p.lam, k);
NPG_UNROLL
    for (int a = 0; a < 3; ++a) acc[a] = k[a], d[a] = (0.5 * h) * k[a];
    if (!walk_stage(m, w, p, d, y)) return false;
    stage_velocity<BLEND>(t, xa, xb, s2, y.c, y.lam, k);
NPG_UNROLL
    for (int a = 0; a < 3; ++a) acc[a] += 2.0 * k[a], d[a] = (0.5 * h) * k[a];
    if (!walk_stage(m, w, p, d, y)) return false;
    stage_velocity<BLEND>(t, xa, xb, s2, y.c, y.lam, k);
NPG_UNROLL
    for (int a = 0; a < 3; ++a) acc[a] += 2.0 * k[a], d[a] = h * k[a];
    if (!walk_stage(m, w, p, d, y)) return false;
    stage_velocity<BLEND>(t, xa, xb, s4, y.c, y.lam, k);
NPG_UNROLL
    for (int a = 0; a < 3; ++a) d[a] = (h / 6.0) * (acc[a] + k[a]);
    y = p;
    int32_t nr = nrefl;
    if (!walk_move(m, w, y, nr, d)) return false;
    if (DIFFUSE) {
        double R[3];
        particle_uniforms(w.key0, w.key1, index, step, R);
        walk_displacement(m, w, y.c, y.lam, h, R, d);
        if (!walk_move(m, w, y, nr, d)) return false;
    }
    p = y;
    nrefl = nr;
    return true;
}

// One particle through a call, as particle_advance: the number of steps taken; fewer than nsub = stuck at the start of that step,
// -1 = lost where the call found it.
template <bool BLEND, bool DIFFUSE, class T>
NPG_HD int64_t particle_walk(const ParticleMesh &m, const WalkTables &w, const T &t, const double *xa, const double *xb,
                             const ParticleCall &call, int64_t nsub, uint64_t index, uint64_t step0, ParticleState &p, int32_t &nrefl) {
    if (!particle_enter(m, p)) return -1;
    for (int64_t j = 0; j < nsub; ++j)
        if (!walk_step<BLEND, DIFFUSE>(m, w, t, xa, xb, call, j, index, step0 + (uint64_t)j, p, nrefl)) return j;
    return nsub;
}

// ---- validation on the host (both libraries): nullptr or what is wrong ------------------------------------------------------------
// has[a]: some face carries a translation on axis a
inline const char *check_wall_tables(const int32_t *nbr, const int8_t *shift, int64_t ncell, const double L[3], bool has[3]) {
    has[0] = has[1] = has[2] = false;
    for (int64_t k = 0; k < ncell * 4; ++k) {
        if (!(nbr[k] >= -1 && nbr[k] < ncell)) return "nbr must lie in [-1, ncell)";
        for (int a = 0; a < 3; ++a) {
            const int s = shift[k * 3 + a];
            if (s < -1 || s > 1) return "shift must be -1, 0 or 1";
            if (s != 0 && !(L[a] > 0.0)) return "shift is nonzero on an axis whose period is 0";
            if (s != 0 && nbr[k] < 0) return "shift is nonzero on a boundary face";
            if (s != 0) has[a] = true;
        }
    }
    return nullptr;
}

inline const char *check_kappa_tables(const double *kh, const double *kv, int64_t ncell, double cd) {
    if (!(std::isfinite(cd) && cd >= 0.0)) return "c_d must be finite and >= 0";
    for (int64_t k = 0; k < ncell * 4; ++k)
        if (!(std::isfinite(kh[k]) && kh[k] >= 0.0 && std::isfinite(kv[k]) && kv[k] >= 0.0)) return "kappa must be finite and >= 0";
    return nullptr;
}

}  // namespace npg
