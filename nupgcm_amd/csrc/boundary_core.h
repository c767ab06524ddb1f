// Quadrature integrals of the finite-element fields over the mesh's BOUNDARY faces (npg_boundary_compute): what ONE boundary triangle
// adds to the NPG_NBND channels.  The arithmetic shared by the device kernel (boundary.hip) and the host library
// (csrc_host/nupgcm_host.cpp), as integrals_core.h is for the volume integrals: GPU() and CPU() evaluate the same expressions in the
// same order, face by face.  Always fp64 (npg_fe_set_precision does not apply).
//
// A face is (cell c, local face k): the side lambda_k = 0 of that cell.  The fields and their gradients are the CELL's - its 30
// velocity, 4 pressure and NB buoyancy nodal values (Dirichlet nodes with their values, the pinned pressure vertex 0) and its 12
// barycentric gradients - evaluated at the 9 points of the face rule of Mesh.surface_load (fe.tri_quadrature_degree4: the 3 x 3
// collapsed Gauss-Jacobi x Gauss-Legendre rule, weights summing to 1/2), lifted into the cell's barycentrics: the face's vertices in
// ascending local index take the face's (mu_0, mu_1, mu_2) - both the cell's and the face's vertices are sorted by vertex id, so this is
// the order of surface_load and the prescribed-load channels are the very sums of the project's load vectors.  The measure is
// qw[q] area2[f] (area2 = twice the face's area from its own nodes), n = the outward unit normal, z(q) = sum_j mu_j z_j over the
// face's own nodes (correct across the periodic seam).
//
// Raw integrals only - the model's prefactors (alpha^2 eps^2, alpha, N2) are the caller's.  acc[k] grows by w integrand_k(q):
//
//    0  1                               area                       1..3  n                  (closed boundary: 0)
//    4  z n_z                           (closed boundary: volume)  5  u . n                 volume flux
//    6  b'                                                         7  b' u . n              advective buoyancy flux
//    8  p                                                          9..11  p n               pressure force
//   12  p u . n                         pressure work              13..15  t = nu (grad u) n, or 2 nu sigma n (full_stress)
//   16  u . t                           viscous work               17  kappa_h (d_x b' n_x + d_y b' n_y) + kappa_v d_z b' n_z
//   18  kappa_v n_z                                                19  tau_x u_x + tau_y u_y    wind work before the alpha
//   20  F                               prescribed flux            21  d_z b'
//   22, 23  u_x, u_y                    the tangential flow
//
// nu, kappa_h, kappa_v, tau_x, tau_y, F: the caller's values at the face points behind has(i); a missing table contributes 0.
// kappa_v = the table's BACKGROUND value plus - cl.kappa_c > 0 - the convection closure of mixing_core.h at the point's own d_z b'.
//
// S: the face shape tables of local face k, point q at r = 9 k + q - qw[q], mu[3 q + j], N2[10 r + i], dN2[4 (10 r + i) + m],
// N1[4 r + m] (= lambda_m); P1 buoyancy reads N1 (d N_i / d lambda_m = delta_im), P2 buoyancy the velocity's tables.
// T: the face tables - cell(f), local(f), area2(f), n(a, f), z(j, f), coef(i, q, f) / has(i), and the engine's G(k, c), u(x, l, c),
// p(x, m, c), b(x, i, c).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "mixing_core.h"

namespace npg {

constexpr int kNBnd = 24;
constexpr int kBndQ = 9;            // points of the face rule
#ifndef NPG_BND_BLOCK
#define NPG_BND_BLOCK 256           // (measured against 64 with tools/boundary_bench.py: DESIGN.md 23)
#endif
constexpr int kBndChunk = NPG_BND_BLOCK;   // faces per partial row: the device's workgroup, the host library's chunk
constexpr int kBndMaxGroups = 8;
enum { kBndNu = 0, kBndKh, kBndKv, kBndTauX, kBndTauY, kBndFlux, kBndNCoef };

// fe.tri_quadrature_degree4 to 17 significant digits: barycentrics with respect to the face's sorted vertices, and the weights
constexpr double kBndMu[kBndQ][3] = {
    {0.8086943856776698, 0.08858795951270393, 0.10271765480962626}, {0.45570602024364804, 0.08858795951270393, 0.45570602024364804},
    {0.10271765480962625, 0.08858795951270393, 0.8086943856776698}, {0.5239790677201007, 0.40946686444073477, 0.0665540678391645},
    {0.2952665677796326, 0.40946686444073477, 0.2952665677796326},  {0.06655406783916451, 0.40946686444073477, 0.5239790677201007},
    {0.18840940595207237, 0.787659461760847, 0.02393113228708062},  {0.1061702691195765, 0.787659461760847, 0.1061702691195765},
    {0.02393113228708063, 0.787659461760847, 0.18840940595207237}};
constexpr double kBndW[kBndQ] = {0.05581442048304436, 0.08930307277287088, 0.05581442048304436, 0.06367808509988508, 0.10188493615981602,
                                 0.06367808509988508, 0.0193963833059595,  0.031034213289535168, 0.0193963833059595};

// the face tables as S wants them (host memory; the device library uploads a copy)
struct BndShape {
    double qw[kBndQ], mu[kBndQ * 3], N2[4 * kBndQ * 10], dN2[4 * kBndQ * 40], N1[4 * kBndQ * 4];
};

// lift the face rule into the cell's barycentrics, once per local face, and tabulate the P2 basis there (the order of fe.p2_tables:
// vertices, then the edges (0,1) (0,2) (1,2) (0,3) (1,3) (2,3))
inline void bnd_shape_tables(BndShape &s) {
    const int ea[6] = {0, 0, 1, 0, 1, 2}, eb[6] = {1, 2, 2, 3, 3, 3};
    for (int q = 0; q < kBndQ; ++q) {
        s.qw[q] = kBndW[q];
        for (int j = 0; j < 3; ++j) s.mu[3 * q + j] = kBndMu[q][j];
    }
    for (int k = 0; k < 4; ++k)
        for (int q = 0; q < kBndQ; ++q) {
            const int r = kBndQ * k + q;
            double lam[4];
            for (int m = 0, j = 0; m < 4; ++m) lam[m] = m == k ? 0.0 : kBndMu[q][j++];
            for (int m = 0; m < 4; ++m) s.N1[4 * r + m] = lam[m];
            for (int i = 0; i < 40; ++i) s.dN2[40 * r + i] = 0.0;
            for (int m = 0; m < 4; ++m) {
                s.N2[10 * r + m] = lam[m] * (2.0 * lam[m] - 1.0);
                s.dN2[4 * (10 * r + m) + m] = 4.0 * lam[m] - 1.0;
            }
            for (int e = 0; e < 6; ++e) {
                s.N2[10 * r + 4 + e] = 4.0 * lam[ea[e]] * lam[eb[e]];
                s.dN2[4 * (10 * r + 4 + e) + ea[e]] = 4.0 * lam[eb[e]];
                s.dN2[4 * (10 * r + 4 + e) + eb[e]] = 4.0 * lam[ea[e]];
            }
        }
}

// the engine's cell tables and the sorted face tables ([component][face] in both libraries, unit stride over the faces of a row)
template <class View>
struct FaceTables : View {
    int64_t nk;                  // faces that count
    const int32_t *cell_;
    const uint8_t *local_;
    const double *area2_, *normal_, *z_;       // [nk], [3][nk], [3][nk]
    const double *coef_[kBndNCoef];            // [9][nk] or null
    NPG_HD int64_t cell(int64_t f) const { return cell_[f]; }
    NPG_HD int local(int64_t f) const { return local_[f]; }
    NPG_HD double area2(int64_t f) const { return area2_[f]; }
    NPG_HD double n(int a, int64_t f) const { return normal_[(size_t)a * (size_t)nk + f]; }
    NPG_HD double z(int j, int64_t f) const { return z_[(size_t)j * (size_t)nk + f]; }
    NPG_HD bool has(int i) const { return coef_[i] != nullptr; }
    NPG_HD double coef(int i, int q, int64_t f) const { return coef_[i][(size_t)q * (size_t)nk + f]; }
};

template <int NB, class S, class T>
NPG_HD void face_integrals(const S &s, const T &t, const double *xu, const double *xb, int64_t f, bool full_stress, const MixClosure &cl,
                           double acc[kNBnd]) {
    const int64_t c = t.cell(f);
    const int r0 = kBndQ * t.local(f);
    double G[12], u[30], p[4], b[NB];
NPG_UNROLL
    for (int k = 0; k < 12; ++k) G[k] = t.G(k, c);
NPG_UNROLL
    for (int l = 0; l < 30; ++l) u[l] = t.u(xu, l, c);
NPG_UNROLL
    for (int m = 0; m < 4; ++m) p[m] = t.p(xu, m, c);
NPG_UNROLL
    for (int i = 0; i < NB; ++i) b[i] = t.b(xb, i, c);
    const double area2 = t.area2(f), nx = t.n(0, f), ny = t.n(1, f), nz = t.n(2, f);
    const double z0 = t.z(0, f), z1 = t.z(1, f), z2 = t.z(2, f);
    for (int q = 0; q < kBndQ; ++q) {
        const int r = r0 + q;
        const double w = s.qw[q] * area2;
        double ux = 0.0, uy = 0.0, uz = 0.0;
NPG_UNROLL
        for (int i = 0; i < 10; ++i) {
            const double n = s.N2[r * 10 + i];
            ux += n * u[3 * i], uy += n * u[3 * i + 1], uz += n * u[3 * i + 2];
        }
        double gu[9];                       // gu[3 a + j] = d_j u_a
NPG_UNROLL
        for (int a = 0; a < 3; ++a) {
            double l0 = 0.0, l1 = 0.0, l2 = 0.0, l3 = 0.0;
NPG_UNROLL
            for (int i = 0; i < 10; ++i) {
                const double *dn = &s.dN2[(r * 10 + i) * 4];
                const double v = u[3 * i + a];
                l0 += dn[0] * v, l1 += dn[1] * v, l2 += dn[2] * v, l3 += dn[3] * v;
            }
NPG_UNROLL
            for (int j = 0; j < 3; ++j) gu[3 * a + j] = l0 * G[j] + l1 * G[3 + j] + l2 * G[6 + j] + l3 * G[9 + j];
        }
        const double *lam = &s.N1[r * 4];
        const double pq = lam[0] * p[0] + lam[1] * p[1] + lam[2] * p[2] + lam[3] * p[3];
        double bq = 0.0, l0, l1, l2, l3;
        if constexpr (NB == 10) {
            l0 = l1 = l2 = l3 = 0.0;
NPG_UNROLL
            for (int i = 0; i < 10; ++i) {
                const double *dn = &s.dN2[(r * 10 + i) * 4];
                bq += s.N2[r * 10 + i] * b[i];
                l0 += dn[0] * b[i], l1 += dn[1] * b[i], l2 += dn[2] * b[i], l3 += dn[3] * b[i];
            }
        } else {
            bq = lam[0] * b[0] + lam[1] * b[1] + lam[2] * b[2] + lam[3] * b[3];
            l0 = b[0], l1 = b[1], l2 = b[2], l3 = b[3];                               // d N_i / d lambda_m = delta_im
        }
        const double gx = l0 * G[0] + l1 * G[3] + l2 * G[6] + l3 * G[9];
        const double gy = l0 * G[1] + l1 * G[4] + l2 * G[7] + l3 * G[10];
        const double gz = l0 * G[2] + l1 * G[5] + l2 * G[8] + l3 * G[11];
        const double *mu = &s.mu[3 * q];
        const double zq = mu[0] * z0 + mu[1] * z1 + mu[2] * z2;
        const double un = ux * nx + uy * ny + uz * nz;
        acc[0] += w;
        acc[1] += w * nx, acc[2] += w * ny, acc[3] += w * nz;
        acc[4] += w * (zq * nz);
        acc[5] += w * un;
        acc[6] += w * bq;
        acc[7] += w * (bq * un);
        acc[8] += w * pq;
        acc[9] += w * (pq * nx), acc[10] += w * (pq * ny), acc[11] += w * (pq * nz);
        acc[12] += w * (pq * un);
        const double nu = t.has(kBndNu) ? t.coef(kBndNu, q, f) : 0.0;
        double tx, ty, tz;
        if (full_stress) {                  // 2 sigma n, sigma = (grad u + grad u') / 2
            tx = (gu[0] + gu[0]) * nx + (gu[1] + gu[3]) * ny + (gu[2] + gu[6]) * nz;
            ty = (gu[3] + gu[1]) * nx + (gu[4] + gu[4]) * ny + (gu[5] + gu[7]) * nz;
            tz = (gu[6] + gu[2]) * nx + (gu[7] + gu[5]) * ny + (gu[8] + gu[8]) * nz;
        } else {
            tx = gu[0] * nx + gu[1] * ny + gu[2] * nz;
            ty = gu[3] * nx + gu[4] * ny + gu[5] * nz;
            tz = gu[6] * nx + gu[7] * ny + gu[8] * nz;
        }
        tx *= nu, ty *= nu, tz *= nu;
        acc[13] += w * tx, acc[14] += w * ty, acc[15] += w * tz;
        acc[16] += w * (ux * tx + uy * ty + uz * tz);
        const double kh = t.has(kBndKh) ? t.coef(kBndKh, q, f) : 0.0;
        double kv = t.has(kBndKv) ? t.coef(kBndKv, q, f) : 0.0;
        if (cl.kappa_c > 0.0) kv = kv + closure_kappa(cl, gz);
        acc[17] += w * (kh * (gx * nx + gy * ny) + kv * (gz * nz));
        acc[18] += w * (kv * nz);
        const double taux = t.has(kBndTauX) ? t.coef(kBndTauX, q, f) : 0.0, tauy = t.has(kBndTauY) ? t.coef(kBndTauY, q, f) : 0.0;
        acc[19] += w * (taux * ux + tauy * uy);
        acc[20] += w * (t.has(kBndFlux) ? t.coef(kBndFlux, q, f) : 0.0);
        acc[21] += w * gz;
        acc[22] += w * ux, acc[23] += w * uy;
    }
}

// One face's place in the layout both libraries share: the faces that count, stably sorted by group; group g's faces fill
// ceil(n_g / kBndChunk) rows of at most kBndChunk faces each - a function of the face counts alone.
struct BndRow {
    int32_t first, count, group;
};
struct BndRowRange {
    int32_t row0[kBndMaxGroups + 1];        // group g's rows are [row0[g], row0[g + 1])
};
struct BndLayout {
    std::vector<int32_t> orig;              // the caller's index of sorted face i: where its row of faces_out goes
    std::vector<BndRow> rows;
    int32_t row0[kBndMaxGroups + 1];        // group g's rows are [row0[g], row0[g + 1])
};

// npg_boundary_create's validation and layout, for both libraries: "" or what is wrong (nothing has been allocated or launched yet)
inline std::string bnd_build_layout(int64_t ncell, int64_t nface, const int32_t *face_cell, const uint8_t *face_local, const uint8_t *face_group,
                                    int ngroup, const double *face_xyz, const double *face_normal, const double *face_area2,
                                    const uint8_t *face_mask, BndLayout &lay) {
    char buf[256];
    if (ngroup < 1 || ngroup > kBndMaxGroups) {
        snprintf(buf, sizeof buf, "npg_boundary_create: ngroup must be 1 .. %d, got %d", kBndMaxGroups, ngroup);
        return buf;
    }
    if (nface < 0 || nface > INT32_MAX) return "npg_boundary_create: nface must be 0 .. 2^31 - 1";
    if (nface > 0 && !(face_cell && face_local && face_group && face_xyz && face_normal && face_area2))
        return "npg_boundary_create: NULL face table";
    for (int64_t f = 0; f < nface; ++f) {
        const char *what = nullptr;
        if (face_cell[f] < 0 || face_cell[f] >= ncell) what = "face_cell is out of range";
        else if (face_local[f] > 3) what = "face_local must be 0 .. 3";
        else if (face_group[f] >= ngroup) what = "face_group is not below ngroup";
        else if (!std::isfinite(face_area2[f])) what = "face_area2 is not finite";
        for (int k = 0; k < 9 && !what; ++k)
            if (!std::isfinite(face_xyz[(size_t)k * nface + f])) what = "face_xyz is not finite";
        for (int k = 0; k < 3 && !what; ++k)
            if (!std::isfinite(face_normal[(size_t)k * nface + f])) what = "face_normal is not finite";
        if (what) {
            snprintf(buf, sizeof buf, "npg_boundary_create: face %lld: %s", (long long)f, what);
            return buf;
        }
    }
    int64_t count[kBndMaxGroups] = {0}, start[kBndMaxGroups + 1] = {0};
    for (int64_t f = 0; f < nface; ++f)
        if (!face_mask || face_mask[f]) ++count[face_group[f]];
    lay.rows.clear();
    for (int g = 0; g < ngroup; ++g) {
        start[g + 1] = start[g] + count[g];
        lay.row0[g] = (int32_t)lay.rows.size();
        for (int64_t i = 0; i < count[g]; i += kBndChunk)
            lay.rows.push_back(BndRow{(int32_t)(start[g] + i), (int32_t)std::min<int64_t>(kBndChunk, count[g] - i), g});
    }
    for (int g = ngroup; g <= kBndMaxGroups; ++g) lay.row0[g] = (int32_t)lay.rows.size();
    lay.orig.assign((size_t)start[ngroup], 0);
    int64_t next[kBndMaxGroups];
    for (int g = 0; g < ngroup; ++g) next[g] = start[g];
    for (int64_t f = 0; f < nface; ++f)
        if (!face_mask || face_mask[f]) lay.orig[(size_t)next[face_group[f]]++] = (int32_t)f;       // stable: the caller's order within a group
    return "";
}

}  // namespace npg
