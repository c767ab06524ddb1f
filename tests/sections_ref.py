"""An independent cutter, a numpy restatement of the section transports (nupgcm_amd.sections) and the checks shared by
tests/test_sections.py (CPU()), tests/test_gpu_sections.py (GPU()) and tests/test_sections_plan.py (the planner under sanitizers).

THE INDEPENDENT CUTTER (independent_plan) shares with the code under test the cut RULE - d in the stated association, below iff d < 0,
t = d_a / (d_a - d_b) - and nothing else: a cell's corners are formed in space as (1 - t) X_a + t X_b, projected on (e1, e2), ordered by
angle about their mean, clipped against the closed half-planes of a bin one after the other and measured by the shoelace formula
relative to the first corner.  A (cell, bin) pair counts iff that area is > 0 and the cell's unclipped polygon has area > 0.

THE RESTATEMENT (restate) takes the plan from SectionTransports.pieces() and is written from the definitions: the rule's points from the
issue's table, the P2 basis from fe.p2_tables at the points' barycentrics, the geometry from the cells' own vertices (inverse of the
edge matrix, not grad_lambda), nodal values through Spaces' native tables, coefficients from the forcing functions at the points.

BOUNDS.  Areas: a corner's in-plane coordinate is an interpolation (3 operations) followed by a three-term inner product of differences
(8 operations): at most 11 roundings relative to the magnitudes |X| + |o| <= Xmax on either side, delta = 22 eps Xmax for both.  Moving
a boundary line or a corner of a convex polygon by delta changes its area by at most delta times its perimeter; the clip lines are data
(exact), the crossings inherit delta from the corners they lie between.  The shoelace / cross product itself adds (n_c + 2) products of
differences at 4 eps D^2 each (D = the polygon's diameter).  So a (cell, bin) area is held to
    AREA_C delta P + 8 (n_c + 2) eps D^2,    AREA_C = 2 (both sides),
with P the perimeter of the cell's UNCLIPPED polygon plus that of the bin's rectangle inside its bounding box (a clipped polygon's
perimeter is at most the polygon's: it is convex).  A bin's area adds its cells' bounds and n eps sum(area) for the n additions.
Integrals: one piece's own term is an inner product whose longest path has fewer than 64 operations (lambda at the point 5, the P2 basis
3, ten products and additions, the contraction with n 5, the products with b' or z, the coefficient and the measure 6, six points 6;
the gradient path is shorter), relative to the MAGNITUDE of its constituents (Higham, Accuracy and Stability, eq. 3.5), on both sides
of the comparison: EVAL_OPS = 128.  A bin adds n pieces x 6 points more.  So every entry is held to
    piece: 128 eps M_piece,        bin: (128 + 6 n) eps sum_pieces M_piece,
with M the term's expression evaluated with every constituent replaced by its magnitude.  "c eps (sum of |terms|)" is read here as
tests/boundary_ref.py reads it: the |terms| are the magnitudes M of what a term is made of, not |term| itself (M >= |term|; a gradient
is a sum of products that cancel, and its rounding is relative to the products).  No other tolerance is used against the
restatement; where a second quantity enters (a closed form, the independent cutter) its own bound of the same kind is added and said
there."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np

import nupgcm_amd as npg
from nupgcm_amd import _lib as L
from nupgcm_amd import fe as F
from nupgcm_amd import gmsh_io
from nupgcm_amd.architectures import Context
from nupgcm_amd.inversion import device_fe
from tests import averages_ref as ar
from tests import boundary_ref as br
from tests import nodal_ref as nr
from tests import sampling_ref as sr

EPS = np.finfo(np.float64).eps
NSEC = 14
NQ = 6
NPG_EINVAL = -1
SEED = 20261021
EVAL_OPS = 128
NEW = {"npg_sections_create", "npg_sections_info", "npg_sections_pieces", "npg_sections_set_coeff", "npg_sections_set_closure",
       "npg_sections_compute", "npg_sections_destroy"}
EA, EB = F._TET_EDGE_A, F._TET_EDGE_B
# the symmetric degree-4 rule on a triangle, area-normalised weights
_WA, _WB = 0.223381589678011, 0.109951743655322
_PA, _PB = (0.108103018168070, 0.445948490915965, 0.445948490915965), (0.816847572980459, 0.091576213509771, 0.091576213509771)
MU = np.array([np.roll(_PA, k) for k in range(3)] + [np.roll(_PB, k) for k in range(3)])
W = np.array([_WA] * 3 + [_WB] * 3)
EDGE_COUNTS = ar.EDGE_COUNTS


def sdot(x, o, a):
    """(x - o) . a in the association of the cut rule, over the last axis"""
    x = np.asarray(x, dtype=np.float64)
    return ((x[..., 0] - o[0]) * a[0] + (x[..., 1] - o[1]) * a[1]) + (x[..., 2] - o[2]) * a[2]


def cell_xyz(mesh):
    return mesh.geo_coords[mesh.cell_geo]


# ---- the independent cutter -------------------------------------------------------------------------------------------------------
def _cell_polygon(Xc, sec):
    """the cut polygon of one cell in (s1, s2), corners ordered by angle, or None"""
    d = sdot(Xc, sec.origin, sec.normal)
    below = d < 0.0
    if below.sum() in (0, 4):
        return None
    pts = []
    for a in np.nonzero(below)[0]:
        for b in np.nonzero(~below)[0]:
            t = d[a] / (d[a] - d[b])
            x = (1.0 - t) * Xc[a] + t * Xc[b]
            pts.append((sdot(x, sec.origin, sec.e1), sdot(x, sec.origin, sec.e2)))
    P = np.array(pts)
    c = P.mean(axis=0)
    return P[np.argsort(np.arctan2(P[:, 1] - c[1], P[:, 0] - c[0]), kind="stable")]


def _keep_side(P, axis, E, sign):
    """the part of the convex polygon P with sign (s - E) >= 0 (closed half-plane)"""
    if len(P) == 0:
        return P
    h = sign * (P[:, axis] - E)
    out = []
    for k in range(len(P)):
        k2 = (k + 1) % len(P)
        if h[k] >= 0.0:
            out.append(P[k])
        if (h[k] > 0.0 and h[k2] < 0.0) or (h[k] < 0.0 and h[k2] > 0.0):
            r = h[k] / (h[k] - h[k2])
            out.append(P[k] + r * (P[k2] - P[k]))
    return np.array(out).reshape(-1, 2)


def _shoelace(P):
    if len(P) < 3:
        return 0.0
    Q = P - P[0]
    return 0.5 * abs(float(np.sum(Q[:-1, 0] * Q[1:, 1] - Q[1:, 0] * Q[:-1, 1])))


def _perimeter(P):
    return float(np.sum(np.linalg.norm(P - np.roll(P, 1, axis=0), axis=1)))


def independent_plan(X, sections, mask=None):
    """{(global bin, cell): (area, bound)} over the bins with area > 0, by the independent cutter; X (ncell, 4, 3)"""
    out, bin0 = {}, 0
    for sec in sections:
        n1, n2 = sec.shape
        xmax = float(np.abs(X).max() + np.abs(sec.origin).max())
        delta = 22.0 * EPS * xmax
        d = sdot(X, sec.origin, sec.normal)
        nb = (d < 0.0).sum(axis=1)
        cand = np.nonzero((nb > 0) & (nb < 4) & (True if mask is None else np.asarray(mask, dtype=bool)))[0]
        for c in cand:
            P = _cell_polygon(X[c], sec)
            if not _shoelace(P) > 0.0:                                     # an edge or a vertex on the plane: a polygon without area
                continue                                                   # has no share in any bin (its crossings would round to slivers)
            lo, hi = P.min(axis=0), P.max(axis=0)
            per, diam = _perimeter(P), float(np.linalg.norm(hi - lo))
            i0, i1 = np.searchsorted(sec.edges1, [lo[0], hi[0]], side="right") - 1
            j0, j1 = np.searchsorted(sec.edges2, [lo[1], hi[1]], side="right") - 1
            for i in range(max(i0, 0), min(i1, n1 - 1) + 1):
                Pi = P
                if np.isfinite(sec.edges1[i]):
                    Pi = _keep_side(Pi, 0, sec.edges1[i], 1.0)
                if np.isfinite(sec.edges1[i + 1]):
                    Pi = _keep_side(Pi, 0, sec.edges1[i + 1], -1.0)
                for j in range(max(j0, 0), min(j1, n2 - 1) + 1):
                    Pj = Pi
                    if np.isfinite(sec.edges2[j]):
                        Pj = _keep_side(Pj, 1, sec.edges2[j], 1.0)
                    if np.isfinite(sec.edges2[j + 1]):
                        Pj = _keep_side(Pj, 1, sec.edges2[j + 1], -1.0)
                    a = _shoelace(Pj)
                    if a > 0.0:
                        box = 2.0 * float(np.sum(hi - lo))                 # the bin's rectangle inside the bounding box, at most
                        out[(bin0 + i * n2 + j, int(c))] = (a, 2.0 * delta * (per + box) + 8.0 * (len(P) + 2) * EPS * diam * diam)
        bin0 += n1 * n2
    return out


def plan_invariants(pl, info, nbin):
    """what every plan satisfies, whatever made it"""
    cell, bins, lam, area, ptr = pl["cell"], pl["bin"], pl["lam"], pl["area"], pl["bin_ptr"]
    n = len(cell)
    assert info["pieces"] == n and info["bins"] == nbin and len(ptr) == nbin + 1 and ptr[0] == 0 and ptr[-1] == n
    if n:
        key = bins.astype(np.int64) * (int(cell.max()) + 1) + cell
        assert (np.diff(key) >= 0).all()                                                # sorted by (bin, cell)
        assert (area > 0.0).all() and np.isfinite(area).all()
        assert lam.min() >= -8 * EPS and lam.max() <= 1.0 + 8 * EPS
        assert (np.abs(lam.sum(axis=2) - 1.0) <= 8 * EPS).all()
        assert bins.min() >= 0 and bins.max() < nbin
    counts = np.bincount(bins, minlength=nbin)
    assert np.array_equal(np.diff(ptr), counts) and info["max_per_bin"] == int(counts.max(initial=0))
    assert info["cut_cells"] == len(np.unique(cell))


def compare_plans(pl, ind, nbin, label):
    """the plan of the code under test against the independent cutter's: the (bin, cell) pairs agree exactly; every pair's area and every
    bin's area within the bound of the module docstring"""
    pairs = {}
    for b, c, a in zip(pl["bin"].tolist(), pl["cell"].tolist(), pl["area"].tolist()):
        pairs.setdefault((b, c), []).append(a)
    only_plan, only_ind = sorted(set(pairs) - set(ind)), sorted(set(ind) - set(pairs))
    assert not only_plan and not only_ind, (label, "pairs of the plan alone", only_plan[:5], "of the independent cutter alone", only_ind[:5])
    got, ref, bound = np.zeros(nbin), np.zeros(nbin), np.zeros(nbin)
    worst = 0.0
    for key, areas in pairs.items():
        a = math.fsum(areas)
        r, bd = ind[key]
        worst = max(worst, abs(a - r) / bd)
        assert abs(a - r) <= bd, (label, key, a, r, bd)
        got[key[0]] += a
        ref[key[0]] += r
        bound[key[0]] += bd
    bound += np.bincount(pl["bin"], minlength=nbin) * EPS * ref
    print(f"sections plan {label}: {len(pl['cell'])} pieces, {len(pairs)} (bin, cell) pairs, worst |area - independent| / bound {worst:.3f}")
    assert (np.abs(got - ref) <= bound).all(), label
    return got, ref, bound


def check_plan(model, sections, label, mask=None):
    """check 2 on one set of sections; returns the SectionTransports and (areas per bin, their bound)"""
    st = npg.SectionTransports(model, sections, mask)
    pl = st.pieces()
    plan_invariants(pl, st.info, st.nbin)
    X = cell_xyz(model.fe_data.mesh)
    got, ref, bound = compare_plans(pl, independent_plan(X, st.sections, mask), st.nbin, label)
    return st, got, bound


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def piece_fields(model, pl, frames):
    """the fields at the 6 points of every piece: u (np, 6, 3), p, b, gb (np, 6, 3), z, xq (np, 6, 3), n (np, 3), W (np, 6), and the
    magnitudes a_* of their constituents"""
    fed = model.fe_data
    m = fed.mesh
    un, pn, bn = br.nodal_values(model)
    cell = pl["cell"]
    X = cell_xyz(m)[cell]
    g = np.linalg.inv(np.transpose(X[:, 1:] - X[:, :1], (0, 2, 1))) if len(cell) else np.zeros((0, 3, 3))
    G = np.concatenate([-g.sum(axis=1, keepdims=True), g], axis=1)                      # (np, 4, 3)
    lamq = np.einsum("qj,pjm->pqm", MU, pl["lam"])
    N, dN = F.p2_tables(lamq.reshape(-1, 4), EA, EB)
    N, dN = N.reshape(len(cell), NQ, 10), dN.reshape(len(cell), NQ, 10, 4)
    uc, pc = un[m.cell_nodes[cell]], pn[m.cells[cell]]
    aN, adN, aG, al = np.abs(N), np.abs(dN), np.abs(G), np.abs(lamq)
    out = {"u": np.einsum("pqi,pia->pqa", N, uc), "a_u": np.einsum("pqi,pia->pqa", aN, np.abs(uc)),
           "p": np.einsum("pqm,pm->pq", lamq, pc), "a_p": np.einsum("pqm,pm->pq", al, np.abs(pc))}
    if fed.spaces.b_order == 2:
        bc = bn[m.cell_nodes[cell]]
        out["b"], out["gb"] = np.einsum("pqi,pi->pq", N, bc), np.einsum("pqik,pi,pkj->pqj", dN, bc, G)
        out["a_b"], out["a_gb"] = np.einsum("pqi,pi->pq", aN, np.abs(bc)), np.einsum("pqik,pi,pkj->pqj", adN, np.abs(bc), aG)
    else:
        bc = bn[m.cells[cell]]
        out["b"], out["a_b"] = np.einsum("pqm,pm->pq", lamq, bc), np.einsum("pqm,pm->pq", al, np.abs(bc))
        out["gb"] = np.broadcast_to(np.einsum("pk,pkj->pj", bc, G)[:, None, :], (len(cell), NQ, 3))
        out["a_gb"] = np.broadcast_to(np.einsum("pk,pkj->pj", np.abs(bc), aG)[:, None, :], (len(cell), NQ, 3))
    out["z"], out["a_z"] = np.einsum("pqm,pm->pq", lamq, X[:, :, 2]), np.einsum("pqm,pm->pq", al, np.abs(X[:, :, 2]))
    out["xq"] = np.einsum("pqm,pmi->pqi", lamq, X)
    out["n"] = frames[pl["section"]].reshape(-1, 4, 3)[:, 1]
    out["W"] = W[None, :] * pl["area"][:, None]
    return out


def _channels(Wt, n, z, u, p, b, gb, kh, kv):
    """the NSEC integrands times the measure; called with the fields, and again with the magnitudes of their constituents"""
    nx, ny, nz = n[:, None, 0], n[:, None, 1], n[:, None, 2]
    un_ = (u * n[:, None, :]).sum(axis=-1)
    gh = gb[..., 0] * nx + gb[..., 1] * ny
    one = np.ones_like(p)
    ch = [one, un_, b, b * un_, z * un_, p, u[..., 0], u[..., 1], u[..., 2], gh + gb[..., 2] * nz, kh * gh + kv * gb[..., 2] * nz, kv * nz * one,
          z, gb[..., 2]]
    return np.stack([Wt * c_ for c_ in ch])


def restate(model, st, coef=None):
    """(terms (NSEC, npiece, 6), mags (NSEC, npiece, 6)) of the model's current state on the plan of `st`.  coef: overrides kh / kv of
    the forcings (numbers, functions of x, None = 0); the convection closure is the model's"""
    f, prm = model.forcings, model.params
    pl = st.pieces()
    ff = piece_fields(model, pl, st._keep["frames"])
    c = dict(kh=f.kappa_h, kv=f.kappa_v)
    c.update(coef or {})
    kh, kv = br._coef(c["kh"], ff["xq"]), br._coef(c["kv"], ff["xq"])
    akv = np.abs(kv)
    if f.conv_param.is_on:
        cp, al, N2 = f.conv_param, float(prm.alpha), float(prm.N2)
        x = -al * (N2 + ff["gb"][..., 2]) / cp.N2min
        kv = kv + cp.kappa_c * (1.0 + np.tanh(x)) / 2.0
        # the constituents of kappa_v0 + kappa_c (1 + tanh x) / 2, as tests/boundary_ref.restate takes them
        akv = akv + 0.5 * cp.kappa_c * (1.0 + np.abs(np.tanh(x))) + 0.5 * cp.kappa_c / np.cosh(x) ** 2 * abs(al) * (abs(N2) + ff["a_gb"][..., 2]) / cp.N2min
    terms = _channels(ff["W"], ff["n"], ff["z"], ff["u"], ff["p"], ff["b"], ff["gb"], kh, kv)
    mags = _channels(ff["W"], np.abs(ff["n"]), ff["a_z"], ff["a_u"], ff["a_p"], ff["a_b"], ff["a_gb"], np.abs(kh), akv)
    return terms, mags


def bin_sums(terms, mags, bin_ptr):
    """(tot, bound) (nbin, NSEC): math.fsum of every bin's terms and (128 + 6 n) eps sum of the magnitudes"""
    nbin = len(bin_ptr) - 1
    tot, bound = np.zeros((nbin, NSEC)), np.zeros((nbin, NSEC))
    for k in range(nbin):
        a, b = int(bin_ptr[k]), int(bin_ptr[k + 1])
        for ch in range(NSEC):
            tot[k, ch] = math.fsum(terms[ch, a:b].ravel())
            bound[k, ch] = (EVAL_OPS + NQ * (b - a)) * EPS * math.fsum(mags[ch, a:b].ravel())
    return tot, bound


def fold_restated(per_piece, bin_ptr):
    """the fold order of csrc/sections_core.h in numpy: 64 accumulators take a bin's pieces round-robin in piece order from 0.0, then
    v[l] += v[l + off] over l < off for off = 32 .. 1.  IEEE additions in the stated order: the library's bits, given its pieces"""
    nbin = len(bin_ptr) - 1
    out = np.zeros((nbin, NSEC))
    for k in range(nbin):
        t = per_piece[:, int(bin_ptr[k]):int(bin_ptr[k + 1])]
        v = np.zeros((NSEC, 64))
        for r in range(0, t.shape[1], 64):                                             # round r: pieces 64 r .. 64 r + 63 of the bin
            chunk = t[:, r:r + 64]
            v[:, :chunk.shape[1]] += chunk
        off = 32
        while off:
            v[:, :off] = v[:, :off] + v[:, off:2 * off]
            off //= 2
        out[k] = v[:, 0]
    return out


def compare(st, raw, per_piece, terms, mags, label, channels=range(NSEC)):
    """every channel of every bin and of every piece within its bound; an empty bin is 14 zeros; prints the worst ratio first"""
    ptr = st.pieces()["bin_ptr"]
    tot, bound = bin_sums(terms, mags, ptr)
    ch = sorted(channels)
    err = np.abs(raw - tot)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))[:, ch]
    worst_p = 0.0
    if per_piece is not None:
        ptot = np.array([[math.fsum(r) for r in terms[k]] for k in range(NSEC)]).reshape(NSEC, -1)
        pbound = EVAL_OPS * EPS * mags.sum(axis=2)
        perr = np.abs(per_piece - ptot)
        pr = np.where(pbound > 0, perr / np.where(pbound > 0, pbound, 1.0), np.where(perr > 0, np.inf, 0.0))[ch]
        worst_p = float(pr.max(initial=0.0))
        assert np.array_equal(fold_restated(per_piece, ptr), raw), (label, "the fold of the library's own pieces in the stated order")
    print(f"sections {label}: {st.npiece} pieces in {st.nbin} bins (largest {st.info['max_per_bin']}), worst |err| / bound: bins "
          f"{float(ratio.max(initial=0.0)):.3f}, pieces {worst_p:.3f}")
    assert np.isfinite(raw).all() and (ratio <= 1.0).all(), (label, float(ratio.max()))
    assert worst_p <= 1.0, (label, "per piece", worst_p)
    empty = np.diff(ptr) == 0
    assert (raw[empty] == 0.0).all(), label
    return tot, bound


# ---- models -----------------------------------------------------------------------------------------------------------------------
def kuhn_cells(n=4):
    """(coords, cells) of n^3 cubes x 6 tetrahedra (Kuhn's triangulation) on [0, 1]^2 x [-1, 0]; dyadic coordinates for n = 4"""
    import itertools
    idx = lambda i, j, k: (i * (n + 1) + j) * (n + 1) + k                            # noqa: E731
    g = np.arange(n + 1) / n
    coords = np.array([[g[i], g[j], g[k] - 1.0] for i in range(n + 1) for j in range(n + 1) for k in range(n + 1)])
    cells = []
    for i, j, k in itertools.product(range(n), repeat=3):
        for perm in itertools.permutations(range(3)):
            v = [i, j, k]
            tet = [idx(*v)]
            for ax in perm:
                v[ax] += 1
                tet.append(idx(*v))
            cells.append(tet)
    return coords, np.array(cells, dtype=np.int64)


def kuhn_cube(arch, b_order=2, n=4):
    """the Kuhn cube as a bare model (no Dirichlet tags) whose boundary facets are the faces with one cell, tagged "surface" on z = 0
    and "wall" elsewhere"""
    coords, cells = kuhn_cells(n)
    count = {}
    for c in cells:
        for k in range(4):
            tri = tuple(sorted(np.delete(c, k)))
            count[tri] = count.get(tri, 0) + 1
    facets = np.array(sorted(t for t, cnt in count.items() if cnt == 1), dtype=np.int64)
    assert len(facets) == 6 * 2 * n * n
    top = (coords[facets][:, :, 2] == 0.0).all(axis=1)
    gm = gmsh_io.GmshModel(dim=3, coords=coords, node_phys=np.zeros(len(coords), dtype=np.uint32), cells=cells, facets=facets,
                           facets_phys=np.where(top, 2, 1).astype(np.uint32), ridges=np.zeros((0, 2), dtype=np.int64),
                           ridges_phys=np.zeros(0, dtype=np.uint32), phys_names=["wall", "surface"])
    return br.bare_model(arch, npg.Mesh(gm), b_order)


def quiet(model, **frc_kw):
    """the model's state and mesh with the closures off (boundary_ref.view): what the bit-for-bit comparisons run on"""
    kw = dict(br.OFF)
    kw.update(frc_kw)
    return br.view(model, **kw)


def bowl(arch, name="bowl_surface_flux", b_order=2):
    return nr.bowl(arch, name, b_order, seed=SEED)


BOWL_SECTIONS = lambda: [npg.Section.longitude(0.1, y_edges=[-0.8, -0.33, 0.02, 0.41, 2.0], z_edges=[-np.inf, -0.37, -0.11, 0.3]),     # noqa: E731
                         npg.Section.level(-0.3, x_edges=np.linspace(-1.03, 1.03, 6), y_edges=[-np.inf, 0.017, np.inf]),
                         npg.Section.latitude(0.0, z_edges=np.linspace(-1.0, 0.0, 9))]


# ---- the checks (arch = npg.CPU() or npg.GPU()) --------------------------------------------------------------------------------------
def check_exports():
    assert {"Section", "SectionTransports", "SectionFluxes", "SectionMaps", "SectionRecorder"} <= set(npg.__all__)
    assert NEW <= set(L.declared_symbols()) and L.NPG_NSEC == NSEC and npg.sections.NSEC == NSEC and len(npg.sections.CHANNELS) == NSEC
    header = open(L.HEADER_PATH).read()
    assert f"#define NPG_NSEC {NSEC}\n" in header
    for path in (L.HOST_LIB_PATH, L.LIB_PATH):
        lib = C.CDLL(path)
        assert not [s for s in NEW if not hasattr(lib, s)], path


def check_plans_bowl(model):
    """check 2 on the golden bowl: the counts measured for the issue, the independent cutter, binned areas = the unbinned section's"""
    for sec, ncut, npiece in ((npg.Section.longitude(0.1), 367, 477), (npg.Section.level(-0.3), 786, 1033)):
        st, area, bound = check_plan(model, sec, sec.name)
        assert (st.info["cut_cells"], st.npiece) == (ncut, npiece), st.info
        per_cell = np.bincount(st.pieces()["cell"])
        assert set(per_cell[per_cell > 0]) <= {1, 2}
    st, _, _ = check_plan(model, BOWL_SECTIONS(), "three binned sections")
    assert st.nbin == 12 + 10 + 8
    one, a1, b1 = check_plan(model, npg.Section.latitude(0.0), "y = 0, one bin")
    X = cell_xyz(model.fe_data.mesh)
    on_plane = np.unique(model.fe_data.mesh.cell_geo[X[:, :, 1] == 0.0])
    print(f"sections bowl y = 0: {len(on_plane)} mesh vertices lie exactly on the plane")
    assert len(on_plane) > 0                                                            # the plane passes exactly through mesh vertices
    many, a8, b8 = check_plan(model, npg.Section.latitude(0.0, z_edges=np.linspace(-1.0, 0.0, 9)), "y = 0, 8 depth bins")
    rel = abs(a8.sum() - a1[0]) / a1[0]
    print(f"sections bowl y = 0: area {a1[0]:.9f}; 8 depth bins sum to it within {rel:.2e} (bound {(b8.sum() + b1[0]) / a1[0]:.2e})")
    assert abs(a8.sum() - a1[0]) <= b8.sum() + b1[0] + 8 * EPS * a1[0]
    assert abs(a1[0] - 0.665044205) < 5e-10                                             # the prototype's figure, as printed in the issue


def check_degenerate(arch, bowl_model, against_host=False):
    """check 3: planes that lie in mesh faces or pass through vertices - every face counted once; with against_host the face-aligned
    pieces (barycentrics that are exactly 0 and 1, both normals) and the planes through the bowl's vertices also go through the
    restatement and the host library, bit for bit"""
    model = kuhn_cube(arch)
    Poly(model)
    zed = [-1.0, -0.75, -0.5, -0.25, 0.0]
    plus = npg.Section.longitude(0.5, name="plus")
    minus = npg.Section("minus", [0.5, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0])
    faces = [plus, minus, npg.Section.longitude(0.5, z_edges=zed, name="binned")]
    st, area, bound = check_plan(model, faces, "Kuhn cube, x = 0.5 in mesh faces")
    check_restatement(model, faces, "Kuhn cube, x = 0.5 in mesh faces", against_host=against_host)
    d = sdot(cell_xyz(model.fe_data.mesh), plus.origin, plus.normal)
    assert ((d == 0.0).sum(axis=1) == 3).sum() == 2 * 32                                # 32 mesh faces lie in the plane, two cells each
    assert st.npiece == 3 * 32                                                          # and each is counted by one of them
    assert abs(area[0] - 1.0) <= bound[0] and abs(area[1] - 1.0) <= bound[1]
    assert (np.abs(area[2:] - 0.25) <= bound[2:]).all() and len(area) == 6
    f = st.compute()
    vt = f.volume_transport
    _, bb = bin_sums(*restate(model, st), st.pieces()["bin_ptr"])
    assert abs(vt["plus"][0, 0] + vt["minus"][0, 0]) <= bb[0, 1] + bb[1, 1] and abs(vt["plus"][0, 0]) > 1e-3
    assert abs(f.area["plus"][0, 0] - f.area["minus"][0, 0]) <= bound[0] + bound[1]
    areas = []
    for y0 in (-1e-7, 0.0, 1e-7):
        st, a, _ = check_plan(bowl_model, npg.Section.latitude(y0), f"bowl y = {y0:g}")
        areas.append(a[0])
        print(f"sections bowl y = {y0:g}: area {a[0]:.9f}, {st.npiece} pieces, {st.info['cut_cells']} cut cells")
    assert max(areas) - min(areas) < 1e-6                                               # continuity: no face dropped or doubled
    through = [npg.Section.latitude(y0, name=f"y = {y0:g}") for y0 in (-1e-7, 0.0, 1e-7)]
    check_restatement(quiet(bowl_model), through, "bowl, y = 0 through mesh vertices and 1e-7 beside it", against_host=against_host)


def host_library(model, st, closure=None, pieces=True):
    """(plan arrays, raw (nbin, NSEC), per piece (NSEC, npiece)) through the host library with the arguments `st` was created with and
    its coefficient tables rebuilt from the model's forcings"""
    E = nr.HostEngine(model)
    H = E.H
    k = st._keep
    S = C.c_void_p()
    E.ok(H.npg_sections_create(E.fe, L.ptr(st._X), len(st.sections), L.ptr(k["frames"]), L.ptr(k["n1"]), L.ptr(k["n2"]), L.ptr(k["e1"]),
                               L.ptr(k["e2"]), None if k["mask"] is None else L.ptr(k["mask"]), C.byref(S)))
    q = [C.c_int64() for _ in range(4)]
    E.ok(H.npg_sections_info(S, *[C.byref(v) for v in q]))
    n, nbin = q[0].value, q[1].value
    cell, bins, lam, area = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros((n, 3, 4)), np.zeros(n)
    E.ok(H.npg_sections_pieces(S, L.ptr(cell), L.ptr(bins), L.ptr(lam), L.ptr(area)))
    pts = st.pieces()["points"]
    for which, v in ((L.NPG_SEC_KH, model.forcings.kappa_h), (L.NPG_SEC_KV, model.forcings.kappa_v)):
        tab = L.as_f64(br._coef(v, pts).T) if n == st.npiece else np.zeros((6, n))
        E.ok(H.npg_sections_set_coeff(S, which, L.ptr(tab)))
    if closure is not None:
        E.ok(H.npg_sections_set_closure(S, *closure))
    x, b = E.vec(model.inversion.solver.x.to_host()), E.vec(model.b_vec.to_host())
    out, po = E.vec(np.zeros(nbin * NSEC)), E.vec(np.zeros(max(1, NSEC * n)))
    E.ok(H.npg_sections_compute(S, x, b, out, po if pieces else None))
    raw, pp = np.empty(nbin * NSEC), np.empty(max(1, NSEC * n))
    E.ok(H.npg_vec_download(out, L.ptr(raw)))
    E.ok(H.npg_vec_download(po, L.ptr(pp)))
    H.npg_sections_destroy(S)
    E.close()
    return dict(cell=cell, bin=bins, lam=lam, area=area, info=[v.value for v in q]), raw.reshape(nbin, NSEC), pp[:NSEC * n].reshape(NSEC, n)


def check_restatement(model, sections, label, mask=None, against_host=False):
    """check 6 (and 8 with against_host): every channel of every bin and piece against the restatement; the device against the host
    library - the same plan, and without the closure the same bits; with it channels 10 and 11 within the restatement's bound"""
    st = npg.SectionTransports(model, sections, mask)
    plan_invariants(st.pieces(), st.info, st.nbin)
    terms, mags = restate(model, st)
    raw, pp = st.compute_raw(pieces=True)
    assert raw.shape == (st.nbin, NSEC) and pp.shape == (NSEC, st.npiece)
    tot, bound = compare(st, raw, pp, terms, mags, label)
    if against_host:
        cp = model.forcings.conv_param
        closure = (float(cp.kappa_c), float(cp.N2min), float(model.params.alpha), float(model.params.N2)) if cp.is_on else None
        hp, hraw, hpp = host_library(model, st, closure)
        pl = st.pieces()
        for key in ("cell", "bin", "lam", "area"):
            assert np.array_equal(hp[key], pl[key]), (label, key)
        assert hp["info"] == [st.npiece, st.nbin, st.info["cut_cells"], st.info["max_per_bin"]]
        same = [c for c in range(NSEC) if closure is None or c not in (10, 11)]
        ok = np.array_equal(raw[:, same], hraw[:, same]) and np.array_equal(pp[same], hpp[same])
        print(f"sections {label}: device = host library, every bit of channels {same[0]}..{same[-1]}: {ok}" + (" (closure on: 10, 11 to the bound)" if closure else ""))
        assert ok, label
        if closure is not None:
            pbound = EVAL_OPS * EPS * mags.sum(axis=2)
            assert (np.abs(raw - hraw)[:, 10:12] <= bound[:, 10:12]).all() and (np.abs(pp - hpp)[10:12] <= pbound[10:12]).all(), label
    return st, raw, pp


def convection_view(model, sections):
    """the model under a convection closure that is active on the sections: alpha and N2 the model's, N2min the 30 % quantile of
    |alpha (N2 + d_z b')| over the piece points of the restatement, kappa_c = 1 (as boundary_ref.convection_view)"""
    st = npg.SectionTransports(model, sections)
    ff = piece_fields(model, st.pieces(), st._keep["frames"])
    a = np.abs(float(model.params.alpha) * (float(model.params.N2) + ff["gb"][..., 2])).ravel()
    N2min = float(np.quantile(a, 0.3))
    assert N2min > 0
    return br.view(model, conv_param=npg.ConvectionParameterization(1.0, N2min, True))


def check_bowl(arch, b_order, against_host=False):
    model = bowl(arch, b_order=b_order)
    check_restatement(quiet(model), BOWL_SECTIONS(), f"bowl P{b_order}", against_host=against_host)
    conv = convection_view(model, BOWL_SECTIONS())
    st, raw, _ = check_restatement(conv, BOWL_SECTIONS(), f"bowl P{b_order}, convection closure on", against_host=against_host)
    off = npg.SectionTransports(quiet(model), BOWL_SECTIONS()).compute_raw()[0]
    assert not np.array_equal(raw[:, 10], off[:, 10]) and np.array_equal(np.delete(raw, [10, 11], axis=1), np.delete(off, [10, 11], axis=1))


def check_single_tet(arch, against_host=False):
    """check 4: one vertex cut off - 1 piece; two from two - 2 pieces; a plane that misses - nothing, and every output zero"""
    for b_order in (2, 1):
        model = quiet(nr.single_tet(arch, b_order))
        X = cell_xyz(model.fe_data.mesh)[0]
        secs = [npg.Section.level(-0.5, name="one off"), npg.Section.longitude(0.25, name="two from two"), npg.Section.level(0.5, name="miss")]
        st, raw, pp = check_restatement(model, secs, f"single tetrahedron P{b_order}", against_host=against_host)
        _, _, abound = check_plan(model, secs, f"single tetrahedron P{b_order}")
        assert np.array_equal(np.diff(st.pieces()["bin_ptr"]), [1, 2, 0]) and (raw[2] == 0.0).all()
        on = lambda a, b, t: X[a] + t * (X[b] - X[a])                                   # noqa: E731
        tri = lambda A, B, Cc: 0.5 * np.linalg.norm(np.cross(B - A, Cc - A))            # noqa: E731
        P = [on(k, 3, (-0.5 - X[k, 2]) / (X[3, 2] - X[k, 2])) for k in range(3)]
        a0 = tri(*P)
        Q = [on(a, b, (0.25 - X[a, 0]) / (X[b, 0] - X[a, 0])) for a, b in ((0, 1), (0, 3), (2, 3), (2, 1))]
        t1, t2 = tri(Q[0], Q[1], Q[2]), tri(Q[0], Q[2], Q[3])
        z1, z2 = np.mean([Q[0][2], Q[1][2], Q[2][2]]), np.mean([Q[0][2], Q[2][2], Q[3][2]])
        _, bb = bin_sums(*restate(model, st), st.pieces()["bin_ptr"])
        assert abs(raw[0, 0] - a0) <= abound[0] and abs(raw[1, 0] - (t1 + t2)) <= abound[1]
        assert abs(raw[0, 12] + 0.5 * a0) <= 0.5 * abound[0] + bb[0, 12]
        assert abs(raw[1, 12] - (t1 * z1 + t2 * z2)) <= abound[1] + bb[1, 12]          # |z| <= 1 on this tetrahedron
        f = st.compute()
        assert np.isnan(f.mean_b["miss"]).all() and f.area["miss"][0, 0] == 0.0 and np.isfinite(f.mean_b["one off"]).all()


class Poly:
    """u quadratic, b' quadratic (P2) or linear (P1), p linear with p = 0 at the pinned vertex: the state and the closed forms"""

    def __init__(self, model):
        fed = model.fe_data
        m, t = fed.mesh, fed.tables
        assert (t.u_pos >= 0).all() and (t.b_pos >= 0).all()
        rng = np.random.default_rng(SEED)
        self.p2 = fed.spaces.b_order == 2
        Hu = rng.standard_normal((3, 3, 3))
        self.Hu, self.A, self.cu = Hu + np.swapaxes(Hu, 1, 2), rng.standard_normal((3, 3)), rng.standard_normal(3)
        Hb = rng.standard_normal((3, 3))
        self.Hb, self.cb, self.gp = (Hb + Hb.T) * (1.0 if self.p2 else 0.0), np.array([0.3, 0.2, -0.1]), np.array([0.7, -1.3, 2.1])
        self.x0 = m.coords[int(np.nonzero(t.p_pos < 0)[0][0])]
        x = np.zeros(fed.dofs.nu + fed.dofs.np)
        x[t.u_pos] = self.u(m.node_coords)
        x[t.p_pos[t.p_pos >= 0]] = self.p(m.coords)[t.p_pos >= 0]
        bvec = np.zeros(fed.dofs.nb)
        bvec[t.b_pos] = self.b(m.node_coords if self.p2 else m.coords)
        model.inversion.solver.x.upload(x)
        model.b_vec.upload(bvec)

    def u(self, X):
        return 0.5 * np.einsum("...i,aij,...j->...a", X, self.Hu, X) + X @ self.A.T + self.cu

    def b(self, X):
        return 0.5 * np.einsum("...i,ij,...j->...", X, self.Hb, X) + X @ self.cb + 1.0

    def gb(self, X):
        return X @ self.Hb + self.cb

    def p(self, X):
        return (X - self.x0) @ self.gp


def check_closed_forms(arch, against_host=False):
    """check 5: globally polynomial fields on the Kuhn cube - every bin of an oblique line, a level and a latitude, none of whose edges
    lies on a grid plane, carries the integral over its rectangle.  The reference is a tensor Gauss-Legendre rule of 4 x 4 points
    (exact to degree 7; the integrands have degree <= 4), so the only error is rounding: the restatement's bound of the bin, plus the
    bin's area bound (check 2) times the largest |integrand| at the rule's points (the pieces tile the rectangle to that much), plus
    64 eps sum |w f| for the rule's own sum."""
    KH, KV = 0.7, 0.3
    gx, gw = np.polynomial.legendre.leggauss(4)
    for b_order in (2, 1):
        model = quiet(kuhn_cube(arch, b_order), kappa_h=KH, kappa_v=KV)
        poly = Poly(model)
        secs = [npg.Section.line([0.1, 0.2], [0.9, 0.7], s_edges=[0.05, 0.31, 0.62, 0.9], z_edges=[-0.93, -0.61, -0.35, -0.07], name="line"),
                npg.Section.level(-0.3, x_edges=[0.07, 0.45, 0.91], y_edges=[0.11, 0.52, 0.83], name="level"),
                npg.Section.latitude(0.35, x_edges=[0.03, 0.6, 0.97], z_edges=[-0.9, -0.33, -0.02], name="latitude")]
        _, _, abound = check_plan(model, secs, f"closed forms P{b_order}")
        st, raw, _ = check_restatement(model, secs, f"closed forms P{b_order}, Kuhn cube", against_host=against_host)
        _, bb = bin_sums(*restate(model, st), st.pieces()["bin_ptr"])
        k, worst = 0, 0.0
        for s in secs:
            n = s.normal
            for i in range(s.shape[0]):
                for j in range(s.shape[1]):
                    a1, b1, a2, b2 = s.edges1[i], s.edges1[i + 1], s.edges2[j], s.edges2[j + 1]
                    s1, s2 = np.meshgrid(0.5 * (a1 + b1) + 0.5 * (b1 - a1) * gx, 0.5 * (a2 + b2) + 0.5 * (b2 - a2) * gx, indexing="ij")
                    w = (0.25 * (b1 - a1) * (b2 - a2) * gw[:, None] * gw[None, :]).ravel()
                    Xq = s.origin + s1.reshape(-1, 1) * s.e1 + s2.reshape(-1, 1) * s.e2
                    u, b, g, p, z = poly.u(Xq), poly.b(Xq), poly.gb(Xq), poly.p(Xq), Xq[:, 2]
                    un, gh = u @ n, g[:, 0] * n[0] + g[:, 1] * n[1]
                    f = [np.ones_like(z), un, b, b * un, z * un, p, u[:, 0], u[:, 1], u[:, 2], g @ n, KH * gh + KV * g[:, 2] * n[2],
                         KV * n[2] * np.ones_like(z), z, g[:, 2]]
                    for ch in range(NSEC):
                        ref = float(w @ f[ch])
                        bound = bb[k, ch] + abound[k] * float(np.abs(f[ch]).max()) + 64 * EPS * float(w @ np.abs(f[ch]))
                        worst = max(worst, abs(raw[k, ch] - ref) / bound if bound > 0 else 0.0)
                        assert abs(raw[k, ch] - ref) <= bound, (s.name, i, j, ch, raw[k, ch], ref, bound)
                    # channels 10 and 11 with constant kappa are kappa times their parts
                    parts = KH * float(w @ gh) + KV * float(w @ (g[:, 2] * n[2]))
                    assert abs(raw[k, 10] - parts) <= bb[k, 10] + abound[k] * float(np.abs(f[10]).max()) + 64 * EPS * float(w @ np.abs(f[10]))
                    assert abs(raw[k, 11] - KV * n[2] * raw[k, 0]) <= bb[k, 11] + 4 * EPS * abs(raw[k, 11])
                    k += 1
        assert k == st.nbin
        print(f"sections closed forms P{b_order}: {st.nbin} bins, worst |err| / bound {worst:.3f}")


def check_dirichlet_and_pin(arch, against_host=False):
    """bowl_wind: Dirichlet DoFs of u and of b enter with their table values; a level through the cells of the pinned pressure vertex"""
    model = bowl(arch, "bowl_wind")
    t, m = model.fe_data.tables, model.fe_data.mesh
    assert (t.u_pos < 0).any() and (t.b_pos < 0).any() and (t.p_pos < 0).sum() == 1
    pin = int(np.nonzero(t.p_pos < 0)[0][0])
    cells = np.nonzero((m.cells == pin).any(axis=1))[0]
    z0 = float(cell_xyz(m)[cells[0]].mean(axis=0)[2])
    secs = [npg.Section.level(z0, name="through the pin's cells"), npg.Section.longitude(0.1, z_edges=[-1.0, -0.5, -0.02, 0.0]),
            npg.Section.latitude(0.0)]
    st, raw, _ = check_restatement(model, secs, "bowl_wind (Dirichlet u and b, pinned p)", against_host=against_host)
    pc = st.pieces()["cell"]
    assert np.isin(pc, cells).any()
    assert (t.u_pos[m.cell_nodes[pc]] < 0).any() and (t.b_pos[m.cell_nodes[pc] if model.fe_data.spaces.b_order == 2 else m.cells[pc]] < 0).any()


def check_channel(arch, b_order, against_host=False):
    """the periodic channel basin: a latitude across the whole period cuts cells at the seam.  The seam cells are those whose TOPOLOGICAL
    vertices (mesh.coords[mesh.cells], one coordinate per glued vertex) lie more than half a period apart; their own geometry
    (geo_coords[cell_geo], what the cut rule reads) is unwrapped and never spans it - asserted both ways, so "pieces exist in the seam
    cells" is asked of the topological extent, not of the cells' own"""
    model = nr.channel(arch, b_order)
    m = model.fe_data.mesh
    assert m.periodic
    X = cell_xyz(m)
    period = float(X[..., 0].max() - X[..., 0].min())
    topo = m.coords[m.cells][..., 0]
    seam = (topo.max(axis=1) - topo.min(axis=1)) > 0.5 * period                         # cells whose topological x-extent spans the seam
    own = (X[..., 0].max(axis=1) - X[..., 0].min(axis=1)) > 0.5 * period
    assert seam.any() and not own.any()
    y0 = float(np.median(X[seam][..., 1].mean(axis=1))) + 0.013                         # a latitude of the periodic part (the channel)
    zmid = float(0.5 * (X[..., 2].min() + X[..., 2].max())) + 0.003
    secs = [npg.Section.latitude(y0, x_edges=np.linspace(X[..., 0].min(), X[..., 0].max() + 1e-9, 5), z_edges=[-np.inf, zmid, np.inf], name="across"),
            npg.Section.longitude(float(X[..., 0].min()) + 0.37 * period, name="meridional"), npg.Section.level(zmid, name="level")]
    st, raw, pp = check_restatement(quiet(model), secs, f"channel basin P{b_order}", against_host=against_host)
    pl = st.pieces()
    hit = seam[pl["cell"]] & (pl["section"] == 0)
    print(f"sections channel basin P{b_order}: {int(seam.sum())} seam cells, {int(hit.sum())} pieces of the latitude lie in them")
    assert hit.any()
    assert np.isfinite(raw).all() and np.isfinite(pp).all()
    st2, area, bound = check_plan(model, secs, f"channel basin P{b_order}")


def piece_masks(model, sec):
    """{count: cell mask} with exactly 0, 1, 63, 64, 65, 255, 256, 257 pieces on `sec`: cut cells in order, a one-piece cell for parity"""
    st = npg.SectionTransports(model, sec)
    per = np.bincount(st.pieces()["cell"], minlength=model.fe_data.mesh.ncell)
    cut = np.nonzero(per)[0]
    assert (per[cut] == 1).sum() == 257 and (per[cut] == 2).sum() == 110 and set(per[cut]) == {1, 2}
    out = {}
    for n in EDGE_COUNTS:
        mk = np.zeros(len(per), dtype=bool)
        tot = 0
        for c in cut:                                                                  # in order, every cell that still fits: a one-piece
            if tot + per[c] <= n:                                                      # cell further on fills the last place
                mk[c] = True
                tot += per[c]
        assert tot == n
        out[n] = mk
    return out


def check_masks(model, against_host=False):
    """check 7: exactly 0 .. 257 pieces through the cell mask, and one bin of more than 256 pieces beside a single-piece bin and empty
    bins (z edges above z = 0)"""
    sec = npg.Section.longitude(0.1)
    for n, mk in piece_masks(model, sec).items():
        st, raw, pp = check_restatement(model, sec, f"mask of {n} pieces", mask=mk, against_host=against_host)
        assert st.npiece == n
    full = npg.SectionTransports(model, sec)
    pl = full.pieces()
    per = np.bincount(pl["cell"], minlength=model.fe_data.mesh.ncell)
    zlo = np.full(len(per), np.inf)
    zhi = np.full(len(per), -np.inf)
    np.minimum.at(zlo, pl["cell"], pl["corners"][:, :, 2].min(axis=1))
    np.maximum.at(zhi, pl["cell"], pl["corners"][:, :, 2].max(axis=1))
    ones = np.nonzero(per == 1)[0]
    c1 = int(ones[np.argmax(zlo[ones])])                                                # the one-piece cell nearest the surface
    zcut = float(zlo[c1]) - 1e-3
    mk = (per > 0) & (zhi < zcut)
    mk[c1] = True
    big = npg.Section.longitude(0.1, z_edges=[-1.5, zcut, 0.25, 0.5, 1.0], name="one large bin")
    st, raw, _ = check_restatement(model, big, "one bin of > 256 pieces, one of 1, two empty", mask=mk, against_host=against_host)
    counts = np.diff(st.pieces()["bin_ptr"])
    assert counts[0] > 256 and list(counts[1:]) == [1, 0, 0] and (raw[2:] == 0.0).all(), counts


def check_determinism_and_handle(model):
    """check 9: two calls - the same bits; pieces=True does not change out; set_coeff(None) restores the bits from before; a failed
    set_coeff leaves the handle as it was"""
    model = quiet(model)
    st = npg.SectionTransports(model, BOWL_SECTIONS())
    a, _ = st.compute_raw()
    b, pb = st.compute_raw(pieces=True)
    c, _ = st.compute_raw()
    d, pd = npg.SectionTransports(model, BOWL_SECTIONS()).compute_raw(pieces=True)
    assert np.array_equal(a, b) and np.array_equal(a, c) and np.array_equal(a, d) and np.array_equal(pb, pd) and np.isfinite(a).all()
    st.set_coeff(L.NPG_SEC_KH, None)
    r0, _ = st.compute_raw()
    assert np.array_equal(np.delete(r0, 10, axis=1), np.delete(a, 10, axis=1)) and not np.array_equal(r0[:, 10], a[:, 10])
    tab = np.random.default_rng(SEED).random((st.npiece, 6))
    st.set_coeff(L.NPG_SEC_KH, tab)
    r1, _ = st.compute_raw()
    assert not np.array_equal(r1[:, 10], r0[:, 10])
    bad = tab.copy()
    bad[st.npiece // 2, 3] = np.nan
    with np.testing.assert_raises(L.DeviceError):
        st.set_coeff(L.NPG_SEC_KH, bad)
    with np.testing.assert_raises(ValueError):
        st.set_coeff(L.NPG_SEC_KH, tab[:-1])
    rc = L.lib().npg_sections_set_coeff(st.h, 2, None)
    assert rc == NPG_EINVAL and "which" in L.lib().npg_last_error().decode()
    assert np.array_equal(st.compute_raw()[0], r1)                                      # the handle is as it was
    st.set_coeff(L.NPG_SEC_KH, None)
    assert np.array_equal(st.compute_raw()[0], r0)
    # the Python conveniences on the same numbers
    f = st.compute(pieces=True)
    nm = st.names[0]
    assert f.raw[nm].shape == (4, 3, NSEC) and np.array_equal(f.volume_transport[nm], f.raw[nm][..., 1])
    psi = f.streamfunction(nm, axis=1)
    assert psi.shape == (4, 4) and (psi[:, 0] == 0.0).all() and np.array_equal(psi[:, 1:], np.cumsum(f.volume_transport[nm], axis=1))
    back = f.streamfunction(nm, axis=0, from_end=True)
    assert back.shape == (5, 3) and (back[-1] == 0.0).all() and np.allclose(back[0], f.volume_transport[nm].sum(axis=0), rtol=0, atol=1e-15)
    assert f.total("area")[nm] == float(f.area[nm].sum()) and f.mean_u[nm].shape == (4, 3, 3)
    with np.testing.assert_raises(ValueError):
        f.total("mean_b")
    mp = f.maps
    assert mp.values.shape == (NSEC, st.npiece) and np.array_equal(mp.values[0], np.ones(st.npiece)) and mp.of(nm).sum() > 0
    assert np.array_equal(np.sort(np.concatenate([np.nonzero(mp.of(n_))[0] for n_ in st.names])), np.arange(st.npiece))
    rec = npg.SectionRecorder(st, every=2)
    for k in range(3):
        rec(model, 0.5 * k)
    t, series = rec.as_arrays()
    assert np.array_equal(t, [0.0, 1.0]) and series.shape == (2, st.nbin, NSEC) and np.array_equal(series[0], r0) and len(rec.fluxes()) == 2


def check_physics(arch):
    """check 10: a stepped closed basin.  The part of the basin on one side of a full section is bounded by the section and by boundary
    faces, so |int_section u . n| <= |int_part div u| + sum_groups |boundary volume flux| <= sqrt(V int (div u)^2) + ... (divergence
    theorem, Cauchy-Schwarz): no tuned number"""
    model = sr.bowl_model(arch, "bowl_surface_flux", nsteps=1)
    bud = npg.MeshIntegrals(model).compute()
    bf = npg.BoundaryIntegrals(model).compute()
    limit = math.sqrt(bud.volume * bud.div2) + sum(abs(v) for v in bf.volume_flux.values())
    secs = [npg.Section.longitude(0.1), npg.Section.latitude(0.0), npg.Section.level(-0.3)]
    f = npg.SectionTransports(model, secs).compute()
    for s in secs:
        vt = f.total("volume_transport")[s.name]
        print(f"sections physics {s.name}: |volume transport| {abs(vt):.3e} / limit {limit:.3e} = {abs(vt) / limit:.3f}; area {f.total('area')[s.name]:.6f}")
        assert abs(vt) <= limit and np.isfinite(vt)
    assert limit > 0.0


def check_python_refusals(model):
    """everything the Python layer refuses, each leaving the model untouched"""
    before = dict(vars(model))
    base = {k: v for k, v in vars(model).items() if k in ("arch", "fe_data", "params", "forcings", "b_vec", "inversion")}
    S = npg.Section
    with np.testing.assert_raises(ValueError):
        npg.SectionTransports(model, [S.latitude(0.0, name="a"), S.level(-0.3, name="a")])
    with np.testing.assert_raises(ValueError):
        npg.SectionTransports(model, [])
    with np.testing.assert_raises(ValueError):
        npg.SectionTransports(model, S.latitude(0.0), mask=np.ones(3, dtype=bool))
    with np.testing.assert_raises(ValueError):
        S.line([0.1, 0.1], [0.1, 0.1])
    with np.testing.assert_raises(ValueError):
        S.latitude(0.0, z_edges=[0.0])
    for bad, word in ((S("skew", [0, 0, 0], [0, 1, 0], [1, 1e-6, 0], [0, 0, 1]), "orthonormal"),
                      (S("long", [0, 0, 0], [0, 2, 0], [1, 0, 0], [0, 0, 1]), "orthonormal"),
                      (S.latitude(0.0, z_edges=[-1.0, -0.5, -0.5, 0.0]), "strictly increasing"),
                      (S.latitude(0.0, z_edges=[0.0, -1.0]), "strictly increasing"),
                      (S.latitude(0.0, z_edges=[-1.0, np.inf, 2.0]), "not finite"),
                      (S.latitude(0.0, x_edges=[-np.inf, -np.inf, 0.0]), "not finite"),
                      (S.latitude(0.0, x_edges=[np.inf, 2.0]), "not finite"),
                      (S.latitude(0.0, z_edges=[-1.0, np.nan]), "not finite"),
                      (S.latitude(np.nan), "frame is not finite"),
                      (S.latitude(0.0, x_edges=np.arange(1026.0), z_edges=np.arange(1026.0)), "2^20 bins")):
        with np.testing.assert_raises(L.DeviceError) as cm:
            npg.SectionTransports(model, bad)
        assert word in str(cm.exception), (word, str(cm.exception))
    part = SimpleNamespace(**base, layout=SimpleNamespace(cell_owner=None, locator_cells=None))
    repl = SimpleNamespace(**base, partition=object())
    comm = SimpleNamespace(**base, comm=object())
    for fake in (part, repl, comm):
        with np.testing.assert_raises(NotImplementedError):
            npg.SectionTransports(fake, S.latitude(0.0))
    assert dict(vars(model)) == before


def check_2d_refused(arch):
    """an embedded 2-D mesh: NotImplementedError in Python, NPG_EINVAL from the library"""
    model = nr.with_config(ar.bowl2d_light(arch), "bowl_mixing")
    with np.testing.assert_raises(NotImplementedError):
        npg.SectionTransports(model, npg.Section.latitude(0.0))
    fe = device_fe(arch, model.fe_data)
    s = npg.Section.latitude(0.0)
    X = np.zeros((model.fe_data.mesh.ncell, 4, 3))
    h = C.c_void_p()
    rc = L.lib().npg_sections_create(fe.h, L.ptr(X), 1, L.ptr(L.as_f64(s.frame)), L.ptr(L.as_i32([1])), L.ptr(L.as_i32([1])), L.ptr(s.edges1),
                                     L.ptr(s.edges2), None, C.byref(h))
    assert rc == NPG_EINVAL and "2-D" in L.lib().npg_last_error().decode() and not h.value


def abi_refusals(lib, fe, X, vec, vecs, other_vec):
    """the C ABI's NPG_EINVAL cases against one library: every line of check_sections_create / _coeff / _closure / _compute with its
    message.  Everything is refused on the host before any launch: no case relies on a device fault."""
    s = npg.Section.longitude(0.1, z_edges=[-1.0, -0.5, 0.0])
    good = dict(fe=fe, X=X, nsec=1, frames=L.as_f64(s.frame), n1=L.as_i32([1]), n2=L.as_i32([2]), e1=L.as_f64(s.edges1), e2=L.as_f64(s.edges2), out=True)

    def create(**kw):
        a = dict(good)
        a.update(kw)
        h = C.c_void_p()
        p = lambda v: None if v is None else L.ptr(v)
        rc = lib.npg_sections_create(a["fe"], p(a["X"]), a["nsec"], p(a["frames"]), p(a["n1"]), p(a["n2"]), p(a["e1"]), p(a["e2"]), None,
                                     C.byref(h) if a["out"] else None)
        return rc, lib.npg_last_error().decode(), h

    def bad(a, i, v):
        a = a.copy()
        a.reshape(-1)[i] = v
        return a
    f = good["frames"]
    for kw, word in ((dict(fe=None), "NULL"), (dict(out=False), "NULL"), (dict(X=None), "NULL table"), (dict(frames=None), "NULL table"),
                     (dict(e2=None), "NULL table"), (dict(nsec=0), "nsec must be"), (dict(nsec=65), "nsec must be"),
                     (dict(frames=bad(f, 1, np.inf)), "frame is not finite"), (dict(frames=bad(f, 3, 0.5)), "orthonormal"),
                     (dict(frames=bad(f, 7, 1e-9)), "orthonormal"), (dict(n1=L.as_i32([0])), "at least one bin"),
                     (dict(n2=L.as_i32([1 << 21])), "2^20 bins"), (dict(e2=L.as_f64([-1.0, -1.0, 0.0])), "strictly increasing"),
                     (dict(e2=L.as_f64([-1.0, np.inf, 2.0])), "not finite"), (dict(e1=L.as_f64([np.nan, 1.0])), "not finite"),
                     (dict(X=bad(X, 40, np.nan)), "vertex is not finite")):
        rc, msg, h = create(**kw)
        assert rc == NPG_EINVAL and word in msg and not h.value, (list(kw), rc, msg)
    rc, msg, h = create()
    assert rc == 0, msg
    q = [C.c_int64() for _ in range(4)]
    assert lib.npg_sections_info(h, *[C.byref(v) for v in q]) == 0 and lib.npg_sections_info(None, None, None, None, None) == NPG_EINVAL
    n, nbin = q[0].value, q[1].value
    assert nbin == 2 and n > 0
    tab = np.ones((6, n))
    for args, word in (((None, 0, L.ptr(tab)), "NULL"), ((h, -1, L.ptr(tab)), "which"), ((h, 2, None), "which"),
                       ((h, 1, L.ptr(bad(tab, 5 * n + 1, np.inf))), "not finite at point 5 of piece 1")):
        assert lib.npg_sections_set_coeff(*args) == NPG_EINVAL and word in lib.npg_last_error().decode(), (word, lib.npg_last_error().decode())
    for args, word in (((None, 1.0, 1.0, 1.0, 1.0), "NULL"), ((h, -1.0, 1.0, 1.0, 1.0), "kappa_c must be"), ((h, 1.0, 1.0, np.nan, 1.0), "kappa_c must be"),
                       ((h, 1.0, 0.0, 1.0, 1.0), "needs N2min > 0")):
        assert lib.npg_sections_set_closure(*args) == NPG_EINVAL and word in lib.npg_last_error().decode(), word
    x, b = vecs
    out = vec(nbin * NSEC, -7.0)
    for args, word in (((h, vec(x[1] - 1)[0], b[0], out[0], None), "flow vector"), ((h, x[0], vec(b[1] + 1)[0], out[0], None), "buoyancy vector"),
                       ((h, x[0], b[0], vec(nbin * NSEC - 1)[0], None), "out holds"), ((h, x[0], b[0], out[0], vec(NSEC * n - 1)[0]), "pieces_out holds"),
                       ((None, x[0], b[0], out[0], None), "NULL"), ((h, None, b[0], out[0], None), "NULL"), ((h, x[0], b[0], None, None), "NULL"),
                       ((h, x[0], other_vec(b[1])[0], out[0], None), "different contexts"), ((h, x[0], b[0], other_vec(nbin * NSEC)[0], None), "different contexts"),
                       ((h, x[0], b[0], out[0], other_vec(NSEC * n)[0]), "different contexts")):
        rc = lib.npg_sections_compute(*args)
        msg = lib.npg_last_error().decode()
        assert rc == NPG_EINVAL and word in msg, (rc, msg)
    assert lib.npg_sections_pieces(None, None, None, None, None) == NPG_EINVAL
    return h, out


def check_abi_refusals(model):
    """check 11 through the library the model runs on: the refusals, nothing launched by a refused compute"""
    lib = L.lib()
    ctx = model.arch.ctx
    fe = device_fe(model.arch, model.fe_data)
    x, b = model.inversion.solver.x, model.b_vec
    keep = []

    def vec(n, fill=0.0):
        v = npg.DeviceVector(ctx, n)
        v.fill(fill)
        keep.append(v)
        return v.h, n
    other_ctx = Context(ctx.device)                                                    # a second context of the same library

    def other_vec(n):
        v = npg.DeviceVector(other_ctx, n)
        keep.append(v)
        return v.h, n
    h, out = abi_refusals(lib, fe.h, L.as_f64(cell_xyz(model.fe_data.mesh)), vec, ((x.h, x.n), (b.h, b.n)), other_vec)
    first = [v for v in keep if v.n == 2 * NSEC][0]
    assert np.array_equal(first.to_host(), np.full(first.n, -7.0))                     # nothing was launched
    L.check(lib.npg_sections_compute(h, x.h, b.h, out[0], None))
    assert not np.array_equal(first.to_host(), np.full(first.n, -7.0))
    L.check(lib.npg_sections_destroy(h))
    L.check(lib.npg_sections_destroy(None))


def check_host_abi_refusals(model):
    """the same NPG_EINVAL cases, with a message, from the host library"""
    E = nr.HostEngine(model)

    def vec(n, fill=0.0):
        return E.vec(np.full(n, fill)), n
    x, b = model.inversion.solver.x, model.b_vec
    ctx2 = C.c_void_p()
    E.ok(E.H.npg_ctx_create(0, C.byref(ctx2)))                                          # a second context of the host library

    def other_vec(n):
        v = C.c_void_p()
        E.ok(E.H.npg_vec_create(ctx2, n, C.byref(v)))
        E.vecs.append(v)
        return v, n
    h, _ = abi_refusals(E.H, E.fe, L.as_f64(cell_xyz(model.fe_data.mesh)), vec, (vec(x.n), vec(b.n)), other_vec)
    E.H.npg_sections_destroy(h)
    E.close()
    E.H.npg_ctx_destroy(ctx2)
