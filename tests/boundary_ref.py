"""A numpy restatement of the boundary integrals (nupgcm_amd.boundary) and the checks shared by tests/test_boundary.py
(CPU()) and tests/test_gpu_boundary.py (GPU()).

The restatement is written from the definitions, not from the code under test: a face finds its cell through a dictionary over the
sides of all cells, the geometry comes from the cells' own vertex coordinates (inverse of the edge matrix, not grad_lambda), the
normal's orientation from the sign of grad lambda_k of the face's cell (not from the opposite vertex), the shape functions
come from fe.p2_tables at the lifted points, nodal values through Spaces' native tables, coefficients from the forcing functions at the
face points.  Per channel it keeps the terms w_q area2 integrand as an array (nface, 9) in the order of BoundaryIntegrals.faces.

Bounds.  A recursive sum of n terms t_k differs from the exact sum by at most (n - 1) eps sum |t_k| (Higham, Accuracy and Stability,
eq. 4.4) in any order; the bound used for every sum of the restatement's own terms is  n_faces n_q eps S_abs  over the faces that
count, as tests/integrals_ref.py does for the cells.  One FACE's own nine terms are compared with face_bound() below: the rounding of
evaluating a term, which n_q eps S_abs does not model (measured on bowl_surface_flux: up to 4.7 x 9 eps S_abs of a face in the
gradient channels 17 and 21, below 0.5 in the others).  Where a second quantity enters (a volume integral, a load vector, a closed
form) its own bound of the same kind is added and said there."""
import math
import os
from types import SimpleNamespace

import numpy as np

import nupgcm_amd as npg
from nupgcm_amd import _lib as L
from nupgcm_amd import fe as F
from nupgcm_amd import gmsh_io
from nupgcm_amd.inversion import device_fe
from tests import helpers
from tests import integrals_ref as ir
from tests import sampling_ref as sr

EPS = np.finfo(np.float64).eps
NBND = 24
NQ = 9
NPG_EINVAL = -1
SEED = 20261019
NEW = {"npg_boundary_create", "npg_boundary_set_coeff", "npg_boundary_set_closure", "npg_boundary_compute", "npg_boundary_destroy"}


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def nodal_values(model):
    """(un (nn, 3), pn (nv,), bn (nb_nodes,)) at the nodes from the device vectors; Dirichlet nodes with their values, the pinned
    pressure vertex 0"""
    un, bn = ir.nodal_values(model)
    t = model.fe_data.tables
    x = model.inversion.solver.x.to_host()
    pn = np.where(t.p_pos >= 0, x[np.maximum(t.p_pos, 0)], 0.0)
    return un, pn, bn


def locate_faces(mesh, faces):
    """(cell, local face, Gmsh nodes (nf, 3), tag mask) of sorted vertex triples, through dictionaries"""
    sides = {}
    for k in range(4):
        for c, tri in enumerate(map(tuple, np.delete(mesh.cells, k, axis=1))):
            sides.setdefault(tri, []).append((c, k))
    facet = {tuple(t): i for i, t in enumerate(mesh._facets)}
    cell, local, geo, phys = [], [], [], []
    for t in map(tuple, np.asarray(faces)):
        assert len(sides[t]) == 1, (t, sides[t])
        cell.append(sides[t][0][0]), local.append(sides[t][0][1])
        geo.append(mesh._facets_geo[facet[t]]), phys.append(int(mesh._facets_phys[facet[t]]))
    return np.array(cell, dtype=np.int64), np.array(local, dtype=np.int64), np.array(geo, dtype=np.int64).reshape(-1, 3), np.array(phys, dtype=np.int64)


def _coef(v, xq):
    if v is None:
        return np.zeros(xq.shape[:2])
    return np.broadcast_to(np.asarray(v(xq), dtype=float), xq.shape[:2]) if callable(v) else np.full(xq.shape[:2], float(v))


def face_fields(model, faces):
    """the fields at the 9 points of every face: dict of u (nf, 9, 3), gu (nf, 9, 3, 3) = d_j u_a, p, b, gb (nf, 9, 3), xq, n (nf, 3),
    W (nf, 9), surface (nf,) bool, absN (nf, 9) = sum_i |N_i|"""
    fed = model.fe_data
    m = fed.mesh
    un, pn, bn = nodal_values(model)
    cell, k, geo, phys = locate_faces(m, faces)
    X = m.geo_coords[m.cell_geo]
    g = np.linalg.inv(np.transpose(X[:, 1:] - X[:, :1], (0, 2, 1)))
    G = np.concatenate([-g.sum(axis=1, keepdims=True), g], axis=1)[cell]                # (nf, 4, 3)
    lam3, w = F.tri_quadrature_degree4()
    lam4 = np.stack([np.insert(lam3, kk, 0.0, axis=1) for kk in range(4)])              # (4, 9, 4): lambda_k = 0
    tabs = [F.p2_tables(lam4[kk], F._TET_EDGE_A, F._TET_EDGE_B) for kk in range(4)]
    N, dN = np.stack([t[0] for t in tabs])[k], np.stack([t[1] for t in tabs])[k]        # (nf, 9, 10), (nf, 9, 10, 4)
    lam = lam4[k]
    uc = un[m.cell_nodes[cell]]
    out = {"u": np.einsum("fqi,fia->fqa", N, uc), "gu": np.einsum("fqik,fia,fkj->fqaj", dN, uc, G),
           "p": np.einsum("fqm,fm->fq", lam, pn[m.cells[cell]])}
    if fed.spaces.b_order == 2:
        bc = bn[m.cell_nodes[cell]]
        out["b"], out["gb"] = np.einsum("fqi,fi->fq", N, bc), np.einsum("fqik,fi,fkj->fqj", dN, bc, G)
    else:
        bc = bn[m.cells[cell]]
        out["b"] = np.einsum("fqm,fm->fq", lam, bc)
        out["gb"] = np.broadcast_to(np.einsum("fk,fkj->fj", bc, G)[:, None, :], (len(cell), NQ, 3))
    aN, adN, aG = np.abs(N), np.abs(dN), np.abs(G)                                      # the magnitudes of every field's constituents
    out["a_u"], out["a_gu"] = np.einsum("fqi,fia->fqa", aN, np.abs(uc)), np.einsum("fqik,fia,fkj->fqaj", adN, np.abs(uc), aG)
    out["a_p"] = np.einsum("fqm,fm->fq", lam, np.abs(pn[m.cells[cell]]))
    if fed.spaces.b_order == 2:
        out["a_b"], out["a_gb"] = np.einsum("fqi,fi->fq", aN, np.abs(bc)), np.einsum("fqik,fi,fkj->fqj", adN, np.abs(bc), aG)
    else:
        out["a_b"] = np.einsum("fqm,fm->fq", lam, np.abs(bc))
        out["a_gb"] = np.broadcast_to(np.einsum("fk,fkj->fj", np.abs(bc), aG)[:, None, :], (len(cell), NQ, 3))
    Xf = m.geo_coords[geo]
    out["xq"] = np.einsum("qj,fji->fqi", lam3, Xf)
    out["a_z"] = np.einsum("qj,fj->fq", lam3, np.abs(Xf[:, :, 2]))
    cr = np.cross(Xf[:, 1] - Xf[:, 0], Xf[:, 2] - Xf[:, 0])
    area2 = np.linalg.norm(cr, axis=1)
    # the DIRECTION from the face's own nodes (every component to rounding, exact zeros on the flat surface - -grad lambda_k / |.| comes
    # out of a matrix inverse with an absolute error per component), the ORIENTATION from the cell: lambda_k decreases outwards
    gk = G[np.arange(len(cell)), k]
    out["n"] = np.where((np.einsum("fi,fi->f", cr, gk) > 0.0)[:, None], -cr, cr) / area2[:, None]
    assert (np.abs(np.einsum("fi,fi->f", out["n"], gk)) >= (1.0 - 1e-9) * np.linalg.norm(gk, axis=1)).all()          # parallel to grad lambda_k
    out["W"] = w[None, :] * area2[:, None]
    surf = np.zeros(len(cell), dtype=bool)
    for nm in m.surface_tags:
        surf |= (phys >> m.tag_bit(nm)) & 1 == 1
    out["surface"], out["cell"], out["local"] = surf, cell, k
    out["absN"] = np.abs(N).sum(axis=2)
    return out


def _channels(W, n, zq, u, gu, p, b, gb, nu, kh, kv, taux, tauy, flux, full):
    """the NBND integrands times W; called with the fields, and again with the magnitudes of their constituents (everything >= 0)"""
    nx, ny, nz = n[:, None, 0], n[:, None, 1], n[:, None, 2]
    un_ = (u * n[:, None, :]).sum(axis=-1)
    S = gu + np.swapaxes(gu, -1, -2) if full else gu
    t = nu[..., None] * np.einsum("fqaj,fj->fqa", S, n)
    one = np.ones_like(p)
    ch = [one, one * nx, one * ny, one * nz, zq * nz, un_, b, b * un_, p, p * nx, p * ny, p * nz, p * un_, t[..., 0], t[..., 1], t[..., 2],
          (u * t).sum(axis=-1), kh * (gb[..., 0] * nx + gb[..., 1] * ny) + kv * gb[..., 2] * nz, kv * nz, taux * u[..., 0] + tauy * u[..., 1],
          flux, gb[..., 2], u[..., 0], u[..., 1]]
    return np.stack([W * c_ for c_ in ch])


def restate(model, faces, coef=None):
    """(terms (NBND, nface, 9), mags (NBND, nface, 9), face_fields).  mags: the same expressions with every constituent replaced by its
    magnitude (sum_i |N_i| |u_i|, sum |dN| |u| |grad lambda|, |n|, ...) - what the rounding of ONE term's evaluation is relative to.
    coef: overrides of the forcings' nu, kh, kv, taux, tauy, flux (numbers or functions of x) and full_stress; the eddy closure leaves nu
    out (the library returns NaN there); the convection closure is the model's"""
    f, prm = model.forcings, model.params
    ff = face_fields(model, faces)
    u, gu, p, b, gb, xq, n, W = (ff[k] for k in ("u", "gu", "p", "b", "gb", "xq", "n", "W"))
    c = dict(nu=None if f.eddy_param.is_on else f.nu, kh=f.kappa_h, kv=f.kappa_v, taux=f.tau_x, tauy=f.tau_y,
             flux=f.b_surface_bc.flux if isinstance(f.b_surface_bc, npg.SurfaceFluxBC) else None)
    c.update(coef or {})
    nu, kh, kv = (_coef(c[k], xq) for k in ("nu", "kh", "kv"))
    on = ff["surface"][:, None]
    taux, tauy, flux = (np.where(on, _coef(c[k], xq), 0.0) for k in ("taux", "tauy", "flux"))
    akv = np.abs(kv)
    if f.conv_param.is_on:
        cp, al, N2 = f.conv_param, float(prm.alpha), float(prm.N2)
        x = -al * (N2 + gb[..., 2]) / cp.N2min
        kv = kv + cp.kappa_c * (1.0 + np.tanh(x)) / 2.0
        # the constituents of kappa_v0 + kappa_c (1 + tanh x) / 2: the sum 1 + tanh x cancels where the column is stable (tanh x -> -1),
        # and d kappa_v = kappa_c sech^2(x) dx / 2 with dx relative to the magnitude of x's constituents
        akv = akv + 0.5 * cp.kappa_c * (1.0 + np.abs(np.tanh(x))) + 0.5 * cp.kappa_c / np.cosh(x) ** 2 * abs(al) * (abs(N2) + ff["a_gb"][..., 2]) / cp.N2min
    full = bool(callable(f.nu) or f.eddy_param.is_on) if "full_stress" not in c else bool(c["full_stress"])
    terms = _channels(W, n, xq[..., 2], u, gu, p, b, gb, nu, kh, kv, taux, tauy, flux, full)
    mags = _channels(W, np.abs(n), ff["a_z"], ff["a_u"], ff["a_gu"], ff["a_p"], ff["a_b"], ff["a_gb"], np.abs(nu), np.abs(kh), akv,
                     np.abs(taux), np.abs(tauy), np.abs(flux), full)
    return terms, mags, ff


def group_sums(terms, group, ngroup, mask=None):
    """(tot, sabs, count) per group: math.fsum of the terms of the faces that count, sum |term|, the number of those faces"""
    tot, sabs, cnt = np.zeros((ngroup, NBND)), np.zeros((ngroup, NBND)), np.zeros(ngroup, dtype=np.int64)
    for g in range(ngroup):
        sel = (group == g) if mask is None else (group == g) & np.asarray(mask, dtype=bool)
        cnt[g] = sel.sum()
        for k in range(NBND):
            tot[g, k], sabs[g, k] = math.fsum(terms[k][sel].ravel()), math.fsum(np.abs(terms[k][sel]).ravel())
    return tot, sabs, cnt


EVAL_OPS = 128


def face_bound(mags):
    """One face's own integrals are nine terms, and here the rounding of EVALUATING a term outweighs that of adding nine: a gradient at a
    point is an inner product of 10 x 4 products dN_ik v_i G_kj that cancel (b' = z / alpha + ...: |d_z b'| is a tenth of sum |dN| |b'|
    |G|), so the error of a term is relative to the magnitude of its constituents, not to |term|.  Standard inner-product analysis
    (Higham eq. 3.5): |fl(term) - term| <= gamma_n x magnitude with n the operations on the longest path - 40 products + 40 additions for a
    gradient component, 3 + 3 for the contraction with n, a handful for the coefficient and the measure: fewer than 64.  Both sides of the
    comparison (library and restatement) err this much: EVAL_OPS = 2 x 64 = 128, times eps, times the magnitude summed over the points
    (which also covers the nine additions: 128 magnitude >= 9 |term|)."""
    return EVAL_OPS * EPS * mags.sum(axis=2)


def summation_bound(nfaces, sabs):
    """per group: nfaces (ngroup,), sabs (ngroup, NBND)"""
    return np.asarray(nfaces)[:, None] * NQ * EPS * np.asarray(sabs)


def compare(bi, raw, per_face, terms, mags, label, mask=None, skip=()):
    """every channel of every group within the summation bound of the restatement, every face's own integrals within the bound of its
    nine terms, and the column sums of the per-face table against the group totals; prints the measured errors first"""
    ng = len(bi.groups)
    tot, sabs, cnt = group_sums(terms, bi.face_group, ng, mask)
    bound = summation_bound(cnt, sabs)
    err = np.abs(raw - tot)
    for g, name in enumerate(bi.groups):
        print(f"boundary {label} [{name}: {cnt[g]} faces]: " + ", ".join(f"ch{k} {err[g, k]:.1e}/{bound[g, k]:.1e}" for k in range(NBND) if k not in skip))
    for g in range(ng):
        for k in range(NBND):
            if k not in skip:
                assert err[g, k] <= bound[g, k], (label, bi.groups[g], k, raw[g, k], tot[g, k], err[g, k], bound[g, k])
    worst = None
    if per_face is not None:
        keep = np.ones(len(bi.faces), dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
        ftot = np.array([[math.fsum(r) for r in terms[k]] for k in range(NBND)])           # (NBND, nface)
        fbound = face_bound(mags)
        ferr = np.abs(per_face - np.where(keep, ftot, 0.0))
        ratio = np.where(fbound > 0, ferr / np.where(fbound > 0, fbound, 1.0), np.where(ferr > 0, np.inf, 0.0))
        worst = [float(ratio[k].max(initial=0.0)) for k in range(NBND)]
        print(f"boundary {label} per face, worst |err| / ({EVAL_OPS} eps magnitude of the face's terms): " + ", ".join(f"ch{k} {worst[k]:.2f}" for k in range(NBND) if k not in skip))
        assert (per_face[:, ~keep] == 0.0).all()
        for k in range(NBND):
            if k not in skip:
                assert (ferr[k] <= fbound[k]).all(), (label, "per face", k, worst[k])
        for g in range(ng):
            sel = (bi.face_group == g) & keep
            cerr = np.abs(np.array([math.fsum(per_face[k][sel]) for k in range(NBND)]) - raw[g])
            print(f"boundary {label} [{bi.groups[g]}] column sums - totals: " + ", ".join(f"ch{k} {cerr[k]:.1e}" for k in range(NBND) if k not in skip))
            for k in range(NBND):
                if k not in skip:
                    assert cerr[k] <= bound[g, k], (label, "column sums", bi.groups[g], k, cerr[k], bound[g, k])
    return err, bound, worst


# ---- models -----------------------------------------------------------------------------------------------------------------------
def view(model, **frc_kw):
    """the model's state and mesh under other forcings, leaving the (shared) model as it is: what BoundaryIntegrals reads"""
    f = model.forcings
    kw = dict(nu=f.nu, kappa_h=f.kappa_h, kappa_v=f.kappa_v, tau_x=f.tau_x, tau_y=f.tau_y, b_surface_bc=f.b_surface_bc,
              conv_param=f.conv_param, eddy_param=f.eddy_param)
    kw.update(frc_kw)
    return SimpleNamespace(arch=model.arch, fe_data=model.fe_data, params=model.params, forcings=npg.Forcings(**kw), b_vec=model.b_vec,
                           inversion=model.inversion, step_index=getattr(model, "step_index", 1))


OFF = dict(conv_param=npg.ConvectionParameterization(0, 0, False), eddy_param=npg.EddyParameterization(0, 0, False))


def channel_random(arch, b_order=2):
    """the small channel basin (periodic seam, function-valued nu: full stress) with a random flow, the closures switched off"""
    model = sr.channel_model(arch, b_order)
    b = model.b_vec.to_host()
    ir.random_state(model)
    model.b_vec.upload(b)
    return model, view(model, **OFF)


def convection_view(model):
    """the model under a convection closure that is active on its boundary: alpha and N2 the model's, N2min the 30 % quantile of
    |alpha (N2 + d_z b')| over the face points of the restatement, kappa_c = 1 (as tests/mixing_ref.choose_closure)"""
    bi = npg.BoundaryIntegrals(model)
    ff = face_fields(model, bi.faces)
    a = np.abs(float(model.params.alpha) * (float(model.params.N2) + ff["gb"][..., 2])).ravel()
    N2min = float(np.quantile(a, 0.3))
    assert N2min > 0
    return view(model, conv_param=npg.ConvectionParameterization(1.0, N2min, True))


def single_tet(arch):
    """one tetrahedron whose four faces carry four different tags: a bare model (as integrals_ref.bare_model) with a random state"""
    coords = np.array([[0.0, 0.0, -1.0], [1.0, 0.1, -0.9], [0.2, 1.1, -0.8], [0.3, 0.2, 0.0]])
    facets = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])
    names = ["f0", "f1", "f2", "surface"]
    gm = gmsh_io.GmshModel(dim=3, coords=coords, node_phys=np.zeros(4, dtype=np.uint32), cells=np.array([[0, 1, 2, 3]]), facets=facets,
                           facets_phys=(1 << np.arange(4)).astype(np.uint32), ridges=np.zeros((0, 2), dtype=np.int64),
                           ridges_phys=np.zeros(0, dtype=np.uint32), phys_names=names)
    return bare_model(arch, npg.Mesh(gm))


def bare_model(arch, mesh=None, b_order=2):
    """what BoundaryIntegrals reads of a model, without toolkits: spaces WITHOUT Dirichlet tags (globally polynomial fields are
    representable), the forcings of bowl_surface_flux"""
    prm, frc, _, _, _, _ = helpers.product_config("bowl_surface_flux")
    mesh = mesh or npg.Mesh(os.path.join(helpers.GOLDEN, "mesh_bowl3D_h0.1.npz"))
    fed = npg.FEData(mesh, npg.Spaces(mesh, b_order=b_order))
    ctx = arch.ctx
    x = npg.DeviceVector(ctx, fed.dofs.nu + fed.dofs.np)
    return SimpleNamespace(arch=arch, fe_data=fed, params=prm, forcings=frc, b_vec=npg.DeviceVector(ctx, fed.dofs.nb),
                           inversion=SimpleNamespace(solver=SimpleNamespace(x=x)), step_index=1)


# ---- the checks (arch = npg.CPU() or npg.GPU()) --------------------------------------------------------------------------------------
def check_channels(model, label, mask=None, groups=None):
    """check 2: every channel, every group and the per-face table against the restatement"""
    bi = npg.BoundaryIntegrals(model, groups, mask)
    terms, mags, _ = restate(model, bi.faces)
    raw, per_face = bi.compute_raw(faces=True)
    assert raw.shape == (len(bi.groups), NBND) and per_face.shape == (NBND, len(bi.faces))
    skip = () if bi.viscous_available else (13, 14, 15, 16)
    if skip:
        assert np.isnan(raw[:, 13:17]).all() and np.isnan(per_face[13:17]).all()
    assert np.isfinite(np.delete(raw, skip, axis=1)).all()
    assert bi.nfaces_counted == (len(bi.faces) if mask is None else int(np.sum(mask)))
    compare(bi, raw, per_face, terms, mags, label, mask, skip)
    return bi, raw, terms


def check_geometry(model, label, periodic=False):
    """check 3: the closed boundary - sum_groups ch1..3 = 0 (on the channel basin the periodic pair carries no faces, so x vanishes as
    well) and sum ch4 = the volume (MeshIntegrals ch0; its own bound n_cells n_q eps V is added); and the fixture exercises the lookup"""
    bi = npg.BoundaryIntegrals(model)
    m = model.fe_data.mesh
    assert m.periodic == periodic
    assert np.unique(bi.face_cell, return_counts=True)[1].max() >= 2, "no cell with two boundary faces"
    assert set(np.unique(bi.face_local)) == {0, 1, 2, 3}
    raw, _ = bi.compute_raw()
    terms, mags, _ = restate(model, bi.faces)
    sabs = np.abs(terms).sum(axis=(1, 2))
    bound = len(bi.faces) * NQ * EPS * sabs
    tot = raw.sum(axis=0)
    V = npg.MeshIntegrals(model).compute_raw()[0]
    vb = bound[4] + m.ncell * len(m.q_w) * EPS * V
    print(f"geometry {label}: sum n = ({tot[1]:.2e}, {tot[2]:.2e}, {tot[3]:.2e}) bounds ({bound[1]:.2e}, {bound[2]:.2e}, {bound[3]:.2e}); "
          f"sum z n_z - V = {tot[4] - V:.2e} (bound {vb:.2e}, V = {V:.12f})")
    for k in (1, 2, 3):
        assert abs(tot[k]) <= bound[k], (k, tot[k], bound[k])
    assert abs(tot[4] - V) <= vb
    assert abs(np.linalg.norm(bi.normals, axis=1) - 1.0).max() <= 4 * EPS
    return tot, bound


def _volume_side(model):
    """(int div u, int (u . grad b' + b' div u)) with their S_abs, restated from integrals_ref's geometry and tables"""
    fed = model.fe_data
    m = fed.mesh
    un, _, bn = nodal_values(model)
    X, G, wdet, lam, w, ea, eb = ir.geometry(m)
    N, dN = F.p2_tables(lam, ea, eb)
    uc = un[m.cell_nodes]
    if fed.spaces.b_order == 2:
        bc, Nb, dNb = bn[m.cell_nodes], N, dN
    else:
        bc, Nb, dNb = bn[m.cells], lam, np.broadcast_to(np.eye(4), (len(w), 4, 4))
    u = np.einsum("qi,cia->cqa", N, uc)
    div = np.einsum("qik,cia,cka->cq", dN, uc, G)
    b = np.einsum("qi,ci->cq", Nb, bc)
    gb = np.einsum("qik,ci,ckj->cqj", dNb, bc, G)
    W = w[None, :] * wdet[:, None]
    t5, t7 = W * div, W * ((u * gb).sum(axis=-1) + b * div)
    return (math.fsum(t5.ravel()), np.abs(t5).sum()), (math.fsum(t7.ravel()), np.abs(t7).sum())


def check_divergence_theorem(model, label):
    """check 4: sum ch5 = int div u and sum ch7 = int (u . grad b' + b' div u) on the discrete fields (integrands of degree <= 4: exact).
    Bound: the boundary's n_faces n_q eps S_abs plus the volume restatement's n_cells n_q eps S_abs."""
    bi = npg.BoundaryIntegrals(model)
    m = model.fe_data.mesh
    raw, _ = bi.compute_raw()
    terms, mags, _ = restate(model, bi.faces)
    sabs = np.abs(terms).sum(axis=(1, 2))
    tot = raw.sum(axis=0)
    out = {}
    for k, (vol, vabs) in zip((5, 7), _volume_side(model)):
        bound = len(bi.faces) * NQ * EPS * sabs[k] + m.ncell * len(m.q_w) * EPS * vabs
        print(f"divergence theorem {label}: sum ch{k} = {tot[k]:.12e}, volume side {vol:.12e}, |difference| {abs(tot[k] - vol):.2e} (bound {bound:.2e})")
        assert abs(tot[k] - vol) <= bound
        out[k] = (abs(tot[k] - vol), bound)
    if model.fe_data.spaces.b_order == 2:                                                  # (MeshIntegrals' own ch9 on the device side)
        mi = npg.MeshIntegrals(model).compute_raw()
        print(f"divergence theorem {label}: MeshIntegrals ch9 = {mi[9]:.12e} (int u . grad b')")
    return out


def check_closed_forms(arch):
    """check 5: a bowl without Dirichlet tags and globally polynomial fields - p linear: sum ch9..11 = grad p V; b' quadratic, constant
    kappa: sum ch17 = (kappa_h (b_xx + b_yy) + kappa_v b_zz) V; u quadratic, constant nu: sum ch13..15 = nu lap u V.  The constants go
    in through npg_boundary_set_coeff.  V = math.fsum of the cells' volumes."""
    model = bare_model(arch)
    fed = model.fe_data
    m, t = fed.mesh, fed.tables
    assert (t.u_pos >= 0).all() and (t.b_pos >= 0).all()
    Xn = m.node_coords
    gp = np.array([0.7, -1.3, 2.1])
    pn = (m.coords - m.coords[-1]) @ gp                                                  # linear, 0 at the pinned vertex
    Hb = np.array([[1.0, -0.5, 0.25], [-0.5, -2.0, 1.0], [0.25, 1.0, 1.5]])            # b' = x' Hb x / 2 + c . x: Hessian Hb
    q = lambda x: 0.5 * np.einsum("...i,ij,...j->...", x, Hb, x) + x @ np.array([0.3, 0.2, -0.1]) + 1.0
    Hu = np.random.default_rng(SEED).standard_normal((3, 3, 3))
    Hu = Hu + np.swapaxes(Hu, 1, 2)                                                      # u_a = x' Hu[a] x / 2 + A x
    A = np.array([[0.3, -1.0, 0.5], [2.0, -0.7, 0.25], [-0.4, 1.5, 1.1]])
    un = 0.5 * np.einsum("ni,aij,nj->na", Xn, Hu, Xn) + Xn @ A.T
    x = np.zeros(fed.dofs.nu + fed.dofs.np)
    x[t.u_pos] = un
    x[t.p_pos[t.p_pos >= 0]] = pn[t.p_pos >= 0]
    b = np.zeros(fed.dofs.nb)
    b[t.b_pos] = q(Xn)
    model.inversion.solver.x.upload(x)
    model.b_vec.upload(b)
    nu, kh, kv = 0.8, 0.3, 1.7
    bi = npg.BoundaryIntegrals(model)
    assert not bi.full_stress
    for which, v in ((L.NPG_BND_NU, nu), (L.NPG_BND_KH, kh), (L.NPG_BND_KV, kv)):
        bi.set_coeff(which, v)
    raw, _ = bi.compute_raw()
    tot = raw.sum(axis=0)
    X = m.geo_coords[m.cell_geo]
    V = math.fsum(np.abs(np.linalg.det(X[:, 1:] - X[:, :1])) / 6.0)
    terms, mags, _ = restate(model, bi.faces, coef=dict(nu=nu, kh=kh, kv=kv))
    bound = len(bi.faces) * NQ * EPS * np.abs(terms).sum(axis=(1, 2))
    exact = {9: gp[0] * V, 10: gp[1] * V, 11: gp[2] * V, 17: (kh * (Hb[0, 0] + Hb[1, 1]) + kv * Hb[2, 2]) * V,
             13: nu * np.trace(Hu[0]) * V, 14: nu * np.trace(Hu[1]) * V, 15: nu * np.trace(Hu[2]) * V}
    print("closed forms: " + ", ".join(f"ch{k} {tot[k]:.9e} vs {v:.9e}: |err| {abs(tot[k] - v):.2e} (bound {bound[k]:.2e})" for k, v in exact.items()))
    for k, v in exact.items():
        assert abs(tot[k] - v) <= bound[k], (k, tot[k], v, bound[k])
    return {k: (abs(tot[k] - v), bound[k]) for k, v in exact.items()}


def check_load_identities(wind_model, flux_model):
    """check 6: the prescribed-load channels are the sums of the project's load vectors (same rule, same points).
    ch19 (surface) = x_u' (wind part of build_b_inversion) / alpha: bound n_faces n_q eps S_abs(ch19) for the channel plus, for the load
    vector's side, (terms per entry = faces around a node x 9) eps |u|' |load| / alpha; ch20 = 1' surface_load(F): the load vector sums
    n_faces 9 x 6 products w F N_i, bound n_faces n_q 6 eps sum |w F N_i|.  Both are exactly 0 away from the surface."""
    out = {}
    for model, k in ((wind_model, 19), (flux_model, 20)):
        fed, f, prm = model.fe_data, model.forcings, model.params
        m = fed.mesh
        bi = npg.BoundaryIntegrals(model)
        raw, _ = bi.compute_raw()
        terms, _, ff = restate(model, bi.faces)
        s = bi.groups.index("surface")
        sel = bi.face_group == s
        nf = int(sel.sum())
        sabs = np.abs(terms[k][sel]).sum()
        if k == 19:
            un, _, _ = nodal_values(model)
            ref, mag = 0.0, 0.0
            for comp, tau in ((0, f.tau_x), (1, f.tau_y)):
                if callable(tau) or float(tau) != 0.0:
                    fn = tau if callable(tau) else (lambda x, c=float(tau): np.full(x.shape[:-1], c))
                    load = m.surface_load(lambda x: prm.alpha * fn(x))
                    aload = m.surface_load(lambda x: np.abs(prm.alpha * fn(x)))
                    ref += math.fsum(un[:, comp] * load) / prm.alpha
                    mag += float(np.abs(un[:, comp]) @ np.abs(aload)) / prm.alpha
            assert mag > 0
            bound = nf * NQ * EPS * sabs + 16 * NQ * 3 * EPS * mag        # (|N_i| <= 1: |load| <= load of |tau|; at most 16 faces around a node)
            name = "x_u' wind / alpha"
        else:
            load = m.surface_load(f.b_surface_bc.flux)
            ref = math.fsum(load)
            absN = np.abs(F.p2_tables(F.tri_quadrature_degree4()[0], F._TRI_EDGE_A, F._TRI_EDGE_B)[0]).sum(axis=1)     # (9,) sum_i |N_i| on the face
            bound = nf * NQ * 6 * EPS * float((np.abs(terms[k][sel]) * absN[None, :]).sum())
            name = "1' surface_load(F)"
        err = abs(raw[s, k] - ref)
        print(f"load identity ch{k}: {raw[s, k]:.12e} vs {name} = {ref:.12e}: |err| {err:.2e} (bound {bound:.2e})")
        assert ref != 0.0 and err <= bound
        for g, nm in enumerate(bi.groups):
            if nm != "surface":
                assert raw[g, 19] == 0.0 and raw[g, 20] == 0.0, nm
        out[k] = (err, bound)
    return out


def check_energy_identity(model, label, strict=False):
    """check 7: the identity DESIGN.md 15 left open - |dissipation - buoyancy production - wind work| <= 2 |x' r|, r = rhs - A x by
    npg_spmv; dissipation and production from MeshIntegrals, the wind work from this feature.  The identity holds for ANY x (it is
    x' (A x - rhs) = -x' r written with integrals), so 2 |x' r| is generous wherever r is a solver's residual: strict=True (the GPU
    file: GMRES stops at 1e-6, |x' r| is 1e-9 or more) asserts exactly that.  CPU() solves these systems DIRECTLY
    (iterative_solve: fewer than 300 000 rows), r is rounding (|x' r| 1e-19) and so are the three integrals: there the summation
    rounding of the integrals by this file's convention, n_cells n_q eps (dissipation + |production|) + n_faces n_q eps |wind work|
    (1e-14 here, five orders below the quantities' own last digits times n), is added - measured on the channel basin
    |lhs| = 1.1e-18 against 2 |x' r| = 3.4e-19, on bowl_wind 5.2e-18 against 8.3e-18."""
    inv = model.inversion
    s = inv.solver
    r = npg.DeviceVector(model.arch.ctx, s.x.n)
    r.copy_from(inv.b)
    inv.B.mul(model.b_vec, r, alpha=1.0, beta=1.0)                                     # rhs = B b + b0 (lift + wind)
    s.A.mul(s.x, r, alpha=-1.0, beta=1.0)                                              # r = rhs - A x
    xr = s.x.dot(r)
    bud = npg.MeshIntegrals(model).compute()
    bi = npg.BoundaryIntegrals(model)
    wind = bi.compute().total("wind_work")
    m = model.fe_data.mesh
    floor = 0.0 if strict else m.ncell * len(m.q_w) * EPS * (bud.dissipation + abs(bud.buoyancy_production)) + len(bi.faces) * NQ * EPS * abs(wind)
    lhs = abs(bud.dissipation - bud.buoyancy_production - wind)
    print(f"energy identity {label}: dissipation {bud.dissipation:.9e}, production {bud.buoyancy_production:.9e}, wind work {wind:.9e}, "
          f"|dissipation - production - wind work| {lhs:.3e}, |x'r| {abs(xr):.3e} (bound 2 |x'r| = {2 * abs(xr):.3e}, rounding floor {floor:.3e})")
    assert bud.dissipation > 0 and wind != 0.0
    assert lhs <= 2 * abs(xr) + floor
    return lhs, abs(xr)


def check_edge_sizes(model, label, group="bottom"):
    """check 8: through the mask keep exactly 0, 1, 63, 64, 65 (around a wave), 255, 256, 257 (around a row of faces = a workgroup) and
    all faces of one group (and nothing else): each total against the restatement on those faces, and mask + complement = whole within
    the bound of the whole"""
    bi = npg.BoundaryIntegrals(model)
    terms, mags, _ = restate(model, bi.faces)
    g = bi.groups.index(group)
    idx = np.nonzero(bi.face_group == g)[0]
    whole, _ = bi.compute_raw()
    skip = () if bi.viscous_available else (13, 14, 15, 16)
    _, sabs, cnt = group_sums(terms, bi.face_group, len(bi.groups))
    wbound = summation_bound(cnt, sabs)
    rng = np.random.default_rng(SEED)
    for n in (0, 1, 63, 64, 65, 255, 256, 257, len(idx)):
        mask = np.zeros(len(bi.faces), dtype=bool)
        mask[rng.choice(idx, n, replace=False)] = True
        bm = npg.BoundaryIntegrals(model, mask=mask)
        assert bm.nfaces_counted == n
        raw, per_face = bm.compute_raw(faces=True)
        compare(bm, raw, per_face, terms, mags, f"{label}: {n} faces of {group}", mask, skip)
        if n == 0:
            assert np.array_equal(np.delete(raw, skip, axis=1), np.zeros((len(bi.groups), NBND - len(skip))))
        comp, _ = npg.BoundaryIntegrals(model, mask=~mask).compute_raw()
        err = np.abs(np.delete(raw + comp - whole, skip, axis=1))
        print(f"boundary {label}: {n} faces + complement - whole, worst |err| / bound {np.max(err / np.maximum(np.delete(wbound, skip, axis=1), 1e-300)):.2e}")
        assert (err <= np.delete(wbound, skip, axis=1)).all()


def check_single_tet(arch):
    """check 8: fewer faces than a wave - one tetrahedron, four groups of one face, every local index once"""
    model = single_tet(arch)
    ir.random_state(model)
    bi, raw, _ = check_channels(model, "single tetrahedron")
    assert len(bi.groups) == 4 and sorted(bi.face_local.tolist()) == [0, 1, 2, 3] and np.array_equal(bi.face_group, np.arange(4))
    tot = raw.sum(axis=0)
    X = model.fe_data.mesh.geo_coords
    V = abs(np.linalg.det(X[1:] - X[0])) / 6.0
    print(f"single tetrahedron: sum n = {tot[1:4]}, sum z n_z = {tot[4]:.15f}, V = {V:.15f}")
    assert np.abs(tot[1:4]).max() <= 4 * NQ * EPS * raw[:, 0].sum() and abs(tot[4] - V) <= 4 * NQ * EPS * np.abs(raw[:, 4]).sum() + 8 * EPS * V


def check_determinism(model):
    """check 9: two compute() calls on the same state - the same bits, totals and per-face table"""
    bi = npg.BoundaryIntegrals(model)
    a, fa = bi.compute_raw(faces=True)
    b, fb = bi.compute_raw(faces=True)
    c, _ = npg.BoundaryIntegrals(model).compute_raw()
    assert np.array_equal(a, b, equal_nan=True) and np.array_equal(fa, fb, equal_nan=True) and np.array_equal(a, c, equal_nan=True)


def check_refusals(model):
    """check 10: every NPG_EINVAL case through ctypes (nothing is launched), and the Python layer's errors"""
    import ctypes as C
    lib = L.lib()
    bi = npg.BoundaryIntegrals(model)
    k = bi._keep
    nf, ng = len(bi.faces), len(bi.groups)
    ctx = model.arch.ctx

    def create(fe=bi.fe.h, nface=nf, cell=k["cell"], local=k["local"], group=k["group"], ngroup=ng, xyz=k["xyz"], normal=k["normal"],
               area2=k["area2"], out=True):
        h = C.c_void_p()
        p = lambda a: None if a is None else L.ptr(a)
        rc = lib.npg_boundary_create(fe, nface, p(cell), p(local), p(group), ngroup, p(xyz), p(normal), p(area2), None, C.byref(h) if out else None)
        return rc, lib.npg_last_error().decode(), h

    def bad(a, i, v):
        a = a.copy()
        a.flat[i] = v
        return a
    for kw, word in ((dict(fe=None), "NULL"), (dict(out=False), "NULL"), (dict(cell=None), "NULL"), (dict(normal=None), "NULL"),
                     (dict(cell=bad(k["cell"], 3, model.fe_data.mesh.ncell)), "face_cell"), (dict(cell=bad(k["cell"], 0, -1)), "face_cell"),
                     (dict(local=bad(k["local"], 5, 4)), "face_local"), (dict(group=bad(k["group"], 7, ng)), "face_group"),
                     (dict(ngroup=0), "ngroup"), (dict(ngroup=9), "ngroup"), (dict(xyz=bad(k["xyz"], 11, np.nan)), "not finite"),
                     (dict(normal=bad(k["normal"], 2, np.inf)), "not finite"), (dict(area2=bad(k["area2"], 1, np.nan)), "not finite")):
        rc, msg, h = create(**kw)
        assert rc == NPG_EINVAL and word in msg and not h.value, (kw.keys(), rc, msg)
        with np.testing.assert_raises(L.DeviceError):
            L.check(rc)
    x, b = model.inversion.solver.x, model.b_vec
    out, fout = npg.DeviceVector(ctx, ng * NBND), npg.DeviceVector(ctx, nf * NBND)
    out.fill(-7.0), fout.fill(-7.0)
    short_x, short_b = npg.DeviceVector(ctx, x.n - 1), npg.DeviceVector(ctx, b.n + 1)
    short_out, short_f = npg.DeviceVector(ctx, ng * NBND - 1), npg.DeviceVector(ctx, nf * NBND - 1)
    for args, word in (((bi.h, short_x.h, b.h, 0, out.h, None), "flow vector"), ((bi.h, x.h, short_b.h, 0, out.h, None), "buoyancy vector"),
                       ((bi.h, x.h, b.h, 0, short_out.h, None), "NPG_NBND"), ((bi.h, x.h, b.h, 0, out.h, short_f.h), "faces_out"),
                       ((bi.h, x.h, b.h, 2, out.h, fout.h), "full_stress"), ((None, x.h, b.h, 0, out.h, None), "NULL"),
                       ((bi.h, None, b.h, 0, out.h, None), "NULL"), ((bi.h, x.h, b.h, 0, None, None), "NULL")):
        rc = lib.npg_boundary_compute(*args)
        msg = lib.npg_last_error().decode()
        assert rc == NPG_EINVAL and word in msg, (rc, msg)
    assert np.array_equal(out.to_host(), np.full(ng * NBND, -7.0)) and np.array_equal(fout.to_host(), np.full(nf * NBND, -7.0))   # nothing was launched
    tab = np.ones((NQ, nf))
    for args, word in (((bi.h, 6, L.ptr(tab)), "which"), ((bi.h, -1, L.ptr(tab)), "which"), ((None, 0, L.ptr(tab)), "NULL"),
                       ((bi.h, 0, L.ptr(bad(tab, 5, np.nan))), "not finite")):
        rc = lib.npg_boundary_set_coeff(*args)
        assert rc == NPG_EINVAL and word in lib.npg_last_error().decode()
    for args, word in (((bi.h, -1.0, 1.0, 1.0, 0.0), "kappa_c"), ((bi.h, 1.0, 0.0, 1.0, 0.0), "N2min"), ((bi.h, np.nan, 1.0, 1.0, 0.0), "kappa_c"),
                       ((None, 0.0, 0.0, 0.0, 0.0), "NULL")):
        rc = lib.npg_boundary_set_closure(*args)
        assert rc == NPG_EINVAL and word in lib.npg_last_error().decode()
    # nface = 0 and an empty group are legal: zeros
    rc, msg, h = create(nface=0, cell=None, local=None, group=None, xyz=None, normal=None, area2=None, ngroup=3)
    assert rc == 0, msg
    out3 = npg.DeviceVector(ctx, 3 * NBND)
    out3.fill(-7.0)
    L.check(lib.npg_boundary_compute(h, x.h, b.h, 0, out3.h, None))
    assert np.array_equal(out3.to_host(), np.zeros(3 * NBND))
    L.check(lib.npg_boundary_destroy(h))
    names = list(bi.groups)
    empty = npg.BoundaryIntegrals(model, groups={names[0]: [names[0]], "nothing": ["interior"]}) if "interior" in model.fe_data.mesh.phys_names else None
    if empty is not None:
        raw, _ = empty.compute_raw()
        assert np.array_equal(raw[1], np.zeros(NBND)) and raw[0, 0] > 0
    # the Python layer
    with np.testing.assert_raises(ValueError):
        npg.BoundaryIntegrals(model, groups={"a": names[:1], "b": names[:2]})               # a face in two groups
    with np.testing.assert_raises(ValueError):
        npg.BoundaryIntegrals(model, mask=np.ones(nf + 1, dtype=bool))
    part = SimpleNamespace(**{**vars(view(model)), "layout": SimpleNamespace(cell_owner=None, locator_cells=None)})
    with np.testing.assert_raises(NotImplementedError):
        npg.BoundaryIntegrals(part)
    repl = SimpleNamespace(**{**vars(view(model)), "partition": object()})
    with np.testing.assert_raises(NotImplementedError):
        npg.BoundaryIntegrals(repl)


def check_2d_refused(arch):
    """an embedded 2-D mesh: NotImplementedError in Python, NPG_EINVAL from the library"""
    import ctypes as C
    model = helpers.build_model("bowl_mixing", mesh="mesh_bowl2D_h0.1", nsteps=1, arch=arch)
    with np.testing.assert_raises(NotImplementedError):
        npg.BoundaryIntegrals(model)
    fe = device_fe(arch, model.fe_data)
    h = C.c_void_p()
    z1, z3, z9 = np.zeros(1), np.zeros(3), np.zeros(9)
    rc = L.lib().npg_boundary_create(fe.h, 1, L.ptr(np.zeros(1, dtype=np.int32)), L.ptr(np.zeros(1, dtype=np.uint8)), L.ptr(np.zeros(1, dtype=np.uint8)),
                                     1, L.ptr(z9), L.ptr(z3), L.ptr(z1), None, C.byref(h))
    assert rc == NPG_EINVAL and "2-D" in L.lib().npg_last_error().decode() and not h.value


def check_eddy_closure(model):
    """the eddy closure: channels 13..16 NaN, the flag False, everything else finite and against the restatement"""
    assert model.forcings.eddy_param.is_on
    bi, raw, _ = check_channels(model, "eddy closure on")
    r = bi.compute()
    assert not r.viscous_available and not bi.viscous_available
    for g in r.groups:
        assert np.isnan(r.viscous_force[g]).all() and np.isnan(r.viscous_work[g]) and np.isfinite(r.pressure_force[g]).all()


def check_fluxes_and_maps(model):
    """the Python layer's arithmetic: BoundaryFluxes from the raw channels, BoundaryMaps from the per-face table"""
    bi = npg.BoundaryIntegrals(model)
    r = bi.compute(faces=True)
    prm = model.params
    a2e2 = prm.alpha ** 2 * prm.eps ** 2
    for g in r.groups:
        raw = r.raw[g]
        assert r.area[g] == raw[0] and r.volume_flux[g] == raw[5] and r.buoyancy_flux_advective[g] == raw[7]
        assert np.array_equal(r.pressure_force[g], raw[9:12]) and np.array_equal(r.viscous_force[g], a2e2 * raw[13:16])
        assert r.wind_work[g] == prm.alpha * raw[19] and r.diffusive_flux[g] == raw[17] + prm.N2 * raw[18] and r.prescribed_flux[g] == raw[20]
        assert r.mean_p[g] == raw[8] / raw[0] and r.mean_b[g] == raw[6] / raw[0] and r.mean_dz_b[g] == raw[21] / raw[0]
        assert r.mean_ux[g] == raw[22] / raw[0] and r.mean_uy[g] == raw[23] / raw[0]
    assert r.total("area") == sum(r.area.values()) and np.array_equal(r.total("pressure_force"), sum(r.pressure_force.values()))
    mp = r.maps
    nf = len(bi.faces)
    assert mp.values.shape == (NBND, nf) and mp.centroids.shape == (nf, 3) and mp.normals.shape == (nf, 3) and mp.group.shape == (nf,)
    assert np.array_equal(mp.values[0], np.ones(nf)) and np.allclose(mp.raw[0], bi.area, rtol=1e-13, atol=0)
    s, bt = mp.of("surface"), mp.of("bottom")
    for (c, v), sel, ref in ((mp.surface_pressure(), s, mp.values[8, s]), (mp.surface_velocity(), s, mp.values[22:24, s].T),
                             (mp.bottom_pressure(), bt, mp.values[8, bt]), (mp.bottom_stress(), bt, a2e2 * mp.values[13:16, bt].T)):
        assert np.array_equal(c, mp.centroids[sel]) and np.array_equal(v, ref) and len(c) == sel.sum() > 0
    assert np.abs(mp.surface_pressure()[0][:, 2]).max() == 0.0                             # the rigid lid


def check_recorder(arch, tmp_path):
    """check 11: BoundaryRecorder as on_plot over 3 steps of run(); u, p, b' after the run are bit-identical to a run without the hook"""
    a = sr.bowl_model(arch, "bowl_wind")
    a.timestepper.t_stop = 10 * a.timestepper.dt
    rec = npg.BoundaryRecorder(a)
    a.on_plot = rec
    npg.run(a, n_plot=1, n_steps=3)
    t, raw = rec.as_arrays()
    ng = len(rec.boundary.groups)
    assert t.shape == (3,) and raw.shape == (3, ng, NBND) and np.isfinite(raw).all()
    assert np.array_equal(raw[-1], npg.BoundaryIntegrals(a).compute_raw()[0])             # the state the hook saw last is the current one
    path = os.path.join(str(tmp_path), "boundary.npz")
    rec.save(path)
    z = np.load(path)
    assert np.array_equal(z["t"], t) and np.array_equal(z["raw"], raw) and len(z["channels"]) == NBND and list(z["groups"]) == list(rec.boundary.groups)
    fl = rec.fluxes()
    assert len(fl) == 3 and fl[0].raw["surface"][0] == raw[0, list(rec.boundary.groups).index("surface"), 0]
    b = sr.bowl_model(arch, "bowl_wind")
    b.timestepper.t_stop = 10 * b.timestepper.dt
    npg.run(b, n_plot=1, n_steps=3)                                                        # no hook
    for f in ("u", "p", "b"):
        assert np.array_equal(getattr(a.state, f), getattr(b.state, f)), f


# ---- the device against the host library (GPU file only) -----------------------------------------------------------------------------
def host_library_raw(model, bi):
    """the channels of the model's current state through libnupgcm_host.so, loaded BESIDE the library the model runs on and driven
    through its C ABI alone, with the face tables and the coefficient tables of `bi`"""
    import ctypes as C
    H = C.CDLL(L.HOST_LIB_PATH)
    L._declare(H, partial=True)

    def ok(rc):
        assert rc == 0, H.npg_last_error().decode()
    fed, f = model.fe_data, model.forcings
    m = fed.mesh
    k = device_fe(model.arch, fed)._keep
    d = L.FeDesc(ncell=m.ncell, nq=len(m.q_w), nloc_b=k["cb"].shape[1], grad_lambda=k["G"].ctypes.data, wdet=k["wdet"].ctypes.data,
                 qw=k["qw"].ctypes.data, N2=k["N2"].ctypes.data, dN2=k["dN2"].ctypes.data, Nb=k["Nb"].ctypes.data, dNb=k["dNb"].ctypes.data,
                 N1=k["N1"].ctypes.data, cell_u=k["cu"].ctypes.data, cell_p=k["cp"].ctypes.data, cell_b=k["cb"].ctypes.data,
                 u_diri=k["ud"].ctypes.data, n_u_diri=k["ud"].size, b_diri=k["bd"].ctypes.data, n_b_diri=k["bd"].size,
                 n_inv=fed.dofs.nu + fed.dofs.np, n_b=fed.dofs.nb)
    ctx, fe, B = C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(H.npg_ctx_create(0, C.byref(ctx)))
    ok(H.npg_fe_create(ctx, C.byref(d), C.byref(fe)))
    q = bi._keep
    nf, ng = len(bi.faces), len(bi.groups)
    ok(H.npg_boundary_create(fe, nf, L.ptr(q["cell"]), L.ptr(q["local"]), L.ptr(q["group"]), ng, L.ptr(q["xyz"]), L.ptr(q["normal"]),
                             L.ptr(q["area2"]), None if q["mask"] is None else L.ptr(q["mask"]), C.byref(B)))
    on = face_fields(model, bi.faces)["surface"][:, None]
    xq = bi.points
    tabs = [(L.NPG_BND_NU, None if f.eddy_param.is_on else _coef(f.nu, xq)), (L.NPG_BND_KH, _coef(f.kappa_h, xq)), (L.NPG_BND_KV, _coef(f.kappa_v, xq)),
            (L.NPG_BND_TAUX, np.where(on, _coef(f.tau_x, xq), 0.0)), (L.NPG_BND_TAUY, np.where(on, _coef(f.tau_y, xq), 0.0))]
    if isinstance(f.b_surface_bc, npg.SurfaceFluxBC):
        tabs.append((L.NPG_BND_FLUX, np.where(on, _coef(f.b_surface_bc.flux, xq), 0.0)))
    for which, tab in tabs:
        if tab is not None:
            ok(H.npg_boundary_set_coeff(B, which, L.ptr(L.as_f64(tab.T))))
    if f.conv_param.is_on:
        ok(H.npg_boundary_set_closure(B, float(f.conv_param.kappa_c), float(f.conv_param.N2min), float(model.params.alpha), float(model.params.N2)))
    vecs = []
    for a in (model.inversion.solver.x.to_host(), model.b_vec.to_host(), np.zeros(ng * NBND), np.zeros(max(1, nf * NBND))):
        v = C.c_void_p()
        ok(H.npg_vec_create(ctx, len(a), C.byref(v)))
        ok(H.npg_vec_upload(v, L.ptr(L.as_f64(a))))
        vecs.append(v)
    ok(H.npg_boundary_compute(B, vecs[0], vecs[1], int(bi.full_stress), vecs[2], vecs[3]))
    out, fout = np.empty(ng * NBND), np.empty(max(1, nf * NBND))
    ok(H.npg_vec_download(vecs[2], L.ptr(out)))
    ok(H.npg_vec_download(vecs[3], L.ptr(fout)))
    H.npg_boundary_destroy(B)
    for v in vecs:
        H.npg_vec_destroy(v)
    H.npg_fe_destroy(fe)
    H.npg_ctx_destroy(ctx)
    return out.reshape(ng, NBND), fout[:nf * NBND].reshape(NBND, nf)


def check_device_against_host(model, label, mask=None):
    """the device kernel against the host library on the same state: the same per-face arithmetic (the per-face table differs by
    rounding of the compilers' code at most: the face's own bound), two summation orders for the totals (the same bound as against
    the restatement)"""
    bi = npg.BoundaryIntegrals(model, mask=mask)
    terms, mags, _ = restate(model, bi.faces)
    raw, per_face = bi.compute_raw(faces=True)
    host, hface = host_library_raw(model, bi)
    skip = [] if bi.viscous_available else [13, 14, 15, 16]
    _, sabs, cnt = group_sums(terms, bi.face_group, len(bi.groups), mask)
    bound = np.delete(summation_bound(cnt, sabs), skip, axis=1)
    err = np.abs(np.delete(raw - host, skip, axis=1))
    fbound = np.delete(face_bound(mags), skip, axis=0)
    ferr = np.abs(np.delete(per_face - hface, skip, axis=0))
    print(f"device vs host library {label}: totals worst |err| / bound {np.max(err / np.maximum(bound, 1e-300)):.2e}, per face worst "
          f"{np.max(ferr / np.maximum(fbound, 1e-300)):.2e}, faces with identical bits {np.mean((ferr == 0).all(axis=0)):.3f}")
    assert (err <= bound).all() and (ferr <= fbound).all()
