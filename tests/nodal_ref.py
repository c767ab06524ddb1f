"""A numpy restatement of the nodal gradient recovery (nupgcm_amd.nodal) and the checks shared by tests/test_nodal.py
(CPU()) and tests/test_gpu_nodal.py (GPU()).

The restatement is written from the definition, not from the code under test: nodal values through Spaces' native tables, the P2 basis
from fe.p2_tables at the four vertices, each cell's own mesh.grad_lambda, the 0.5 (a + b) rule for the mid-nodes, and per node the sum
over its cells in ascending cell order (one numpy pass per rank of an incidence within its node).

Bounds.  One cell's gradient component is an inner product of at most 10 x 4 products dN_i/dlambda_k v_i G_k,a: the rounding of
evaluating it - on both sides of the comparison - is at most 64 eps A_c with A_c the sum of the products' absolute values (fewer than
64 operations on the longest path, Higham eq. 3.5); adding `valence` weighted terms costs valence eps sum_c w_c A_c more.  So every entry
is held to (valence + 64) eps (sum_c w_c A_c) / W, channel 15 (W, a plain sum of positive weights) to valence eps W, the valence is exact.
No other tolerance is used against the restatement."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np

import nupgcm_amd as npg
from nupgcm_amd import _lib as L
from nupgcm_amd import fe as F
from nupgcm_amd import io as nio
from nupgcm_amd.inversion import device_fe
from tests import averages_ref as ar
from tests import boundary_ref as br
from tests import helpers
from tests import integrals_ref as ir
from tests import sampling_ref as sr

EPS = np.finfo(np.float64).eps
NCH = 17
NPG_EINVAL = -1
SEED = 20261020
NEW = {"npg_nodal_create", "npg_nodal_compute", "npg_nodal_info", "npg_nodal_destroy"}
EA, EB = F._TET_EDGE_A, F._TET_EDGE_B


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def incidences(mesh):
    """(node, cell, local, rank) of all 10 ncell incidences sorted by (node, cell); rank = the incidence's place within its node"""
    nc = mesh.ncell
    node = mesh.cell_nodes.ravel()
    cell, local = np.repeat(np.arange(nc), 10), np.tile(np.arange(10), nc)
    order = np.lexsort((cell, node))
    node, cell, local = node[order], cell[order], local[order]
    first = np.searchsorted(node, node, side="left")
    return node, cell, local, np.arange(len(node)) - first


def cell_node_gradients(model):
    """(g, A) each (ncell, 10, 15): per cell and local node the channels 0..14 (d_j u_a at 3 a + j, grad b', grad p) and the sums of the
    absolute values of the products they are made of"""
    fed = model.fe_data
    m = fed.mesh
    un, pn, bn = br.nodal_values(model)
    _, dN = F.p2_tables(np.eye(4), EA, EB)                               # (vertex, basis, barycentric)
    G = m.grad_lambda
    uc, pc = un[m.cell_nodes], pn[m.cells]

    def both(expr, *ops):
        return np.einsum(expr, *ops), np.einsum(expr, *[np.abs(o) for o in ops])
    gu, au = both("kim,cia,cmj->ckaj", dN, uc, G)
    gp, ap = both("cm,cmj->cj", pc, G)
    if fed.spaces.b_order == 2:
        gb, ab = both("kim,ci,cmj->ckj", dN, bn[m.cell_nodes], G)
    else:
        gb, ab = both("cm,cmj->cj", bn[m.cells], G)
        gb, ab = np.repeat(gb[:, None], 4, axis=1), np.repeat(ab[:, None], 4, axis=1)
    nc = m.ncell
    out = []
    for u_, b_, p_ in ((gu, gb, gp), (au, ab, ap)):
        v = np.concatenate([u_.reshape(nc, 4, 9), b_, np.repeat(p_[:, None], 4, axis=1)], axis=2)       # (nc, 4 vertices, 15)
        out.append(np.concatenate([v, 0.5 * (v[:, EA] + v[:, EB])], axis=1))
    return out[0], out[1]


def restate(model, weight="volume"):
    """(val (17, nn), bound (17, nn), valence (nn,)) on all nodes"""
    m = model.fe_data.mesh
    g, A = cell_node_gradients(model)
    node, cell, local, rank = incidences(m)
    w = m.detJ[cell] if weight == "volume" else np.ones(len(cell))
    S, SA, W = np.zeros((m.nn, 15)), np.zeros((m.nn, 15)), np.zeros(m.nn)
    for r in range(int(rank.max()) + 1):                                 # ascending cell order: the r-th cell of every node at once
        k = rank == r
        S[node[k]] += w[k, None] * g[cell[k], local[k]]
        SA[node[k]] += w[k, None] * A[cell[k], local[k]]
        W[node[k]] += w[k]
    val_n = np.bincount(node, minlength=m.nn).astype(np.float64)
    val = np.vstack([(S / W[:, None]).T, W[None], val_n[None]])
    bound = np.vstack([((val_n + 64)[:, None] * EPS * SA / W[:, None]).T, (val_n * EPS * W)[None], np.zeros((1, m.nn))])
    return val, bound, val_n


def compare(raw, val, bound, label, nodes=None, channels=range(NCH)):
    """every selected entry of the channels within its bound, NaN everywhere else; prints the worst |err| / bound first"""
    sel = np.ones(raw.shape[1], dtype=bool) if nodes is None else nodes
    ch = np.zeros(NCH, dtype=bool)
    ch[list(channels)] = True
    err = np.abs(raw - val)[np.ix_(ch, sel)]
    bd = bound[np.ix_(ch, sel)]
    ratio = np.where(bd > 0, err / np.where(bd > 0, bd, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = ratio.max(initial=0.0)
    print(f"nodal {label}: {int(sel.sum())} nodes, worst |err| / bound {worst:.3f}"
          + ("" if not sel.any() else f" (channel {np.nonzero(ch)[0][np.unravel_index(ratio.argmax(), ratio.shape)[0]]})"))
    assert np.isfinite(raw[np.ix_(ch, sel)]).all() and (err <= bd).all(), (label, worst)
    assert np.isnan(raw[:, ~sel]).all(), label
    return worst


# ---- models -----------------------------------------------------------------------------------------------------------------------
def with_config(model, name="bowl_surface_flux"):
    """a light model (averages_ref.light) with the parameters and forcings of a named configuration"""
    model.params, model.forcings = helpers.product_config(name)[:2]
    return model


def bowl(arch, name="bowl_surface_flux", b_order=2, seed=SEED):
    model = with_config(ar.bowl_light(arch, name, b_order), name)
    ir.random_state(model, seed=seed)
    return model


def single_tet(arch, b_order=2):
    mesh = br.single_tet(arch).fe_data.mesh
    model = br.bare_model(arch, mesh, b_order)
    ir.random_state(model, seed=SEED + b_order)
    return model


def channel(arch, b_order):
    model = sr.channel_model(arch, b_order)
    ir.random_state(model, seed=SEED + 7)
    return model


# ---- the checks (arch = npg.CPU() or npg.GPU()) --------------------------------------------------------------------------------------
def check_exports():
    assert {"NodalFields", "NodalGradients"} <= set(npg.__all__)
    assert NEW <= set(L.declared_symbols()) and L.NPG_NODAL_NCH == NCH
    for path in (L.HOST_LIB_PATH, L.LIB_PATH):
        lib = C.CDLL(path)
        assert not [s for s in NEW if not hasattr(lib, s)], path


def check_restatement(model, label, nodes=None, weights=("volume", "count"), against_host=False):
    """checks 2 and 3: every channel against the restatement for both weights; on request the bits of the host library"""
    out = {}
    for weight in weights:
        val, bound, _ = restate(model, weight)
        nf = npg.NodalFields(model, weight=weight, nodes=nodes)
        raw = nf.compute_raw()
        assert raw.shape == (NCH, model.fe_data.mesh.nn)
        compare(raw, val, bound, f"{label}, weight={weight}", nodes)
        sel = slice(None) if nodes is None else nodes
        assert np.array_equal(raw[16, sel], val[16, sel]) and np.array_equal(nf.valence, val[16, nf.sel])
        assert np.array_equal(np.sort(nf.sel), np.arange(len(val[16]))[sel])
        if against_host:
            host = host_library_raw(model, nf)
            same = np.array_equal(raw, host, equal_nan=True)
            print(f"nodal {label}, weight={weight}: device = host library, every bit: {same}")
            assert same
        out[weight] = raw
    return out


def check_single_tet(arch, against_host=False):
    for b_order in (2, 1):
        model = single_tet(arch, b_order)
        m = model.fe_data.mesh
        assert m.nn == 10 and m.ncell == 1
        raw = check_restatement(model, f"single tetrahedron P{b_order}", against_host=against_host)
        g, A = cell_node_gradients(model)
        assert (raw["count"][16] == 1.0).all() and (raw["count"][15] == 1.0).all() and np.array_equal(raw["volume"][15], np.full(10, m.detJ[0]))
        err = np.abs(raw["count"][:15].T - g[0])                           # valence 1, weight 1.0: the cell's own gradient
        assert (err <= 64 * EPS * A[0]).all()


def check_bowl_shapes(model, against_host=False):
    """the bowl's node count is ragged against the workgroup and its valences spread from a corner's 1 or 2 to an interior vertex's"""
    m = model.fe_data.mesh
    _, _, val_n = restate(model, "count")
    print(f"nodal bowl: nn = {m.nn}, ncell = {m.ncell}, valence min {int(val_n.min())} median {int(np.median(val_n))} max {int(val_n.max())}")
    assert m.nn % 256 != 0 and val_n.min() in (1, 2) and val_n.max() >= 16
    check_restatement(model, "bowl", against_host=against_host)


def check_masks(model, against_host=False):
    m = model.fe_data.mesh
    val, bound, _ = restate(model, "volume")
    for n, mk in ar.masks(m.nn, SEED).items():
        assert mk.sum() == n
        nf = npg.NodalFields(model, nodes=mk)
        raw = nf.compute_raw()
        compare(raw, val, bound, f"mask of {n} nodes", mk)
        assert len(nf.sel) == n
        if against_host:
            assert np.array_equal(raw, host_library_raw(model, nf), equal_nan=True), n
    full = npg.NodalFields(model).compute_raw()
    mk = ar.masks(m.nn, SEED)[257]
    assert np.array_equal(npg.NodalFields(model, nodes=mk).compute_raw()[:, mk], full[:, mk])      # a node's bits do not depend on the mask


def check_dirichlet_and_pin(arch, against_host=False):
    """bowl_wind: Dirichlet DoFs of u and of b enter with their table values; the pinned pressure vertex (p = 0) is selected"""
    model = bowl(arch, "bowl_wind")
    t = model.fe_data.tables
    assert (t.u_pos < 0).any() and (t.b_pos < 0).any() and (t.p_pos < 0).sum() == 1
    check_restatement(model, "bowl_wind (Dirichlet u and b)", against_host=against_host)
    m = model.fe_data.mesh
    pin = int(np.nonzero(t.p_pos < 0)[0][0])
    mk = np.zeros(m.nn, dtype=bool)
    mk[pin] = True
    mk[m.cell_nodes[np.nonzero((m.cells == pin).any(axis=1))[0]].ravel()] = True               # and the nodes of its cells
    raw = check_restatement(model, "the pinned pressure vertex and its cells", nodes=mk, against_host=against_host)
    assert np.abs(raw["volume"][12:15, pin]).max() > 0


def check_channel(arch, b_order, against_host=False):
    """the periodic channel basin: a node on the seam has cells from both sides, each with its own geometry"""
    model = channel(arch, b_order)
    m = model.fe_data.mesh
    assert m.periodic
    X = m.geo_coords[m.cell_geo][..., 0]                                                       # x of each cell's own vertices
    lo, hi = np.full(m.nv, np.inf), np.full(m.nv, -np.inf)
    np.minimum.at(lo, m.cells.ravel(), X.ravel())
    np.maximum.at(hi, m.cells.ravel(), X.ravel())
    seam = np.nonzero(hi - lo > 0.5 * (X.max() - X.min()))[0]
    print(f"nodal channel basin P{b_order}: {len(seam)} seam vertices of {m.nv}")
    assert len(seam) > 0                                                                       # one vertex, cells at both ends of the period
    raw = check_restatement(model, f"channel basin P{b_order}", against_host=against_host)
    assert np.isfinite(raw["volume"][:, seam]).all()


def _polynomial_state(model):
    """u quadratic, b' quadratic (P2) or linear (P1), p linear, as boundary_ref.check_closed_forms builds them"""
    fed = model.fe_data
    m, t = fed.mesh, fed.tables
    assert (t.u_pos >= 0).all() and (t.b_pos >= 0).all()
    Xn = m.node_coords
    gp = np.array([0.7, -1.3, 2.1])
    pn = (m.coords - m.coords[-1]) @ gp
    p2 = fed.spaces.b_order == 2
    Hb = np.array([[1.0, -0.5, 0.25], [-0.5, -2.0, 1.0], [0.25, 1.0, 1.5]]) * (1.0 if p2 else 0.0)
    cb = np.array([0.3, 0.2, -0.1])
    Hu = np.random.default_rng(SEED).standard_normal((3, 3, 3))
    Hu = Hu + np.swapaxes(Hu, 1, 2)
    A = np.array([[0.3, -1.0, 0.5], [2.0, -0.7, 0.25], [-0.4, 1.5, 1.1]])
    un = 0.5 * np.einsum("ni,aij,nj->na", Xn, Hu, Xn) + Xn @ A.T
    Xb = Xn if p2 else m.coords
    x = np.zeros(fed.dofs.nu + fed.dofs.np)
    x[t.u_pos] = un
    x[t.p_pos[t.p_pos >= 0]] = pn[t.p_pos >= 0]
    b = np.zeros(fed.dofs.nb)
    b[t.b_pos] = 0.5 * np.einsum("...i,ij,...j->...", Xb, Hb, Xb) + Xb @ cb + 1.0
    model.inversion.solver.x.upload(x)
    model.b_vec.upload(b)
    exact = np.full((NCH, m.nn), np.nan)
    exact[0:9] = (np.einsum("aij,nj->nai", Hu, Xn) + A[None]).reshape(m.nn, 9).T
    exact[9:12] = (Xn @ Hb + cb).T
    exact[12:15] = gp[:, None]
    return exact


def check_closed_forms(arch):
    """check 5: polynomial fields in the spaces - every node, boundary nodes included, carries the analytic gradient within the bound of
    check 2, for both weights (a convex combination of exact values is exact); the derived fields follow"""
    for b_order in (2, 1):
        model = br.bare_model(arch, b_order=b_order)
        exact = _polynomial_state(model)
        for weight in ("volume", "count"):
            _, bound, _ = restate(model, weight)
            nf = npg.NodalFields(model, weight=weight)
            g = nf.compute()
            compare(g.raw, exact, bound, f"closed forms P{b_order}, weight={weight}", channels=range(15))
            # derived: sums and differences of bounded entries, one more rounding each (2 eps |result| covers it)
            ge = np.moveaxis(exact[0:9].reshape(3, 3, -1), -1, 0)
            B = np.moveaxis(bound[0:9].reshape(3, 3, -1), -1, 0)
            vort = np.stack([ge[:, 2, 1] - ge[:, 1, 2], ge[:, 0, 2] - ge[:, 2, 0], ge[:, 1, 0] - ge[:, 0, 1]], axis=1)
            vb = np.stack([B[:, 2, 1] + B[:, 1, 2], B[:, 0, 2] + B[:, 2, 0], B[:, 1, 0] + B[:, 0, 1]], axis=1)
            assert (np.abs(g.vorticity() - vort) <= vb + 2 * EPS * np.abs(vort)).all()
            div = ge[:, 0, 0] + ge[:, 1, 1] + ge[:, 2, 2]
            db = B[:, 0, 0] + B[:, 1, 1] + B[:, 2, 2]
            assert (np.abs(g.divergence() - div) <= db + 4 * EPS * (np.abs(ge[:, 0, 0]) + np.abs(ge[:, 1, 1]) + np.abs(ge[:, 2, 2]))).all()
            N2 = float(model.params.N2)
            f = lambda X: 1.0 + 0.5 * X[:, 1]                                                   # noqa: E731
            fx = f(model.fe_data.mesh.node_coords)
            pv = fx * (N2 + exact[11])
            assert (np.abs(g.N2() - (N2 + exact[11])) <= bound[11] + 2 * EPS * (abs(N2) + np.abs(exact[11]))).all()
            assert (np.abs(g.pv(f) - pv) <= np.abs(fx) * bound[11] + 4 * EPS * np.abs(fx) * (abs(N2) + np.abs(exact[11]))).all()
            assert np.array_equal(g.pv(2.0), 2.0 * g.N2()) and np.array_equal(g.pv(fx), g.pv(f))
            assert np.array_equal(g.alpha_bz(), float(model.params.alpha) * g.N2())
            prm_f = getattr(model.params, "f", None)
            if prm_f is not None:
                assert np.array_equal(g.pv(), g.pv(prm_f))


def closure_model(arch, b_order):
    """a bowl with a random state, the convection and the eddy closure on"""
    f = lambda X: 1 + 0.5 * X[:, 1]                                                             # noqa: E731
    model = bowl(arch, "bowl_surface_flux", b_order)
    frc = SimpleNamespace(eddy_param=npg.EddyParameterization(f=f, N2min=1e-2, is_on=True),
                          conv_param=npg.ConvectionParameterization(kappa_c=1.0, N2min=1e-3, is_on=True), nu=1.0,
                          kappa_v=lambda X: 1e-2 + np.exp(-(X[:, 2] + 0.5) / 0.05))
    model.forcings = frc
    return model


def full_buoyancy(model):
    """N2 z + b' at the P2 nodes as io._nodal_fields forms it (a P1 buoyancy: mid-nodes take half the sum of their edge)"""
    m = model.fe_data.mesh
    _, _, bn = br.nodal_values(model)
    if len(bn) == m.nv:
        bn = np.concatenate([bn, 0.5 * (bn[m.edges[:, 0]] + bn[m.edges[:, 1]])])
    return float(model.params.N2) * m.node_coords[:, 2] + bn


def check_closures_against_io(arch):
    """check 6: weight="count" is the average io._nodal_closure_fields takes.  The tolerance is that function's own rounding: it
    differentiates the FULL buoyancy N2 z + b' cell by cell (40 products dN b G_z per incidence) and averages - valence eps mean|terms|
    per node with |terms| an incidence's summed absolute products, times alpha.  nu and kappa_v are functions of alpha*b_z: a difference
    da moves them by at most their Lipschitz constants f^2 2 / (3 sqrt 3 N2min^2) (eddy: v = f^2 / sqrt(N2min^2 + a^2), d nu / d v <= 1)
    and kappa_c / (2 N2min) (convection: tanh' <= 1), plus 8 eps of their own evaluation."""
    for b_order in (2, 1):
        model = closure_model(arch, b_order)
        m, prm, frc = model.fe_data.mesh, model.params, model.forcings
        b_full = full_buoyancy(model)
        abz0, nu0, kv0 = nio._nodal_closure_fields(model, b_full)
        _, dN = F.p2_tables(np.vstack([np.eye(4), 0.5 * (np.eye(4)[EA] + np.eye(4)[EB])]), EA, EB)
        terms = np.einsum("qak,ca,ck->cq", np.abs(dN), np.abs(b_full[m.cell_nodes]), np.abs(m.grad_lambda[:, :, 2]))
        tot = np.zeros(m.nn)
        np.add.at(tot, m.cell_nodes.ravel(), terms.ravel())
        tol = abs(prm.alpha) * EPS * tot                                                        # valence x eps x mean = eps x sum
        abz, nu, kv = npg.NodalFields(model, weight="count").compute(("b",)).closures()
        err = np.abs(abz - abz0)
        print(f"nodal closures P{b_order}: alpha*b_z worst |err| / (valence eps mean|terms|) {np.max(err / tol):.3f}")
        assert (err <= tol).all()
        fx = frc.eddy_param.f(m.node_coords)
        lip_nu = fx * fx * 2.0 / (3.0 * np.sqrt(3.0) * frc.eddy_param.N2min ** 2)
        lip_kv = frc.conv_param.kappa_c / (2.0 * frc.conv_param.N2min)
        assert (np.abs(nu - nu0) <= lip_nu * tol + 8 * EPS * np.abs(nu0)).all()
        assert (np.abs(kv - kv0) <= lip_kv * tol + 8 * EPS * np.abs(kv0)).all()
        assert (nu0 != 1.0).any() and (kv0 != frc.kappa_v(m.node_coords)).any()               # both closures act


def _arr(a, fmt):
    return "\n".join(" ".join(fmt % v for v in row) for row in np.atleast_2d(a))


def parent_vtk_text(model):
    """the file save_vtk wrote before it took `nodal`, assembled from io._nodal_fields / io._nodal_closure_fields"""
    m = model.fe_data.mesh
    u, p, b = nio._nodal_fields(model)
    abz, nu, kv = nio._nodal_closure_fields(model, b)
    t = 0.0 if model.timestepper is None else float(model.timestepper.t)
    conn = m.cell_nodes[:, nio._VTK_P2]
    nc = len(conn)
    s = '<?xml version="1.0"?>\n<VTKFile type="UnstructuredGrid" version="0.1" byte_order="LittleEndian">\n'
    s += "<UnstructuredGrid>\n<FieldData>\n"
    s += f'<DataArray type="Float64" Name="t" NumberOfTuples="1" format="ascii">{t!r}</DataArray>\n</FieldData>\n'
    s += f'<Piece NumberOfPoints="{m.nn}" NumberOfCells="{nc}">\n<Points>\n'
    s += '<DataArray type="Float64" NumberOfComponents="3" format="ascii">\n' + _arr(m.node_coords, "%.17g") + "\n</DataArray>\n</Points>\n<Cells>\n"
    s += '<DataArray type="Int64" Name="connectivity" format="ascii">\n' + _arr(conn, "%d") + "\n</DataArray>\n"
    s += '<DataArray type="Int64" Name="offsets" format="ascii">\n' + _arr((10 * np.arange(1, nc + 1)).reshape(-1, 1), "%d") + "\n</DataArray>\n"
    s += '<DataArray type="UInt8" Name="types" format="ascii">\n' + _arr(np.full((nc, 1), 24), "%d") + "\n</DataArray>\n</Cells>\n<PointData>\n"
    s += '<DataArray type="Float64" Name="u" NumberOfComponents="3" format="ascii">\n' + _arr(u, "%.17g") + "\n</DataArray>\n"
    for name, a in (("p", p), ("b", b), ("alpha*b_z", abz), ("nu", nu), ("kappa_v", kv)):
        s += f'<DataArray type="Float64" Name="{name}" format="ascii">\n' + _arr(a.reshape(-1, 1), "%.17g") + "\n</DataArray>\n"
    return s + "</PointData>\n</Piece>\n</UnstructuredGrid>\n</VTKFile>\n"


def read_point_array(text, name):
    mt = re.search(r'<DataArray type="Float64" Name="%s"[^>]*>\n(.*?)\n</DataArray>' % re.escape(name), text, flags=re.S)
    assert mt, name
    return np.array([[float(v) for v in row.split()] for row in mt.group(1).split("\n")])


def check_vtk(model, tmp_path):
    """check 6: without `nodal` the file is the parent's, byte for byte; with it the five arrays follow and parse back to the values"""
    old = os.path.join(str(tmp_path), "old.vtu")
    new = os.path.join(str(tmp_path), "new.vtu")
    npg.save_vtk(model, old)
    expect = parent_vtk_text(model)
    got = open(old).read()
    assert got == expect
    nf = npg.NodalFields(model)
    npg.save_vtk(model, new, nodal=nf)
    text = open(new).read()
    tail = "</PointData>\n</Piece>\n</UnstructuredGrid>\n</VTKFile>\n"
    assert text.startswith(expect[:-len(tail)]) and text.endswith(tail)
    names = re.findall(r'<DataArray type="Float64" Name="([^"]+)"', text[text.index("<PointData>"):])
    assert names == ["u", "p", "b", "alpha*b_z", "nu", "kappa_v", "grad_b", "vorticity", "div_u", "N2", "pv"]
    g = nf.compute()
    for name, a in (("grad_b", g.grad_b), ("vorticity", g.vorticity()), ("div_u", g.divergence()), ("N2", g.N2()), ("pv", g.pv())):
        assert np.array_equal(read_point_array(text, name), a.reshape(len(a), -1)), name


def check_determinism_and_selection(model):
    """check 7: two calls - the same bits; a field group alone - the bits of the full call's channels, NaN elsewhere"""
    nf = npg.NodalFields(model)
    a, b = nf.compute_raw(), nf.compute_raw()
    c = npg.NodalFields(model).compute_raw()
    assert np.array_equal(a, b) and np.array_equal(a, c) and np.isfinite(a).all()
    groups = {"u": range(0, 9), "b": range(9, 12), "p": range(12, 15)}
    for fields in (("b",), ("u",), ("p",), ("u", "p"), ("p", "b")):
        r = nf.compute_raw(fields)
        keep = np.zeros(NCH, dtype=bool)
        keep[15:] = True
        for f in fields:
            keep[list(groups[f])] = True
        assert np.array_equal(r[keep], a[keep]) and np.isnan(r[~keep]).all(), fields
        dv = nf.compute_device(fields)
        assert dv.n == int(keep.sum()) * model.fe_data.mesh.nn
    assert np.array_equal(nf.compute_raw(), a)                                             # the scratch of a smaller call does not linger
    byval = npg.NodalFields(model, ordered=True)
    assert np.array_equal(nf.sel, np.arange(len(a[0]))) and (np.diff(byval.valence) >= 0).all() and (np.diff(byval.sel) < 0).any()
    assert np.array_equal(byval.compute_raw(), a)                                          # the order of the rows does not touch a node's bits
    g = nf.compute(("b",))
    assert np.array_equal(g.grad_b, a[9:12].T) and np.isnan(g.grad_u).all() and np.isnan(g.vorticity()).all() and np.isnan(g.grad_p).all()
    assert nf.nbytes > 0


def check_python_refusals(model):
    """everything NodalFields refuses, each leaving the model untouched"""
    nn = model.fe_data.mesh.nn
    before = dict(vars(model))
    x0, b0 = model.inversion.solver.x.to_host(), model.b_vec.to_host()
    base = {k: v for k, v in vars(model).items() if k in ("arch", "fe_data", "params", "forcings", "b_vec", "inversion")}
    for bad in (np.ones(nn + 1, dtype=bool), np.ones(nn, dtype=np.int32), np.ones((nn, 1), dtype=bool)):
        with np.testing.assert_raises(ValueError):
            npg.NodalFields(model, nodes=bad)
    with np.testing.assert_raises(ValueError):
        npg.NodalFields(model, weight="area")
    nf = npg.NodalFields(model)
    for fields in (("u", "q"), (), ("grad_b",)):
        with np.testing.assert_raises(ValueError):
            nf.compute(fields)
    part = SimpleNamespace(**base, layout=SimpleNamespace(cell_owner=None, locator_cells=None))
    repl = SimpleNamespace(**base, partition=object())
    comm = SimpleNamespace(**base, comm=object())
    for fake in (part, repl, comm):
        with np.testing.assert_raises(NotImplementedError):
            npg.NodalFields(fake)
    assert dict(vars(model)) == before
    assert np.array_equal(model.inversion.solver.x.to_host(), x0) and np.array_equal(model.b_vec.to_host(), b0)


def check_2d_refused(arch):
    """an embedded 2-D mesh: NotImplementedError in Python, NPG_EINVAL from the library"""
    model = with_config(ar.bowl2d_light(arch), "bowl_mixing")
    with np.testing.assert_raises(NotImplementedError):
        npg.NodalFields(model)
    fe = device_fe(arch, model.fe_data)
    h = C.c_void_p()
    rc = L.lib().npg_nodal_create(fe.h, 1, L.ptr(L.as_i64([0, 1])), L.ptr(L.as_i32([0])), 0, C.byref(h))
    assert rc == NPG_EINVAL and "2-D" in L.lib().npg_last_error().decode() and not h.value


def abi_refusals(lib, fe, ncell, ptr, inc, vec, vecs):
    """the C ABI's NPG_EINVAL cases against one library: `lib` with its engine `fe`; vec(n) makes a vector of that library, vecs =
    (x_inv, b) of the right sizes.  Everything is refused on the host before any launch: no case relies on a device fault."""
    nsel = len(ptr) - 1

    def create(fe=fe, nsel=nsel, ptr=ptr, inc=inc, mode=0, out=True):
        h = C.c_void_p()
        p = lambda a: None if a is None else L.ptr(a)
        rc = lib.npg_nodal_create(fe, nsel, p(ptr), p(inc), mode, C.byref(h) if out else None)
        return rc, lib.npg_last_error().decode(), h

    def bad(a, i, v):
        a = a.copy()
        a[i] = v
        return a
    dec = bad(ptr, 3, ptr[2] - 1)
    two = int(np.nonzero(np.diff(ptr) >= 2)[0][0])                                         # a node with two cells
    empty = ptr.copy()
    empty[5:] -= ptr[5] - ptr[4]                                                           # node 4 loses its list
    for kw, word in ((dict(fe=None), "NULL"), (dict(out=False), "NULL"), (dict(ptr=None), "NULL"), (dict(inc=None), "NULL"),
                     (dict(inc=bad(inc, 7, 16 * ncell + 2)), "incidence cell"), (dict(inc=bad(inc, 2, -5)), "incidence cell"),
                     (dict(inc=bad(inc, 9, (inc[9] & ~15) | 10)), "local node"), (dict(ptr=dec), "decreases"), (dict(ptr=bad(ptr, 0, 1)), "start at 0"),
                     (dict(ptr=empty), "no incidence"), (dict(mode=2), "weight_mode"), (dict(nsel=-1), "nsel"),
                     (dict(inc=bad(inc, ptr[two] + 1, inc[ptr[two]])), "ascending")):
        rc, msg, h = create(**kw)
        assert rc == NPG_EINVAL and word in msg and not h.value, (list(kw), rc, msg)
    rc, msg, h = create()
    assert rc == 0, msg
    x, b = vecs
    nchs = {7: 17, 2: 5}
    out = vec(17 * nsel, -7.0)
    for args, word in (((h, vec(x[1] - 1)[0], b[0], 7, out[0]), "flow vector"), ((h, x[0], vec(b[1] + 1)[0], 7, out[0]), "buoyancy vector"),
                       ((h, x[0], b[0], 7, vec(17 * nsel - 1)[0]), "out holds"), ((h, x[0], b[0], 2, vec(nchs[2] * nsel - 1)[0]), "out holds"),
                       ((h, x[0], b[0], 0, out[0]), "fields_mask"), ((h, x[0], b[0], 8, out[0]), "fields_mask"),
                       ((None, x[0], b[0], 7, out[0]), "NULL"), ((h, None, b[0], 7, out[0]), "NULL"), ((h, x[0], b[0], 7, None), "NULL")):
        rc = lib.npg_nodal_compute(*args)
        msg = lib.npg_last_error().decode()
        assert rc == NPG_EINVAL and word in msg, (rc, msg)
    return h, out


def check_abi_refusals(model):
    """check 7 through the library the model runs on: the refusals, nothing launched by a refused compute, info, nsel = 0"""
    lib = L.lib()
    ctx = model.arch.ctx
    nf = npg.NodalFields(model)
    ptr, inc = nf._table
    x, b = model.inversion.solver.x, model.b_vec

    def vec(n, fill=0.0):
        v = npg.DeviceVector(ctx, n)
        v.fill(fill)
        keep.append(v)
        return v.h, n
    keep = []
    h, out = abi_refusals(lib, nf.fe.h, model.fe_data.mesh.ncell, ptr, inc, vec, ((x.h, x.n), (b.h, b.n)))
    assert np.array_equal(keep[0].to_host(), np.full(keep[0].n, -7.0))                     # nothing was launched
    q = [C.c_int64() for _ in range(4)]
    L.check(lib.npg_nodal_info(h, *[C.byref(v) for v in q]))
    assert [v.value for v in q] == [len(ptr) - 1, len(inc), nf.max_valence, 0]              # no compute yet: no scratch
    assert lib.npg_nodal_info(None, None, None, None, None) == NPG_EINVAL
    L.check(lib.npg_nodal_compute(h, x.h, b.h, 7, out[0]))
    assert np.array_equal(keep[0].to_host().reshape(NCH, -1), nf.compute_raw()[:, nf.sel])      # row j is node sel[j]
    L.check(lib.npg_nodal_destroy(h))
    L.check(lib.npg_nodal_destroy(None))
    h0 = C.c_void_p()
    L.check(lib.npg_nodal_create(nf.fe.h, 0, L.ptr(L.as_i64([0])), None, 0, C.byref(h0)))   # nsel = 0 is legal
    L.check(lib.npg_nodal_compute(h0, x.h, b.h, 7, vec(0)[0]))
    L.check(lib.npg_nodal_destroy(h0))
    empty = npg.NodalFields(model, nodes=np.zeros(model.fe_data.mesh.nn, dtype=bool)).compute_raw()
    assert np.isnan(empty).all()


# ---- the device against the host library (GPU file only) -----------------------------------------------------------------------------
class HostEngine:
    """libnupgcm_host.so loaded BESIDE the library the model runs on, with an engine of the model's tables, driven through its C ABI"""

    def __init__(self, model):
        H = C.CDLL(L.HOST_LIB_PATH)
        L._declare(H, partial=True)
        self.H = H
        fed = model.fe_data
        m = fed.mesh
        k = device_fe(model.arch, fed)._keep
        d = L.FeDesc(ncell=m.ncell, nq=len(m.q_w), nloc_b=k["cb"].shape[1], grad_lambda=k["G"].ctypes.data, wdet=k["wdet"].ctypes.data,
                     qw=k["qw"].ctypes.data, N2=k["N2"].ctypes.data, dN2=k["dN2"].ctypes.data, Nb=k["Nb"].ctypes.data, dNb=k["dNb"].ctypes.data,
                     N1=k["N1"].ctypes.data, cell_u=k["cu"].ctypes.data, cell_p=k["cp"].ctypes.data, cell_b=k["cb"].ctypes.data,
                     u_diri=k["ud"].ctypes.data, n_u_diri=k["ud"].size, b_diri=k["bd"].ctypes.data, n_b_diri=k["bd"].size,
                     n_inv=fed.dofs.nu + fed.dofs.np, n_b=fed.dofs.nb)
        self.ctx, self.fe = C.c_void_p(), C.c_void_p()
        self.ok(H.npg_ctx_create(0, C.byref(self.ctx)))
        self.ok(H.npg_fe_create(self.ctx, C.byref(d), C.byref(self.fe)))
        self.vecs = []

    def ok(self, rc):
        assert rc == 0, self.H.npg_last_error().decode()

    def vec(self, a):
        a = L.as_f64(a)
        v = C.c_void_p()
        self.ok(self.H.npg_vec_create(self.ctx, len(a), C.byref(v)))
        if len(a):
            self.ok(self.H.npg_vec_upload(v, L.ptr(a)))
        self.vecs.append(v)
        return v

    def close(self):
        for v in self.vecs:
            self.H.npg_vec_destroy(v)
        self.H.npg_fe_destroy(self.fe)
        self.H.npg_ctx_destroy(self.ctx)


def host_library_raw(model, nf, fields=("u", "b", "p")):
    """(17, nn) of the model's current state through the host library with the incidence table of `nf`"""
    from nupgcm_amd import nodal as nd
    E = HostEngine(model)
    H = E.H
    ptr, inc = nf._table
    nsel = len(nf.sel)
    mask = nd.mask_of(fields)
    ch = nd.channels_of(mask)
    N = C.c_void_p()
    E.ok(H.npg_nodal_create(E.fe, nsel, L.ptr(ptr), L.ptr(inc) if len(inc) else None, nd.WEIGHTS[nf.weighting], C.byref(N)))
    x, b, out = E.vec(model.inversion.solver.x.to_host()), E.vec(model.b_vec.to_host()), E.vec(np.zeros(len(ch) * nsel))
    E.ok(H.npg_nodal_compute(N, x, b, mask, out))
    got = np.empty(len(ch) * nsel)
    if got.size:
        E.ok(H.npg_vec_download(out, L.ptr(got)))
    H.npg_nodal_destroy(N)
    E.close()
    raw = np.full((NCH, nf.nn), np.nan)
    raw[np.ix_(ch, nf.sel)] = got.reshape(len(ch), nsel)
    return raw


def check_host_abi_refusals(model):
    """the same NPG_EINVAL cases, with a message, from the host library"""
    E = HostEngine(model)
    nf = npg.NodalFields(model)
    ptr, inc = nf._table

    def vec(n, fill=0.0):
        return E.vec(np.full(n, fill)), n
    x, b = model.inversion.solver.x, model.b_vec
    h, _ = abi_refusals(E.H, E.fe, model.fe_data.mesh.ncell, ptr, inc, vec, (vec(x.n), vec(b.n)))
    E.H.npg_nodal_destroy(h)
    E.close()
