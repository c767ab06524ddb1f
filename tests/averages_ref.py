"""A numpy restatement of the time means and eddy co-moments (nupgcm_amd.averages) and the checks shared by
tests/test_averages.py (CPU()) and tests/test_gpu_averages.py (GPU()).

The restatement is two things:
  * RefAcc - the same recurrence in plain numpy fp64 (numpy's elementwise add, subtract and multiply are single IEEE operations, no
    contraction), with a node table built independently from spaces.u_dof, spaces.b_dof, mesh.edges and the inverse permutations.
    The library must have its BITS: the kernels have only IEEE add, subtract and multiply in a fixed association.
  * two_pass - a two-pass weighted mean and covariance in np.longdouble (64-bit mantissa on this platform, asserted).

The accuracy bounds are each entry's own terms, n the number of samples:
  means        |err| <= (n + 8) eps max_n |a_n|
  co-moments   |err| <= (n + 8) eps [sum w |da db| + max |a| sum w |db| + max |b| sum w |da|]
(the second and third term: a delta inherits the rounding of the stored mean).  A numpy prototype of the recurrence stays at <= 0.2
(means) and <= 0.09 (co-moments) of these bounds for n from 2 to 3000 on random sequences."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np

import nupgcm_amd as npg
from nupgcm_amd import _lib as L
from tests import helpers
from tests import integrals_ref as ir

EPS = np.finfo(np.float64).eps
SEED = 20261021
NEW = {"npg_tavg_create", "npg_tavg_accumulate", "npg_tavg_info", "npg_tavg_destroy"}
EDGE_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257)
PAIRS = ("uu", "uv", "uw", "vv", "vw", "ww", "ub", "vb", "wb", "bb")
PA = (0, 0, 0, 1, 1, 2, 0, 1, 2, 3)
PB = (0, 1, 2, 1, 2, 2, 3, 3, 3, 3)
WEIGHTS = (0.7, 1.3, 0.25, 2.0, 0.9, 1e-3, 3.1)                  # unequal, not dyadic: r and q round


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def ref_table(fed):
    """iu (nn, 3), ib (nn, 2) in MESH node order from the native DoF numbers and the inverse permutations; -1 = Dirichlet"""
    if getattr(fed, "_averages_ref_table", None) is not None:
        return fed._averages_ref_table
    m, s, d = fed.mesh, fed.spaces, fed.dofs
    pos_x = np.empty(d.nu + d.np, dtype=np.int64)
    pos_x[d.p_inversion] = np.arange(d.nu + d.np)               # native index -> position in x_inv
    pos_b = np.empty(d.nb, dtype=np.int64)
    pos_b[d.p_b] = np.arange(d.nb)
    iu = np.full((m.nn, 3), -1, dtype=np.int64)
    for n in range(m.nn):
        for c in range(3):
            if s.u_dof[n, c] >= 0:
                iu[n, c] = pos_x[s.u_dof[n, c]]
    bp = lambda node: pos_b[s.b_dof[node]] if s.b_dof[node] >= 0 else -1
    ib = np.full((m.nn, 2), -1, dtype=np.int64)
    for n in range(m.nn):
        if s.b_order == 2 or n < m.nv:
            ib[n] = bp(n)
        else:
            ib[n] = [bp(m.edges[n - m.nv, 0]), bp(m.edges[n - m.nv, 1])]
    fed._averages_ref_table = (iu, ib)
    return iu, ib


def node_values(tab, x, b, dtype=np.float64):
    """(4, nn): what enters a node's deltas - u, v, w and b (a P1 mid-node: half the sum of its vertices); a Dirichlet DoF counts 0
    (it is constant in time: any constant drops out of a delta)"""
    iu, ib = tab
    x, b = np.asarray(x, dtype=dtype), np.asarray(b, dtype=dtype)
    at = lambda a, i: np.where(i >= 0, a[np.maximum(i, 0)], dtype(0)) if len(a) else np.zeros(i.shape, dtype=dtype)
    b0, b1 = at(b, ib[:, 0]), at(b, ib[:, 1])
    return np.stack([at(x, iu[:, 0]), at(x, iu[:, 1]), at(x, iu[:, 2]), np.where(ib[:, 0] == ib[:, 1], b0, dtype(0.5) * (b0 + b1))])


class RefAcc:
    """the recurrence in numpy fp64, one bin, co-moments (10, nn) in mesh node order"""

    def __init__(self, fed, n_inv, n_b):
        self.tab = ref_table(fed)
        self.W, self.mx, self.mb = 0.0, np.zeros(n_inv), np.zeros(n_b)
        self.C = np.zeros((10, fed.mesh.nn))

    def add(self, x, b, w):
        W1 = self.W + w
        r, q = w / W1, w * (self.W / W1)
        dx, db = x - self.mx, b - self.mb
        d = node_values(self.tab, dx, db)                        # the subtraction entry by entry, then the gather (P1 mid-node: 0.5 (d0 + d1))
        for p in range(10):
            self.C[p] = self.C[p] + (q * d[PA[p]]) * d[PB[p]]
        self.mx = self.mx + r * dx
        self.mb = self.mb + r * db
        self.W = W1
        return self


def two_pass(tab, xs, bs, ws):
    """longdouble: W, mean x, mean b, the node co-moments (10, nn), and for the bounds max |a| (x, b, nodes) and sum w |da|, sum w |da db|"""
    LD = np.longdouble
    assert np.finfo(LD).nmant == 63
    ws = [LD(w) for w in ws]
    W = sum(ws, LD(0))
    mx = sum((w * np.asarray(x, dtype=LD) for w, x in zip(ws, xs)), np.zeros(len(xs[0]), dtype=LD)) / W
    mb = sum((w * np.asarray(b, dtype=LD) for w, b in zip(ws, bs)), np.zeros(len(bs[0]), dtype=LD)) / W
    nm = node_values(tab, mx, mb, LD)
    nn = nm.shape[1]
    Cm, Sab, Sa, amax = np.zeros((10, nn), dtype=LD), np.zeros((10, nn), dtype=LD), np.zeros((4, nn), dtype=LD), np.zeros((4, nn), dtype=LD)
    for w, x, b in zip(ws, xs, bs):
        a = node_values(tab, x, b, LD)
        d = a - nm
        amax = np.maximum(amax, np.abs(a))
        Sa += w * np.abs(d)
        for p in range(10):
            Cm[p] += w * d[PA[p]] * d[PB[p]]
            Sab[p] += w * np.abs(d[PA[p]] * d[PB[p]])
    xmax = np.max(np.abs(np.stack(xs)), axis=0) if len(xs[0]) else np.zeros(0)
    bmax = np.max(np.abs(np.stack(bs)), axis=0) if len(bs[0]) else np.zeros(0)
    return SimpleNamespace(W=W, mx=mx, mb=mb, C=Cm, Sab=Sab, Sa=Sa, amax=amax, xmax=xmax, bmax=bmax)


def bounds(tp, n, extra=0):
    """(bound of mean x, of mean b, of the co-moments (10, nn)) for n samples; extra: further terms (one per merged bin)"""
    f = (n + 8 + extra) * EPS
    cb = np.stack([tp.Sab[p] + tp.amax[PA[p]] * tp.Sa[PB[p]] + tp.amax[PB[p]] * tp.Sa[PA[p]] for p in range(10)])
    return f * tp.xmax, f * tp.bmax, (f * cb).astype(np.float64)


# ---- models and states --------------------------------------------------------------------------------------------------------------
def light(arch, fed):
    """what TimeAverages reads of a model, without toolkits"""
    ctx = arch.ctx
    x = npg.DeviceVector(ctx, fed.dofs.nu + fed.dofs.np)
    return SimpleNamespace(arch=arch, fe_data=fed, b_vec=npg.DeviceVector(ctx, fed.dofs.nb), inversion=SimpleNamespace(solver=SimpleNamespace(x=x)),
                           step_index=1)


def bowl_mesh():
    return npg.Mesh(os.path.join(helpers.GOLDEN, "mesh_bowl3D_h0.1.npz"))


def bowl_light(arch, name="bowl_surface_flux", b_order=2, mesh=None):
    """the spaces of a named configuration on the bowl h = 0.1 golden mesh (bowl_wind: buoyancy Dirichlet nodes), P2 or P1"""
    _, _, btags, bvals, _, _ = helpers.product_config(name)
    mesh = mesh or bowl_mesh()
    spaces = npg.Spaces(mesh, u_diri_tags=helpers.U_TAGS, u_diri_vals=helpers.U_VALS, u_diri_masks=helpers.U_MASKS, b_diri_tags=btags,
                        b_diri_vals=bvals, b_order=b_order)
    return light(arch, npg.FEData(mesh, spaces))


def bowl2d_light(arch):
    return bowl_light(arch, "bowl_mixing", mesh=npg.Mesh(os.path.join(helpers.GOLDEN, "mesh_bowl2D_h0.1.npz")))


def states(model, n, seed=SEED, offset=0.0, scale=1.0):
    """n synthetic states (x, b): integrals_ref.random_state with a varying seed and scale, shifted by a fixed random offset field"""
    nx, nb = model.inversion.solver.x.n, model.b_vec.n
    rng = np.random.default_rng(seed)
    ox, ob = offset * (1.0 + rng.random(nx)), offset * (1.0 + rng.random(nb))
    out = []
    for k in range(n):
        x, b = ir.random_state(model, seed=seed + 1 + k, scale=scale * (1.0 + 0.5 * (k % 3)))
        out.append((x + ox, b + ob))
    return out


def feed(model, ta, x, b, w, t=0.0):
    model.inversion.solver.x.upload(x)
    model.b_vec.upload(b)
    ta.add_sample(model.inversion.solver.x, model.b_vec, w, t)


def masks(nn, seed=SEED):
    rng = np.random.default_rng(seed)
    out = {}
    for n in EDGE_COUNTS:
        mk = np.zeros(nn, dtype=bool)
        mk[rng.permutation(nn)[:n]] = True
        out[n] = mk
    return out


def comoments(ta, bin=None):
    """(10, nn): the co-moments C themselves (not C / W) of a bin in mesh node order, NaN at unselected nodes"""
    k = 0 if bin is None else bin
    out = np.full((10, ta.nnode_mesh), np.nan)
    out[:, ta.sel] = ta.comom[k].to_host().reshape(10, len(ta.sel))
    return out


def same_selected(got, ref, mask):
    """array_equal at the selected nodes, NaN at all others"""
    sel = np.ones(got.shape[1], dtype=bool) if mask is None else mask
    return np.array_equal(got[:, sel], ref[:, sel]) and np.isnan(got[:, ~sel]).all()


# ---- the host library beside the one the model runs on -------------------------------------------------------------------------------
def host_library(ta, samples, ws):
    """(mean_x, mean_b, comom (10, nsel)) after the samples through libnupgcm_host.so, loaded BESIDE the library the model runs on and
    driven through its C ABI alone with the node table of `ta`"""
    H = C.CDLL(L.HOST_LIB_PATH)
    L._declare(H, partial=True)

    def ok(rc):
        assert rc == 0, H.npg_last_error().decode()
    ctx, T = C.c_void_p(), C.c_void_p()
    ok(H.npg_ctx_create(0, C.byref(ctx)))
    iu, ib = ta._table
    nsel = len(ta.sel)
    ok(H.npg_tavg_create(ctx, ta.n_inv, ta.n_b, nsel, L.ptr(iu), L.ptr(ib), C.byref(T)))
    vecs = []
    for n in (ta.n_inv, ta.n_b, ta.n_inv, ta.n_b, 10 * nsel):
        v = C.c_void_p()
        ok(H.npg_vec_create(ctx, n, C.byref(v)))
        vecs.append(v)
    W = 0.0
    for (x, b), w in zip(samples, ws):
        ok(H.npg_vec_upload(vecs[0], L.ptr(L.as_f64(x))))
        ok(H.npg_vec_upload(vecs[1], L.ptr(L.as_f64(b))))
        W1 = W + w
        ok(H.npg_tavg_accumulate(T, w / W1, w * (W / W1), *vecs))
        W = W1
    out = [np.empty(ta.n_inv), np.empty(ta.n_b), np.empty(10 * nsel)]
    for v, a in zip(vecs[2:], out):
        if a.size:
            ok(H.npg_vec_download(v, L.ptr(a)))
    H.npg_tavg_destroy(T)
    for v in vecs:
        H.npg_vec_destroy(v)
    H.npg_ctx_destroy(ctx)
    return out[0], out[1], out[2].reshape(10, nsel)


# ---- the checks (arch = npg.CPU() or npg.GPU()) --------------------------------------------------------------------------------------
def check_exports():
    assert {"TimeAverages", "Covariance", "phase_bin"} <= set(npg.__all__)
    assert NEW <= set(L.declared_symbols())
    for path in (L.HOST_LIB_PATH, L.LIB_PATH):
        lib = C.CDLL(path)
        assert not [s for s in NEW if not hasattr(lib, s)], path


def check_bits(model, label, mask=None, against_host=False, seed=SEED):
    """check 2: after 1, 2, 3 and 7 samples of unequal weights the means and all ten co-moments ARE the numpy recurrence's (array_equal);
    unselected nodes NaN, the means untouched by the mask.  against_host: the device against the host library, every entry identical"""
    fed = model.fe_data
    ta = npg.TimeAverages(model, nodes=mask, weight="steps")
    assert model.averages is ta
    ref = RefAcc(fed, ta.n_inv, ta.n_b)
    samples = states(model, 7, seed)
    for k, ((x, b), w) in enumerate(zip(samples, WEIGHTS), 1):
        feed(model, ta, x, b, w)
        ref.add(x, b, w)
        if k in (1, 2, 3, 7):
            mx, mb = ta.mean_state()
            got = comoments(ta)
            assert ta.weight() == ref.W
            assert np.array_equal(mx.to_host(), ref.mx) and np.array_equal(mb.to_host(), ref.mb), (label, k)
            assert same_selected(got, ref.C, mask), (label, k)
            if k == 1:
                assert np.array_equal(ref.mx, x) and np.array_equal(ref.mb, b) and not np.nan_to_num(got).any()     # r = 1, q = 0
    cov = ta.covariance()
    sel = np.ones(fed.mesh.nn, dtype=bool) if mask is None else mask
    for p, name in enumerate(PAIRS):
        assert np.array_equal(getattr(cov, name)[sel], ref.C[p][sel] / ref.W) and np.isnan(getattr(cov, name)[~sel]).all()
    assert np.array_equal(cov.eddy_flux[sel], np.stack([ref.C[6], ref.C[7], ref.C[8]], axis=1)[sel] / ref.W)
    # (three non-negative terms: the two ways of writing it differ by a few roundings, relative to the result)
    assert np.allclose(cov.eke[sel], ((ref.C[0] + ref.C[3] + ref.C[5]) / (2.0 * ref.W))[sel], rtol=4 * EPS, atol=0.0)
    assert np.array_equal(cov.b_variance[sel], cov.bb[sel])
    if sel.any() and ta.n_b:
        assert np.nan_to_num(got).any()
    if against_host:
        hx, hb, hc = host_library(ta, samples, WEIGHTS)
        dev = (ta.mean_x[0].to_host(), ta.mean_b[0].to_host(), ta.comom[0].to_host().reshape(10, len(ta.sel)))
        share = [float(np.mean(a == h)) if a.size else 1.0 for a, h in zip(dev, (hx, hb, hc))]
        print(f"device vs host library {label}: share of identical entries mean x {share[0]:.6f}, mean b {share[1]:.6f}, co-moments {share[2]:.6f}")
        assert share == [1.0, 1.0, 1.0], (label, share)
    ta.detach()
    assert model.averages is None
    return ta, ref


def check_accuracy(model, label, offset, n=50):
    """check 3: the library's fp64 recurrence against the longdouble two-pass result, entry by entry; prints the worst ratios"""
    ta = npg.TimeAverages(model, weight="steps")
    samples = states(model, n, SEED + 100, offset=offset, scale=1.0 if offset == 0.0 else 1e-6 * offset)
    rng = np.random.default_rng(SEED + 5)
    ws = 0.25 + rng.random(n) * 2.0
    for (x, b), w in zip(samples, ws):
        feed(model, ta, x, b, float(w))
    tab = ref_table(model.fe_data)
    tp = two_pass(tab, [s[0] for s in samples], [s[1] for s in samples], ws)
    bx, bb, bc = bounds(tp, n)
    mx, mb = ta.mean_state()
    ex = np.abs(mx.to_host().astype(np.longdouble) - tp.mx).astype(np.float64)
    eb = np.abs(mb.to_host().astype(np.longdouble) - tp.mb).astype(np.float64)
    ec = np.abs(comoments(ta).astype(np.longdouble) - tp.C).astype(np.float64)
    ratio = lambda e, bnd: float(np.max(e[bnd > 0] / bnd[bnd > 0])) if (bnd > 0).any() else 0.0
    print(f"accuracy {label} (n = {n}): worst |err| / bound: mean x {ratio(ex, bx):.3f}, mean b {ratio(eb, bb):.3f}, co-moments {ratio(ec, bc):.3f}")
    assert (ex <= bx).all() and (eb <= bb).all() and (ec <= bc).all(), label
    assert abs(ta.weight() - float(tp.W)) <= n * EPS * float(tp.W)
    ta.detach()
    return ratio(ex, bx), ratio(eb, bb), ratio(ec, bc)


def check_dirichlet(model, label):
    """co-moments at Dirichlet DoFs are exactly 0; a P1 mid-node next to a Dirichlet vertex has the restatement's bits"""
    fed = model.fe_data
    ta, ref = check_bits(model, label)
    iu, ib = ref.tab
    got = np.full((10, fed.mesh.nn), np.nan)
    got[:, ta.sel] = ta.comom[0].to_host().reshape(10, len(ta.sel))
    bd = (ib < 0).all(axis=1)
    assert bd.any() and not bd.all()
    for p in (6, 7, 8, 9):
        assert not got[p][bd].any()
    for c in range(3):
        ud = iu[:, c] < 0
        assert ud.any()
        for p in range(10):
            if PA[p] == c or PB[p] == c:
                assert not got[p][ud].any()
    if fed.spaces.b_order == 1:
        half = (ib[:, 0] != ib[:, 1]) & ((ib < 0).sum(axis=1) == 1)          # a mid-node between a Dirichlet and a free vertex
        assert half.any() and got[9][half].any() and np.array_equal(got[:, half], ref.C[:, half])


def check_phases(model, label):
    """check 5: P = 4 bins over a period - sample times on bin edges, before t0 and several periods out; every bin is the restatement's
    and a single-bin accumulator's fed that bin's samples; mean_state(None) / covariance(None) against the longdouble result"""
    fed = model.fe_data
    P, T, t0 = 4, 2.0, 0.5
    times = [0.5, 0.75, 1.0, 1.5, 2.0, 2.4999, 2.5, -0.25, 0.0, 0.49, 7.25, -5.5, 1.0 + 6 * T, 2.0 - 3 * T, 3.1, 0.9]
    want = [0, 0, 1, 2, 3, 3, 0, 2, 3, 3, 1, 0, 1, 3, 1, 0]
    assert [npg.phase_bin(t, P, T, t0) for t in times] == want and set(want) == set(range(P))
    n = len(times)
    samples = states(model, n, SEED + 200, offset=0.5)
    ws = [WEIGHTS[k % len(WEIGHTS)] for k in range(n)]
    ta = npg.TimeAverages(model, phases=P, period=T, t0=t0, weight="steps")
    one = [npg.TimeAverages(model, weight="steps") for _ in range(P)]
    refs = [RefAcc(fed, ta.n_inv, ta.n_b) for _ in range(P)]
    for (x, b), w, t, k in zip(samples, ws, times, want):
        feed(model, ta, x, b, w, t)
        feed(model, one[k], x, b, w, t)
        refs[k].add(x, b, w)
    for k in range(P):
        mx, mb = ta.mean_state(k)
        assert ta.weight(k) == refs[k].W == one[k].weight()
        assert np.array_equal(mx.to_host(), refs[k].mx) and np.array_equal(mb.to_host(), refs[k].mb)
        assert np.array_equal(comoments(ta, k), refs[k].C)
        assert np.array_equal(mx.to_host(), one[k].mean_x[0].to_host()) and np.array_equal(mb.to_host(), one[k].mean_b[0].to_host())
        assert np.array_equal(ta.comom[k].to_host(), one[k].comom[0].to_host())
    assert ta.weight() == sum(r.W for r in refs)
    tp = two_pass(ref_table(fed), [s[0] for s in samples], [s[1] for s in samples], ws)
    bx, bb, bc = bounds(tp, n, extra=P)
    mx, mb = ta.mean_state()
    W = float(tp.W)
    cov = ta.covariance()
    C_all = np.stack([getattr(cov, name) for name in PAIRS]).astype(np.longdouble) * np.longdouble(cov.weight)
    ex = np.abs(mx.to_host().astype(np.longdouble) - tp.mx).astype(np.float64)
    eb = np.abs(mb.to_host().astype(np.longdouble) - tp.mb).astype(np.float64)
    ec = np.abs(C_all - tp.C).astype(np.float64)
    bc = bc + 2 * EPS * np.abs(tp.C).astype(np.float64)                    # covariance() divides by W, the line above multiplies again
    r = lambda e, bnd: float(np.max(e[bnd > 0] / bnd[bnd > 0]))
    print(f"phases {label}: merged bins against longdouble, worst |err| / bound: mean x {r(ex, bx):.3f}, mean b {r(eb, bb):.3f}, "
          f"co-moments {r(ec, bc):.3f}")
    assert abs(cov.weight - W) <= n * EPS * W
    assert (ex <= bx).all() and (eb <= bb).all() and (ec <= bc).all()
    model.averages = None


def check_applied(model):
    """check 6: inside the context MeshIntegrals sees the mean flow; after it - also when the body raises - the old bits are back"""
    import pytest
    ta = npg.TimeAverages(model, weight="steps")
    for (x, b), w in zip(states(model, 3, SEED + 300), WEIGHTS):
        feed(model, ta, x, b, w)
    x0, b0 = ir.random_state(model, seed=SEED + 301)
    mi = npg.MeshIntegrals(model)
    now = mi.compute_raw()
    mx, mb = (v.to_host() for v in ta.mean_state())
    with ta.applied(model):
        inside = mi.compute_raw()
        assert np.array_equal(model.inversion.solver.x.to_host(), mx) and np.array_equal(model.b_vec.to_host(), mb)
    assert np.array_equal(model.inversion.solver.x.to_host(), x0) and np.array_equal(model.b_vec.to_host(), b0)
    with pytest.raises(RuntimeError, match="body"):
        with ta.applied(model):
            raise RuntimeError("body")
    assert np.array_equal(model.inversion.solver.x.to_host(), x0) and np.array_equal(model.b_vec.to_host(), b0)
    model.inversion.solver.x.upload(mx)
    model.b_vec.upload(mb)
    by_hand = mi.compute_raw()
    assert np.array_equal(inside, by_hand) and not np.array_equal(inside, now)
    ta.detach()


def loop_model(arch):
    """bowl_surface_flux on the small channel basin under the adaptive BDF1 (as forcing_ref.check_in_the_loop)"""
    from nupgcm_amd import channel_basin as cb
    from nupgcm_amd import workloads
    prm, frc, _, _, _, b0 = helpers.product_config("bowl_surface_flux")
    mesh = npg.Mesh(cb.channel_basin_model(0.125, workloads.CB_ALPHA, dz=0.125))
    fed = npg.FEData(mesh, npg.Spaces(mesh, u_diri_tags=helpers.U_TAGS, u_diri_vals=helpers.U_VALS, u_diri_masks=helpers.U_MASKS))
    ts = npg.BDF1(t_start=0.0, t_stop=1e9, dt=0.3, adaptive=True)
    model = npg.Model(arch, prm, frc, fed, npg.InversionToolkit(arch, fed, prm, frc), npg.EvolutionToolkit(arch, fed, prm, frc, ts), ts)
    npg.set_b(model, lambda x: b0(x) + 20.0 * np.sin(2 * np.pi * x[..., 0]) * x[..., 2])     # a zonal gradient: a flow above u_min, a changing dt
    return model


def check_run(arch, tmp_path):
    """check 7: five steps of run() with averages attached: W = sum of the dt taken, the mean is the restatement's fed the per-step
    states, the run itself has the bits of a run without averages, and save / load after three steps continues to the same bits"""
    plain = loop_model(arch)
    assert plain.averages is None
    npg.run(plain, n_steps=5)
    model = loop_model(arch)
    ta = npg.TimeAverages(model)
    seen, dts = [], []

    def hook(m, t):
        seen.append((m.inversion.solver.x.to_host(), m.b_vec.to_host(), t))
        dts.append(m.timestepper.dt)
    model.on_plot = hook
    npg.run(model, n_steps=5, n_plot=1)
    assert len(seen) == 5 and len(set(dts)) > 1, dts
    W = 0.0
    for dt in dts:
        W = W + dt
    assert ta.weight() == W and ta.nsamples == 5
    ref = RefAcc(model.fe_data, ta.n_inv, ta.n_b)
    for (x, b, _), dt in zip(seen, dts):
        ref.add(x, b, dt)
    mx, mb = ta.mean_state()
    assert np.array_equal(mx.to_host(), ref.mx) and np.array_equal(mb.to_host(), ref.mb) and np.array_equal(comoments(ta), ref.C)
    u, p, b = ta.mean()
    d = model.fe_data.dofs
    assert np.array_equal(np.r_[u, p], ref.mx[d.inv_p_inversion]) and np.array_equal(b, ref.mb[d.inv_p_b])
    for a, c in ((model.state.u, plain.state.u), (model.state.p, plain.state.p), (model.state.b, plain.state.b)):
        assert np.array_equal(a, c)
    # save after three steps, load into a fresh object, two more steps
    again = loop_model(arch)
    first = npg.TimeAverages(again)
    npg.run(again, n_steps=3)
    path = os.path.join(str(tmp_path), "averages_checkpoint")
    first.save(path)
    first.detach()
    second = npg.TimeAverages(again)
    second.load(path)
    npg.run(again, n_steps=2)
    assert second.weight() == ta.weight() and second.nsamples == 5
    assert np.array_equal(second.mean_x[0].to_host(), ta.mean_x[0].to_host()) and np.array_equal(second.mean_b[0].to_host(), ta.mean_b[0].to_host())
    assert np.array_equal(second.comom[0].to_host(), ta.comom[0].to_host())


def check_every(model):
    """every = 3: a sample on every third call carrying the three weights; means only (covariances=False)"""
    ta = npg.TimeAverages(model, covariances=False, every=3, weight="steps")
    ref = RefAcc(model.fe_data, ta.n_inv, ta.n_b)
    samples = states(model, 7, SEED + 400)
    for k, ((x, b), w) in enumerate(zip(samples, WEIGHTS), 1):
        feed(model, ta, x, b, w)
        if k % 3 == 0:
            ref.add(x, b, (WEIGHTS[k - 3] + WEIGHTS[k - 2]) + WEIGHTS[k - 1])
    assert ta.nsamples == 2 and ta.weight() == ref.W and ta.pending == WEIGHTS[6]
    assert np.array_equal(ta.mean_x[0].to_host(), ref.mx) and np.array_equal(ta.mean_b[0].to_host(), ref.mb)
    assert ta.nbytes == 8 * (ta.n_inv + ta.n_b)
    ta.reset()
    assert ta.weight() == 0.0 and not ta.mean_x[0].to_host().any() and ta.pending == 0.0
    ta.detach()


def check_refusals(model):
    """check 8: every refusal leaves the model as it was; a failed npg_tavg_accumulate leaves the accumulators' bits"""
    import pytest
    nn = model.fe_data.mesh.nn
    fake = lambda **kw: SimpleNamespace(**{**model.__dict__, **kw})
    assert getattr(model, "averages", None) is None
    for kw in (dict(layout=SimpleNamespace(cell_owner=np.zeros(1))), dict(layout=SimpleNamespace(locator_cells=1)), dict(comm=object()),
               dict(partition=object())):
        with pytest.raises(NotImplementedError):
            npg.TimeAverages(fake(**kw))
    bad = [dict(nodes=np.ones(nn + 1, dtype=bool)), dict(nodes=np.ones(nn)), dict(every=0), dict(every=-2), dict(phases=0),
           dict(phases=4), dict(phases=4, period=0.0), dict(phases=4, period=-1.0), dict(period=np.inf), dict(phases=2, period=np.nan),
           dict(weight="area")]
    for kw in bad:
        with pytest.raises(ValueError):
            npg.TimeAverages(model, **kw)
        assert getattr(model, "averages", None) is None
    ta = npg.TimeAverages(model)
    samples = states(model, 2, SEED + 500)
    feed(model, ta, *samples[0], 1.0)
    feed(model, ta, *samples[1], 2.0)
    before = (ta.mean_x[0].to_host(), ta.mean_b[0].to_host(), ta.comom[0].to_host(), ta.weight(), ta.nsamples)
    x, b = model.inversion.solver.x, model.b_vec
    for w in (np.nan, np.inf, -1.0):
        with pytest.raises(ValueError):
            ta.add_sample(x, b, w)
        with pytest.raises(ValueError):
            ta.accumulate(model, 0.0, w)
    ta.add_sample(x, b, 0.0)                                                               # no weight: no sample
    lib = L.lib()
    short = npg.DeviceVector(ta.ctx, ta.n_inv + 1)
    args = lambda **kw: [kw.get(k, v) for k, v in (("r", 0.5), ("q", 0.5), ("x", x.h), ("b", b.h), ("mx", ta.mean_x[0].h), ("mb", ta.mean_b[0].h),
                                                   ("c", ta.comom[0].h))]
    for kw, word in ((dict(x=short.h), b"entries"), (dict(mx=short.h), b"entries"), (dict(c=short.h), b"entries"), (dict(r=0.0), b"r must"),
                     (dict(r=1.5), b"r must"), (dict(r=np.nan), b"r must"), (dict(q=-1.0), b"q must"), (dict(q=np.inf), b"q must"),
                     (dict(mx=x.h), b"must not"), (dict(b=None), b"NULL")):
        assert lib.npg_tavg_accumulate(ta.h, *args(**kw)) != 0 and word in lib.npg_last_error(), kw
    h = C.c_void_p()
    iu = L.as_i32(np.full((3, 2), ta.n_inv))
    ib = L.as_i32(np.zeros((2, 2)) - 1)
    assert lib.npg_tavg_create(ta.ctx.h, ta.n_inv, ta.n_b, 2, L.ptr(iu), L.ptr(ib), C.byref(h)) != 0 and b"outside" in lib.npg_last_error()
    iu[:] = -2
    assert lib.npg_tavg_create(ta.ctx.h, ta.n_inv, ta.n_b, 2, L.ptr(iu), L.ptr(ib), C.byref(h)) != 0
    v = [C.c_int64() for _ in range(3)]
    assert lib.npg_tavg_info(ta.h, *[C.byref(a) for a in v]) == 0 and [a.value for a in v] == [len(ta.sel), ta.n_inv, ta.n_b]
    after = (ta.mean_x[0].to_host(), ta.mean_b[0].to_host(), ta.comom[0].to_host(), ta.weight(), ta.nsamples)
    assert all(np.array_equal(a, c) for a, c in zip(before, after))
    ta.detach()
