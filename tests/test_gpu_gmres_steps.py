"""Step-level parity of the product GMRES kernels (csrc/gmres.hip) with the fp64 restatement of tests/gmres_steps_ref.py.

Every case runs solves with atol = rtol = 0 and itmax = k from a non-zero x0 and asserts, for each k:
  - history:     history()[0..k] against the restatement's estimates, |d| <= tol * history[0]   (K1 / K2 / row kernels, Givens)
  - R1:          history()[0] = ||P (b - A x0)|| formed on the host in fp64; for k > memory the entries after a restart rest on
                 the cycle's true residual, which the restatement forms on the host from its own iterate
  - iterate:     x_k against the restatement's x_k                                               (XU: back substitution, x += V y)
  - determinism: the largest k again in a fresh workspace, bit-identical history and iterate
  - instance:    last_config() is the instance the case is named for
  - second passes: the full-kernel cases assert that stats["nreorth"] > 0 (every column for eta > 1)
fp32 instances are compared with the restatement that rounds where they round (basis32 / gather32); on the history the plain fp64
restatement misses that bar by at least 100x (asserted).  The iterate separates less (10-100x on the synthetic systems): x += V y
reads the fp32 columns, where a last-bit difference of wt flips the rounding of single stored entries.  Such flips also set the
floor of the two size-edge cases: at 400 k synthetic rows the history separates by 30x, on bowl3D h = 0.04 by only 5.8x over 43
steps (1.5e-10 against 8.9e-10), so there the full history shows no more than "fp32-ish"; its first steps (history 0..2, before a
flip has propagated) are held to the mirror at 2e-14, which the plain restatement misses by 3.7e5x (asserted).

Measured maxima on one MI355X (|d history| / history[0], max |d x| / max |x|); every case has its own bars, within 30x of its
maxima (1e-15 where the maximum is 0):
  fused n=1 m=1 none: history 0.00e+00 iterate 0.00e+00
  fused n=2 m=5 scalar: history 7.17e-17 iterate 2.23e-16
  fused n=31 m=5 vector: history 2.03e-15 iterate 5.30e-15
  fused n=33 m=8 none: history 3.06e-15 iterate 1.27e-15
  fused n=511 m=9 scalar: history 2.66e-15 iterate 1.14e-15
  fused n=513 m=20 vector: history 7.88e-14 iterate 1.20e-15
  fused n=513 m=30 none: history 1.50e-12 iterate 1.01e-15
  fused n=8191 m=1 vector: history 2.08e-16 iterate 4.39e-16
  fused n=8191 m=30 scalar: history 3.71e-12 iterate 1.59e-15
  split fp64-full n=20001 m=30 vector: history 6.21e-17 iterate 6.90e-16
  split fp64-full-even n=20000 m=9 scalar: history 5.52e-16 iterate 6.72e-16
  split fp64-fast n=20001 m=30 none: history 3.12e-13 iterate 8.05e-16
  split fp32-fast-xg0 n=20001 m=30 vector: history 1.50e-10 iterate 1.24e-09 | plain fp64 restatement: history 6.14e-06 iterate 1.07e-07
  split fp32-full n=20001 m=30 scalar: history 2.24e-11 iterate 8.16e-10 | plain fp64 restatement: history 1.11e-08 iterate 6.80e-08
  split xg2-plain-csr n=120001 m=20 vector: history 6.18e-12 iterate 2.12e-11 | plain fp64 restatement: history 5.92e-08 iterate 7.14e-08
  split fp64-beyond-row-grid n=400001 m=20 scalar: history 2.29e-15 iterate 8.33e-16
  split fp32-beyond-row-pair-grid n=400001 m=20 vector: history 6.79e-10 iterate 6.90e-09 | plain fp64 restatement: history 2.04e-08 iterate 1.09e-07
  split lanes4 n=20001 m=9 none: history 7.63e-15 iterate 2.18e-15
  split lanes8 n=20001 m=9 scalar: history 5.57e-15 iterate 1.16e-15
  split lanes16 n=20001 m=9 vector: history 4.68e-15 iterate 1.95e-15
  split lanes32 n=20001 m=9 none: history 7.06e-15 iterate 1.79e-15
  safe-mode switch, solve 0 (fast 1): history 2.67e-16 iterate 6.40e-16
  safe-mode switch, solve 1 (fast 0): history 2.67e-16 iterate 6.40e-16
  one-rank distributed n=20001 m=9: history 3.79e-15 iterate 7.84e-16
  one-rank distributed n=12001 m=20: history 2.50e-14 iterate 9.82e-16
  bowl h=0.1 xg1-ordinary-tiles m=20: history 1.60e-16 iterate 2.55e-15 | plain fp64 restatement: history 1.22e-08 iterate 4.36e-07
  bowl h=0.1 xg1-windowed-wl4 m=20: history 1.60e-16 iterate 3.57e-15 | plain fp64 restatement: history 1.22e-08 iterate 4.36e-07
  bowl h=0.1 xg1-windowed-wl8 m=9: history 1.60e-16 iterate 1.95e-15 | plain fp64 restatement: history 2.76e-09 iterate 3.19e-07
  bowl h=0.1 fp64-full node-blocked L=4: history 1.60e-16 iterate 8.06e-15
  bowl h=0.1 fp64-full node-blocked L=32: history 1.60e-16 iterate 5.18e-15
  bowl h=0.1 N9 fp64: history 2.98e-17 iterate 5.91e-15
  bowl h=0.1 N9 xg1: history 2.24e-16 iterate 8.58e-15 | plain fp64 restatement: history 4.32e-09 iterate 4.49e-07
  bowl h=0.1 one-rank distributed: history 1.96e-15 iterate 5.95e-15
  bowl h=0.04 xg1 windowed n=263159: history 1.54e-10 iterate 6.95e-08 | plain fp64 restatement: history 8.87e-10 iterate 8.58e-07
    history 0..2: 9.70e-16 | plain fp64 restatement: 3.59e-10
  bowl h=0.04 fp64 n=263159: history 1.55e-16 iterate 2.01e-14
  bowl h=0.1 xg1-windowed-wl4-ORD m=20 (child process): history 1.20e-16 iterate 5.44e-15 | plain fp64 restatement: history 2.16e-09
  bowl h=0.1 xg1-windowed-wl8-ORD m=20 (child process): history 2.00e-16 iterate 4.08e-15 | plain fp64 restatement: history 2.16e-09
  ghost-node windowed product: rel 1.43e-16 (304 ghost nodes)"""
import os

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

import nupgcm_amd as npg  # noqa: E402
from nupgcm_amd import _lib as L  # noqa: E402
from tests.gmres_steps_ref import gmres_steps, true_residual  # noqa: E402
from tests.helpers import build_fe_data  # noqa: E402

KS = (1, 2, 7, 8, 9, 16, 17)


@pytest.fixture(scope="module")
def arch():
    a = npg.GPU()
    a.ctx
    return a


def synth(n, seed, long_row=0):
    """well-conditioned nonsymmetric system (condition number ~30): 19 random entries per row in [0, 1) plus a diagonal in [3, 4);
    long_row > 0: row n // 2 gets that many extra off-diagonal entries of 1e-3 scale (one row longer than a tile)"""
    rng = np.random.default_rng(seed)
    k = min(n, 19)
    rows = np.repeat(np.arange(n), k)
    cols = rng.integers(0, n, n * k)
    vals = rng.random(n * k)
    if long_row:
        rows = np.concatenate([rows, np.full(long_row, n // 2)])
        cols = np.concatenate([cols, rng.choice(n, long_row, replace=False)])
        vals = np.concatenate([vals, 1e-3 * rng.random(long_row)])
    A = sp.csr_matrix((vals, (rows, cols)), shape=(n, n)) + sp.diags(3.0 + rng.random(n))
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    return A, rng.standard_normal(n), 0.1 * rng.standard_normal(n), 0.5 + rng.random(n)


def ks_for(memory, kmax=None):
    ks = sorted({k for k in KS + (memory, memory + 1, 2 * memory + 3)})
    return [k for k in ks if kmax is None or k <= kmax]


def device_prec(arch, P):
    if P is None:
        return None
    if np.isscalar(P):
        return npg.Diagonal(scalar=float(P))
    return npg.Diagonal(npg.on_architecture(arch, np.asarray(P)))


def one_solve(arch, dA, b, x0, n, memory, k, P, setup, eta):
    ws = npg.GmresWorkspace(arch.ctx, n, memory=memory)
    setup(ws)
    x = npg.on_architecture(arch, x0)
    st = ws.solve(dA, npg.on_architecture(arch, b), x, device_prec(arch, P), atol=0.0, rtol=0.0, itmax=k, reorth_eta=eta)
    return st, ws.history(), x.to_host(), ws.last_config()


def run_case(arch, name, A, dA, b, x0, memory, P, want, tol_h, tol_x, ks, setup=lambda ws: None, eta=0.1, mirror=None,
             loose=None, separate=True, reorth=None, prefix=None, solve_A=None):
    """mirror: restatement switches of the fp32 instances (None: the fp64 restatement, CGS2).  loose: (history, iterate) bars of
    the fp32 instance against the PLAIN fp64 restatement; separate: the plain restatement misses the mirror's history bar by at
    least 100x (the mirror tracks the device's rounding, not merely "fp32-ish").  reorth: "some" / "all" - the full kernels
    took a second Gram-Schmidt pass on some / every column of the largest k.  prefix: (kp, bar) - history entries 0..kp against
    the mirror at a tighter bar, which the plain restatement misses by at least 100x."""
    n = A.shape[0]
    kmax = max(ks)
    ref = gmres_steps(A, b, x0, memory, kmax, P=P, xs_at=tuple(ks), **(mirror or {}))
    plain = gmres_steps(A, b, x0, memory, kmax, P=P, xs_at=tuple(ks)) if mirror else ref
    r0 = true_residual(A, b, x0, P)
    worst_h = worst_x = worst_ph = worst_px = pre = pre_plain = 0.0
    for k in ks:
        st, hist, xk, cfg = one_solve(arch, dA if solve_A is None else solve_A, b, x0, n, memory, k, P, setup, eta)
        assert st["niter"] == k and len(hist) == k + 1, (name, k, st)
        for key, v in want.items():
            assert cfg[key] == v, (name, k, key, cfg[key], v, cfg)
        assert abs(hist[0] - r0) <= 1e-13 * r0, (name, hist[0], r0)              # R1 on x0
        dh = np.max(np.abs(hist - ref["hist"][:k + 1])) / hist[0]
        dx = np.max(np.abs(xk - ref["xs"][k])) / np.max(np.abs(ref["xs"][k]))
        worst_h, worst_x = max(worst_h, dh), max(worst_x, dx)
        if prefix:
            kp = min(k, prefix[0]) + 1
            pre = max(pre, np.max(np.abs(hist[:kp] - ref["hist"][:kp])) / hist[0])
            pre_plain = max(pre_plain, np.max(np.abs(hist[:kp] - plain["hist"][:kp])) / hist[0])
        if mirror:
            worst_ph = max(worst_ph, np.max(np.abs(hist - plain["hist"][:k + 1])) / hist[0])
            worst_px = max(worst_px, np.max(np.abs(xk - plain["xs"][k])) / np.max(np.abs(plain["xs"][k])))
    print(f"STEPS {name}: history {worst_h:.2e} iterate {worst_x:.2e}" +
          (f" | plain fp64 restatement: history {worst_ph:.2e} iterate {worst_px:.2e}" if mirror else "") +
          (f" | history 0..{prefix[0]}: {pre:.2e}, plain {pre_plain:.2e}" if prefix else "") +
          f" | nreorth {st['nreorth']} | {cfg}")
    # determinism: the largest k once more in a fresh workspace
    st2, hist2, x2, _ = one_solve(arch, dA if solve_A is None else solve_A, b, x0, n, memory, kmax, P, setup, eta)
    assert np.array_equal(hist2, hist) and np.array_equal(x2, xk), name
    if reorth == "all":
        assert st["nreorth"] == kmax, (name, st)
    elif reorth == "some":
        assert st["nreorth"] > 0, (name, st)
    if prefix:
        assert pre <= prefix[1] and pre_plain >= 100 * prefix[1], (name, pre, pre_plain)
    assert worst_h <= tol_h and worst_x <= tol_x, (name, worst_h, worst_x)
    if mirror:
        assert worst_ph <= loose[0] and worst_px <= loose[1], (name, worst_ph, worst_px)
        if separate:
            assert worst_ph >= 100 * tol_h, (name, worst_ph, tol_h)
    return cfg


# ---- fused organisation, plain CSR (n < 8192) ------------------------------------------------------------------------------
FUSED = [  # (n, memory, precond, long row, bars (history, iterate): within 30x of the measured maxima, 1e-15 where those are 0)
    (1, 1, "none", 0, (1e-15, 1e-15)), (2, 5, "scalar", 0, (1e-15, 4e-15)), (31, 5, "vector", 0, (3e-14, 1e-13)),
    (33, 8, "none", 0, (5e-14, 2e-14)), (511, 9, "scalar", 0, (4e-14, 2e-14)), (513, 20, "vector", 0, (1e-12, 2e-14)),
    (513, 30, "none", 0, (2e-11, 2e-14)), (8191, 1, "vector", 0, (3e-15, 6e-15)), (8191, 30, "scalar", 6000, (5e-11, 3e-14)),
]


def _prec(kind, dv):
    return {"none": None, "scalar": 0.37, "vector": dv}[kind]


@pytest.mark.parametrize("n,memory,prec,long_row,bars", FUSED, ids=[f"n{c[0]}-m{c[1]}-{c[2]}{'-longrow' if c[3] else ''}" for c in FUSED])
def test_fused_plain_csr(arch, n, memory, prec, long_row, bars):
    A, b, x0, dv = synth(n, n + memory, long_row)
    if long_row:
        assert np.diff(A.indptr).max() > 5824                 # longer than kTileNnz: the whole-workgroup long-row path
    dA = npg.on_architecture(arch, A)
    run_case(arch, f"fused n={n} m={memory} {prec}", A, dA, b, x0, memory, _prec(prec, dv),
             dict(split=0, basis=64, xg=0, windowed=0, pk9=0, distributed=0), bars[0], bars[1], ks_for(memory, kmax=n))


# ---- split organisation, synthetic ------------------------------------------------------------------------------------------
SPLIT = [  # (name, n, memory, precond, setup, eta, want, mirror, bars (history, iterate), plain-fp64 bars, lanes)
    ("fp64-full", 20001, 30, "vector", dict(split=1, basis=64), 0.9, dict(basis=64, fast=0), None, (1e-15, 1e-14), None, 0),
    ("fp64-full-even", 20000, 9, "scalar", dict(split=1, basis=64), 0.9, dict(basis=64, fast=0), None, (8e-15, 1e-14), None, 0),
    ("fp64-fast", 20001, 30, "none", dict(split=1, basis=64), 0.1, dict(basis=64, fast=1), None, (5e-12, 1.5e-14), None, 0),
    ("fp32-fast-xg0", 20001, 30, "vector", dict(split=1, basis=32, gather=0), 0.1, dict(basis=32, fast=1, xg=0),
     dict(basis32=True, passes=1, pyth_eta=0.1), (1e-9, 1e-8), (3e-5, 1e-6), 0),
    ("fp32-full", 20001, 30, "scalar", dict(split=1, basis=32, gather=0), 2.0, dict(basis=32, fast=0, xg=0),
     dict(basis32=True, passes=2), (1e-10, 1e-8), (1e-7, 1e-6), 0),
    ("xg2-plain-csr", 120001, 20, "vector", dict(split=1, basis=32), 0.1, dict(basis=32, fast=1, xg=2),
     dict(basis32=True, gather32=True, passes=1, pyth_eta=0.1), (1e-10, 3e-10), (1e-6, 1e-6), 0),
    ("fp64-beyond-row-grid", 400001, 20, "scalar", dict(split=1, basis=64), 0.9, dict(basis=64, fast=0), None, (3e-14, 1e-14), None, 0),
    ("fp32-beyond-row-pair-grid", 400001, 20, "vector", dict(split=1, basis=32, gather=0), 0.1, dict(basis=32, fast=1, xg=0),
     dict(basis32=True, passes=1, pyth_eta=0.1), (3e-9, 3e-8), (1e-7, 1e-6), 0),
    ("lanes4", 20001, 9, "none", dict(split=1, basis=64), 0.1, dict(L=4), None, (1e-13, 3e-14), None, 4),
    ("lanes8", 20001, 9, "scalar", dict(split=1, basis=64), 0.1, dict(L=8), None, (1e-13, 3e-14), None, 8),
    ("lanes16", 20001, 9, "vector", dict(split=1, basis=64), 0.1, dict(L=16), None, (1e-13, 3e-14), None, 16),
    ("lanes32", 20001, 9, "none", dict(split=1, basis=64), 0.1, dict(L=32), None, (1e-13, 3e-14), None, 32),
]


def _setup(kw):
    def f(ws):
        if "split" in kw:
            ws.set_split(kw["split"])
        if "basis" in kw:
            ws.set_basis(kw["basis"])
        if "gather" in kw:
            ws.set_gather(kw["gather"])
    return f


@pytest.mark.parametrize("case", SPLIT, ids=[c[0] for c in SPLIT])
def test_split_synthetic(arch, case):
    name, n, memory, prec, setup, eta, want, mirror, bars, loose, lanes = case
    A, b, x0, dv = synth(n, n % 1000 + memory)
    dA = npg.on_architecture(arch, A)
    if lanes:
        dA.set_lanes(lanes)
    ks = ks_for(memory) if n < 100000 else [memory, memory + 1, 2 * memory + 3]
    cfg = run_case(arch, f"split {name} n={n} m={memory} {prec}", A, dA, b, x0, memory, _prec(prec, dv),
                   dict(split=1, pk9=0, distributed=0, **want), bars[0], bars[1], ks, setup=_setup(setup), eta=eta, mirror=mirror,
                   loose=loose, separate=n < 400000, reorth=("all" if eta > 1 else "some") if want.get("fast") == 0 else None)
    if n > 400000:
        # more rows than one grid of the row kernels (768 x 256 rows, 768 x 512 row pairs) and more tiles than the Arnoldi grid
        assert cfg["row_grid"] * 256 * (2 if cfg["basis"] == 32 else 1) < n and cfg["tiles"] > cfg["grid"], cfg


def test_fast_kernels_then_safe_mode(arch):
    """I + 1e-3 R (test_gmres_fast_mode_falls_back_when_a_second_pass_is_due): the first solve of a workspace runs the fast kernels
    and flags the columns that were due a second pass; the next solve of the SAME workspace runs the full kernels - both step by
    step against the fp64 restatement"""
    rng = np.random.default_rng(42)
    n = 600
    A = sp.csr_matrix(sp.eye(n) + 1e-3 * sp.random(n, n, density=0.05, random_state=rng, format="csr"))
    b, x0 = rng.standard_normal(n), 0.1 * rng.standard_normal(n)
    dA, db = npg.on_architecture(arch, A), npg.on_architecture(arch, b)
    ws = npg.GmresWorkspace(arch.ctx, n, memory=30)
    ws.set_split(1)
    k = 4                                          # (the residual falls by 1e-3 per step: four steps reach 1e-12)
    ref = gmres_steps(A, b, x0, 30, k)
    for solve, fast in ((0, 1), (1, 0)):
        x = npg.on_architecture(arch, x0)
        st = ws.solve(dA, db, x, None, atol=0.0, rtol=0.0, itmax=k)
        cfg = ws.last_config()
        assert cfg["split"] == 1 and cfg["fast"] == fast and cfg["basis"] == 64, cfg
        assert (st["nflagged"] > 0) if fast else (st["nreorth"] > 0 and st["nflagged"] == 0), st
        dh = np.max(np.abs(ws.history() - ref["hist"])) / ref["hist"][0]
        dx = np.max(np.abs(x.to_host() - ref["x"])) / np.max(np.abs(ref["x"]))
        print(f"STEPS safe-mode switch, solve {solve} (fast {fast}): history {dh:.2e} iterate {dx:.2e}")
        assert dh <= 5e-15 and dx <= 1e-14, (solve, dh, dx)


def _halo_setup(arch, n, keep):
    from nupgcm_amd import distributed
    plan = dict(peers=np.zeros(0, np.int32), send_ptr=np.zeros(1, np.int64), send_idx=np.zeros(0, np.int32),
                recv_ptr=np.zeros(1, np.int64))

    def f(ws):
        halo = distributed.Halo(arch.ctx, n, 0, plan)
        keep.append(halo)
        L.check(L.lib().npg_gmres_set_halo(ws.h, halo.h))
    return f


@pytest.mark.parametrize("n,memory", [(20001, 9), (12001, 20)])
def test_one_rank_distributed(arch, n, memory):
    """the distributed code path with no peers: Pythagorean norms (pyth), partial rows folded to one row (fold_rows)"""
    A, b, x0, dv = synth(n, 5 + memory)
    dA = npg.on_architecture(arch, A)
    keep = []
    run_case(arch, f"one-rank distributed n={n} m={memory}", A, dA, b, x0, memory, dv, dict(distributed=1, pyth=1, fast=1, split=1),
             1e-13, 2e-14, ks_for(memory), setup=_halo_setup(arch, n, keep))


# ---- profile mode and the graph cache ---------------------------------------------------------------------------------------
PROFILE = [  # (name, n, memory, setup, distributed, want)
    ("fused", 513, 5, dict(), False, dict(split=0)),
    ("split-fp64", 20001, 9, dict(split=1, basis=64), False, dict(split=1, basis=64, fusedrows=0)),
    ("split-fp32", 20001, 9, dict(split=1, basis=32), False, dict(split=1, basis=32, fusedrows=1)),
    ("one-rank-distributed", 12001, 9, dict(), True, dict(distributed=1, split=1)),
]


@pytest.mark.parametrize("case", PROFILE, ids=[c[0] for c in PROFILE])
def test_profile_mode_same_bits(arch, case):
    """set_profile(True) (eager launches, the Arnoldi kernels timed by events: what bench.py --full takes its roofline figure from)
    changes no bit: two full cycles and a third that stops at itmax, against the same solve replayed from the captured graphs.
    The two full cycles are the ones counted: 2 * memory timed launches."""
    name, n, memory, setup, distributed, want = case
    A, b, x0, dv = synth(n, 11 + memory)
    dA = npg.on_architecture(arch, A)
    keep, profiled = [], []
    base = _halo_setup(arch, n, keep) if distributed else _setup(setup)

    def with_profile(ws):
        base(ws)
        ws.set_profile(True)
        profiled.append(ws)

    k = 2 * memory + 3
    st, hist, x, cfg = one_solve(arch, dA, b, x0, n, memory, k, dv, base, 0.1)
    stp, histp, xp, cfgp = one_solve(arch, dA, b, x0, n, memory, k, dv, with_profile, 0.1)
    for key, v in want.items():
        assert cfg[key] == v, (name, key, cfg)
    assert st["niter"] == k and len(hist) == k + 1, (name, st)
    assert np.array_equal(histp, hist) and np.array_equal(xp, x), name
    for key in ("niter", "nreorth", "nflagged", "status"):
        assert stp[key] == st[key], (name, key, stp, st)
    assert cfgp == cfg, (name, cfgp, cfg)
    ms, launches = profiled[0].get_profile()
    assert ms > 0.0 and launches == 2 * memory, (name, ms, launches)


def test_lanes_change_recaptures(arch):
    """npg_csr_set_lanes between two solves of ONE workspace with the SAME device vectors (no kernel argument changes): the captured
    cycle has the lane instance baked in, so the second solve has to capture again - it is, bit for bit, a fresh workspace's solve
    at the new lane count"""
    n, memory = 20001, 9
    A, b, x0, _ = synth(n, 3 + memory)
    dA, db, x = npg.on_architecture(arch, A), npg.on_architecture(arch, b), npg.on_architecture(arch, x0)
    setup = _setup(dict(split=1, basis=64))
    k = 2 * memory + 3
    ws = npg.GmresWorkspace(arch.ctx, n, memory=memory)
    setup(ws)
    for lanes in (4, 32):
        dA.set_lanes(lanes)
        x.upload(x0)
        ws.solve(dA, db, x, None, atol=0.0, rtol=0.0, itmax=k, reorth_eta=0.1)
        assert ws.last_config()["L"] == lanes, ws.last_config()
    hist, x = ws.history(), x.to_host()
    _, hist32, x32, cfg32 = one_solve(arch, dA, b, x0, n, memory, k, None, setup, 0.1)
    assert cfg32["L"] == 32, cfg32
    assert np.array_equal(hist, hist32) and np.array_equal(x, x32)


# ---- inversion matrices (bowl3D) -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bowl():
    fed, prm, frc, dt, b0 = build_fe_data("bowl_mixing")
    return fed, prm


def _inversion(arch, fed, prm, env=None):
    old = {}
    for k, v in (env or {}).items():
        old[k] = os.environ.get(k)
        os.environ[k] = v
    try:
        A = npg.build_A_inversion(arch, fed, prm, 1.0)
        ref = A.to_scipy_csr()
        d = fed.dofs
        assert A.block_nodes(d.n_full, d.n_surf)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    return A, ref


def _inv_rhs(ref, seed):
    rng = np.random.default_rng(seed)
    n = ref.shape[0]
    return ref @ np.cos(np.arange(n, dtype=float)) * 1e-3, 1e-4 * rng.standard_normal(n)


INV = [  # (name, env at the matrix build, setup, want, memory, bars (history, iterate))
    ("xg1-ordinary-tiles", None, dict(basis=32, gather=2), dict(xg=1, windowed=0), 20, (3e-15, 6e-14)),
    ("xg1-windowed-wl4", {"NPG_SPMV_WLANES": "4"}, dict(basis=32), dict(xg=1, windowed=1, wl=4, word=0), 20, (3e-15, 6e-14)),
    ("xg1-windowed-wl8", {"NPG_SPMV_WLANES": "8"}, dict(basis=32), dict(xg=1, windowed=1, wl=8, word=0), 9, (3e-15, 4e-14)),
]


@pytest.mark.parametrize("case", INV, ids=[c[0] for c in INV])
def test_inversion_gather_layout(arch, bowl, case):
    name, env, setup, want, memory, bars = case
    fed, prm = bowl
    A, ref = _inversion(arch, fed, prm, env)
    h = fed.mesh.median_edge_length()
    b, x0 = _inv_rhs(ref, 3)
    P = 1 / h ** 3
    run_case(arch, f"bowl h=0.1 {name} m={memory}", ref, A, b, x0, memory, P, dict(split=1, basis=32, fast=1, pk9=0, **want),
             bars[0], bars[1], ks_for(memory), setup=_setup(setup), mirror=dict(basis32=True, gather32=True, passes=1, pyth_eta=0.1),
             loose=(1e-7, 3e-6))


def test_inversion_fp64(arch, bowl):
    """split fp64 basis, full kernels (second passes taken), the plain-CSR inversion matrix and the node-blocked one at two lane
    counts"""
    fed, prm = bowl
    A, ref = _inversion(arch, fed, prm)
    h = fed.mesh.median_edge_length()
    b, x0 = _inv_rhs(ref, 4)
    setup = _setup(dict(split=1, basis=64))
    for lanes in (4, 32):
        A.set_lanes(lanes)
        run_case(arch, f"bowl h=0.1 fp64-full node-blocked L={lanes}", ref, A, b, x0, 20, 1 / h ** 3,
                 dict(split=1, basis=64, fast=0, xg=0, L=lanes), 3e-15, 1e-13, ks_for(20), setup=setup, eta=0.9, reorth="some")
    A.set_lanes(0)


N9_XG = (0, 1)              # full node records: the SpMV input in fp64 / from the fp32 gather copy


def test_inversion_full_node_records(arch, bowl):
    """pack_nodes on the full-stress matrix of a function-valued viscosity: the N9 instances, gather copy off and on"""
    fed, prm = bowl
    d = fed.dofs
    nu = lambda x: 1.0 + 0.5 * np.sin(3.0 * x[..., 0]) * np.cos(2.0 * x[..., 2])
    A = npg.build_A_inversion(arch, fed, prm, nu, structural=True)
    ref = A.to_scipy_csr()
    assert A.pack_nodes(d.n_full, d.n_surf)
    h = fed.mesh.median_edge_length()
    b, x0 = _inv_rhs(ref, 5)
    for xg in N9_XG:
        if xg == 0:
            run_case(arch, "bowl h=0.1 N9 fp64", ref, A, b, x0, 9, 1 / h ** 3, dict(split=1, pk9=1, xg=0, basis=64), 8e-16, 1e-13,
                     ks_for(9), setup=_setup(dict(basis=64)), eta=0.9, reorth="some")
        else:
            run_case(arch, "bowl h=0.1 N9 xg1", ref, A, b, x0, 9, 1 / h ** 3, dict(split=1, pk9=1, xg=1, basis=32, fast=1), 3e-15,
                     6e-14, ks_for(9), setup=_setup(dict(basis=32, gather=1)),
                     mirror=dict(basis32=True, gather32=True, passes=1, pyth_eta=0.1), loose=(1e-7, 3e-6))


def test_inversion_distributed_one_rank(arch, bowl):
    fed, prm = bowl
    A, ref = _inversion(arch, fed, prm)
    h = fed.mesh.median_edge_length()
    b, x0 = _inv_rhs(ref, 6)
    keep = []
    run_case(arch, "bowl h=0.1 one-rank distributed", ref, A, b, x0, 20, 1 / h ** 3, dict(distributed=1, pyth=1, split=1), 3e-14, 1e-13,
             ks_for(20), setup=_halo_setup(arch, ref.shape[0], keep))


def test_inversion_h004_beyond_one_grid(arch):
    """bowl3D h = 0.04 (~270 k unknowns): more windowed tiles than the Arnoldi grid (a workgroup loops over several tiles) and more
    rows than one grid of the fp64 row kernels"""
    from nupgcm_amd import workloads
    fed = workloads.example_fe_data(workloads.bowl_mesh_model("bowl3D_h0.04"))
    prm, _ = workloads.example_parameters()
    A, ref = _inversion(arch, fed, prm)
    h = fed.mesh.median_edge_length()
    b, x0 = _inv_rhs(ref, 7)
    n = ref.shape[0]
    info = A.window_info()
    cfg = run_case(arch, f"bowl h=0.04 xg1 windowed n={n}", ref, A, b, x0, 20, 1 / h ** 3, dict(split=1, xg=1, windowed=1), 1e-9, 1e-6,
                   [1, 2, 20, 21, 43], setup=_setup(dict(basis=32)), mirror=dict(basis32=True, gather32=True, passes=1, pyth_eta=0.1),
                   loose=(1e-8, 1e-5), separate=False, prefix=(2, 2e-14))
    assert info["tiles"] == cfg["tiles"] > cfg["grid"], (info, cfg)
    cfg = run_case(arch, f"bowl h=0.04 fp64 n={n}", ref, A, b, x0, 20, 1 / h ** 3, dict(split=1, basis=64, xg=0), 3e-15, 3e-13,
                   [20, 21], setup=_setup(dict(basis=64)), eta=0.9, reorth="some")
    assert n > 768 * 256 and cfg["row_grid"] * 256 < n, cfg


ORD_CASES = [(4, (3e-15, 6e-14)), (8, (3e-15, 6e-14))]        # (WL, bars (history, iterate))


def test_windowed_ord_instances(arch, bowl, tmp_path):
    """the windowed instances WITH ordinary tiles (ORD): NPG_WIN_ORD=1 is read once per process, so one child process
    (tests/gmres_ord_worker.py) runs the solves on bowl3D h = 0.1 with WL = 4 and 8; the comparisons are made here"""
    import subprocess
    import sys
    fed, prm = bowl
    _, ref = _inversion(arch, fed, prm)
    h = fed.mesh.median_edge_length()
    b, x0 = _inv_rhs(ref, 8)
    memory, ks = 20, ks_for(20)
    out = str(tmp_path / "ord")
    np.savez(out + ".in.npz", b=b, x0=x0)
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "gmres_ord_worker.py"), out, str(memory), ",".join(map(str, ks))],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = np.load(out + ".out.npz")
    P = 1 / h ** 3
    mir = gmres_steps(ref, b, x0, memory, max(ks), P=P, xs_at=tuple(ks), basis32=True, gather32=True, passes=1, pyth_eta=0.1)
    plain = gmres_steps(ref, b, x0, memory, max(ks), P=P, xs_at=tuple(ks))
    r0 = true_residual(ref, b, x0, P)
    for wl, bars in ORD_CASES:
        A = sp.csr_matrix((res[f"wl{wl}_data"], res[f"wl{wl}_indices"], res[f"wl{wl}_indptr"]), shape=ref.shape)
        assert (A != ref).nnz == 0                                 # the child assembled the same matrix
        dh = dx = ph = 0.0
        for k in ks:
            hist, xk = res[f"wl{wl}_k{k}_r0_hist"], res[f"wl{wl}_k{k}_r0_x"]
            cfg = dict(zip(npg.GmresWorkspace.CONFIG_KEYS, res[f"wl{wl}_k{k}_r0_cfg"].tolist()))
            want = dict(split=1, basis=32, fast=1, xg=1, windowed=1, wl=wl, word=1, pk9=0, distributed=0)
            assert {key: cfg[key] for key in want} == want, (wl, k, cfg)
            assert int(res[f"wl{wl}_k{k}_r0_niter"]) == k and len(hist) == k + 1
            assert abs(hist[0] - r0) <= 1e-13 * r0
            dh = max(dh, np.max(np.abs(hist - mir["hist"][:k + 1])) / hist[0])
            dx = max(dx, np.max(np.abs(xk - mir["xs"][k])) / np.max(np.abs(mir["xs"][k])))
            ph = max(ph, np.max(np.abs(hist - plain["hist"][:k + 1])) / hist[0])
        kmax = max(ks)
        assert np.array_equal(res[f"wl{wl}_k{kmax}_r1_hist"], res[f"wl{wl}_k{kmax}_r0_hist"])
        assert np.array_equal(res[f"wl{wl}_k{kmax}_r1_x"], res[f"wl{wl}_k{kmax}_r0_x"])
        print(f"STEPS bowl h=0.1 xg1-windowed-wl{wl}-ORD m={memory}: history {dh:.2e} iterate {dx:.2e} | plain fp64 restatement: "
              f"history {ph:.2e}")
        assert dh <= bars[0] and dx <= bars[1], (wl, dh, dx)
        assert ph >= 100 * bars[0], (wl, ph)


# ---- the ghost slots of a rank's row block in the stand-alone gather-layout product ----------------------------------------
def test_windowed_product_of_a_row_block_with_ghost_nodes(arch, bowl):
    """npg_spmv_gather32(windowed=1) on rank 0's row block of a 2-rank node partition with ghost nodes (npg_csr_set_ghost_nodes,
    then block_nodes, as partition.py builds it): the windowed tiles read ghost columns from their node slots of the fp32 copy,
    which the product has to fill - it equals the fp64 product of the fp32-rounded vector"""
    from nupgcm_amd import partition
    fed, prm = bowl
    Ag = npg.build_A_inversion(arch, fed, prm, 1.0).to_scipy_csr()
    part = partition.NodePartition(fed, 2)
    lay = partition.RankLayout(fed, part, 0)
    Pr = Ag[lay.inv.owned]
    lc = lay.inv.lut[Pr.indices]
    assert (lc >= 0).all() and (lc < lay.inv.n_sol).all()
    Al = sp.csr_matrix((Pr.data, lc, Pr.indptr), shape=(lay.inv.n_own, lay.inv.n_sol))
    Al.sort_indices()
    A = npg.on_architecture(arch, Al)
    first, ncomp = lay.ghost_nodes(fed)
    assert len(first) > 0
    A.set_ghost_nodes(first, ncomp)
    assert A.block_nodes(*part.local_nodes(0)) and A.window_info()["tiles"] > 0
    rng = np.random.default_rng(11)
    x = rng.standard_normal(Al.shape[1])
    xr = x.astype(np.float32).astype(np.float64)
    want = A.mul(npg.on_architecture(arch, xr)).to_host()
    assert np.max(np.abs(want - Al @ xr)) <= 1e-13 * np.max(np.abs(want))
    yw = A.mul_gather32(npg.on_architecture(arch, x), windowed=True).to_host()
    err = np.linalg.norm(yw - want) / np.linalg.norm(want)
    print(f"STEPS ghost-node windowed product: rel {err:.2e} ({len(first)} ghost nodes)")
    assert err < 1e-13, err


# ---- coverage ------------------------------------------------------------------------------------------------------------------
# The Arnoldi instances launch_arnoldi_split (gmres.hip, "static void launch_arnoldi_split": nine branches) and the fused launch in
# launch_cycle_L can dispatch on one GPU, as last_config() keys (split, xg, pk9, windowed, wl, word).  word (ORD) is set by
# gmres_plan as NPG_WIN_ORD || (no row tiles in the windowed set && rows behind the block rows); the bowl inversion matrices
# have row tiles, so the ORD instances run in the child process of test_windowed_ord_instances.  Row kernels (launch_rows_kernel):
# NG = (j + 8) / 8 for j < memory, basis 64 / 32, fast or full orthogonalisation - reached by every split case with memory >= 25 at
# k = 2 memory + 3.
ARNOLDI = {   # (split, xg, pk9, windowed, wl, word)
    (0, 0, 0, 0, 0, 0): "k_gmres_arnoldi<L, true> (fused)",
    (1, 0, 0, 0, 0, 0): "k_gmres_arnoldi<L, false>",
    (1, 0, 1, 0, 0, 0): "k_gmres_arnoldi<L, false, 0, true> (N9)",
    (1, 1, 1, 0, 0, 0): "k_gmres_arnoldi<L, false, 1, true> (N9, XG 1)",
    (1, 2, 0, 0, 0, 0): "k_gmres_arnoldi<L, false, 2> (plain CSR, XG 2)",
    (1, 1, 0, 0, 0, 0): "k_gmres_arnoldi<L, false, 1> (ordinary tiles)",
    (1, 1, 0, 1, 4, 0): "k_gmres_arnoldi<L, false, 1, false, 4, false>",
    (1, 1, 0, 1, 8, 0): "k_gmres_arnoldi<L, false, 1, false, 8, false>",
    (1, 1, 0, 1, 4, 1): "k_gmres_arnoldi<L, false, 1, false, 4, true> (ORD)",
    (1, 1, 0, 1, 8, 1): "k_gmres_arnoldi<L, false, 1, false, 8, true> (ORD)",
}
ROWS = {(64, 1), (64, 0), (32, 1), (32, 0)}          # (basis, fast), each with NG 1..4
LANES = {4, 8, 16, 32}


def test_instance_coverage():
    """every case above declares (and asserts through last_config) the instance it covers; together they cover every instance the
    dispatch can select on one GPU - a new instance has to be added to ARNOLDI and get a case"""
    arn, rows, lanes = set(), set(), set()
    arn.add((0, 0, 0, 0, 0, 0))                           # FUSED
    for c in SPLIT:
        w = c[6]
        arn.add((1, w.get("xg", 0), 0, 0, 0, 0))
        if c[2] >= 25:
            rows.add((w.get("basis", 64), w.get("fast", 1 if c[5] <= 0.1 else 0)))
        if c[10]:
            lanes.add(c[10])
    for c in INV:
        w = c[3]
        arn.add((1, w["xg"], 0, w["windowed"], w.get("wl", 0), w.get("word", 0)))
    for xg in N9_XG:                                      # test_inversion_full_node_records
        arn.add((1, xg, 1, 0, 0, 0))
    for wl, _ in ORD_CASES:                               # test_windowed_ord_instances
        arn.add((1, 1, 0, 1, wl, 1))
    assert arn == set(ARNOLDI), ({ARNOLDI[k] for k in set(ARNOLDI) - arn}, arn - set(ARNOLDI))
    assert len(ARNOLDI) == 10                             # fused + the nine branches of launch_arnoldi_split
    assert ROWS <= rows, ROWS - rows
    assert LANES <= lanes, LANES - lanes
