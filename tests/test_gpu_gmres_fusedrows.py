"""NPG_GMRES_FUSEDROWS changes no bit of any result (csrc/gmres.hip).

With the switch on (the default) a step of the one-GPU, split, fast, fp32-basis cycle runs its Gram-Schmidt sums, their fold and the
update as one resident launch (k_gmres_rows_fused), which keeps a thread's last trips on chip across a grid-wide hand-off; with
NPG_GMRES_FUSEDROWS=0 it runs k_gmres_dots_rows, k_gmres_fold_first and k_gmres_orth_rows (and with NPG_GMRES_ONEFOLD=0 as well,
the two row kernels without the fold kernel).  Partial rows, fold order, the expression of the basis column and the order of the
norm's sums are the same, so residual history, iterate, niter / nreorth / nflagged / status and every entry of last_config() but
`fusedrows` itself are compared with np.array_equal - no tolerance.  One fresh child process per arrangement
(tests/gmres_fusedrows_worker.py, which lists the solves); the three run side by side, once per module."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import nupgcm_amd as npg  # noqa: E402
from tests.gmres_fusedrows_worker import BIG_KS, INV_KS, SYN30_KS, SYN_KS  # noqa: E402

KEYS = npg.GmresWorkspace.CONFIG_KEYS
ARRANGEMENTS = (("0", "1"), ("1", "1"), ("0", "0"))      # (NPG_GMRES_FUSEDROWS, NPG_GMRES_ONEFOLD): separate, fused, pre-fold


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    here = os.path.dirname(os.path.abspath(__file__))
    tmp = tmp_path_factory.mktemp("fusedrows")
    procs = []
    for fr, of in ARRANGEMENTS:
        out = str(tmp / f"fr{fr}_of{of}.npz")
        procs.append((out, subprocess.Popen([sys.executable, os.path.join(here, "gmres_fusedrows_worker.py"), out, fr, of],
                                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    res = []
    for out, p in procs:
        log, _ = p.communicate(timeout=600)
        assert p.returncode == 0, log[-3000:]
        res.append(dict(np.load(out)))
    return res


def cfg_of(r, key):
    return dict(zip(KEYS, r[key + "_cfg"].tolist()))


def same(runs, prefix, fused):
    """every array of every solve under `prefix` is the same in the three arrangements (last_config: but for `fusedrows`, which is
    `fused` in the fused arrangement and 0 in the others); returns the fused arrangement's results"""
    assert KEYS[-1] == "fusedrows"
    off, on, pre = runs
    keys = sorted(k for k in off if k.startswith(prefix))
    assert keys and keys == sorted(k for k in on if k.startswith(prefix)) == sorted(k for k in pre if k.startswith(prefix)), prefix
    for k in keys:
        for other in (off, pre):
            a, b = other[k], on[k]
            if k.endswith("_cfg"):
                assert a[-1] == 0 and b[-1] == fused, (k, a, b)
                a, b = a[:-1], b[:-1]
            assert a.shape == b.shape and np.array_equal(a, b), (k, a, b)
    return on


@pytest.mark.parametrize("name,want", [("win", dict(xg=1, windowed=1)), ("ord", dict(xg=1, windowed=0))])
def test_bowl_inversion(runs, name, want):
    r = same(runs, f"inv_{name}_", 1)
    for k in INV_KS:
        cfg = cfg_of(r, f"inv_{name}_k{k}")
        assert {key: cfg[key] for key in want} == want and cfg["split"] == 1 and cfg["basis"] == 32 and cfg["fast"] == 1, cfg
        assert r[f"inv_{name}_k{k}_stats"][0] == k and len(r[f"inv_{name}_k{k}_hist"]) == k + 1
    assert sum(k % 20 != 0 for k in INV_KS) >= 3                     # (solves that end in the middle of a cycle)
    niter, _, nflagged, status = r[f"inv_{name}_k0_stats"]
    hist = r[f"inv_{name}_k0_hist"]
    assert status == 1 and len(hist) == niter + 1 and hist[-1] <= 1e-6 * hist[0], (niter, status, hist[-1] / hist[0])


@pytest.mark.parametrize("name,memory,ks", [("m20", 20, SYN_KS), ("m30", 30, SYN30_KS)])
def test_synthetic_odd_n_one_trip(runs, name, memory, ks):
    r = same(runs, f"syn_{name}_", 1)
    for k in ks:
        cfg = cfg_of(r, f"syn_{name}_k{k}")
        assert cfg["split"] == 1 and cfg["basis"] == 32 and cfg["fast"] == 1 and cfg["xg"] == 0 and cfg["memory"] == memory, cfg
        assert cfg["n"] == 20001 and cfg["row_grid"] == 40, cfg       # (40 row-pair blocks: one trip per thread)
        assert r[f"syn_{name}_k{k}_stats"][0] == k
    hist = r[f"syn_{name}_k{ks[-1]}_hist"][:memory + 1]
    assert np.all(np.diff(hist) <= 0.0) and hist[-1] < hist[0], hist   # (real solves: the estimate never rises within a cycle)


def test_several_trips_not_all_kept(runs):
    r = same(runs, "big_r", 1)
    for k in BIG_KS:
        cfg = cfg_of(r, f"big_r0_k{k}")
        assert cfg["fusedrows"] == 1 and cfg["basis"] == 32 and cfg["fast"] == 1 and cfg["memory"] == 20, cfg
        assert cfg["n"] == 200001 and cfg["row_grid"] == 64, cfg      # (391 row-pair blocks on 64 workgroups: 6 or 7 trips)
        assert r[f"big_r0_k{k}_stats"][0] == k


def test_repeatable(runs):
    """the hand-off state only ever grows: a second run of every solve in the same process (graph replays, then a new solve)"""
    for r in runs:
        for k in BIG_KS:
            for what in ("hist", "x", "stats", "cfg"):
                assert np.array_equal(r[f"big_r0_k{k}_{what}"], r[f"big_r1_k{k}_{what}"]), (k, what)


def test_fallbacks(runs):
    r = same(runs, "syn_b64_", 0)
    assert cfg_of(r, "syn_b64_k9")["basis"] == 64
    r = same(runs, "safe_", 0)
    for solve, fast in ((0, 1), (1, 0)):
        cfg = cfg_of(r, f"safe_s{solve}")
        niter, nreorth, nflagged, _ = r[f"safe_s{solve}_stats"]
        assert cfg["split"] == 1 and cfg["fast"] == fast and cfg["fusedrows"] == 0, cfg
        assert niter == 4 and ((nflagged > 0) if fast else (nreorth > 0 and nflagged == 0)), r[f"safe_s{solve}_stats"]
    r = same(runs, "dist_", 0)
    cfg = cfg_of(r, "dist_k23")
    assert cfg["distributed"] == 1 and cfg["fusedrows"] == 0 and r["dist_k23_stats"][0] == 23, cfg
