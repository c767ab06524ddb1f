"""The 20-column instance of the resident fused row launch changes no bit of any result (csrc/gmres.hip).

Steps of 17-20 basis columns (j = 16..19) of the one-GPU, split, fast, fp32-basis cycle run k_gmres_rows_fused<20>, which splits its
dots pass by columns (columns 0..9, then columns 10..19 with w and wt) and keeps a thread's last B = 2 trips on chip: columns 0..9
in L = 2 LDS slots, columns 10..19 and the w pair in registers.  NPG_GMRES_FUSED_COLS=16 keeps the separate launches for those
steps, NPG_GMRES_FUSEDROWS=0 for all of them.  Partial rows, fold order, the expression of the basis column and every summation
order are the same, so residual history, iterate, niter / nreorth / nflagged / status and every entry of last_config() (but
`fusedrows` against the separate launches) are compared with np.array_equal - no tolerance - and fused_cols() proves which
instance ran.  One fresh child process per arrangement (tests/gmres_fusedcols_worker.py lists the solves and the trip counts they
are chosen for: nt = 0, 1, B, B + 1, B + 2 and 6-7); the three run side by side, once per module."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import nupgcm_amd as npg  # noqa: E402
from tests.gmres_fusedcols_worker import BIG_KS, ONE_KS, TRIP_KS, TRIP_NS  # noqa: E402

KEYS = npg.GmresWorkspace.CONFIG_KEYS
MODES = ("sep", "c16", "c20")
COLS = {"sep": 0, "c16": 16, "c20": 20}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    here = os.path.dirname(os.path.abspath(__file__))
    tmp = tmp_path_factory.mktemp("fusedcols")
    procs = []
    for mode in MODES:
        out = str(tmp / f"{mode}.npz")
        procs.append((out, subprocess.Popen([sys.executable, os.path.join(here, "gmres_fusedcols_worker.py"), out, mode],
                                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    res = {}
    for mode, (out, p) in zip(MODES, procs):
        log, _ = p.communicate(timeout=600)
        assert p.returncode == 0, log[-3000:]
        res[mode] = dict(np.load(out))
    return res


def cfg_of(r, key):
    return dict(zip(KEYS, r[key + "_cfg"].tolist()))


def same(runs, prefix, n, memory, row_grid, ks):
    """every solve `prefix`k is the same in the three arrangements, ran the instance its arrangement names and made k iterations;
    returns the default arrangement's results"""
    assert KEYS[-1] == "fusedrows"
    for k in ks:
        key = f"{prefix}{k}"
        for mode in MODES:
            r = runs[mode]
            cfg = cfg_of(r, key)
            assert cfg["split"] == 1 and cfg["basis"] == 32 and cfg["fast"] == 1 and cfg["xg"] == 0, (mode, cfg)
            assert cfg["n"] == n and cfg["memory"] == memory and cfg["row_grid"] == row_grid, (mode, cfg)
            assert cfg["fusedrows"] == (0 if mode == "sep" else 1), (mode, cfg)
            assert r[key + "_cols"][0] == COLS[mode], (mode, key, r[key + "_cols"])
            assert r[key + "_stats"][0] == k and len(r[key + "_hist"]) == k + 1, (mode, key, r[key + "_stats"])
        ref = runs["c20"]
        for mode in ("sep", "c16"):
            for what in ("hist", "x", "stats"):
                a, b = runs[mode][f"{key}_{what}"], ref[f"{key}_{what}"]
                assert a.shape == b.shape and np.array_equal(a, b), (mode, key, what, a, b)
            a, b = runs[mode][key + "_cfg"], ref[key + "_cfg"]
            if mode == "sep":
                a, b = a[:-1], b[:-1]
            assert np.array_equal(a, b), (mode, key, a, b)
    return runs["c20"]


@pytest.mark.parametrize("memory", sorted(ONE_KS))
def test_one_trip_odd_n(runs, memory):
    """n = 20 001: 40 row-pair blocks, one trip per thread.  Memory 20: a solve ends on each step of the new instance, on the cycle
    boundary and in the second cycle; 18: the cycle ends inside its range; 30: steps 16..19 fused, j >= 20 separate launches"""
    ks = ONE_KS[memory]
    r = same(runs, f"one_m{memory}_k", 20001, memory, 40, ks)
    hist = r[f"one_m{memory}_k{ks[-1]}_hist"][:memory + 1]
    assert np.all(np.diff(hist) <= 0.0) and hist[-1] < hist[0], hist   # (real solves: the estimate never rises within a cycle)


@pytest.mark.parametrize("n", TRIP_NS)
def test_trip_boundaries(runs, n):
    """64 workgroups: exactly B = 2 trips everywhere (n = 65 535), one workgroup with a one-row third trip whose first trip is read
    again (65 537), three and four trips (98 305)"""
    same(runs, f"trip_n{n}_k", n, 20, 64, TRIP_KS)


def test_many_trips_and_replay(runs):
    """n = 200 001: 391 row-pair blocks on 64 workgroups, six or seven trips; every solve twice in one workspace"""
    for rep in (0, 1):
        same(runs, f"big_r{rep}_k", 200001, 20, 64, BIG_KS)
    for mode in MODES:
        r = runs[mode]
        for k in BIG_KS:
            for what in ("hist", "x", "stats", "cfg", "cols"):
                assert np.array_equal(r[f"big_r0_k{k}_{what}"], r[f"big_r1_k{k}_{what}"]), (mode, k, what)
