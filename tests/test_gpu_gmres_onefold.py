"""NPG_GMRES_ONEFOLD changes no bit of any result (csrc/gmres.hip).

With the switch on (the default) the fast kernels of the split organisation sum the dots kernel's partial rows once
(k_gmres_fold_first) and the dots kernel forms the fp32-stored basis column; with NPG_GMRES_ONEFOLD=0 every orthogonalisation
workgroup sums the rows and the Arnoldi epilogue stores the column.  The sums are taken in the same order and the column from the
same expression, so residual history, iterate, niter / nreorth / nflagged / status and last_config() of every solve are compared
with np.array_equal - no tolerance.  One fresh child process per arrangement (tests/gmres_onefold_worker.py, which lists the
solves); both run side by side, once per module."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import nupgcm_amd as npg  # noqa: E402
from tests.gmres_onefold_worker import INV_KS, SYN_KS  # noqa: E402

KEYS = npg.GmresWorkspace.CONFIG_KEYS


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    here = os.path.dirname(os.path.abspath(__file__))
    tmp = tmp_path_factory.mktemp("onefold")
    procs = []
    for sw in ("0", "1"):
        out = str(tmp / f"sw{sw}.npz")
        procs.append((out, subprocess.Popen([sys.executable, os.path.join(here, "gmres_onefold_worker.py"), out, sw],
                                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    res = []
    for out, p in procs:
        log, _ = p.communicate(timeout=600)
        assert p.returncode == 0, log[-3000:]
        res.append(dict(np.load(out)))
    return res


def cfg_of(r, key):
    return dict(zip(KEYS, r[key + "_cfg"].tolist()))


def same(runs, prefix):
    off, on = runs
    keys = sorted(k for k in off if k.startswith(prefix))
    assert keys and keys == sorted(k for k in on if k.startswith(prefix)), (prefix, keys)
    for k in keys:
        assert off[k].shape == on[k].shape and np.array_equal(off[k], on[k]), (k, off[k], on[k])
    return off


@pytest.mark.parametrize("name,want", [("win", dict(xg=1, windowed=1)), ("ord", dict(xg=1, windowed=0))])
def test_bowl_inversion(runs, name, want):
    r = same(runs, f"inv_{name}_")
    for k in INV_KS:
        cfg = cfg_of(r, f"inv_{name}_k{k}")
        assert {key: cfg[key] for key in want} == want and cfg["split"] == 1 and cfg["basis"] == 32 and cfg["fast"] == 1, cfg
        assert r[f"inv_{name}_k{k}_stats"][0] == k and len(r[f"inv_{name}_k{k}_hist"]) == k + 1
    assert sum(k % 20 != 0 for k in INV_KS) >= 3                     # (solves that end in the middle of a cycle)
    niter, _, nflagged, status = r[f"inv_{name}_k0_stats"]
    hist = r[f"inv_{name}_k0_hist"]
    print(f"ONEFOLD bowl h=0.1 {name}: solve to rtol 1e-6 took {niter} iterations (status {status}, flagged {nflagged}), "
          f"residual {hist[0]:.3e} -> {hist[-1]:.3e}")
    assert status == 1 and len(hist) == niter + 1 and hist[-1] <= 1e-6 * hist[0], (niter, status, hist[-1] / hist[0])


@pytest.mark.parametrize("name,bits", [("b32", 32), ("b64", 64)])
def test_synthetic_odd_n(runs, name, bits):
    r = same(runs, f"syn_{name}_")
    for k in SYN_KS:
        cfg = cfg_of(r, f"syn_{name}_k{k}")
        assert cfg["split"] == 1 and cfg["basis"] == bits and cfg["fast"] == 1 and cfg["xg"] == 0 and cfg["distributed"] == 0, cfg
        assert cfg["n"] == 20001 and cfg["n"] >= 8192 and cfg["n"] % 512 != 0 and cfg["n"] % 2 == 1, cfg
        assert r[f"syn_{name}_k{k}_stats"][0] == k
    # the solves are real ones: within one cycle (30 steps, memory 30) GMRES's residual estimate never rises
    hist = r[f"syn_{name}_k30_hist"]
    assert len(hist) == 31 and np.all(np.diff(hist) <= 0.0) and hist[-1] < hist[0], hist


def test_fast_then_safe_mode(runs):
    r = same(runs, "safe_")
    for solve, fast in ((0, 1), (1, 0)):
        cfg = cfg_of(r, f"safe_s{solve}")
        niter, nreorth, nflagged, _ = r[f"safe_s{solve}_stats"]
        assert cfg["split"] == 1 and cfg["fast"] == fast and cfg["basis"] == 64, cfg
        assert niter == 4 and ((nflagged > 0) if fast else (nreorth > 0 and nflagged == 0)), r[f"safe_s{solve}_stats"]


def test_one_rank_distributed(runs):
    r = same(runs, "dist_")
    for k in (20, 43):
        cfg = cfg_of(r, f"dist_k{k}")
        assert cfg["distributed"] == 1 and cfg["pyth"] == 1 and cfg["split"] == 1 and cfg["fast"] == 1, cfg
        assert r[f"dist_k{k}_stats"][0] == k
