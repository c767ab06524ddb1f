"""Child process of tests/test_gpu_gmres_onefold.py: one arrangement of the split GMRES cycle per process.  argv: output file,
value of NPG_GMRES_ONEFOLD (set before the first solve).  Runs the solves listed below and saves, for every one, the
residual history, the iterate, (niter, nreorth, nflagged, status) and last_config(); the parent makes every comparison.

  inv_*    bowl3D h = 0.1 inversion matrix (the system of test_inversion_gather_layout), fp32-stored basis: the windowed instance
           and the one on ordinary tiles; itmax = k with atol = rtol = 0 (k = 9, 21, 43 end in the middle of a cycle) and one solve
           to rtol = 1e-6, which ends where the tolerance is met
  syn_*    synthetic split-mode system, n = 20001 (odd: the last row pair has one row; 40 row-pair blocks, not a multiple of 512
           rows), memory 30 (one to four column groups): fp32-stored basis without the gather copy, and the fp64 basis
  safe_*   test_fast_kernels_then_safe_mode's two solves of one workspace: fast kernels, then the full ones
  dist_*   test_one_rank_distributed's setup: the distributed path with no peers"""
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import nupgcm_amd as npg                                     # noqa: E402
from nupgcm_amd import _lib as L                             # noqa: E402
from tests.helpers import build_fe_data                      # noqa: E402

INV_KS = (1, 9, 20, 21, 43)
SYN_KS = (1, 8, 9, 17, 30, 31, 63)


def synth(n, seed):
    """the well-conditioned nonsymmetric system of tests/test_gpu_gmres_steps.py"""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n), 19)
    A = sp.csr_matrix((rng.random(n * 19), (rows, rng.integers(0, n, n * 19))), shape=(n, n)) + sp.diags(3.0 + rng.random(n))
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    return A, rng.standard_normal(n), 0.1 * rng.standard_normal(n), 0.5 + rng.random(n)


def record(res, key, ws, st, x):
    cfg = ws.last_config()
    res[key + "_hist"] = ws.history()
    res[key + "_x"] = x.to_host()
    res[key + "_stats"] = np.array([st["niter"], st["nreorth"], st["nflagged"], st["status"]])
    res[key + "_cfg"] = np.array([cfg[k] for k in npg.GmresWorkspace.CONFIG_KEYS])


def main():
    out = sys.argv[1]
    os.environ["NPG_GMRES_ONEFOLD"] = sys.argv[2]          # (read by every solve)
    arch = npg.GPU()
    res = {}

    fed, prm, frc, dt, b0 = build_fe_data("bowl_mixing")
    A = npg.build_A_inversion(arch, fed, prm, 1.0)
    ref = A.to_scipy_csr()
    d = fed.dofs
    assert A.block_nodes(d.n_full, d.n_surf)
    n = ref.shape[0]
    h = fed.mesh.median_edge_length()
    b = npg.on_architecture(arch, ref @ np.cos(np.arange(n, dtype=float)) * 1e-3)
    x0 = 1e-4 * np.random.default_rng(3).standard_normal(n)
    P = npg.Diagonal(scalar=1 / h ** 3)
    for name, gather in (("win", None), ("ord", 2)):
        for k in INV_KS + (0,):
            ws = npg.GmresWorkspace(arch.ctx, n, memory=20)
            ws.set_basis(32)
            if gather is not None:
                ws.set_gather(gather)
            x = npg.on_architecture(arch, x0)
            if k:
                st = ws.solve(A, b, x, P, atol=0.0, rtol=0.0, itmax=k)
            else:
                st = ws.solve(A, b, x, P, atol=0.0, rtol=1e-6, itmax=20000)
            record(res, f"inv_{name}_k{k}", ws, st, x)

    n = 20001
    A, b, x0, dv = synth(n, 51)
    dA, db = npg.on_architecture(arch, A), npg.on_architecture(arch, b)
    Pv = npg.Diagonal(npg.on_architecture(arch, dv))
    for name, bits in (("b32", 32), ("b64", 64)):
        for k in SYN_KS:
            ws = npg.GmresWorkspace(arch.ctx, n, memory=30)
            ws.set_split(1)
            ws.set_basis(bits)
            ws.set_gather(0)
            x = npg.on_architecture(arch, x0)
            st = ws.solve(dA, db, x, Pv, atol=0.0, rtol=0.0, itmax=k)
            record(res, f"syn_{name}_k{k}", ws, st, x)

    rng = np.random.default_rng(42)
    n = 600
    A = sp.csr_matrix(sp.eye(n) + 1e-3 * sp.random(n, n, density=0.05, random_state=rng, format="csr"))
    b, x0 = rng.standard_normal(n), 0.1 * rng.standard_normal(n)
    dA, db = npg.on_architecture(arch, A), npg.on_architecture(arch, b)
    ws = npg.GmresWorkspace(arch.ctx, n, memory=30)
    ws.set_split(1)
    for solve in (0, 1):
        x = npg.on_architecture(arch, x0)
        st = ws.solve(dA, db, x, None, atol=0.0, rtol=0.0, itmax=4)
        record(res, f"safe_s{solve}", ws, st, x)

    from nupgcm_amd import distributed
    n, memory = 12001, 20
    A, b, x0, dv = synth(n, 5 + memory)
    dA, db = npg.on_architecture(arch, A), npg.on_architecture(arch, b)
    plan = dict(peers=np.zeros(0, np.int32), send_ptr=np.zeros(1, np.int64), send_idx=np.zeros(0, np.int32),
                recv_ptr=np.zeros(1, np.int64))
    for k in (memory, 2 * memory + 3):
        ws = npg.GmresWorkspace(arch.ctx, n, memory=memory)
        halo = distributed.Halo(arch.ctx, n, 0, plan)
        L.check(L.lib().npg_gmres_set_halo(ws.h, halo.h))
        x = npg.on_architecture(arch, x0)
        st = ws.solve(dA, db, x, npg.Diagonal(npg.on_architecture(arch, dv)), atol=0.0, rtol=0.0, itmax=k)
        record(res, f"dist_k{k}", ws, st, x)
        del ws, halo

    np.savez(out, **res)


if __name__ == "__main__":
    main()
