"""Child process of tests/test_gpu_gmres_fusedrows.py: one arrangement of the split GMRES cycle per process.  argv: output file,
value of NPG_GMRES_FUSEDROWS, value of NPG_GMRES_ONEFOLD (both set before the first solve; NPG_GMRES_ROWS_WG=64 in every child).
Runs the solves listed below and saves, for every one, the residual history, the iterate, (niter, nreorth, nflagged, status) and
last_config(); the parent makes every comparison.

  inv_*    bowl3D h = 0.1 inversion matrix, fp32-stored basis: the windowed Arnoldi instance and the one on ordinary tiles; itmax = k
           with atol = rtol = 0 (k = 9, 21, 43 end in the middle of a cycle) and one solve to rtol = 1e-6
  syn_*    synthetic split-mode system, n = 20001 (odd: the last row pair has one row; 40 row-pair blocks, one trip per thread),
           fp32-stored basis at memory 20 and at memory 30 (steps past the widest fused instance take the separate launches),
           and the fp64 basis (no fused kernel)
  big_*    the same kind of system with n = 200001: 391 row-pair blocks over 64 workgroups, six or seven trips per thread - trips
           read again, trips kept in LDS and trips kept in registers at every column count; every solve twice in one process
  safe_*   test_fast_kernels_then_safe_mode's two solves of one workspace: fast kernels, then the full ones
  dist_*   the distributed path with no peers"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import nupgcm_amd as npg                                     # noqa: E402
from nupgcm_amd import _lib as L                             # noqa: E402
from tests.gmres_onefold_worker import INV_KS, record, synth  # noqa: E402
from tests.helpers import build_fe_data                      # noqa: E402

SYN_KS = (1, 9, 17, 21, 43)
SYN30_KS = (9, 30, 47)
BIG_KS = (5, 13, 20, 27)


def main():
    out = sys.argv[1]
    os.environ["NPG_GMRES_FUSEDROWS"] = sys.argv[2]        # (read by every solve)
    os.environ["NPG_GMRES_ONEFOLD"] = sys.argv[3]
    os.environ["NPG_GMRES_ROWS_WG"] = "64"                 # (read once, by the first solve of the process)
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
    for name, bits, memory, ks in (("m20", 32, 20, SYN_KS), ("m30", 32, 30, SYN30_KS), ("b64", 64, 20, (9, 21))):
        for k in ks:
            ws = npg.GmresWorkspace(arch.ctx, n, memory=memory)
            ws.set_split(1)
            ws.set_basis(bits)
            ws.set_gather(0)
            x = npg.on_architecture(arch, x0)
            st = ws.solve(dA, db, x, Pv, atol=0.0, rtol=0.0, itmax=k)
            record(res, f"syn_{name}_k{k}", ws, st, x)

    n = 200001
    A, b, x0, dv = synth(n, 52)
    dA, db = npg.on_architecture(arch, A), npg.on_architecture(arch, b)
    Pv = npg.Diagonal(npg.on_architecture(arch, dv))
    ws = npg.GmresWorkspace(arch.ctx, n, memory=20)
    ws.set_split(1)
    ws.set_basis(32)
    ws.set_gather(0)
    for rep in (0, 1):
        for k in BIG_KS:
            x = npg.on_architecture(arch, x0)
            st = ws.solve(dA, db, x, Pv, atol=0.0, rtol=0.0, itmax=k)
            record(res, f"big_r{rep}_k{k}", ws, st, x)

    import scipy.sparse as sp
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
    ws = npg.GmresWorkspace(arch.ctx, n, memory=memory)
    halo = distributed.Halo(arch.ctx, n, 0, plan)
    L.check(L.lib().npg_gmres_set_halo(ws.h, halo.h))
    x = npg.on_architecture(arch, x0)
    st = ws.solve(dA, db, x, npg.Diagonal(npg.on_architecture(arch, dv)), atol=0.0, rtol=0.0, itmax=23)
    record(res, "dist_k23", ws, st, x)
    del ws, halo

    np.savez(out, **res)


if __name__ == "__main__":
    main()
