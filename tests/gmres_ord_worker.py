"""Child process of tests/test_gpu_gmres_steps.py::test_windowed_ord_instances: NPG_WIN_ORD is read once per process, so the
windowed Arnoldi instances that carry ordinary tiles (ORD) run here, with the switch set before the first solve.  Builds the bowl3D
h = 0.1 inversion matrix with WL = 4 and WL = 8 windowed tiles, runs the parent's solves (itmax = k, atol = rtol = 0) and saves
history, iterate and last_config() of every solve; the parent does every comparison."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
os.environ["NPG_WIN_ORD"] = "1"
import nupgcm_amd as npg                                     # noqa: E402
from tests.helpers import build_fe_data                      # noqa: E402


def main():
    out, memory, ks = sys.argv[1], int(sys.argv[2]), [int(k) for k in sys.argv[3].split(",")]
    arch = npg.GPU()
    fed, prm, frc, dt, b0 = build_fe_data("bowl_mixing")
    d = fed.dofs
    h = fed.mesh.median_edge_length()
    res = {}
    for wl in (4, 8):
        os.environ["NPG_SPMV_WLANES"] = str(wl)             # read per windowed-set build
        A = npg.build_A_inversion(arch, fed, prm, 1.0)
        ref = A.to_scipy_csr()
        res[f"wl{wl}_indptr"], res[f"wl{wl}_indices"], res[f"wl{wl}_data"] = ref.indptr, ref.indices, ref.data
        assert A.block_nodes(d.n_full, d.n_surf)           # (the windowed set is built here)
        del os.environ["NPG_SPMV_WLANES"]
        b, x0 = np.load(out + ".in.npz")["b"], np.load(out + ".in.npz")["x0"]
        for rep, k in [(0, k) for k in ks] + [(1, max(ks))]:       # (rep 1: the largest k again, fresh workspace)
            ws = npg.GmresWorkspace(arch.ctx, A.shape[0], memory=memory)
            ws.set_basis(32)
            x = npg.on_architecture(arch, x0)
            st = ws.solve(A, npg.on_architecture(arch, b), x, npg.Diagonal(scalar=1 / h ** 3), atol=0.0, rtol=0.0, itmax=k)
            cfg = ws.last_config()
            res[f"wl{wl}_k{k}_r{rep}_hist"] = ws.history()
            res[f"wl{wl}_k{k}_r{rep}_x"] = x.to_host()
            res[f"wl{wl}_k{k}_r{rep}_cfg"] = np.array([cfg[key] for key in npg.GmresWorkspace.CONFIG_KEYS])
            res[f"wl{wl}_k{k}_r{rep}_niter"] = np.array(st["niter"])
    np.savez(out + ".out.npz", **res)


if __name__ == "__main__":
    main()
