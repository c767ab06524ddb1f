"""Child process of tests/test_gpu_gmres_fusedcols.py: one arrangement of the split GMRES cycle's row launches per process.  argv:
output file, arrangement - "sep" (NPG_GMRES_FUSEDROWS=0: the separate launches at every step), "c16" (NPG_GMRES_FUSED_COLS=16:
fused launches up to 16 columns, separate ones from there) or "c20" (the default: fused launches up to 20 columns).
NPG_GMRES_ROWS_WG=64 in every child.  Every solve: set_split(1), set_basis(32), set_gather(0), atol = rtol = 0, itmax = k.  Saves
the residual history, the iterate, (niter, nreorth, nflagged, status), last_config() and fused_cols() of every solve; the parent
makes every comparison.

The 20-column instance keeps a thread's last B = 2 trips on chip (columns 0..9 in L = 2 LDS slots, columns 10..19 and the w pair in
registers) and reads the trips before them again, so with 512 rows per trip and workgroup:

  one_*   n = 20 001 on 40 workgroups: one trip per thread, an odd last pair; at memory 20 (k ends a solve on every step of the new
          instance, on the cycle boundary and in the second cycle), memory 18 (the cycle ends inside the instance's range) and
          memory 30 (fused steps 16..19, then separate launches for j >= 20)
  trip_*  n = 65 535 (128 blocks on 64 workgroups: exactly B trips everywhere), 65 537 (129: one workgroup has a third trip of one
          row - its first trip is read again) and 98 305 (193: three trips, four in workgroup 0 - one and two trips read again)
  big_*   n = 200 001 (391 blocks: six or seven trips), every solve twice in ONE workspace: graph replay, a hand-off state that
          only grows"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import nupgcm_amd as npg                                     # noqa: E402
from tests.gmres_onefold_worker import record, synth         # noqa: E402

ONE_KS = {20: (16, 17, 18, 19, 20, 21, 37, 40), 18: (18, 36), 30: (30, 47)}
TRIP_NS = (65535, 65537, 98305)
TRIP_KS = (20, 39)
BIG_KS = (20, 27)
ENV = {"sep": {"NPG_GMRES_FUSEDROWS": "0"}, "c16": {"NPG_GMRES_FUSED_COLS": "16"}, "c20": {}}


def main():
    out, mode = sys.argv[1], sys.argv[2]
    for name in ("NPG_GMRES_FUSEDROWS", "NPG_GMRES_FUSED_COLS", "NPG_GMRES_ONEFOLD"):
        os.environ.pop(name, None)
    os.environ.update(ENV[mode])                           # (read by every solve)
    os.environ["NPG_GMRES_ROWS_WG"] = "64"                 # (read once, by the first solve of the process)
    arch = npg.GPU()
    res = {}

    def solve(key, ws, dA, db, x0, Pv, k):
        x = npg.on_architecture(arch, x0)
        st = ws.solve(dA, db, x, Pv, atol=0.0, rtol=0.0, itmax=k)
        record(res, key, ws, st, x)
        res[key + "_cols"] = np.array([ws.fused_cols()])

    def workspace(n, memory):
        ws = npg.GmresWorkspace(arch.ctx, n, memory=memory)
        ws.set_split(1)
        ws.set_basis(32)
        ws.set_gather(0)
        return ws

    def system(n, seed):
        A, b, x0, dv = synth(n, seed)
        return npg.on_architecture(arch, A), npg.on_architecture(arch, b), x0, npg.Diagonal(npg.on_architecture(arch, dv))

    n = 20001
    dA, db, x0, Pv = system(n, 51)
    for memory, ks in ONE_KS.items():
        for k in ks:
            solve(f"one_m{memory}_k{k}", workspace(n, memory), dA, db, x0, Pv, k)

    for n in TRIP_NS:
        dA, db, x0, Pv = system(n, 53)
        for k in TRIP_KS:
            solve(f"trip_n{n}_k{k}", workspace(n, 20), dA, db, x0, Pv, k)

    n = 200001
    dA, db, x0, Pv = system(n, 52)
    ws = workspace(n, 20)
    for rep in (0, 1):
        for k in BIG_KS:
            solve(f"big_r{rep}_k{k}", ws, dA, db, x0, Pv, k)

    np.savez(out, **res)


if __name__ == "__main__":
    main()
