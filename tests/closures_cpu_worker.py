"""Child process of tests/test_gpu_closures.py: what the CPU() architecture (sparse LU inversions) gives for the cases the GPU() tests
compare against (one process runs on one architecture).  argv: output .npz.

  f_{bb, xb, delta, lam, apply, apply_adjoint}   check F: golden bowl, bowl_mixing after two BDF1 steps with both closures on; the base
                                                 state of the closures="tangent" linearisation and what it gives for delta and lam
  g_{bb, xb, sigma, kappa, gap, vectors, n, M}   check G: the embedded 2-D bowl with both closures on after 5 steps, its dense oracle"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import nupgcm_amd as npg  # noqa: E402
from tests import closures_ref as cr  # noqa: E402

if __name__ == "__main__":
    arch = npg.CPU()
    out = {f"f_{k}": v for k, v in cr.worker_case(arch, True, True).items()}
    _, lin, ref = cr.eigen_reference(arch)
    out.update({f"g_{k}": v for k, v in ref.items()})
    out.update(g_bb=lin.b_base.to_host(), g_xb=lin.x_base.to_host())
    np.savez(sys.argv[1], **out)
