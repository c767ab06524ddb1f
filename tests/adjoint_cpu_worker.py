"""Child process of tests/test_gpu_adjoint.py: what the CPU() architecture (sparse LU inversions) gives for the cases the GPU() tests
compare against (one process runs on one architecture).  argv: output .npz.

  d_<case>_{bb, xb}                   check D: the base states of bowl_mixing after 3 steps / bowl_wind
  e_<nsteps>_{bb, xb, ...}            checks F, G: base state of the embedded 2-D bowl, its dense oracle with both sets of vectors
                                      (tests/adjoint_ref.oracle_pairs) and the CPU() run's own left sigma and residuals"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import nupgcm_amd as npg  # noqa: E402
from tests import adjoint_ref as ar  # noqa: E402
from tests import linearized_ref as lr  # noqa: E402

if __name__ == "__main__":
    arch, out = npg.CPU(), {}
    for case, config, nsteps in (("mixing", "bowl_mixing", 3), ("wind", "bowl_wind", 0)):
        model, bb, xb, _ = lr.derivative_case(arch, config, nsteps)
        out.update({f"d_{case}_bb": bb, f"d_{case}_xb": xb})
    for nsteps in (0, 5):
        model, lin = lr.eigen_case(arch, nsteps)
        ref = ar.oracle_pairs(lin, lr.DT_EIG)
        del ref["J"]
        em = lin.eigenmodes(ref["n"], lr.DT_EIG, side="left")
        out.update({f"e_{nsteps}_{k}": v for k, v in ref.items()})
        out.update({f"e_{nsteps}_bb": lin.b_base.to_host(), f"e_{nsteps}_xb": lin.x_base.to_host(), f"e_{nsteps}_cpu_sigma_left": em.sigma,
                    f"e_{nsteps}_cpu_residuals_left": em.residuals})
    np.savez(sys.argv[1], **out)
