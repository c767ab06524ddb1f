"""Child process of tests/test_gpu_linearized.py: what the CPU() architecture (sparse LU inversions) gives for the cases the GPU() tests
compare against (one process runs on one architecture).  argv: output .npz.

  d_<case>_{bb, xb, delta, apply}     check 3: base state, perturbation and J delta of bowl_mixing after 3 steps / bowl_wind
  e_<nsteps>_{bb, xb, ...}            check 6: base state of the embedded 2-D bowl, its dense oracle (tests/linearized_ref.oracle_modes)
                                      and the CPU() run's own sigma and residuals"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import nupgcm_amd as npg  # noqa: E402
from tests import linearized_ref as lr  # noqa: E402

if __name__ == "__main__":
    arch, out = npg.CPU(), {}
    for case, config, nsteps in (("mixing", "bowl_mixing", 3), ("wind", "bowl_wind", 0)):
        model, bb, xb, delta = lr.derivative_case(arch, config, nsteps)
        lin = npg.LinearizedModel(model)
        got = lin.apply(npg.DeviceVector.from_host(arch.ctx, delta)).to_host()
        out.update({f"d_{case}_bb": bb, f"d_{case}_xb": xb, f"d_{case}_delta": delta, f"d_{case}_apply": got})
    for nsteps in (0, 5):
        model, lin = lr.eigen_case(arch, nsteps)
        ref = lr.oracle_modes(lin, lr.DT_EIG)
        em = lin.eigenmodes(ref["n"], lr.DT_EIG)
        out.update({f"e_{nsteps}_{k}": v for k, v in ref.items()})
        out.update({f"e_{nsteps}_bb": lin.b_base.to_host(), f"e_{nsteps}_xb": lin.x_base.to_host(), f"e_{nsteps}_cpu_sigma": em.sigma,
                    f"e_{nsteps}_cpu_residuals": em.residuals})
    np.savez(sys.argv[1], **out)
