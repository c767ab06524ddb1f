"""Child process of tests/test_gpu_diagnostics.py: the CPU() architecture's grid integrals of a configuration after three steps (one
process runs on one architecture).  argv: configuration name, buoyancy order, output .npz, state .npz."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import nupgcm_amd as npg  # noqa: E402
from tests import diagnostics_ref as dr  # noqa: E402
from tests import sampling_ref as sr  # noqa: E402

if __name__ == "__main__":
    name, order, out, state = sys.argv[1], int(sys.argv[2]), sys.argv[3], sys.argv[4]
    model = sr.bowl_model(npg.CPU(), name, b_order=order, nsteps=3)
    npg.save_state(model, state)
    r = npg.GridDiagnostics(model, 24, 24, 24).compute()
    g = npg.sample_to_grid(model, 24, 24, 24, fields=("u", "b", "grad_b"))
    _, _, sc, sz = dr.integrals_of_samples(g)                            # max|f| per channel, for the bounds
    np.savez(out, col=r.col, zon=r.zon, scales_c=np.array(sc), scales_z=np.array(sz))
