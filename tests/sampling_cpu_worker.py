"""Child process of tests/test_gpu_sampling.py: the CPU() architecture's samples of the same configuration at the same points (one
process runs on one architecture).  argv: configuration name, buoyancy order, output .npz, state .npz."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import nupgcm_amd as npg  # noqa: E402
from tests import sampling_ref as sr  # noqa: E402

if __name__ == "__main__":
    name, order, out, state = sys.argv[1], int(sys.argv[2]), sys.argv[3], sys.argv[4]
    model = sr.bowl_model(npg.CPU(), name, b_order=order, nsteps=3)
    npg.save_state(model, state)
    pts = sr.box_points(model, 2500)
    loc = npg.PointLocator(model).locate(pts)
    np.savez(out, pts=pts, cells=loc.cells, **{f: npg.nan_eval(model, f, pts, loc) for f in ("u", "p", "b", "grad_b")})
