"""Child process of tests/test_gpu_surfaces.py: the CPU() architecture's maps on buoyancy surfaces of the same configuration (one process
runs on one architecture).  argv: configuration name, timesteps before the maps, output .npz, state .npz."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import nupgcm_amd as npg  # noqa: E402
from tests import sampling_ref as sr  # noqa: E402
from tests import surfaces_ref as ur  # noqa: E402

if __name__ == "__main__":
    name, nsteps, out, state = sys.argv[1], int(sys.argv[2]), sys.argv[3], sys.argv[4]
    model = sr.bowl_model(npg.CPU(), name, nsteps=nsteps)
    npg.save_state(model, state)
    xy, levels = ur.cross_setup(model)
    S = npg.BuoyancySurfaces(model, levels, points=xy)
    M = S.compute()
    np.savez(out, xy=xy, levels=levels, z=M.z, z_low=M.z_low, ncross=M.ncross, status=M.status, u=M.u, grad_B=M.grad_B, nseg=S.nseg,
             z_top=M.z_top, z_bot=M.z_bot)
