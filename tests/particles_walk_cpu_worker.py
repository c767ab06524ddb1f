"""Child process of tests/test_gpu_particles_walk.py: the CPU() architecture's diffusing particles through the same configuration from
the same seeds (one process runs on one architecture).  argv: configuration name, timesteps before tracking, output .npz, state .npz."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import nupgcm_amd as npg  # noqa: E402
from tests import particles_walk_ref as wr  # noqa: E402
from tests import sampling_ref as sr  # noqa: E402

if __name__ == "__main__":
    name, nsteps, out, state = sys.argv[1], int(sys.argv[2]), sys.argv[3], sys.argv[4]
    model = sr.bowl_model(npg.CPU(), name, nsteps=nsteps)
    npg.save_state(model, state)
    seeds, h, cd, kap = wr.one_step_setup(model)
    seed = 4242
    tr = npg.ParticleTracker(model, seeds, nsub=1, diffusion=(kap, kap, cd), seed=seed)
    for _ in range(20):
        tr.advance(h)
    np.savez(out, seeds=seeds, h=h, c_d=cd, seed=seed, t0=model.timestepper.t, nsteps=20, x=tr.positions, status=tr.status, cells=tr.cells,
             t_lost=tr.t_lost, wind=tr.wind, reflections=tr.reflections)
