"""Times of the mixing table (npg_classes_mixing) on the bench mesh (bowl3D h = 0.02), 64 x 64 bins, level = 1, after a warm-up
call, by device events, best and median of --reps:
  * npg_classes_mixing (memset + k_class_scan + k_classes_fold + k_class_bin + k_classes_convert) with the closure off and with it on
    (the difference is the cost of the tanh and the arithmetic around it), the diffusivities the model's own functions as tables;
  * the closure-off call with scalar diffusivities: what reading the two [ns][ncell] tables costs;
  * npg_classes_compute in the same process and on the same state: the yardstick.  The expectation to confirm or refute: the
    closure-off call costs no more than it (the same atomics, no velocity gathers).
Usage: python tools/mixing_bench.py [--workload L] [--steps K] [--reps R] [--bins N] [--level V] [--out FILE]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import nupgcm_amd as npg  # noqa: E402
from nupgcm_amd import _lib as L, workloads  # noqa: E402
from tools.classes_bench import sample_B_y, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bowl3D_h0.02")
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--level", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    arch = npg.GPU()
    ctx = arch.ctx
    t0 = time.time()
    model = workloads.example_model(arch, a.workload)
    npg.run(model, n_steps=a.steps)
    m = model.fe_data.mesh
    say(f"{ctx.name()}; {a.workload}: {m.ncell} cells, P{model.fe_data.spaces.b_order} buoyancy; set-up + {a.steps} steps {time.time() - t0:.1f} s")
    lam, _ = npg.watermass.default_rule(a.level)
    B, y = sample_B_y(model, lam)
    be = np.linspace(B.min(), B.max(), a.bins + 1)[1:-1]
    ye = np.linspace(y.min(), y.max(), a.bins + 1)[1:-1]
    K = npg.BuoyancyClasses(model, be, ye, level=a.level)
    x, b = model.inversion.solver.x, model.b_vec
    N2, alpha = float(model.params.N2), float(model.params.alpha)
    on = (1.0, alpha * max(N2, 1.0), alpha, N2)            # |a| / N2min about 1: the tanh in its mid-range, not saturated

    def mixing(closure):
        return lambda: L.check(L.lib().npg_classes_mixing(K.h, b.h, N2, *closure, K._table.h, K._info.h))
    t0 = time.time()
    K.set_diffusivity()
    say(f"set_diffusivity (kappa_h, kappa_v of the model at {m.ncell * len(lam)} sample points, host evaluation + transpose + upload): "
        f"{time.time() - t0:.2f} s, once per handle")
    T = K.mixing()
    T2 = K.mixing()
    assert np.array_equal(T.raw, T2.raw)                                 # the same bits on every call
    C0 = K.compute()
    assert np.array_equal(T.raw[..., 0], C0.raw[..., 0])                 # channel 0 is the census
    Ton = K.mixing(closure=on)
    say(f"{T}; occupied bins {int((T.volume > 0).sum())} of {T.volume.size}; closure on {on}: convective part of int kappa_v "
        f"{Ton.raw[..., 7].sum() / Ton.raw[..., 4].sum():.3f}")
    cls = timed(ctx, lambda: L.check(L.lib().npg_classes_compute(K.h, x.h, b.h, N2, K._table.h, K._info.h)), a.reps)
    off = timed(ctx, mixing((0.0, 0.0, 0.0, 0.0)), a.reps)
    won = timed(ctx, mixing(on), a.reps)
    cls2 = timed(ctx, lambda: L.check(L.lib().npg_classes_compute(K.h, x.h, b.h, N2, K._table.h, K._info.h)), a.reps)
    K.set_diffusivity(1e-2, 1e-2)
    sca = timed(ctx, mixing((0.0, 0.0, 0.0, 0.0)), a.reps)
    ns = m.ncell * len(lam)
    say(f"npg_classes_compute ({a.bins} x {a.bins} bins, {len(lam)} samples per cell) by events: best {cls[0]:.3f} ms, median {cls[1]:.3f} ms of "
        f"{a.reps}; again after the mixing calls: best {cls2[0]:.3f} ms, median {cls2[1]:.3f} ms")
    say(f"npg_classes_mixing closure off: best {off[0]:.3f} ms, median {off[1]:.3f} ms ({ns / off[0] / 1e3:.1f} Msamples/s)")
    say(f"npg_classes_mixing closure on:  best {won[0]:.3f} ms, median {won[1]:.3f} ms ({ns / won[0] / 1e3:.1f} Msamples/s)")
    say(f"npg_classes_mixing closure off, scalar diffusivities (no table reads): best {sca[0]:.3f} ms, median {sca[1]:.3f} ms")
    say(f"ratio mixing (closure off) / npg_classes_compute = {off[0] / cls[0]:.2f} (best), {off[1] / cls[1]:.2f} (median)")
    say(f"ratio mixing (closure on) / npg_classes_compute = {won[0] / cls[0]:.2f} (best), {won[1] / cls[1]:.2f} (median)")
    say(f"cost of the tanh (on - off, both passes evaluate it): {won[0] - off[0]:.3f} ms (best), {won[1] - off[1]:.3f} ms (median) = "
        f"{(won[0] - off[0]) * 1e6 / (2 * ns):.3f} ns per evaluation")
    say(f"cost of the table reads (tables - scalars, closure off): {off[0] - sca[0]:.3f} ms (best), {off[1] - sca[1]:.3f} ms (median)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
