"""The explicit dense inverse (NPG_PC_DENSE, fp64 storage) on the systems of tests/dense_ref.py: max |A X - I| of the whole
inverse at the sizes around 256 and 512, and the set-up time at 2 053 / 8 192 / 16 384 unknowns.  Run from the repository root:
python tools/dense_inverse_probe.py; NPG_AB_LIB=<another build of the library> compares two builds of dense_build
(profiles/dense_inverse_getri.txt)."""
import sys, time
import numpy as np
sys.path.insert(0, ".")
import nupgcm_amd as npg
from nupgcm_amd import multigrid as mgm
from tests import dense_ref as dr

arch = npg.GPU(); ctx = arch.ctx
print("device", ctx.name(), flush=True)
A = npg.DeviceCSR.from_scipy(ctx, dr.system(64)); mgm.DenseInversePreconditioner(arch, A, storage="fp64")     # warm-up
for n in (255, 256, 257, 511, 512, 513):
    As = dr.system(n); Ad = As.toarray()
    P = mgm.DenseInversePreconditioner(arch, npg.DeviceCSR.from_scipy(ctx, As), storage="fp64")
    r, z = npg.DeviceVector(ctx, n), npg.DeviceVector(ctx, n)
    X = np.empty((n, n))
    for j in range(n):
        e = np.zeros(n); e[j] = 1.0
        r.upload(e); X[:, j] = P.apply(r, z).to_host()
    E = np.abs(Ad @ X - np.eye(n))
    bad = np.nonzero(E.max(axis=0) > 1e-10)[0]
    print(f"n = {n}: max |A X - I| = {E.max():.3e}; columns off by > 1e-10: {len(bad)}"
          + (f" (first {bad[0]}, last {bad[-1]})" if len(bad) else ""), flush=True)
for n in (2053, 8192, 16384):
    As = dr.system(n)
    Adev = npg.DeviceCSR.from_scipy(ctx, As)
    ts = []
    for rep in range(3):
        t = time.perf_counter()
        P = mgm.DenseInversePreconditioner(arch, Adev, storage="fp64")
        ts.append(time.perf_counter() - t)
    rng = np.random.default_rng(1); b = rng.standard_normal(n)
    zz = P.apply(npg.DeviceVector.from_host(ctx, b), npg.DeviceVector(ctx, n)).to_host()
    print(f"n = {n}: set-up {min(ts) * 1e3:.1f} ms (three: {[round(x * 1e3, 1) for x in ts]}), |A z - b| / |b| = "
          f"{np.linalg.norm(As @ zz - b) / np.linalg.norm(b):.2e}", flush=True)
    del P
