"""CPU checks of the step-level GMRES restatement (tests/gmres_steps_ref.py) that the GPU step tests measure the kernels against:
with its rounding switches off it is restarted GMRES as Krylov.jl runs it (oracle/krylov_oracle.py, modified Gram-Schmidt) and as
the host library runs it, to fp64 rounding, iterate and residual history, across restarts."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from nupgcm_amd import _lib as L
from oracle import krylov_oracle as ko
from tests.gmres_steps_ref import gmres_steps, true_residual


def _system(n, seed):
    """well-conditioned (condition number ~30 at n = 400), nonsymmetric: about 20 random entries per row plus a diagonal; GMRES
    gains about a digit per 6 iterations, so 63 iterations stay far from the fp64 floor"""
    rng = np.random.default_rng(seed)
    A = sp.random(n, n, density=min(1.0, 20.0 / n), random_state=rng, format="csr") + sp.diags(3.0 + rng.random(n))
    return sp.csr_matrix(A), rng.standard_normal(n), 0.1 * rng.standard_normal(n), 0.5 + rng.random(n)


def _rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b))


@pytest.mark.parametrize("memory", [1, 8, 9, 30])
@pytest.mark.parametrize("prec", ["none", "scalar", "vector"])
def test_restatement_is_krylov_jl_gmres(memory, prec):
    A, b, x0, dv = _system(400, memory)
    P = {"none": None, "scalar": 0.37, "vector": dv}[prec]
    k = 2 * memory + 3
    ref = gmres_steps(A, b, x0, memory, k, P=P, xs_at=(memory, memory + 1))
    xo, so = ko.gmres(A, b, x0=x0, M=P, memory=memory, atol=0.0, rtol=0.0, itmax=k)
    for kk in (memory, memory + 1):          # the iterate a solve stopped after kk iterations returns
        assert _rel(ref["xs"][kk], ko.gmres(A, b, x0=x0, M=P, memory=memory, atol=0.0, rtol=0.0, itmax=kk)[0]) <= 1e-12
    ho = np.asarray(so["residuals"])
    assert ref["niter"] == so["niter"] == k and ref["status"] == 2 and len(ref["hist"]) == len(ho) == k + 1
    assert np.max(np.abs(ref["hist"] - ho)) <= 1e-12 * ho[0]
    assert _rel(ref["x"], xo) <= 1e-12
    # every cycle starts from the true residual of the iterate the previous one left
    assert len(ref["betas"]) == (k + memory - 1) // memory and ref["betas"][0] == ref["hist"][0]
    # the Hessenberg matrix of a cycle is P A restricted to its Krylov space: H[:m, :m] = V' P A V with V the cycle's basis
    # (orthonormal to rounding), and the subdiagonal holds the norms of the orthogonalised vectors
    H, V = ref["H"][0], ref["V"][0]
    PAV = (A @ V.T) * (1.0 if P is None else (P if np.isscalar(P) else P[:, None]))
    assert H.shape == (memory + 1, memory) and np.all(np.diag(H, -1) > 0)
    assert np.max(np.abs(V @ V.T - np.eye(memory))) <= 1e-13
    assert np.max(np.abs(V @ PAV - H[:memory])) <= 1e-12 * np.max(np.abs(H))


def test_restatement_rounding_switches():
    """basis32 / gather32 move the answer by what fp32 rounding of the stored columns / the SpMV input can (~1e-7 relative),
    not by more; one pass with the Pythagorean norm agrees with CGS2 to the loss of orthogonality classical Gram-Schmidt has in
    fp64 (measured 2.8e-12 of the first residual over 25 iterations of this system)."""
    A, b, x0, dv = _system(400, 3)
    k = 25
    r64 = gmres_steps(A, b, x0, 20, k, P=dv)
    one = gmres_steps(A, b, x0, 20, k, P=dv, passes=1, pyth_eta=0.1)
    assert np.max(np.abs(one["hist"] - r64["hist"])) <= 1e-11 * r64["hist"][0] and _rel(one["x"], r64["x"]) <= 1e-10
    for kw in (dict(basis32=True), dict(gather32=True), dict(basis32=True, gather32=True)):
        r32 = gmres_steps(A, b, x0, 20, k, P=dv, passes=1, pyth_eta=0.1, **kw)
        d = np.max(np.abs(r32["hist"] - r64["hist"])) / r64["hist"][0]
        assert 1e-10 < d < 1e-5, (kw, d)
        assert 1e-10 < _rel(r32["x"], r64["x"]) < 1e-4, kw
    # true_residual is R1's quantity
    assert abs(true_residual(A, b, x0, dv) - r64["hist"][0]) <= 1e-15 * r64["hist"][0]


def test_restatement_stops_like_the_device():
    """exact solve of a 2 x 2 system in two steps (breakdown / solved), a zero right-hand side, and the stopping rule"""
    A = sp.csr_matrix(np.array([[4.0, 1.0], [0.5, 3.0]]))
    b = np.array([1.0, 2.0])
    ref = gmres_steps(A, b, np.zeros(2), 5, 10)
    assert ref["niter"] == 2 and ref["status"] in (1, 3) and _rel(ref["x"], np.linalg.solve(A.toarray(), b)) < 1e-14
    z = gmres_steps(A, np.zeros(2), np.zeros(2), 5, 10)
    assert z["status"] == 4 and z["niter"] == 0 and list(z["hist"]) == [0.0]
    A, b, x0, dv = _system(400, 5)
    ref = gmres_steps(A, b, x0, 10, 500, atol=0.0, rtol=1e-10)
    xo, so = ko.gmres(A, b, x0=x0, memory=10, atol=0.0, rtol=1e-10, itmax=500)
    assert ref["status"] == 1 and ref["niter"] == so["niter"] and _rel(ref["x"], xo) < 1e-12


@pytest.mark.skipif(not os.path.exists(L.HOST_LIB_PATH), reason="libnupgcm_host.so not built (make -C nupgcm_amd/csrc_host)")
def test_restatement_matches_the_host_library():
    """the host build of npg_gmres_solve (Krylov.jl's order of operations in C++) - run in a child process: one process runs on
    one architecture"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
import nupgcm_amd as npg
from tests.test_gmres_steps_ref import _system
from tests.gmres_steps_ref import gmres_steps
ctx = npg.CPU().ctx
worst = 0.0
for memory, prec in [(1, "none"), (8, "scalar"), (9, "vector"), (30, "vector")]:
    A, b, x0, dv = _system(400, 10 + memory)
    P = {"none": None, "scalar": 0.37, "vector": dv}[prec]
    k = 2 * memory + 3
    ref = gmres_steps(A, b, x0, memory, k, P=P)
    ws = npg.GmresWorkspace(ctx, 400, memory=memory)
    x = npg.DeviceVector.from_host(ctx, x0)
    Pd = None if P is None else (npg.Diagonal(scalar=P, n=400) if np.isscalar(P) else npg.Diagonal(npg.DeviceVector.from_host(ctx, dv)))
    st = ws.solve(npg.DeviceCSR.from_scipy(ctx, A), npg.DeviceVector.from_host(ctx, b), x, Pd, atol=0.0, rtol=0.0, itmax=k)
    h = ws.history()
    assert st["niter"] == k and len(h) == k + 1, (st, len(h))
    worst = max(worst, np.max(np.abs(h - ref["hist"])) / h[0], np.max(np.abs(x.to_host() - ref["x"])) / np.max(np.abs(ref["x"])))
print("WORST", worst)
"""
    out = subprocess.run([sys.executable, "-c", code, root], capture_output=True, text=True, timeout=300, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    worst = float(out.stdout.split("WORST")[1])
    assert worst <= 1e-12, worst
