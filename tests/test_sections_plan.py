"""The host planner of the section transports (csrc/sections_core.h) without a GPU and outside Python: tests/sections_plan_main.cpp is
compiled with g++ under AddressSanitizer and UBSan and run as a child process.  Every plan is compared with the independent cutter of
tests/sections_ref.py - the same (bin, cell) pairs, areas within its bound - and checked for the invariants of a plan; the refusals come
back as messages."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import nupgcm_amd as npg
from tests import sections_ref as xr

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = {"i64": np.int64, "i32": np.int32, "f64": np.float64, "u8": np.uint8}
S = npg.Section
UNIT_TET = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]])


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/sections_plan_main.cpp")
    exe = str(tmp_path_factory.mktemp("sections_plan") / "sections_plan_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                    os.path.join(HERE, "sections_plan_main.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def kuhn():
    coords, cells = xr.kuhn_cells(4)
    return coords[cells]


def plan(planner, d, X, sections, mask=None):
    """run the planner on the cells X (ncell, 4, 3) in directory d; returns (meta, message, arrays)"""
    shutil.rmtree(d, ignore_errors=True)
    os.makedirs(d)
    put = lambda name, a, t: np.ascontiguousarray(a, dtype=t).tofile(os.path.join(d, name))       # noqa: E731
    put("cell_xyz.f64", X, "<f8")
    put("frames.f64", np.stack([s.frame for s in sections]), "<f8")
    put("n1.i32", [s.shape[0] for s in sections], "<i4")
    put("n2.i32", [s.shape[1] for s in sections], "<i4")
    put("edges1.f64", np.concatenate([s.edges1 for s in sections]), "<f8")
    put("edges2.f64", np.concatenate([s.edges2 for s in sections]), "<f8")
    if mask is not None:
        put("mask.u8", mask, "u1")
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write(f"ncell {len(X)}\nnsec {len(sections)}\n")
    subprocess.run([planner, d], check=True)            # (a sanitizer report ends the child with a non-zero status)
    meta = {}
    with open(os.path.join(d, "out_meta.txt")) as f:
        for line in f:
            k, v = line.split()
            meta[k] = int(v)
    arr = {}
    for name in os.listdir(d):
        if name.startswith("out_") and not name.endswith(".txt"):
            base, ext = name[4:].rsplit(".", 1)
            arr[base] = np.fromfile(os.path.join(d, name), dtype=DTYPES[ext])
    return meta, open(os.path.join(d, "out_message.txt")).read().strip(), arr


def checked(planner, d, X, sections, label, mask=None):
    """plan, check the invariants, compare with the independent cutter; returns (pieces per bin, area per bin, bound per bin)"""
    meta, msg, a = plan(planner, str(d), X, sections, mask)
    assert meta["status"] == 0 and msg == "", msg
    nbin = sum(s.shape[0] * s.shape[1] for s in sections)
    pl = dict(cell=a["cell"], bin=a["bin"], lam=a["lam"].reshape(-1, 3, 4), area=a["area"], bin_ptr=a["bin_ptr"])
    info = dict(pieces=meta["npiece"], bins=meta["nbin"], cut_cells=meta["ncut_cells"], max_per_bin=meta["max_per_bin"])
    xr.plan_invariants(pl, info, nbin)
    assert np.array_equal(a["sec_bin0"], np.concatenate([[0], np.cumsum([s.shape[0] * s.shape[1] for s in sections])]))
    assert np.array_equal(a["sec"], np.searchsorted(a["sec_bin0"], a["bin"], side="right") - 1)
    got, ref, bound = xr.compare_plans(pl, xr.independent_plan(X, sections, mask), nbin, label)
    return np.diff(a["bin_ptr"]), got, bound


def test_kuhn_cube_face_aligned_planes_and_bins(planner, kuhn, tmp_path):
    grid = [0.0, 0.25, 0.5, 0.75, 1.0]
    zed = [-1.0, -0.75, -0.5, -0.25, 0.0]
    secs = [S.longitude(0.5, y_edges=grid, z_edges=zed), S.latitude(0.25, x_edges=grid, z_edges=zed), S.level(-0.5, x_edges=grid, y_edges=grid),
            S("minus", [0.5, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], grid, zed)]
    counts, area, bound = checked(planner, tmp_path, kuhn, secs, "Kuhn cube, face-aligned")
    assert len(counts) == 64 and (counts == 2).all()                                   # every grid square: its two mesh faces, once each
    assert (np.abs(area - 0.0625) <= bound).all()
    # the outer faces of the cube: the plane x = 0 sees nothing below it, the plane x = 1 with the inward normal nothing either
    counts, area, _ = checked(planner, tmp_path, kuhn, [S.longitude(0.0), S("far", [1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0])], "Kuhn cube, outer faces")
    assert list(counts) == [0, 0]
    counts, area, bound = checked(planner, tmp_path, kuhn, [S("in", [0.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]), S.longitude(1.0)], "Kuhn cube, outer faces, other side")
    assert list(counts) == [32, 32] and (np.abs(area - 1.0) <= bound).all()


def test_single_tetrahedron_through_a_vertex_an_edge_and_a_face(planner, tmp_path):
    n = np.array([2.0, -2.0, 1.0]) / 3.0
    e1 = np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)
    r = 1.0 / np.sqrt(2.0)
    secs = [S("vertex, cutting", [0, 0, 0], n, e1, np.cross(n, e1)),                   # through v0 alone, v2 below: one corner AT v0
            S.level(1.0, name="vertex, touching"),                                     # through v3 alone, the rest below: three corners at v3
            S("edge", [0, 0, 0], [r, -r, 0.0], [r, r, 0.0], [0, 0, 1.0]),              # contains the edge (v0, v3), v2 below
            S("edge, touching", [0, 0, 0], [0.0, -r, -r], [1.0, 0, 0], [0.0, r, -r]),  # contains the edge (v0, v1), the rest below
            S("face, above", [0, 0, 0], [0, 0, 1.0], [1.0, 0, 0], [0, 1.0, 0]),        # contains the face (v0, v1, v2), v3 above: not this cell's
            S("face, below", [0, 0, 0], [0, 0, -1.0], [1.0, 0, 0], [0, 1.0, 0])]       # the same plane, v3 below: the face, once
    counts, area, bound = checked(planner, tmp_path, UNIT_TET, secs, "unit tetrahedron")
    assert list(counts) == [1, 0, 1, 0, 0, 1]
    assert abs(area[2] - 0.5 * r) <= bound[2] and abs(area[5] - 0.5) <= bound[5]
    d = xr.sdot(UNIT_TET[0], np.zeros(3), n)
    assert d[0] == 0.0 and d[2] < 0 < min(d[1], d[3])


def test_a_plane_that_misses_and_infinite_edges(planner, kuhn, tmp_path):
    inf = np.inf
    secs = [S.level(0.5, name="above"), S.longitude(-0.25, name="beside", y_edges=[-inf, 0.3, inf]),
            S.latitude(0.37, x_edges=[-inf, 0.21, 0.5, inf], z_edges=[-inf, -0.33, inf], name="open both ways"),
            S.latitude(0.37, x_edges=[-inf, 0.21], z_edges=[-0.33, inf], name="one corner"),
            S.latitude(0.37, x_edges=[2.0, inf], name="outside the edges")]
    counts, area, bound = checked(planner, tmp_path, kuhn, secs, "misses and infinite edges")
    assert list(counts[:3]) == [0, 0, 0] and (counts[3:9] > 0).all() and counts[9] > 0 and counts[10] == 0
    assert abs(area[3:9].sum() - 1.0) <= bound[3:9].sum() + 8 * xr.EPS                # the open bins cover the whole section
    assert abs(area[9] - 0.21 * 0.33) <= bound[9] + 8 * xr.EPS


def test_bin_grids_of_1x1_and_64x64(planner, kuhn, tmp_path):
    one = S.line([0.1, 0.2], [0.9, 0.7], s_edges=[0.0, 8.0], name="1 x 1")          # (the strip leaves the cube at s = 1.06)
    fine = S.line([0.1, 0.2], [0.9, 0.7], s_edges=np.linspace(0.0, 8.0, 65), z_edges=np.linspace(-1.5, 6.5, 65), name="64 x 64")
    counts, area, bound = checked(planner, tmp_path, kuhn, [one, fine], "1 x 1 and 64 x 64 bins")
    assert len(counts) == 1 + 4096 and counts[0] > 0
    grid = counts[1:].reshape(64, 64)
    assert (grid[9:] == 0).all() and (grid[:, 12:] == 0).all() and (grid[:, :4] == 0).all() and (grid > 0).sum() < 0.02 * 4096
    assert abs(area[1:].sum() - area[0]) <= bound.sum()
    mask = np.zeros(len(kuhn), dtype=bool)
    mask[::3] = True
    mcounts, marea, _ = checked(planner, tmp_path, kuhn, [one], "1 x 1 bins, every third cell", mask)
    assert 0 < mcounts[0] < counts[0] and marea[0] < area[0]


def test_refusals_come_back_as_messages(planner, kuhn, tmp_path):
    for secs, word in (([S.latitude(0.3, z_edges=[-1.0, -1.0, 0.0])], "strictly increasing"), ([S.latitude(0.3, z_edges=[-1.0, np.inf, 2.0])], "not finite"),
                       ([S("skew", [0, 0, 0], [0, 1.0, 0], [1.0, 1e-6, 0], [0, 0, 1.0])], "orthonormal"), ([S.latitude(np.inf)], "frame is not finite"),
                       ([S.latitude(0.1 * k) for k in range(65)], "nsec must be"),
                       ([S.latitude(0.3, x_edges=np.arange(1026.0), z_edges=np.arange(1026.0))], "2^20 bins")):
        meta, msg, _ = plan(planner, str(tmp_path), kuhn, secs)
        assert meta["status"] == 1 and word in msg, (word, msg)
    bad = kuhn.copy()
    bad[17, 2, 1] = np.nan
    meta, msg, _ = plan(planner, str(tmp_path), bad, [S.latitude(0.3)])
    assert meta["status"] == 1 and "cell 17" in msg
