"""The geodesic checker (tests/geodesic_ref.py) against the reference's own
error score in tests/golden/G11_geodesic.npz, the maker's tie and threshold
assertions re-checked from the fixture, and the argument errors of the Python
layer. Runs without a GPU."""
import types

import numpy as np
import pytest

from conftest import load_golden

import geodesic_ref as G
from mofhip import _lib as L
from mofhip import geodesic as M

MESHES = {"W1": "G1_ico642", "G2_cap641": "G2_cap641"}


@pytest.fixture(scope="module")
def g11():
    return load_golden("G11_geodesic")


@pytest.fixture(scope="module")
def cases(g11):
    """Per mesh: points, triangles, the csr graph and the per-frame vertex lists."""
    g10 = load_golden("G10_winding")
    out = {}
    for name, src in MESHES.items():
        g = load_golden(src)
        pts = g10["W1_coordinates"] if name == "W1" else g["coordinates"]
        e = G.mesh_edges(g["triangles"])
        F = int(g11[name + "_n_frames"])
        out[name] = dict(points=pts, triangles=g["triangles"], graph=G.graph(len(pts), e[:, 0], e[:, 1],
                                                                           G.edge_lengths(pts, e)),
                         det=G.split_frames(g11[name + "_det_vertex"], g11[name + "_det_frame"], F),
                         true=G.split_frames(g11[name + "_true_vertex"], g11[name + "_true_frame"], F), F=F)
    return out


def stored_dist(g11, name):
    src = g11[name + "_src_vertex"].tolist()
    rows = g11[name + "_src_rows"]
    return lambda a, b: float(rows[src.index(int(a))][int(b)])


@pytest.mark.parametrize("name", list(MESHES))
def test_checker_distances_equal_the_stored_rows(g11, cases, name):
    c = cases[name]
    rows = G.distances(c["graph"], g11[name + "_src_vertex"])
    assert rows.dtype == np.float64 and np.array_equal(rows, g11[name + "_src_rows"])
    assert np.isfinite(rows).all() and (rows[np.arange(len(rows)), g11[name + "_src_vertex"]] == 0).all()
    # repeated, unsorted sources and a limit
    src = g11[name + "_src_vertex"][[2, 0, 2, 1]]
    lim = float(np.median(rows))
    got = G.distances(c["graph"], src, lim)
    ref = g11[name + "_src_rows"][[2, 0, 2, 1]]
    assert np.array_equal(got[ref <= lim], ref[ref <= lim]) and np.isinf(got[ref > lim]).all()


@pytest.mark.parametrize("name", list(MESHES))
def test_checker_snaps_like_the_reference(g11, cases, name):
    pts = cases[name]["points"]
    assert np.array_equal(G.closest_vertices(pts, g11[name + "_det_points"]), g11[name + "_det_vertex"])
    assert np.array_equal(G.closest_vertices(pts, g11[name + "_true_points"]), g11[name + "_true_vertex"])


@pytest.mark.parametrize("name", list(MESHES))
def test_checker_score_equals_the_reference(g11, cases, name):
    c = cases[name]
    thr, tp = float(g11[name + "_threshold"]), int(g11[name + "_turning_point"])
    rows = G.distances(c["graph"], g11[name + "_src_vertex"])
    src = g11[name + "_src_vertex"].tolist()
    dist = lambda a, b: float(rows[src.index(int(a))][int(b)])  # noqa: E731
    el, ef = g11[name + "_err_list"], g11[name + "_err_list_frame"]
    for t in range(c["F"]):
        err, err_list, matched, spare, missed = G.displacement_difference(thr, c["det"][t], c["true"][t], dist, t, tp)
        assert err == g11[name + "_frame_err"][t] and err_list == el[ef == t].tolist()
        assert (matched, spare, missed) == tuple(int(g11[name + "_frame_" + k][t]) for k in ("matched", "spare", "missed"))
    tot = G.err_for_all(c["true"], c["det"], thr, dist, tp)
    assert list(tot[:4]) == g11[name + "_total"].tolist() and list(tot[4:]) == g11[name + "_total_int"].tolist()
    # both branches and both outcomes are in the fixture
    assert tp < c["F"] and (g11[name + "_frame_matched"][:tp] > 1).any() and (g11[name + "_frame_missed"][:tp] > 0).any()
    assert (g11[name + "_frame_spare"] > 0).any()
    assert any(len(d) == 0 for d in c["det"]) and float(g11[name + "_ref_seconds_per_frame"]) > 0


@pytest.mark.parametrize("name", list(MESHES))
def test_no_tie_and_no_minimum_at_the_threshold(g11, cases, name):
    c = cases[name]
    thr, tp = float(g11[name + "_threshold"]), int(g11[name + "_turning_point"])
    dist = stored_dist(g11, name)
    seen = 0
    for t in range(tp):
        for a in c["true"][t]:
            if not len(c["det"][t]):
                continue
            row = np.sort([dist(a, b) for b in c["det"][t]])
            assert len(row) == 1 or row[1] > row[0]
            assert abs(row[0] - thr) >= 1e-9
            seen += 1
    assert seen >= 5


def test_edge_lengths_widen_float32_points():
    g = load_golden("G3_ico642_f32")
    pts = g["coordinates"]
    assert pts.dtype == np.float32
    e = G.mesh_edges(g["triangles"])
    assert len(e) == 3 * len(g["triangles"]) // 2 and (e[:, 0] < e[:, 1]).all()
    w = G.edge_lengths(pts, e)
    d = pts[e[:, 0]].astype(np.float64) - pts[e[:, 1]].astype(np.float64)
    assert w.dtype == np.float64 and np.array_equal(w, np.sqrt((d[:, 0] ** 2 + d[:, 1] ** 2) + d[:, 2] ** 2))
    d32 = pts[e[:, 0]] - pts[e[:, 1]]  # subtracted in float32: not the definition
    assert not np.array_equal(w, np.sqrt((d32[:, 0] ** 2 + d32[:, 1] ** 2) + d32[:, 2] ** 2).astype(np.float64))


def test_python_argument_errors():
    mesh = types.SimpleNamespace(N=10)  # rejected before any handle is asked for
    for bad in ([], [[0, 1]], [0.5], [-1], [10], np.zeros(0, dtype=np.int32)):
        with pytest.raises(ValueError):
            M.geodesic_distances(mesh, bad)
        with pytest.raises(ValueError):
            M.geodesic_distances(mesh, [0], targets=bad)
    for lim in (0.0, -1.0, np.nan):
        with pytest.raises(ValueError):
            M.geodesic_distances(mesh, [0], limit=lim)
    with pytest.raises(ValueError):
        M.geodesic_distances_device(mesh, np.array([0], dtype=np.int32))  # no torch tensor on the GPU


def test_binding_and_exports():
    import mofhip
    from utils import find_singularity_point as F
    for name in ("mof_geodesic", "mof_geodesic_edges", "mof_test_geodesic_pass", "mof_test_geodesic_tile",
                 "mof_geodesic_timing", "mof_geodesic_counters"):
        assert name in L.EXPORTS and hasattr(L.lib(), name)
    for name in ("geodesic_distances", "geodesic_distances_device", "geodesic_distance", "geodesic_edges",
                 "compute_displacement_difference", "compute_err_for_all_Vk"):
        assert callable(getattr(mofhip, name))
    assert F.compute_displacement_difference.__module__ == F.__name__
    assert F.compute_err_for_all_Vk.__module__ == F.__name__
    lib = L.lib()
    assert lib.mof_geodesic(None, None, 1, None, 0, 1.0, 0, None, None) == L.MOF_E_ARG
    assert b"NULL" in lib.mof_last_error()
    assert lib.mof_geodesic_counters(None) == L.MOF_E_ARG and lib.mof_geodesic_timing(None) == L.MOF_E_ARG
    assert lib.mof_test_geodesic_pass(0) == L.MOF_OK and lib.mof_test_geodesic_tile(0) == L.MOF_OK


def test_score_matching_on_plain_distances():
    """The host half of the port on hand-made distances: the first minimum
    wins, a taken nearest point hides a farther free one, the + 1 and the
    fixed branch."""
    D = np.array([[1.0, 1.0, 5.0], [1.5, 0.5, 5.0], [0.2, 3.0, 0.1]])
    assert M._match(2.0, D, 3, 3, 0, 4) == (1.0 + 0.5 + 0.1, [1.0, 0.5, 0.1], 4, 0, 0)
    D = np.array([[1.0, 1.8], [1.2, 1.9], [2.5, 2.6]])
    assert M._match(2.0, D, 3, 2, 0, 4) == (1.0, [1.0], 2, 0, 2)
    assert M._match(2.0, None, 3, 0, 0, 4) == (0, [], 0, 0, 3)
    assert M._match(2.0, None, 3, 5, 4, 4) == (0, [], 1, 0, 2)
    assert M._match(2.0, np.empty((0, 5)), 0, 5, 0, 4) == (0, [], 1, 3, 0)
