"""Geodesic distances on the GPU (mof_geodesic, mof_geodesic_edges) and the
reference's error score on them, against tests/geodesic_ref.py (scipy's
Dijkstra on the edges the library exports; pinned to the reference's outputs
by test_geodesic.py) and tests/golden/G11_geodesic.npz.

Bars. Every distance comparison is ``np.array_equal``, no vertex or source
excluded: the definition (include/mof.h) is the fixed point of
d[v] = min(d[v], d[u] + w) from +inf, which Dijkstra's algorithm and any
schedule of relaxations reach in the same bits. The score's integers and
per-match errors compare exactly; its sums too, since the port adds in the
reference's order.
"""
import ctypes

import numpy as np
import pytest

from conftest import load_golden

import geodesic_ref as G
from mofhip import DeviceMesh, synth
from mofhip import _lib as L
from mofhip.geodesic import (compute_displacement_difference, compute_err_for_all_Vk, geodesic_counters,
                             geodesic_distance, geodesic_distances, geodesic_distances_device, geodesic_edges,
                             geodesic_timing)

pytestmark = pytest.mark.gpu

TILE = 32  # vertices per tile the library chooses (csrc/mof_geodesic.hip kGeoTile)
FIXTURES = {"W1": "G1_ico642", "G2_cap641": "G2_cap641", "G3_ico642_f32": "G3_ico642_f32"}


@pytest.fixture(scope="module")
def g11():
    return load_golden("G11_geodesic")


@pytest.fixture(scope="module")
def meshes():
    """(points, triangles, handle) per fixture and vertex order, made once."""
    g10 = load_golden("G10_winding")
    made = {}

    def get(name, reorder=True):
        if (name, reorder) not in made:
            g = load_golden(FIXTURES[name])
            if name == "W1":
                pts, nrm, areas = (g10["W1_" + k] for k in ("coordinates", "normals", "areas"))
            else:
                pts, nrm, areas = g["coordinates"], g["normals"], g["areas"]
            made[name, reorder] = (pts, g["triangles"], DeviceMesh(pts, nrm, g["triangles"], areas, reorder=reorder))
        return made[name, reorder]

    yield get
    for rec in made.values():
        rec[2].close()


@pytest.fixture(scope="module")
def graphs(meshes):
    """The checker's graph on the edges the library exports, per fixture."""
    made = {}

    def get(name):
        if name not in made:
            pts, _, m = meshes(name)
            e, w = geodesic_edges(m)
            made[name] = G.graph(len(pts), e[:, 0], e[:, 1], w)
        return made[name]

    return get


@pytest.fixture(scope="module")
def big():
    """The shuffled 10,242-vertex sphere: the handle, 70 seeded sources and
    scipy's rows for them on the exported edges; computed once, never modified."""
    p, t = synth.icosphere(32, jitter=0.005)
    p, t, _ = synth.permute_vertices(p, t, seed=3)
    m = DeviceMesh(p, synth.vertex_normals(p, t), t, synth.triangle_areas(p, t))
    e, w = geodesic_edges(m)
    assert np.array_equal(e, G.mesh_edges(t)) and np.array_equal(w, G.edge_lengths(p, e))
    src = np.random.default_rng(11).choice(len(p), 70, replace=False).astype(np.int32)
    ref = G.distances(G.graph(len(p), e[:, 0], e[:, 1], w), src)
    ref.setflags(write=False)
    yield m, src, ref
    m.close()


@pytest.fixture
def hooks():
    lib = L.lib()

    def set_(tile=0, pass_=0):
        assert lib.mof_test_geodesic_tile(tile) == L.MOF_OK and lib.mof_test_geodesic_pass(pass_) == L.MOF_OK
    yield set_
    lib.mof_test_geodesic_tile(0)
    lib.mof_test_geodesic_pass(0)


def boundary_vertices(tri):
    edges = np.sort(np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]), axis=1)
    uniq, cnt = np.unique(edges, axis=0, return_counts=True)
    return np.unique(uniq[cnt == 1])


def sources_for(name, tri, n, S):
    """S seeded sources, unsorted, with repeats from S = 3 on; on the cap a boundary vertex among them."""
    src = np.random.default_rng(100 + S).integers(0, n, S).astype(np.int32)
    if name == "G2_cap641":
        src[0] = boundary_vertices(tri)[5]
    if S >= 3:
        src[2] = src[0]
    return src


def device_rows(m, src, targets=None, limit=np.inf):
    import torch
    dev = torch.device("cuda", 0)
    s = torch.from_numpy(np.ascontiguousarray(src, dtype=np.int32)).to(dev)
    t = None if targets is None else torch.from_numpy(np.ascontiguousarray(targets, dtype=np.int32)).to(dev)
    return geodesic_distances_device(m, s, t, limit).cpu().numpy()


@pytest.mark.parametrize("name", list(FIXTURES))
def test_edge_export(meshes, name):
    pts, tri, m = meshes(name)
    e, w = geodesic_edges(m)
    assert e.dtype == np.int32 and w.dtype == np.float64
    ref = G.mesh_edges(tri)
    assert np.array_equal(e, ref)
    p = np.asarray(pts).astype(np.float64)
    d = p[ref[:, 0]] - p[ref[:, 1]]
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    assert np.array_equal(w, np.sqrt((dx * dx + dy * dy) + dz * dz))
    # the capacity convention of mof_winding_rings
    total = ctypes.c_int64(-7)
    a, b, ww = np.full(len(ref), -7, np.int32), np.full(len(ref), -7, np.int32), np.full(len(ref), -7.0)
    with m.lock():
        rc = L.lib().mof_geodesic_edges(m.handle(), len(ref) - 1, ctypes.byref(total), L.ptr(a), L.ptr(b), L.ptr(ww))
        assert rc == L.MOF_E_ARG and total.value == len(ref) and b"total" in L.lib().mof_last_error()
        assert (a == -7).all() and (b == -7).all() and (ww == -7).all()
        rc = L.lib().mof_geodesic_edges(m.handle(), len(ref), ctypes.byref(total), L.ptr(a), L.ptr(b), L.ptr(ww))
    assert rc == L.MOF_OK and np.array_equal(np.stack([a, b], axis=1), ref) and np.array_equal(ww, w)


@pytest.mark.parametrize("name", ["W1", "G2_cap641"])
@pytest.mark.parametrize("S", [1, 3, 64, 65, 130])
def test_full_rows(meshes, graphs, name, S):
    pts, tri, m = meshes(name)
    _, _, m0 = meshes(name, reorder=False)
    src = sources_for(name, tri, len(pts), S)
    ref = G.distances(graphs(name), src)
    got = geodesic_distances(m, src)
    assert got.dtype == np.float64 and got.shape == (S, len(pts))
    assert np.array_equal(got, ref)
    assert geodesic_counters()["passes"] == (len(np.unique(src)) + 63) // 64
    assert np.array_equal(device_rows(m, src), ref)
    assert np.array_equal(geodesic_distances(m0, src), ref)
    assert np.array_equal(device_rows(m0, src), ref)


def test_float32_points_rows(meshes, graphs):
    pts, tri, m = meshes("G3_ico642_f32")
    src = sources_for("G3_ico642_f32", tri, len(pts), 65)
    assert np.array_equal(geodesic_distances(m, src), G.distances(graphs("G3_ico642_f32"), src))


def test_schedule_independence(meshes, graphs, hooks):
    pts, tri, m = meshes("W1")
    src = sources_for("W1", tri, len(pts), 20)
    ref = G.distances(graphs("W1"), src)
    for tile in (1, 100, 256, 0):  # 1: clamped to the smallest supported; 100: a ragged last tile of 42; 256: the largest
        for pass_ in (1, 7, 0):
            hooks(tile, pass_)
            got = geodesic_distances(m, src)
            c = geodesic_counters()
            print("tile", tile, "pass", pass_, c)
            assert np.array_equal(got, ref), (tile, pass_)
            U = len(np.unique(src))
            assert c["pass"] == (pass_ or 64) and c["passes"] == -(-U // c["pass"])
            assert c["tile"] == {1: 4, 100: 100, 256: 256, 0: TILE}[tile] and c["tiles"] == -(-len(pts) // c["tile"])
            assert c["rounds"] >= c["passes"] and c["launches"] >= c["rounds"]
            if tile == 1:
                assert c["tiles"] == 161 and c["rounds"] > 2 * c["passes"]  # many tiles: more than one round a pass
                assert c["tile_executions"] > c["tiles"]
    hooks(0, 0)
    assert np.array_equal(geodesic_distances(m, src), ref)


def test_many_rounds_at_the_default_tile(big):
    m, src, ref = big
    got = geodesic_distances(m, src)
    c, ms = geodesic_counters(), geodesic_timing()
    print(c, ms)
    assert np.array_equal(got, ref)
    assert c["tile"] == TILE and c["tiles"] == -(-10242 // TILE) and c["passes"] == 2
    assert c["rounds"] > 2 * c["passes"] and c["tile_executions"] > c["tiles"] * c["passes"]
    assert np.array_equal(device_rows(m, src[:5]), ref[:5])


def test_targets(meshes, graphs, big):
    pts, tri, m = meshes("G2_cap641")
    src = sources_for("G2_cap641", tri, len(pts), 65)
    full = geodesic_distances(m, src)
    tgt = np.array([5, 640, 5, 0, int(src[0]), 333, 5], dtype=np.int32)
    got = geodesic_distances(m, src, tgt)
    assert got.shape == (65, 7) and np.array_equal(got, full[:, tgt])
    assert np.array_equal(device_rows(m, src, tgt), full[:, tgt])
    one = geodesic_distances(m, src, [17])
    assert one.shape == (65, 1) and np.array_equal(one[:, 0], full[:, 17])
    d = geodesic_distance(m, int(src[3]), 17)
    assert type(d) is float and d == full[3, 17] and geodesic_distance(m, 9, 9) == 0.0
    bm, bsrc, bref = big
    tgt = np.random.default_rng(5).integers(0, bref.shape[1], 300).astype(np.int32)
    assert np.array_equal(geodesic_distances(bm, bsrc, tgt), bref[:, tgt])


def test_limit(big):
    m, src, ref = big
    src, ref = src[:3], ref[:3]
    geodesic_distances(m, src)
    unlimited = geodesic_counters()["tile_executions"]
    dmax = float(ref.max())
    attained = float(np.sort(ref[1])[len(ref[1]) // 3])  # exactly one distance value of source 1
    for lim in (dmax / 4, dmax / 2, attained):
        got = geodesic_distances(m, src, limit=lim)
        c = geodesic_counters()
        keep = ref <= lim
        assert keep.any() and not keep.all()
        assert np.array_equal(got[keep], ref[keep]) and np.isposinf(got[~keep]).all()
        assert np.array_equal(device_rows(m, src, None, lim), got)
        if lim == dmax / 4:
            print("tile executions: unlimited", unlimited, "at a quarter of the largest distance", c["tile_executions"])
            assert c["tile_executions"] < unlimited
    assert (geodesic_distances(m, src, limit=attained)[1] == attained).any()
    tgt = np.array([int(src[0]), 7, 4000], dtype=np.int32)
    got = geodesic_distances(m, src, tgt, limit=dmax / 4)
    assert np.array_equal(got, np.where(ref[:, tgt] <= dmax / 4, ref[:, tgt], np.inf))


def test_unreachable():
    """Two disjoint copies of the cap in one mesh: +inf across, each copy as alone."""
    g = load_golden("G2_cap641")
    pts, tri, n = g["coordinates"], g["triangles"], len(g["coordinates"])
    p2 = np.concatenate([pts, pts + np.array([40.0, 0.0, 0.0])])
    t2 = np.concatenate([tri, tri + n]).astype(np.int32)
    m = DeviceMesh(p2, np.concatenate([g["normals"]] * 2), t2, np.concatenate([g["areas"]] * 2))
    try:
        e, w = geodesic_edges(m)
        assert np.array_equal(e, G.mesh_edges(t2))
        src = np.array([3, n + 100, 3], dtype=np.int32)
        ref = G.distances(G.graph(2 * n, e[:, 0], e[:, 1], w), src)
        got = geodesic_distances(m, src)
        assert np.array_equal(got, ref)
        assert np.isposinf(got[0, n:]).all() and np.isfinite(got[0, :n]).all()
        assert np.isposinf(got[1, :n]).all() and np.isfinite(got[1, n:]).all()
        assert np.isposinf(geodesic_distance(m, 3, n + 3))
    finally:
        m.close()


@pytest.mark.parametrize("name", ["W1", "G2_cap641"])
def test_score_reproduces_the_reference(g11, meshes, name):
    _, _, m = meshes(name)
    thr, tp, F = float(g11[name + "_threshold"]), int(g11[name + "_turning_point"]), int(g11[name + "_n_frames"])
    det = [list(x) for x in G.split_frames(g11[name + "_det_points"], g11[name + "_det_frame"], F)]
    true = [list(x) for x in G.split_frames(g11[name + "_true_points"], g11[name + "_true_frame"], F)]
    el, ef = g11[name + "_err_list"], g11[name + "_err_list_frame"]
    # the distance rows the reference's run used
    rows = geodesic_distances(m, g11[name + "_src_vertex"])
    assert np.array_equal(rows, g11[name + "_src_rows"])
    for t in range(F):
        err, err_list, matched, spare, missed = compute_displacement_difference(thr, det[t], true[t], m, t, tp)
        assert err_list == el[ef == t].tolist() and all(type(x) is float for x in err_list)
        assert err == g11[name + "_frame_err"][t]  # added in the reference's order
        assert (matched, spare, missed) == tuple(int(g11[name + "_frame_" + k][t]) for k in ("matched", "spare", "missed"))
        assert all(type(x) is int for x in (matched, spare, missed))
    tot = compute_err_for_all_Vk(true, det, thr, m, tp)
    assert geodesic_counters()["passes"] == 1  # one distance call for all frames
    n, total = len(el), g11[name + "_total"]
    assert abs(tot[0] - total[0]) <= n * 2.0 ** -52 * total[0] and tot[0] == total[0]
    assert list(tot[1:4]) == total[1:].tolist() and list(tot[4:]) == g11[name + "_total_int"].tolist()
    from utils import find_singularity_point as F_
    assert F_.compute_err_for_all_Vk(true, det, thr, m, tp) == tot
    # the reference's errors on too few matches
    import statistics
    with pytest.raises(ValueError):
        compute_err_for_all_Vk(true[3:4], det[3:4], thr, m, tp)  # no detected point: no match at all
    with pytest.raises(statistics.StatisticsError):
        compute_err_for_all_Vk([true[1][:1]], [det[1]], 1e9, m, tp)  # one match


def test_error_paths(meshes):
    _, _, m = meshes("G2_cap641")
    lib = L.lib()
    out = np.full((2, 641), -7.0)

    def call(src, S, tgt=None, Q=0, limit=np.inf, dist=out):
        s = np.ascontiguousarray(src, dtype=np.int32)
        t = None if tgt is None else np.ascontiguousarray(tgt, dtype=np.int32)
        with m.lock():
            rc = lib.mof_geodesic(m.handle(), L.ptr(s), S, None if t is None else L.ptr(t), Q, limit, 0, None,
                                  None if dist is None else L.ptr(dist))
            return rc, lib.mof_last_error()

    for args in (dict(src=[0, 641], S=2), dict(src=[-1, 0], S=2), dict(src=[0, 1], S=0),
                 dict(src=[0, 1], S=2, tgt=[641], Q=1), dict(src=[0, 1], S=2, tgt=[0], Q=0),
                 dict(src=[0, 1], S=2, limit=float("nan")), dict(src=[0, 1], S=2, limit=0.0),
                 dict(src=[0, 1], S=2, limit=-1.0), dict(src=[0, 1], S=2, dist=None)):
        rc, msg = call(**args)
        assert rc == L.MOF_E_ARG and len(msg) > 0, args
        assert (out == -7).all()
    assert b"641" in call([0, 641], 2)[1] and b"limit" in call([0, 1], 2, limit=float("nan"))[1]
    with pytest.raises(L.MofError):
        L.check(call([0, 641], 2)[0])
    rc, _ = call([0, 1], 2)
    assert rc == L.MOF_OK and (out[[0, 1], [0, 1]] == 0).all() and (out >= 0).all()
