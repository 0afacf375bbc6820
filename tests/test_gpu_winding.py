"""Winding numbers on the GPU (mof_winding_map, mof_winding_levels,
mof_winding_rings, mof_closest_vertices) against the reference's
S7_winding_line.py: the golden vectors of tests/golden/G10_winding.npz and
the numpy checker tests/winding_ref.py (pinned to them by test_winding.py).

Bars. Ring tables, counts, types and index compare exactly, no vertex or
query excluded: on every ring the fixture evaluates adjacent polar keys differ
by >= 1e-9 and every angle keeps >= 1e-6 from +-pi (asserted by the maker and
by test_winding.py), and the fixture's winding numbers sit >= 9e-4 inside
their thresholds. A winding number compares within n_ring * sqrt(8 * 2^-52) /
2 pi, from each ring's size: arccos near +-1 turns one rounding of the dot
into about 3e-8 of angle at worst, which bounds any reordering of the same
operations. What must not depend on the order of anything -- the map against
the levels, the handle's vertex order, the pass size, where the pointers live
-- compares bit for bit.
"""
import ctypes

import numpy as np
import pytest

from conftest import load_golden

import winding_ref as W
from mofhip import DeviceMesh
from mofhip import _lib as L
from mofhip.winding import (calculate_winding_numbers, closest_vertices, winding_levels, winding_lines, winding_map,
                            winding_rings)

pytestmark = pytest.mark.gpu

FIXTURES = {"W1": ("G1_ico642", (25, 8)), "G2_cap641": ("G2_cap641", (25, 8)), "G3_ico642_f32": ("G3_ico642_f32", (8,))}


@pytest.fixture(scope="module")
def g10():
    return load_golden("G10_winding")


@pytest.fixture(scope="module")
def meshes(g10):
    """(points, triangles, e, handle) per fixture and vertex order, made once."""
    made = {}

    def get(name, reorder=True):
        if (name, reorder) not in made:
            g = load_golden(FIXTURES[name][0])
            if name == "W1":
                pts, nrm, areas, e = (g10["W1_" + k] for k in ("coordinates", "normals", "areas", "e"))
            else:
                pts, nrm, areas, e = g["coordinates"], g["normals"], g["areas"], g["e"]
            made[name, reorder] = (pts, g["triangles"], e, DeviceMesh(pts, nrm, g["triangles"], areas, reorder=reorder))
        return made[name, reorder]

    yield get
    for rec in made.values():
        rec[3].close()


@pytest.fixture(scope="module")
def g2ref(g10, meshes):
    """winding_ref on G2: adjacency, every vertex's sorted rings to level 3 and
    their winding numbers for every field; computed once, never modified."""
    pts, tri, e, _ = meshes("G2_cap641")
    V = g10["G2_cap641_V"]
    adj = W.adjacency(tri, len(pts))
    rings = [W.centre_rings(pts, tri, e, c, 3, adj) for c in range(len(pts))]
    wn = np.full((len(V), len(pts), 3), np.nan)
    for c, rs in enumerate(rings):
        for l, r in enumerate(rs):
            for k in range(len(V)):
                wn[k, c, l] = W.winding_number(V[k], e, c, r)
    wn.setflags(write=False)
    return adj, rings, wn


def ring_sizes(off):
    return np.diff(off, axis=1)


def assert_wn(wn, ref, sizes, what):
    """NaN where the reference is NaN, else within the bound of the ring's size."""
    assert np.array_equal(np.isnan(wn), np.isnan(ref)), what
    ok = ~np.isnan(ref)
    dev = np.abs(wn - ref)[ok]
    bound = np.broadcast_to(W.wn_bound(sizes), ref.shape)[ok]
    print(what, "max |wn - ref| %.3g (bound there %.3g)" % (dev.max(), bound[np.argmax(dev)]))
    assert (dev <= bound).all(), what
    return dev.max()


def raw_levels(m, V, frame, centre, max_level, flags=0, wn=True, count=True, typ=True):
    """mof_winding_levels itself with prefilled outputs: (rc, wn, count, type)."""
    V = np.ascontiguousarray(V, dtype=np.float64)
    f, c = np.ascontiguousarray(frame, dtype=np.int32), np.ascontiguousarray(centre, dtype=np.int32)
    o_wn = np.full((len(f), max_level), -7.0)
    o_c = np.full(len(f), -7, dtype=np.int32)
    o_t = np.full(len(f), -7, dtype=np.int8)
    with m.lock():
        rc = L.lib().mof_winding_levels(m.handle(), L.ptr(V), len(V), L.ptr(f), L.ptr(c), len(f), max_level, flags,
                                        None, L.ptr(o_wn) if wn else None, L.ptr(o_c) if count else None,
                                        L.ptr(o_t) if typ else None)
    return rc, o_wn, o_c, o_t


@pytest.mark.parametrize("name", list(FIXTURES))
def test_map_against_reference(g10, meshes, name):
    pts, tri, e, m = meshes(name)
    assert np.array_equal(m.geometry()[0], e)  # the handle's basis is the reference's, bit for bit
    wn0, index = winding_map(m, g10[name + "_V"])
    assert wn0.dtype == np.float64 and index.dtype == np.int8
    assert np.array_equal(index, g10[name + "_index"])
    deg = np.array([len(a) for a in W.adjacency(tri, len(pts))])
    assert_wn(wn0, g10[name + "_wn0"], deg, name + " map")
    assert (np.abs(wn0 - np.rint(wn0)) <= W.wn_bound(deg)).all()


@pytest.mark.parametrize("name", list(FIXTURES))
def test_levels_against_reference(g10, meshes, name):
    pts, tri, e, m = meshes(name)
    V, sp, fld, cen = (g10[name + k] for k in ("_V", "_sp_points", "_sp_field", "_sp_centre"))
    assert np.array_equal(closest_vertices(m, sp), cen)
    sizes = ring_sizes(g10[name + "_sp_ring_off"])
    for Lv in FIXTURES[name][1]:
        rc, rt, rw = (g10["%s_sp_%s%d" % (name, k, Lv)] for k in ("count", "type", "wn"))
        wn, count, typ = winding_levels(m, V, fld, cen, Lv)
        assert count.dtype == np.int32 and typ.dtype == np.int8
        assert np.array_equal(count, rc) and np.array_equal(typ, rt)
        assert_wn(wn, rw, sizes[:, :Lv], "%s levels at %d" % (name, Lv))
        ok = ~np.isnan(wn)
        assert (np.abs(wn - np.rint(wn))[ok] <= np.broadcast_to(W.wn_bound(sizes[:, :Lv]), wn.shape)[ok]).all()
        # the reference's function, per field, and its __main__'s dict over all of them
        per_frame = [[p for p in sp[fld == k]] for k in range(len(V))]
        for k in range(len(V)):
            counts, types = calculate_winding_numbers(m, per_frame[k], V[k], e, pts, max_level=Lv)
            t = rt[fld == k]
            assert counts == rc[fld == k].tolist() and types == t[t != 0].tolist()
            assert all(type(x) is int for x in counts + types)
        lines = winding_lines(m, per_frame, V, max_level=Lv)
        assert list(lines) == [str(k) for k in range(len(V)) if (fld == k).any()]
        for k in range(len(V)):
            keep = (fld == k) & (rc > 0)
            if (fld == k).any():
                got = lines[str(k)]
                assert [x[1:] for x in got] == [[int(a), int(b)] for a, b in zip(rc[keep], rt[keep])]
                assert all(np.array_equal(x[0], p) for x, p in zip(got, sp[keep]))


@pytest.mark.parametrize("name", list(FIXTURES))
def test_rings_against_reference(g10, meshes, name):
    _, _, _, m = meshes(name)
    cen = g10[name + "_sp_centre"]
    off, vtx = winding_rings(m, cen, FIXTURES[name][1][0])
    assert off.dtype == np.int64 and vtx.dtype == np.int32
    assert np.array_equal(off, g10[name + "_sp_ring_off"]) and np.array_equal(vtx, g10[name + "_sp_ring_vtx"])


def test_every_vertex_all_levels(g10, meshes, g2ref):
    """Every vertex of G2 a centre, every field, max_level 3 with
    MOF_WIND_ALL_LEVELS, against the checker; and the map against the levels,
    bit for bit."""
    pts, tri, e, m = meshes("G2_cap641")
    V = g10["G2_cap641_V"]
    adj, rings, ref = g2ref
    K, N = len(V), len(pts)
    frame, centre = np.repeat(np.arange(K), N), np.tile(np.arange(N), K)
    wn, count, typ = winding_levels(m, V, frame, centre, 3, all_levels=True)
    sizes = np.array([[len(r) for r in rs] + [0] * (3 - len(rs)) for rs in rings])
    assert_wn(wn.reshape(K, N, 3), ref, sizes[None], "G2 every vertex, all levels")
    wn2, count2, typ2 = winding_levels(m, V, frame, centre, 3)
    assert np.array_equal(count, count2) and np.array_equal(typ, typ2)  # unchanged by the flag
    stop = np.isnan(wn2) & ~np.isnan(wn)
    assert stop.any() and not stop[:, :2].any()  # level 1 is always evaluated
    assert np.array_equal(wn2[~stop], wn[~stop], equal_nan=True)
    for q in range(0, K * N, 97):
        w, c, t = W.levels(pts, e, V[frame[q]], int(centre[q]), rings[centre[q]], 3)
        assert (c, t) == (count2[q], typ2[q]) and np.array_equal(np.isnan(w), np.isnan(wn2[q]))
    wn0, index = winding_map(m, V)
    assert np.array_equal(wn0.reshape(-1), wn[:, 0]) and np.array_equal(index.reshape(-1), typ)


def boundary_vertices(tri):
    edges = np.sort(np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]), axis=1)
    uniq, cnt = np.unique(edges, axis=0, return_counts=True)
    return np.unique(uniq[cnt == 1])


def test_boundary_exhausting_and_wide_rings(g10, meshes, g2ref):
    pts, tri, e, m = meshes("G2_cap641")
    V = g10["G2_cap641_V"]
    adj = g2ref[0]
    b = int(boundary_vertices(tri)[3])
    off68 = g10["G2_cap641_sp_ring_off"]
    q68 = int(np.argmax(ring_sizes(off68).max(axis=1)))
    wide = int(g10["G2_cap641_sp_centre"][q68])
    Lv = 60  # past the last ring of every centre of a 641-vertex mesh
    cen = np.array([b, wide, 0, 640], dtype=np.int32)
    off, vtx = winding_rings(m, cen, Lv)
    o2, v2 = W.ring_table(pts, tri, e, cen, Lv, adj)
    assert np.array_equal(off, o2) and np.array_equal(vtx, v2)
    sizes = ring_sizes(off)
    assert sizes.max() == 68 and (sizes[:, -1] == 0).all() and (sizes.sum(axis=1) == 640).all()
    wn, count, typ = winding_levels(m, V, np.full(4, 2), cen, Lv, all_levels=True)
    for q, c in enumerate(cen.tolist()):
        rs = W.centre_rings(pts, tri, e, c, Lv, adj)
        ref, rc, rt = W.levels(pts, e, V[2], c, rs, Lv, all_levels=True)
        assert len(rs) < Lv and np.isnan(wn[q, len(rs):]).all()  # nothing after the mesh is exhausted
        assert_wn(wn[q], ref, sizes[q], "G2 centre %d, 60 levels" % c)
        assert (count[q], typ[q]) == (rc, rt)


def test_small_shapes_and_query_order(g10, meshes, g2ref):
    pts, tri, e, m = meshes("G2_cap641")
    V = g10["G2_cap641_V"]
    _, rings, ref = g2ref
    # Q = 1, K = 1, max_level = 1
    wn, count, typ = winding_levels(m, V[3], [0], [72], 1)
    assert wn.shape == (1, 1) and abs(wn[0, 0] - ref[3, 72, 0]) <= W.wn_bound(len(rings[72][0]))
    assert (count[0], typ[0]) == (1, -1) == (g10["G2_cap641_sp_count25"][3], g10["G2_cap641_sp_type25"][3])
    # repeated, unsorted queries sharing centres across frames
    frame = np.array([3, 0, 3, 1, 2, 0, 3, 3], dtype=np.int32)
    centre = np.array([500, 72, 72, 500, 9, 72, 500, 9], dtype=np.int32)
    a = winding_levels(m, V, frame, centre, 3, all_levels=True)
    for q in range(len(frame)):
        one = winding_levels(m, V[frame[q]], [0], [centre[q]], 3, all_levels=True)
        assert all(np.array_equal(x[q], y[0], equal_nan=True) for x, y in zip(a, one))
    assert np.array_equal(a[0][0], a[0][6], equal_nan=True) and np.array_equal(a[0][2], a[0][2])
    assert_wn(a[0], ref[frame, centre], np.array([[len(r) for r in rings[c]] for c in centre]), "G2 unsorted queries")


def test_nan_and_zero_vectors(g10, meshes, g2ref):
    pts, tri, e, m = meshes("G2_cap641")
    _, rings, _ = g2ref
    V = g10["G2_cap641_V"][2:3].copy()
    q = int(np.flatnonzero(g10["G2_cap641_sp_field"] == 2)[1])
    c = int(g10["G2_cap641_sp_centre"][q])
    assert g10["G2_cap641_sp_count8"][q] == 8
    wn, count, typ = winding_levels(m, np.full_like(V, np.nan), [0], [c], 8)
    assert np.isnan(wn[0, :2]).all() and np.isnan(wn).all() and (count[0], typ[0]) == (0, 0)
    wn0, index = winding_map(m, np.full_like(V, np.nan))
    assert np.isnan(wn0).all() and not index.any()
    V[0, rings[c][2][5]] = 0.0  # one vertex of ring 2: 0 / 0 in the normalisation
    wn, count, typ = winding_levels(m, V, [0], [c], 8)
    ref, rc, rt = W.levels(pts, e, V[0], c, W.centre_rings(pts, tri, e, c, 8), 8)
    assert np.isfinite(wn[0, :2]).all() and np.isnan(wn[0, 2:]).all() and np.array_equal(np.isnan(ref), np.isnan(wn[0]))
    assert (count[0], typ[0]) == (2, g10["G2_cap641_sp_type8"][q]) == (rc, rt)
    wn_all = winding_levels(m, V, [0], [c], 8, all_levels=True)[0]
    assert np.isnan(wn_all[0, 2]) and np.isfinite(wn_all[0, 3:]).all()


def test_vertex_order_of_the_handle(g10, meshes):
    """Reordered (RCM) against MOF_NO_REORDER handles, bit for bit; on G1's
    unjittered sphere too, where polar keys tie exactly beyond level 8 and the
    smaller caller's id decides whatever the internal order is."""
    for name in ("W1", "G2_cap641"):
        _, _, _, m = meshes(name)
        _, _, _, m0 = meshes(name, reorder=False)
        V, fld, cen = (g10[name + k] for k in ("_V", "_sp_field", "_sp_centre"))
        for x, y in zip(winding_map(m, V), winding_map(m0, V)):
            assert np.array_equal(x, y, equal_nan=True)
        for x, y in zip(winding_levels(m, V, fld, cen, 25, all_levels=True),
                        winding_levels(m0, V, fld, cen, 25, all_levels=True)):
            assert np.array_equal(x, y, equal_nan=True)
        for x, y in zip(winding_rings(m, cen, 25), winding_rings(m0, cen, 25)):
            assert np.array_equal(x, y)
    g = load_golden("G1_ico642")
    args = (g["coordinates"], g["normals"], g["triangles"], g["areas"])
    a, b = DeviceMesh(*args), DeviceMesh(*args, reorder=False)
    try:
        cen = np.array([0, 17, 300, 641], dtype=np.int32)
        ra, rb = winding_rings(a, cen, 14), winding_rings(b, cen, 14)
        assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1])
        V = g10["W1_V"]
        for x, y in zip(winding_levels(a, V, [0, 1, 2, 2], cen, 14, all_levels=True),
                        winding_levels(b, V, [0, 1, 2, 2], cen, 14, all_levels=True)):
            assert np.array_equal(x, y, equal_nan=True)
    finally:
        a.close()
        b.close()


@pytest.fixture
def pass_fields():
    def set_(n):
        assert L.lib().mof_test_winding_pass(n) == L.MOF_OK
    yield set_
    L.lib().mof_test_winding_pass(0)


def test_passes_and_device_pointers(g10, meshes, pass_fields):
    import torch
    _, _, _, m = meshes("G2_cap641")
    V = g10["G2_cap641_V"]
    K, N = len(V), 641
    host = winding_map(m, V)
    dev = torch.device("cuda", 0)
    Vd = torch.from_numpy(V.copy()).to(dev)
    for n in (1, 3, 4, 0):
        pass_fields(n)
        for x, y in zip(winding_map(m, V), host):
            assert np.array_equal(x, y, equal_nan=True)
        wd = torch.full((K, N), -7.0, dtype=torch.float64, device=dev)
        ix = torch.full((K, N), -7, dtype=torch.int8, device=dev)
        torch.cuda.synchronize()
        with m.lock():
            L.check(L.lib().mof_winding_map(m.handle(), ctypes.c_void_p(Vd.data_ptr()), K, L.MOF_IO_DEVICE, None,
                                            ctypes.c_void_p(wd.data_ptr()), None))
            assert (ix.cpu().numpy() == -7).all()
            L.check(L.lib().mof_winding_map(m.handle(), ctypes.c_void_p(Vd.data_ptr()), K, L.MOF_IO_DEVICE, None, None,
                                            ctypes.c_void_p(ix.data_ptr())))
        assert np.array_equal(wd.cpu().numpy(), host[0]) and np.array_equal(ix.cpu().numpy(), host[1])
    # host pointers: a NULL output leaves nothing written
    wn0 = np.full((K, N), -7.0)
    with m.lock():
        L.check(L.lib().mof_winding_map(m.handle(), L.ptr(np.ascontiguousarray(V)), K, 0, None, L.ptr(wn0), None))
        assert L.lib().mof_winding_map(m.handle(), L.ptr(np.ascontiguousarray(V)), K, 0, None, None,
                                       None) == L.MOF_E_ARG
    assert np.array_equal(wn0, host[0])
    # the levels: device against host pointers, and NULL outputs
    fld, cen = g10["G2_cap641_sp_field"], g10["G2_cap641_sp_centre"]
    Q = len(fld)
    ref = winding_levels(m, V, fld, cen, 25)
    fd, cd = torch.from_numpy(fld.astype(np.int32)).to(dev), torch.from_numpy(cen.astype(np.int32)).to(dev)
    outs = (torch.full((Q, 25), -7.0, dtype=torch.float64, device=dev),
            torch.full((Q,), -7, dtype=torch.int32, device=dev), torch.full((Q,), -7, dtype=torch.int8, device=dev))
    torch.cuda.synchronize()
    with m.lock():
        L.check(L.lib().mof_winding_levels(m.handle(), ctypes.c_void_p(Vd.data_ptr()), K,
                                           ctypes.c_void_p(fd.data_ptr()), ctypes.c_void_p(cd.data_ptr()), Q, 25,
                                           L.MOF_IO_DEVICE, None, *(ctypes.c_void_p(o.data_ptr()) for o in outs)))
    for o, r in zip(outs, ref):
        assert np.array_equal(o.cpu().numpy(), r, equal_nan=True)
    for keep in range(3):
        flags = [i == keep for i in range(3)]
        rc, *got = raw_levels(m, V, fld, cen, 25, 0, *flags)
        assert rc == L.MOF_OK
        for i in range(3):
            assert np.array_equal(got[i], ref[i], equal_nan=True) if flags[i] else (got[i] == -7).all()
    assert raw_levels(m, V, fld, cen, 25, 0, False, False, False)[0] == L.MOF_E_ARG
    assert raw_levels(m, V, [len(V)], [0], 25)[0] == L.MOF_E_ARG  # a frame outside the fields
    assert raw_levels(m, V, [0], [N], 25)[0] == L.MOF_E_ARG  # a centre that is no vertex


def test_ring_capacity(g10, meshes):
    _, _, _, m = meshes("G2_cap641")
    cen = np.ascontiguousarray(g10["G2_cap641_sp_centre"], dtype=np.int32)
    want_off, want_vtx = g10["G2_cap641_sp_ring_off"], g10["G2_cap641_sp_ring_vtx"]
    total = ctypes.c_int64(-7)
    with m.lock():
        rc = L.lib().mof_winding_rings(m.handle(), L.ptr(cen), len(cen), 25, 0, ctypes.byref(total), None, None)
        assert rc == L.MOF_E_ARG and total.value == len(want_vtx)
        off = np.full((len(cen), 26), -7, dtype=np.int64)
        vtx = np.full(len(want_vtx), -7, dtype=np.int32)
        total.value = -7
        rc = L.lib().mof_winding_rings(m.handle(), L.ptr(cen), len(cen), 25, len(want_vtx) - 1, ctypes.byref(total),
                                       L.ptr(off), L.ptr(vtx))
        assert rc == L.MOF_E_ARG and total.value == len(want_vtx) and (off == -7).all() and (vtx == -7).all()
        assert b"total" in L.lib().mof_last_error()
        rc = L.lib().mof_winding_rings(m.handle(), L.ptr(cen), len(cen), 25, len(want_vtx), ctypes.byref(total),
                                       L.ptr(off), L.ptr(vtx))
        assert rc == L.MOF_OK and np.array_equal(off, want_off) and np.array_equal(vtx, want_vtx)


def test_closest_vertices(g10, meshes):
    rng = np.random.default_rng(7)
    for name in ("G2_cap641", "G3_ico642_f32"):
        pts, tri, _, m = meshes(name)
        p64 = np.asarray(pts, dtype=np.float64)
        bary = rng.dirichlet(np.ones(3), size=200)
        t = tri[rng.integers(0, len(tri), 200)]
        inner = (bary[:, :, None] * p64[t]).sum(axis=1)
        far = rng.normal(size=(50, 3)) * 40
        for q in (p64, inner, far, p64[:1]):
            got = closest_vertices(m, q)
            assert got.dtype == np.int32 and np.array_equal(got, W.closest_vertices(p64, q))
        assert np.array_equal(closest_vertices(m, p64), np.arange(len(pts)))
    # the lower id at the midpoint of an edge (and of a face) of an integer mesh
    xyz = np.array([[0.0, 0, 0], [2, 0, 0], [0, 2, 0], [2, 2, 0]])
    tri = np.array([[0, 1, 2], [1, 3, 2]], dtype=np.int32)
    m = DeviceMesh(xyz, np.tile([0.0, 0, 1], (4, 1)), tri, np.full(2, 2.0))
    m0 = DeviceMesh(xyz, np.tile([0.0, 0, 1], (4, 1)), tri, np.full(2, 2.0), reorder=False)
    try:
        q = np.array([[1.0, 0, 0], [1, 1, 0], [2, 1, 0], [1, 2, 5], [0, 1, -3]])
        for h in (m, m0):
            assert closest_vertices(h, q).tolist() == [0, 0, 1, 2, 0]
    finally:
        m.close()
        m0.close()
