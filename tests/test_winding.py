"""Winding numbers (S7_winding_line.py), the parts that need no GPU: the numpy
checker tests/winding_ref.py reproduces tests/golden/G10_winding.npz -- the
reference's own ring orders, level-0 winding numbers at every vertex, and the
counts, types and per-level winding numbers of its singular points -- and the
package's argument checks raise before the library is called.

Bars. Ring tables, counts, types and index compare exactly. A winding number
compares within n_ring * sqrt(8 * 2^-52) / 2 pi, computed from each ring's
size: arccos near +-1 turns one rounding of the dot into an angle error of
about 3e-8 at worst, which bounds any reordering of the same operations and
sits five orders below the narrowest threshold (1e-3)."""
import numpy as np
import pytest

from conftest import load_golden

import winding_ref as W

import mofhip.winding  # noqa: F401  (the feature under test)

FIXTURES = {"W1": ("G1_ico642", (25, 8)), "G2_cap641": ("G2_cap641", (25, 8)), "G3_ico642_f32": ("G3_ico642_f32", (8,))}


@pytest.fixture(scope="module")
def g10():
    return load_golden("G10_winding")


def mesh_of(g10, name):
    g = load_golden(FIXTURES[name][0])
    if name == "W1":
        return g10["W1_coordinates"], g["triangles"], g10["W1_e"]
    return g["coordinates"], g["triangles"], g["e"]


@pytest.fixture(scope="module")
def checked(g10):
    """winding_ref's dense map on every mesh, computed once and never modified."""
    made = {}

    def get(name):
        if name not in made:
            pts, tri, e = mesh_of(g10, name)
            adj = W.adjacency(tri, len(pts))
            wn0, idx = W.winding_map(pts, tri, e, g10[name + "_V"], adj)
            wn0.setflags(write=False)
            idx.setflags(write=False)
            made[name] = (adj, wn0, idx)
        return made[name]

    return get


@pytest.mark.parametrize("name", list(FIXTURES))
def test_checker_reproduces_level0_everywhere(g10, checked, name):
    adj, wn0, idx = checked(name)
    assert np.array_equal(idx, g10[name + "_index"])
    bound = W.wn_bound(np.array([len(a) for a in adj]))
    assert np.isfinite(wn0).all()
    assert (np.abs(wn0 - g10[name + "_wn0"]) <= bound).all()
    assert (np.abs(wn0 - np.rint(wn0)) <= bound).all()  # a closed polygon of vectors winds a whole number of times


@pytest.mark.parametrize("name", list(FIXTURES))
def test_checker_reproduces_the_singular_points(g10, checked, name):
    pts, tri, e = mesh_of(g10, name)
    adj = checked(name)[0]
    V, sp, fld = g10[name + "_V"], g10[name + "_sp_points"], g10[name + "_sp_field"]
    cen = W.closest_vertices(pts, sp)
    assert np.array_equal(cen, g10[name + "_sp_centre"])
    levels = FIXTURES[name][1]
    off, vtx = W.ring_table(pts, tri, e, cen, levels[0], adj)
    assert np.array_equal(off, g10[name + "_sp_ring_off"]) and np.array_equal(vtx, g10[name + "_sp_ring_vtx"])
    for L in levels:
        for q, c in enumerate(cen.tolist()):
            rings = W.centre_rings(pts, tri, e, c, L, adj)
            wn, cnt, typ = W.levels(pts, e, V[fld[q]], c, rings, L)
            ref = g10["%s_sp_wn%d" % (name, L)][q]
            assert cnt == g10["%s_sp_count%d" % (name, L)][q] and typ == g10["%s_sp_type%d" % (name, L)][q]
            assert np.array_equal(np.isnan(wn), np.isnan(ref))
            for l in np.flatnonzero(~np.isnan(wn)):
                b = W.wn_bound(len(rings[l]))
                assert abs(wn[l] - ref[l]) <= b and abs(wn[l] - round(wn[l])) <= b
        # the reference-named function: its list shapes
        for k in np.unique(fld):
            sel = fld == k
            counts, types = W.calculate_winding_numbers(pts, tri, e, sp[sel], V[k], L, adj)
            t = g10["%s_sp_type%d" % (name, L)][sel]
            assert counts == g10["%s_sp_count%d" % (name, L)][sel].tolist() and types == t[t != 0].tolist()


@pytest.mark.parametrize("name", list(FIXTURES))
def test_fixture_conditions(g10, checked, name):
    """What the maker asserted from the reference's own operations, from the
    checker's: on every ring evaluated, the failing one included, adjacent
    polar keys differ by >= 1e-9 and pi - |angle| >= 1e-6."""
    pts, tri, e = mesh_of(g10, name)
    adj = checked(name)[0]
    V = g10[name + "_V"]
    gap = ang = np.inf
    for c in range(len(pts)):
        ring = W.sort_ring(pts, e, c, adj[c])
        k = W.polar_keys(pts, e, c, ring)
        gap = min(gap, np.diff(k).min())
        for Vk in V:
            ang = min(ang, (np.pi - np.abs(W.ring_angles(Vk, e, c, ring))).min())
    L = FIXTURES[name][1][0]
    wn_ref = g10["%s_sp_wn%d" % (name, L)]
    for q, c in enumerate(g10[name + "_sp_centre"].tolist()):
        rings = W.centre_rings(pts, tri, e, c, L, adj)
        for l in np.flatnonzero(~np.isnan(wn_ref[q])):
            gap = min(gap, np.diff(W.polar_keys(pts, e, c, rings[l])).min())
            ang = min(ang, (np.pi - np.abs(W.ring_angles(V[g10[name + "_sp_field"][q]], e, c, rings[l]))).min())
    print(name, "min key gap %.3g, min pi - |angle| %.3g" % (gap, ang))
    assert gap >= 1e-9 and ang >= 1e-6


def test_fixture_covers_the_cases(g10):
    t = g10["W1_sp_type25"]
    assert (t == 1).sum() >= 4 and (t == -1).sum() >= 2  # nodes and saddles
    assert g10["W1_sp_count25"].max() >= 20 and g10["W1_sp_count8"].max() == 8
    assert np.diff(g10["G2_cap641_sp_ring_off"], axis=1).max() == 68  # a ring wider than a wave
    assert (g10["G2_cap641_sp_count25"] == 0).any()  # level 0 fails, level 1 is still evaluated
    q = int(np.flatnonzero(g10["G2_cap641_sp_count25"] == 0)[0])
    assert np.isfinite(g10["G2_cap641_sp_wn25"][q, :2]).all() and np.isnan(g10["G2_cap641_sp_wn25"][q, 2:]).all()
    assert g10["W1_coordinates"].dtype == np.float64 and float(g10["W1_ref_seconds_per_point"]) > 0.01


def test_empty_rings_and_thresholds():
    # a single triangle: one ring, then the mesh is exhausted
    tri = np.array([[0, 1, 2]])
    adj = W.adjacency(tri, 3)
    assert [r.tolist() for r in W.rings(adj, 0, 5)] == [[1, 2]]
    pts = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    e = np.tile(np.array([[1.0, 0, 0], [0, 1, 0]]), (3, 1, 1))
    wn, cnt, typ = W.levels(pts, e, np.ones((3, 3)), 0, W.centre_rings(pts, tri, e, 0, 5, adj), 5)
    assert abs(wn[0]) <= W.wn_bound(2) and np.isnan(wn[1:]).all() and cnt == 0 and typ == 0
    assert W.level0_type(0.99) == 1 and W.level0_type(-1.01) == -1 and W.level0_type(np.nan) == 0
    assert W.check_property(1.001, 1) and not W.check_property(0.99, 1) and not W.check_property(1.0, 0)
    # equal keys go to the smaller id
    pts = np.array([[0.0, 0, 0], [2, 0, 0], [1, 0, 0], [0, 1, 0]])
    e = np.tile(np.array([[1.0, 0, 0], [0, 1, 0]]), (4, 1, 1))
    assert W.sort_ring(pts, e, 0, np.array([1, 2, 3])).tolist() == [1, 2, 3]
    assert W.closest_vertices(np.array([[0.0, 0, 0], [2, 0, 0], [2, 0, 0]]), [[1.0, 0, 0], [3, 0, 0]]).tolist() == [0, 1]


def test_entry_points_are_exported():
    from mofhip import _lib as L
    for name in ("mof_winding_rings", "mof_winding_levels", "mof_winding_map", "mof_test_winding_pass",
                 "mof_winding_timing", "mof_closest_vertices"):
        assert name in L.EXPORTS
        assert hasattr(L.lib(), name)
    assert L.lib().mof_abi_version() == 4 and L.MOF_WIND_ALL_LEVELS == 1024


def test_package_exports_winding():
    import mofhip
    import mofhip.winding as S
    for name in ("winding_map", "winding_map_device", "winding_levels", "winding_levels_device", "winding_rings",
                 "closest_vertices", "calculate_winding_numbers", "winding_lines"):
        assert callable(getattr(S, name))
        assert getattr(mofhip, name) is getattr(S, name)


class _NoDevice:
    """A mesh stand-in whose handle must never be asked for."""
    N, f32_points = 7, False
    _xyz = np.zeros((7, 3))

    def handle(self, device=None):
        raise AssertionError("the library was called")

    lock = handle


def test_python_argument_errors():
    import mofhip.winding as S
    m = _NoDevice()
    good = np.ones((2, 7, 3))
    for bad in (np.ones((2, 6, 3)), np.ones((2, 7, 2)), np.ones((0, 7, 3)), np.ones(21),
                np.ones((2, 7, 3), dtype=complex)):
        with pytest.raises(ValueError):
            S.winding_map(m, bad)
        with pytest.raises(ValueError):
            S.winding_levels(m, bad, [0], [0])
        with pytest.raises(ValueError):
            S.winding_lines(m, [[np.zeros(3)]], bad)
    for frame, centre, ml in (([2], [0], 25), ([0], [7], 25), ([-1], [0], 25), ([0, 1], [0], 25), ([], [], 25),
                              ([0.5], [0], 25), ([0], [0], 0), ([0], [0], 2.5), ([0], [0], 2 ** 15)):
        with pytest.raises(ValueError):
            S.winding_levels(m, good, frame, centre, ml)
    for centres, ml in (([7], 3), ([-1], 3), ([], 3), ([[0]], 3), ([0], 0)):
        with pytest.raises(ValueError):
            S.winding_rings(m, centres, ml)
    for pts in (np.zeros(2), np.zeros((2, 2)), np.zeros((0, 3)), np.zeros((1, 1, 3)), np.full((1, 3), "x")):
        with pytest.raises(ValueError):
            S.closest_vertices(m, pts)
    with pytest.raises(ValueError):
        S.calculate_winding_numbers(m, [np.zeros(3)], good)  # two fields
    with pytest.raises(ValueError):
        S.calculate_winding_numbers(m, [np.zeros(3)], good[0], e=np.zeros((7, 3, 2)))
    with pytest.raises(ValueError):
        S.calculate_winding_numbers(m, [np.zeros(3)], good[0], max_level=0)
    with pytest.raises(ValueError):
        S.winding_lines(m, [[], [], []], good)  # more frames than fields
    for args, kw in (((0, 2), {"wn0_ptr": 8}), ((8, 0), {"wn0_ptr": 8}), ((8, 2), {})):
        with pytest.raises(ValueError):
            S.winding_map_device(m, *args, **kw)
    for args, kw in (((8, 2, 8, 8, 0), {"wn_ptr": 8}), ((8, 2, 0, 8, 4), {"wn_ptr": 8}), ((8, 2, 8, 8, 4), {}),
                     ((8, 2, 8, 8, 4), {"wn_ptr": 8, "max_level": 0})):
        with pytest.raises(ValueError):
            S.winding_levels_device(m, *args, **kw)
    assert S.calculate_winding_numbers(m, [], good[0]) == ([], [])
    assert S.winding_lines(m, [[], []], good) == {}
