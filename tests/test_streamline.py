"""Streamlines (S6_streamline.py), the parts that need no GPU: the numpy
checker tests/streamline_ref.py reproduces tests/golden/G9_streamlines.npz --
the successor map, the walk lengths and the line lists derived from the
reference's own output -- exactly, and the package's argument checks raise
before the library is called."""
import numpy as np
import pytest

from conftest import load_golden

import streamline_ref

MESHES = ["G1_ico642", "G2_cap641", "G3_ico642_f32"]


@pytest.fixture(scope="module")
def g9():
    return load_golden("G9_streamlines")


@pytest.fixture(scope="module")
def checked(g9):
    """streamline_ref on every mesh, computed once and never modified."""
    made = {}

    def get(name):
        if name not in made:
            g = load_golden(name)
            V = g9[name + "_V"]
            det = {}
            nxt = streamline_ref.successor_map(g["coordinates"], g["triangles"], g["e"], V, details=det)
            length = streamline_ref.lengths(nxt, V)
            for a in (nxt, length):
                a.setflags(write=False)
            made[name] = (nxt, length, det)
        return made[name]

    return get


@pytest.mark.parametrize("name", MESHES)
def test_checker_reproduces_the_reference(g9, checked, name):
    nxt, length, det = checked(name)
    assert np.array_equal(nxt, g9[name + "_next"])
    assert np.array_equal(length, g9[name + "_length"])
    assert np.array_equal(det["boundary_tests"], g9[name + "_boundary_tests"])
    assert not det["boundary_passed"].any()  # every boundary-edge test ends the walk
    # the condition the fixture was made under: decisions compare exactly
    V = g9[name + "_V"]
    assert (det["margin"].min(axis=1) >= 1e-6 * np.abs(V).max(axis=(1, 2))).all()


@pytest.mark.parametrize("name", ["G1_ico642", "G2_cap641"])
def test_checker_lists_at_default_length(g9, checked, name):
    nxt, length, _ = checked(name)
    off, vtx = streamline_ref.line_lists(nxt[0], length[0], 20)
    assert np.array_equal(off, g9[name + "_lines20_off"])
    assert np.array_equal(vtx, g9[name + "_lines20_vtx"])


def test_fixture_covers_the_ending_cases(g9):
    assert (g9["G1_ico642_next"] >= 0).all()  # no terminal vertex: every walk ends on a repeat
    assert int(g9["G1_ico642_length"].max()) == 164
    assert list(g9["G2_cap641_boundary_tests"]) == [51, 48, 72]
    assert list((g9["G2_cap641_next"] < 0).sum(axis=1)) == [51, 48, 72]
    assert (g9["G1_ico642_ref_seconds_per_frame"] > 1).all()


def test_vertex_subset_matches_full_run(g9, checked):
    g = load_golden("G2_cap641")
    sub = list(range(0, 641, 37))
    part = streamline_ref.successor_map(g["coordinates"], g["triangles"], g["e"], g9["G2_cap641_V"], vertices=sub)
    assert np.array_equal(part, checked("G2_cap641")[0][:, sub])


def test_walk_ends_on_terminal_and_on_repeat():
    nxt = np.array([1, 2, 3, 1, -1, 4], dtype=np.int32)
    assert streamline_ref.walk(nxt, 0) == [0, 1, 2, 3]
    assert streamline_ref.walk(nxt, 2) == [2, 3, 1]
    assert streamline_ref.walk(nxt, 5) == [5, 4]
    assert streamline_ref.walk(nxt, 4) == [4]
    V = np.ones((6, 3))
    V[5] = 0
    assert list(streamline_ref.lengths(nxt, V)[0]) == [4, 3, 3, 3, 1, 0]


def test_entry_points_are_exported():
    from mofhip import _lib as L
    for name in ("mof_streamline_map", "mof_streamlines", "mof_test_streamline_pass"):
        assert name in L.EXPORTS
        assert hasattr(L.lib(), name)
    assert L.lib().mof_abi_version() == 4


def test_package_exports_streamline():
    import mofhip
    import mofhip.streamline as S
    for name in ("streamline_map", "streamline_map_device", "streamline_lists",
                 "track_static_vectorfields_over_time", "extract_static_streamline_dot_product"):
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
    import mofhip.streamline as S
    m = _NoDevice()
    good = np.ones((2, 7, 3))
    for bad in (np.ones((2, 6, 3)), np.ones((2, 7, 2)), np.ones((0, 7, 3)), np.ones((2, 2, 7, 3)), np.ones(21),
                np.ones((2, 7, 3), dtype=complex), np.full((2, 7, 3), "x")):
        with pytest.raises(ValueError):
            S.streamline_map(m, bad)
        with pytest.raises(ValueError):
            S.streamline_lists(m, bad)
    with pytest.raises(ValueError):
        S.streamline_lists(m, good, min_streamline_length=2.5)
    with pytest.raises(ValueError):
        S.streamline_lists(m, good, min_streamline_length=2 ** 31)
    with pytest.raises(ValueError):
        S.streamline_map_device(m, 0, 2, next_ptr=8)
    with pytest.raises(ValueError):
        S.streamline_map_device(m, 8, 0, next_ptr=8)
    with pytest.raises(ValueError):
        S.streamline_map_device(m, 8, 2)
    with pytest.raises(ValueError):
        S.track_static_vectorfields_over_time(m, good, 1, 3)
    with pytest.raises(ValueError):
        S.extract_static_streamline_dot_product(np.zeros(3), good, m)
    with pytest.raises(ValueError):
        S.extract_static_streamline_dot_product(np.zeros(2), good[0], m)
