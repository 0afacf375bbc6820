"""The fp64 residual of the mixed-precision refinement with a row slice's
geometry staged in LDS and the systems on waves (k_residual_lds + the fold
of its per-slice partials) against the row kernel k_residual_rcn (forced by
the test hook mof_test_force_residual_rows): the same terms in the same
order and the same partial-sum tree, so V, the residuals, the iteration
counts and the failure / recovery counts are bit-identical. Mixed precision
with the multigrid preconditioner throughout.

Which kernel a solve really launched is read from the library's launch
counters (mof_test_residual_launches), not from the probe. Launches of fewer
than 1,024 workgroups take the staged kernel with one system pair per wave;
the flagship's take four pairs per wave in turn. The small meshes reach that
instance through mof_test_force_residual_trips (``trips=True``), one 65,612-
vertex mesh reaches it by its size."""
import contextlib

import numpy as np
import pytest

from mofhip import DecomposedMesh, DeviceMesh, synth
from mofhip.mesh import force_residual_rows, force_residual_trips, residual_launches, residual_probe

pytestmark = pytest.mark.gpu

COUNTS = ("iterations", "max_iterations", "outer_steps", "failed", "recovered", "recovered_f64", "systems",
          "batches")

_MESHES = {}


def small_mesh(name):
    if name not in _MESHES:
        if name == "ico642":  # 11 slices, the last with 2 live lanes; 3 row blocks, the last with 3 slices
            p, t = synth.icosphere(8)
        elif name == "cap641":  # open surface: boundary rows, padding incidences
            p, t = synth.spherical_cap(16)
        elif name == "hull900":
            p, t = synth.random_sphere(900, 10.0, seed=2)
        else:
            p, t = synth.random_sphere(1500, 10.0, seed=0)
        _MESHES[name] = (p, t, synth.vertex_normals(p, t), synth.triangle_areas(p, t))
    return _MESHES[name]


def solve(make, I, tk, forced, staged=True, trips=False, **kw):
    """One solve on a fresh handle, with the row kernel (``forced``) or as the
    library decides: ``staged`` says which kernel that must be, and the launch
    counters must agree -- rows only, or the staged kernel only, in its
    four-trip instance when ``trips`` forces it and its one-trip instance
    otherwise (None: either, the mesh's size decides)."""
    with force_residual_rows() if forced else contextlib.nullcontext():
        m = make()
    c0 = residual_launches()
    with force_residual_trips() if trips else contextlib.nullcontext():
        V, st = m.solve_range(I, tk, 0, len(I) - 1, 0.01, precision="mixed", precond="amg", **kw)
    m.close()
    d = {k: v - c0[k] for k, v in residual_launches().items()}
    assert st["failed"] == st["recovered"] == 0, st
    if forced or not staged:
        assert d["rows"] > 0 and d["staged_one"] == d["staged_multi"] == 0, d
    elif trips is None:
        assert d["rows"] == 0 and d["staged_one"] + d["staged_multi"] > 0, d
    elif trips:
        assert d["rows"] == d["staged_one"] == 0 and d["staged_multi"] > 0, d
    else:
        assert d["rows"] == d["staged_multi"] == 0 and d["staged_one"] > 0, d
    return V, st


def same(a, b):
    assert np.array_equal(a[0], b[0])
    assert a[1]["max_rel_residual"] == b[1]["max_rel_residual"]
    for k in COUNTS:
        assert a[1][k] == b[1][k], k


def test_icosphere_is_staged():
    p, t, n, a = small_mesh("ico642")
    assert residual_probe(t, len(p)) == {"staged_bytes": 92928, "staged_used": True}
    I = synth.travelling_wave(p, 6)
    tk = np.arange(6.0)
    mk = lambda: DeviceMesh(p, n, t, a)  # noqa: E731
    same(solve(mk, I, tk, False), solve(mk, I, tk, True))


@pytest.mark.parametrize("trips", [False, True])
def test_odd_batches(trips):
    """Batches of 1, 3 and 5: the second system slot of the last pair is
    empty and most waves of the workgroup have no pair. The handle's choice
    of kernel is the same at every batch (solve() checks the launches)."""
    p, t, n, a = small_mesh("ico642")
    I = synth.travelling_wave(p, 6)
    tk = np.arange(6.0)
    mk = lambda: DeviceMesh(p, n, t, a)  # noqa: E731
    ref = None
    for batch in (1, 3, 5):
        st, rows = solve(mk, I, tk, False, trips=trips, batch=batch), solve(mk, I, tk, True, batch=batch)
        same(st, rows)
        ref = ref or st
        assert np.array_equal(st[0], ref[0]) and st[1]["iterations"] == ref[1]["iterations"]


@pytest.mark.parametrize("trips", [False, True])
def test_batch_past_one_workgroup(trips):
    """169 systems = 85 pairs in one batch. One trip per wave: 16 pairs per
    workgroup, the sixth chunk with 5 pairs (11 idle waves, the last pair half
    empty). Four trips: 64 pairs per workgroup, the second chunk with 21 --
    waves 0-4 leave after their second trip, waves 5-15 after their first."""
    p, t, n, a = small_mesh("ico642")
    T = 170
    I = synth.travelling_wave(p, T)
    tk = np.arange(float(T))
    mk = lambda: DeviceMesh(p, n, t, a)  # noqa: E731
    st, rows = solve(mk, I, tk, False, trips=trips, batch=T - 1), solve(mk, I, tk, True, batch=T - 1)
    assert st[1]["batches"] == 1 and st[1]["systems"] == T - 1
    same(st, rows)


def test_systems_retiring_at_different_steps():
    """Wave rows of amplitudes 0.1 ... 10 in one batch: the systems take two
    or three refinement steps, so single systems of a pair, whole pairs and
    (in the last launches) whole workgroups are inactive."""
    p, t, n, a = small_mesh("ico642")
    T = 9
    I = synth.travelling_wave(p, T) * np.logspace(-1.0, 1.0, T)[:, None]
    tk = np.arange(float(T))
    mk = lambda: DeviceMesh(p, n, t, a)  # noqa: E731
    its = []
    m = mk()
    for k in range(T - 1):
        _, s1 = m.solve_range(I[k:k + 2], tk[k:k + 2], 0, 1, 0.01, precision="mixed", precond="amg")
        assert s1["failed"] == s1["recovered"] == 0
        its.append(s1["iterations"])
    m.close()
    assert max(its) >= min(its) + 3, its  # they really stop at different points
    st, rows = solve(mk, I, tk, False, batch=T - 1), solve(mk, I, tk, True, batch=T - 1)
    same(st, rows)
    assert st[1]["iterations"] == sum(its)


def test_pairs_retiring_between_trips():
    """The four-trip kernel on 80 systems of amplitudes 5 ... 0.1 (towards 10
    the multigrid solve of neighbouring rows of unequal amplitude needs its
    recovery, with either residual kernel): 40 pairs,
    so waves 0-7 take three trips and waves 8-15 two, and the systems leave
    after two or three refinement steps -- a wave's first pair still active
    while a later one has retired and the other way round (the `continue`
    over an inactive pair), then whole workgroups inactive."""
    p, t, n, a = small_mesh("ico642")
    T = 81
    I = synth.travelling_wave(p, T) * np.logspace(np.log10(5.0), -1.0, T)[:, None]
    tk = np.arange(float(T))
    mk = lambda: DeviceMesh(p, n, t, a)  # noqa: E731
    st, rows = solve(mk, I, tk, False, trips=True, batch=T - 1), solve(mk, I, tk, True, batch=T - 1)
    same(st, rows)
    assert st[1]["outer_steps"] >= 3  # not every system left after the second step


def test_large_mesh_takes_four_trips_by_itself():
    """icosphere(81): 65,612 vertices, 1,026 slices -- past the 1,024
    workgroups from which a launch takes the flagship's four-trip kernel, no
    hook involved. 9 systems of amplitudes 0.1 ... 10 (5 pairs, the last half
    empty; trips 2-4 of every wave past the batch)."""
    p, t = synth.icosphere(81)
    n, a = synth.vertex_normals(p, t), synth.triangle_areas(p, t)
    assert len(p) == 65612 and residual_probe(t, len(p))["staged_used"]
    T = 10
    I = synth.travelling_wave(p, T) * np.logspace(-1.0, 1.0, T)[:, None]
    tk = np.arange(float(T))
    mk = lambda: DeviceMesh(p, n, t, a)  # noqa: E731
    c0 = residual_launches()
    st, rows = solve(mk, I, tk, False, trips=None), solve(mk, I, tk, True)
    c1 = residual_launches()
    assert c1["staged_multi"] > c0["staged_multi"] and c1["staged_one"] == c0["staged_one"]
    same(st, rows)


def test_open_cap():
    p, t, n, a = small_mesh("cap641")
    assert residual_probe(t, len(p))["staged_used"]
    I = synth.travelling_wave(p, 6)
    tk = np.arange(6.0)
    mk = lambda: DeviceMesh(p, n, t, a)  # noqa: E731
    same(solve(mk, I, tk, False), solve(mk, I, tk, True))


def test_irregular_hull_falls_back():
    """random_sphere(1500): a vertex of valence 12 makes one slice 180,480 B,
    past the 160 KiB the staged kernel may use, so the handle keeps the row
    kernel and the two solves are the same code."""
    p, t, n, a = small_mesh("hull1500")
    assert residual_probe(t, len(p)) == {"staged_bytes": 180480, "staged_used": False}
    I = synth.travelling_wave(p, 6)
    tk = np.arange(6.0)
    mk = lambda: DeviceMesh(p, n, t, a)  # noqa: E731
    same(solve(mk, I, tk, False, staged=False), solve(mk, I, tk, True))


@pytest.mark.parametrize("trips", [False, True])
def test_irregular_hull_staged(trips):
    """random_sphere(900, seed=2): valence up to 10 (11 a2 slots: three load
    batches, the last with three live slots; 151,296 B), slices of different
    widths after the degree sort -- still staged."""
    p, t, n, a = small_mesh("hull900")
    assert residual_probe(t, len(p)) == {"staged_bytes": 151296, "staged_used": True}
    I = synth.travelling_wave(p, 6)
    tk = np.arange(6.0)
    mk = lambda: DeviceMesh(p, n, t, a)  # noqa: E731
    same(solve(mk, I, tk, False, trips=trips), solve(mk, I, tk, True))


@pytest.mark.parametrize("trips", [False, True])
def test_decomposed_two_parts(trips):
    """2 parts of the icosphere, in-process: each part decides for itself (the
    launch counters show that both took the staged kernel) and
    sums its owned rows only (ghost rows are computed, never summed); against
    the forced row kernel, and within 1e-6 of the single domain."""
    p, t, n, a = small_mesh("ico642")
    I = synth.travelling_wave(p, 5)
    tk = np.arange(5.0)
    mk = lambda: DecomposedMesh(p, n, t, a, 2)  # noqa: E731
    st, rows = solve(mk, I, tk, False, trips=trips), solve(mk, I, tk, True)
    same(st, rows)
    one = solve(lambda: DeviceMesh(p, n, t, a), I, tk, False)
    assert np.abs(st[0] - one[0]).max() <= 1e-6 * max(1.0, np.abs(one[0]).max())
