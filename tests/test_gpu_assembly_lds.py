"""The mixed-precision row assembly with a row slice's geometry staged in LDS
and the systems on waves (k_assemble_lds) against the row kernel
k_assemble_rows_rc (forced by the test hook mof_test_force_assembly_rows): the
same per-incidence and per-slot functions in the same order, so the fp32
operator A32, its bf16 copy A0h, the right-hand side -- read back from the
workspace and compared byte for byte at the positions the kernels write -- and
with them V, the residuals, the iteration counts and the failure / recovery
counts are identical.

Which kernel a solve really launched is read from the library's launch
counters (mof_test_assembly_launches), not from the probe. Launches of fewer
than 1,024 workgroups take the staged kernel with one system per wave; the
flagship's take eight systems per wave in turn (8 waves per workgroup). The
small meshes reach that instance through mof_test_force_assembly_trips
(``trips=True``), one 65,612-vertex mesh reaches it by its size."""
import contextlib

import numpy as np
import pytest

from mofhip import DecomposedMesh, DeviceMesh, synth
from mofhip.mesh import (assembly_launches, assembly_probe, assembly_readback, force_assembly_rows,
                         force_assembly_trips, index_probe)

pytestmark = pytest.mark.gpu

COUNTS = ("iterations", "max_iterations", "outer_steps", "failed", "recovered", "recovered_f64", "systems",
          "batches")

_MESHES = {}


def small_mesh(name):
    if name not in _MESHES:
        if name == "ico642":  # 11 slices, the last with 2 live lanes
            p, t = synth.icosphere(8)
        elif name == "cap641":  # open surface: boundary rows, padding incidences
            p, t = synth.spherical_cap(16)
        elif name == "hull30":  # one slice with 30 live lanes; valence 7 = the 8 register slots
            p, t = synth.random_sphere(30, 10.0, seed=1)
        elif name == "hull900":  # valence 10: too wide
            p, t = synth.random_sphere(900, 10.0, seed=2)
        else:  # S1-like patch of 625 vertices: butterfly subdivision leaves valence-8 vertices
            p, t = synth.electrode_surface(7, subdivisions=2)
        p, t = np.asarray(p), np.asarray(t)
        ip = index_probe(t, len(p))
        written = ip["mir"] >= 0  # not padding ...
        if ip["sym_used"]:  # ... and not a lower block the symmetric layout reads transposed
            written &= (ip["mir"] & (1 << 30)) == 0
        _MESHES[name] = (p, t, synth.vertex_normals(p, t), synth.triangle_areas(p, t), written)
    return _MESHES[name]


def solve(make, I, tk, forced, staged=True, trips=False, systems=(0,), written=None, **kw):
    """One solve on a fresh handle, with the row kernel (``forced``) or as the
    library decides: ``staged`` says which kernel that must be, and the launch
    counters must agree -- rows only, or the staged kernel only, in its
    multi-trip instance when ``trips`` forces it and its one-trip instance
    otherwise (None: either, the mesh's size decides). Returns V, the stats and
    (single handles) the written bytes of the last batch's ``systems``."""
    kw.setdefault("precond", "amg")
    kw.setdefault("batch", len(I) - 1)  # one batch unless the test splits it: ``systems`` index the last one
    with force_assembly_rows() if forced else contextlib.nullcontext():
        m = make()
    c0 = assembly_launches()
    with force_assembly_trips() if trips else contextlib.nullcontext():
        V, st = m.solve_range(I, tk, 0, len(I) - 1, 0.01, precision="mixed", **kw)
    d = {k: v - c0[k] for k, v in assembly_launches().items()}
    back = []
    if written is not None:
        for b in systems:
            r = assembly_readback(m, b)
            back.append((r["A32"][written].tobytes(), None if r["A0h"] is None else r["A0h"][written].tobytes(),
                         r["rhs"].tobytes()))
    m.close()
    assert st["failed"] == st["recovered"] == 0, st
    if forced or not staged:
        assert d["rows"] > 0 and d["staged_one"] == d["staged_multi"] == 0, d
    elif trips is None:
        assert d["rows"] == 0 and d["staged_one"] + d["staged_multi"] > 0, d
    elif trips:
        assert d["rows"] == d["staged_one"] == 0 and d["staged_multi"] > 0, d
    else:
        assert d["rows"] == d["staged_multi"] == 0 and d["staged_one"] > 0, d
    return V, st, back


def same(a, b, a0h=True):
    assert np.array_equal(a[0], b[0])
    assert a[1]["max_rel_residual"] == b[1]["max_rel_residual"]
    for k in COUNTS:
        assert a[1][k] == b[1][k], k
    assert len(a[2]) == len(b[2])
    for (A, H, f), (Ar, Hr, fr) in zip(a[2], b[2]):
        assert A == Ar, "A32 differs"
        assert (H is not None) == (Hr is not None) and H == Hr, "A0h differs"
        assert f == fr, "rhs differs"
        if a0h is not None:
            assert (H is not None) == a0h


@pytest.mark.parametrize("trips", [False, True])
def test_icosphere_is_staged(trips):
    p, t, n, a, w = small_mesh("ico642")
    assert assembly_probe(t, len(p)) == {"staged_bytes": 67584, "staged_used": True}
    I = synth.travelling_wave(p, 6)
    mk = lambda: DeviceMesh(p, n, t, a)  # noqa: E731
    for tk in (np.arange(6.0), np.arange(6.0) / 512):  # dt = 1 and the recordings' 1 / 512 s
        same(solve(mk, I, tk, False, trips=trips, systems=(0, 4), written=w),
             solve(mk, I, tk, True, systems=(0, 4), written=w))


@pytest.mark.parametrize("trips", [False, True])
def test_odd_batches(trips):
    """Batches of 1, 3 and 5: most waves of the workgroup have no system. The
    handle's choice of kernel is the same at every batch (solve() checks the
    launches)."""
    p, t, n, a, w = small_mesh("ico642")
    I = synth.travelling_wave(p, 6)
    tk = np.arange(6.0)
    mk = lambda: DeviceMesh(p, n, t, a)  # noqa: E731
    ref = None
    for batch in (1, 3, 5):
        st = solve(mk, I, tk, False, trips=trips, written=w, batch=batch)
        same(st, solve(mk, I, tk, True, written=w, batch=batch))
        ref = ref or st
        assert np.array_equal(st[0], ref[0]) and st[1]["iterations"] == ref[1]["iterations"]


@pytest.mark.parametrize("trips", [False, True])
def test_batch_past_one_workgroup(trips):
    """169 systems in one batch. One trip per wave: 8 systems per workgroup,
    the 22nd chunk with 1 (7 idle waves). Eight trips: 64 systems per
    workgroup, the third chunk with 41 -- wave 0 leaves after its sixth trip,
    waves 1-7 after their fifth."""
    p, t, n, a, w = small_mesh("ico642")
    T = 170
    I = synth.travelling_wave(p, T)
    tk = np.arange(float(T))
    mk = lambda: DeviceMesh(p, n, t, a)  # noqa: E731
    sy = (0, 7, 8, 63, 64, 160, 167, 168)
    st = solve(mk, I, tk, False, trips=trips, systems=sy, written=w, batch=T - 1)
    rows = solve(mk, I, tk, True, systems=sy, written=w, batch=T - 1)
    assert st[1]["batches"] == 1 and st[1]["systems"] == T - 1
    same(st, rows)


def test_block_jacobi_branch():
    """precond="jacobi": the assembly writes the 2x2 inverses (dinv32) itself
    and no bf16 copy."""
    p, t, n, a, w = small_mesh("ico642")
    I = synth.travelling_wave(p, 6)
    tk = np.arange(6.0)
    mk = lambda: DeviceMesh(p, n, t, a)  # noqa: E731
    same(solve(mk, I, tk, False, systems=(0, 4), written=w, precond="jacobi"),
         solve(mk, I, tk, True, systems=(0, 4), written=w, precond="jacobi"), a0h=False)


def test_second_image_array():
    """I2 given: I1 is a block of its own, not I0 + one row (the two-block
    J0 / J1 layout of the gathered rows)."""
    p, t, n, a, w = small_mesh("ico642")
    I = synth.travelling_wave(p, 6)
    I2 = synth.travelling_wave(p, 6, kappa=2.0, omega=0.45)
    tk = np.arange(6.0)
    mk = lambda: DeviceMesh(p, n, t, a)  # noqa: E731
    st = solve(mk, I, tk, False, systems=(0, 4), written=w, I2=I2)
    same(st, solve(mk, I, tk, True, systems=(0, 4), written=w, I2=I2))
    assert not np.array_equal(st[0], solve(mk, I, tk, False)[0])  # I2 really took part


def test_open_cap():
    p, t, n, a, w = small_mesh("cap641")
    assert assembly_probe(t, len(p))["staged_used"]
    I = synth.travelling_wave(p, 6)
    tk = np.arange(6.0)
    mk = lambda: DeviceMesh(p, n, t, a)  # noqa: E731
    same(solve(mk, I, tk, False, systems=(0, 4), written=w), solve(mk, I, tk, True, systems=(0, 4), written=w))


@pytest.mark.parametrize("trips", [False, True])
def test_row_as_wide_as_the_register_slots(trips):
    """random_sphere(30, seed=1): valence up to 7, so a row fills all 8 slots;
    one slice with 30 live lanes. Too small for a multigrid hierarchy worth
    the name: block Jacobi."""
    p, t, n, a, w = small_mesh("hull30")
    val = np.bincount(np.unique(np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1),
                                axis=0).ravel(), minlength=len(p))
    assert len(p) == 30 and val.max() == 7
    assert assembly_probe(t, len(p))["staged_used"]
    I = synth.travelling_wave(p, 6)
    tk = np.arange(6.0)
    mk = lambda: DeviceMesh(p, n, t, a)  # noqa: E731
    same(solve(mk, I, tk, False, trips=trips, systems=(0, 4), written=w, precond="jacobi"),
         solve(mk, I, tk, True, systems=(0, 4), written=w, precond="jacobi"), a0h=False)


@pytest.mark.parametrize("trips", [False, True])
def test_decomposed_two_parts(trips):
    """2 parts of the icosphere, in-process: each part decides for itself (the
    launch counters show that both took the staged kernel), its ghost rows and
    columns get identity bf16 blocks (nown); against the forced row kernel, and
    within 1e-6 of the single domain."""
    p, t, n, a, _ = small_mesh("ico642")
    I = synth.travelling_wave(p, 5)
    tk = np.arange(5.0)
    mk = lambda: DecomposedMesh(p, n, t, a, 2)  # noqa: E731
    st = solve(mk, I, tk, False, trips=trips)
    same(st, solve(mk, I, tk, True))
    one = solve(lambda: DeviceMesh(p, n, t, a), I, tk, False)
    assert np.abs(st[0] - one[0]).max() <= 1e-6 * max(1.0, np.abs(one[0]).max())


@pytest.mark.parametrize("name", ["hull900", "patch"])
def test_wide_rows_fall_back(name):
    """Valence 10 (random_sphere(900, seed=2)) and valence 8 (the S1-like
    patch): rows wider than the 8 register slots keep k_assemble_rows_rc<16>,
    and the two solves are the same code."""
    p, t, n, a, w = small_mesh(name)
    assert not assembly_probe(t, len(p))["staged_used"]
    I = synth.config_wave("S1s", p, 6) if name == "patch" else synth.travelling_wave(p, 6)
    tk = np.arange(6.0)
    mk = lambda: DeviceMesh(p, n, t, a)  # noqa: E731
    same(solve(mk, I, tk, False, staged=False, systems=(0, 4), written=w),
         solve(mk, I, tk, True, systems=(0, 4), written=w))


def test_large_mesh_takes_the_multi_trip_kernel_by_itself():
    """icosphere(81): 65,612 vertices, 1,026 slices -- past the 1,024
    workgroups from which a launch takes the flagship's multi-trip kernel, no
    hook involved. 9 systems: wave 0 takes two trips, waves 1-7 one."""
    p, t = synth.icosphere(81)
    n, a = synth.vertex_normals(p, t), synth.triangle_areas(p, t)
    assert len(p) == 65612 and assembly_probe(t, len(p))["staged_used"]
    ip = index_probe(t, len(p))
    w = (ip["mir"] >= 0) & (~np.bool_(ip["sym_used"]) | ((ip["mir"] & (1 << 30)) == 0))
    T = 10
    I = synth.travelling_wave(p, T)
    tk = np.arange(float(T))
    mk = lambda: DeviceMesh(p, n, t, a)  # noqa: E731
    c0 = assembly_launches()
    st = solve(mk, I, tk, False, trips=None, systems=(0, 8), written=w)
    c1 = assembly_launches()
    assert c1["staged_multi"] > c0["staged_multi"] and c1["staged_one"] == c0["staged_one"]
    same(st, solve(mk, I, tk, True, systems=(0, 8), written=w))
