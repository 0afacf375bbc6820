"""The level-0 row products reading one packed index word per SELL position
(k_pcg_spmv, k_res0_ns, k_post0_ns; mof_rowkern.h kIxPack) against the same
kernels on the two 32-bit tables (forced by the test hook
mof_test_force_index32): the same blocks, operands and order of sums, so V,
the iteration counts and the failure / recovery counts are bit-identical.
Mixed precision with the multigrid preconditioner throughout."""
import numpy as np
import pytest

from mofhip import DecomposedMesh, DeviceMesh, synth
from mofhip.mesh import force_index32, index_probe

pytestmark = pytest.mark.gpu

COUNTS = ("iterations", "max_iterations", "outer_steps", "failed", "recovered", "recovered_f64", "systems",
          "batches")


def small_mesh(name):
    if name == "ico642":
        p, t = synth.icosphere(8)
    elif name == "cap641":
        p, t = synth.spherical_cap(16)
    else:
        p, t = synth.random_sphere(1500, 10.0, seed=0)
    return p, t, synth.vertex_normals(p, t), synth.triangle_areas(p, t)


def solve(make, I, tk, forced, **kw):
    """One solve on a fresh handle, with the packed words or the 32-bit tables."""
    if forced:
        with force_index32():
            m = make()
    else:
        m = make()
    V, st = m.solve_range(I, tk, 0, len(I) - 1, 0.01, precision="mixed", precond="amg", **kw)
    m.close()
    assert st["failed"] == st["recovered"] == 0, st
    return V, st


def same(a, b):
    assert np.array_equal(a[0], b[0])
    assert a[1]["max_rel_residual"] == b[1]["max_rel_residual"]
    for k in COUNTS:
        assert a[1][k] == b[1][k], k


@pytest.mark.parametrize("name", ["ico642", "cap641", "hull1500"])
def test_packed_words_match_the_32_bit_tables(monkeypatch, name):
    p, t, n, a = small_mesh(name)
    if name == "hull1500":  # plain reads by itself: rows of up to 13 slots, two load chunks
        monkeypatch.setenv("MOF_SYM_READS", "1")
    pr = index_probe(t, len(p), sym=1 if name == "hull1500" else -1)
    assert pr["sym_used"] and pr["packed_used"]  # so the two solves below differ in their index source
    I = synth.travelling_wave(p, 6)
    tk = np.arange(6.0)
    mk = lambda: DeviceMesh(p, n, t, a)  # noqa: E731
    same(solve(mk, I, tk, False), solve(mk, I, tk, True))


def test_odd_system_groups():
    """Batches of 1, 3 and 5: the second system slot of the last thread pair is empty."""
    p, t, n, a = small_mesh("ico642")
    I = synth.travelling_wave(p, 6)
    tk = np.arange(6.0)
    mk = lambda: DeviceMesh(p, n, t, a)  # noqa: E731
    ref = None
    for batch in (1, 3, 5):
        pk, f32 = solve(mk, I, tk, False, batch=batch), solve(mk, I, tk, True, batch=batch)
        same(pk, f32)
        ref = ref or pk
        assert np.array_equal(pk[0], ref[0]) and pk[1]["iterations"] == ref[1]["iterations"]


def test_systems_converging_at_different_iterations():
    """Wave rows of amplitudes 0.1 ... 10 (a1 ~ |grad I|^2 against lambda a2;
    past 10 the multigrid solve needs its recovery): the systems of one batch
    take two or three refinement steps and 14 to 19 iterations, so they stop
    at different iterations and the tail launches cover the running systems
    only (SysMap)."""
    p, t, n, a = small_mesh("ico642")
    T = 9
    I = synth.travelling_wave(p, T) * np.logspace(-1.0, 1.0, T)[:, None]
    tk = np.arange(float(T))
    mk = lambda: DeviceMesh(p, n, t, a)  # noqa: E731
    its = []
    m = mk()
    for k in range(T - 1):
        _, st = m.solve_range(I[k:k + 2], tk[k:k + 2], 0, 1, 0.01, precision="mixed", precond="amg")
        assert st["failed"] == st["recovered"] == 0
        its.append(st["iterations"])
    m.close()
    assert max(its) >= min(its) + 3, its  # they really stop at different iterations
    pk, f32 = solve(mk, I, tk, False, batch=T - 1), solve(mk, I, tk, True, batch=T - 1)
    same(pk, f32)
    assert pk[1]["iterations"] == sum(its)


def test_open_cap_with_boundary_sweeps(monkeypatch):
    """k_bsweep's ring blocks are gathered through the 32-bit mirror table
    (k_bsw_extract) and must be the blocks the packed row products read."""
    monkeypatch.setenv("MOF_AMG_BSW", "2")
    p, t, n, a = small_mesh("cap641")
    I = synth.travelling_wave(p, 6)
    tk = np.arange(6.0)
    mk = lambda: DeviceMesh(p, n, t, a)  # noqa: E731
    pk, f32 = solve(mk, I, tk, False), solve(mk, I, tk, True)
    same(pk, f32)
    monkeypatch.setenv("MOF_AMG_BSW", "0")
    off = solve(mk, I, tk, False)
    assert off[1]["iterations"] != pk[1]["iterations"]  # the sweeps really ran


def test_decomposed_two_parts():
    """2 parts of the 642-vertex icosphere, in-process: each part builds its
    own words (or keeps its tables); against the forced 32-bit tables, and
    within 1e-6 of the single domain."""
    p, t, n, a = small_mesh("ico642")
    I = synth.travelling_wave(p, 5)
    tk = np.arange(5.0)
    mk = lambda: DecomposedMesh(p, n, t, a, 2)  # noqa: E731
    pk, f32 = solve(mk, I, tk, False), solve(mk, I, tk, True)
    same(pk, f32)
    one = solve(lambda: DeviceMesh(p, n, t, a), I, tk, False)
    assert np.abs(pk[0] - one[0]).max() <= 1e-6 * max(1.0, np.abs(one[0]).max())
