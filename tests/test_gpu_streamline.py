"""Streamlines on the GPU (mof_streamline_map, mof_streamlines) against the
reference's S6_streamline.py: the golden vectors of
tests/golden/G9_streamlines.npz and the numpy checker tests/streamline_ref.py
(pinned to them exactly by test_streamline.py).

Bars. The results are integers: everything is compared exactly, no vertex
excluded. That is sound because the golden fields keep, at every vertex,
min(top - second, |top|) of the dot products above 1e-6 max|V| (asserted by
the fixture's maker and by test_streamline.py; measured 1.4e-4 to 7.3e-4),
eight orders above the rounding of the few operations behind a dot product,
so no decision depends on the order of a sum. Exactly tied maxima (G1's
solved field) are not compared with the reference, whose choice there follows
VTK's neighbour order, but between two vertex orders of the handle.
"""
import ctypes

import numpy as np
import pytest

from conftest import load_golden

import streamline_ref
from mofhip import DeviceMesh
from mofhip import _lib as L
from mofhip.streamline import (extract_static_streamline_dot_product, streamline_lists, streamline_map,
                               streamline_map_device, track_static_vectorfields_over_time)

pytestmark = pytest.mark.gpu

MESHES = ["G1_ico642", "G2_cap641", "G3_ico642_f32"]


@pytest.fixture(scope="module")
def g9():
    return load_golden("G9_streamlines")


@pytest.fixture(scope="module")
def meshes():
    made = {}

    def get(name, reorder=True):
        if (name, reorder) not in made:
            g = load_golden(name)
            made[name, reorder] = (g, DeviceMesh(g["coordinates"], g["normals"], g["triangles"], g["areas"],
                                                 reorder=reorder))
        return made[name, reorder]

    yield get
    for _, m in made.values():
        m.close()


@pytest.fixture(scope="module")
def g2ref(g9):
    """streamline_ref on G2's fields with its details, computed once and never modified."""
    g = load_golden("G2_cap641")
    V = g9["G2_cap641_V"]
    det = {}
    nxt = streamline_ref.successor_map(g["coordinates"], g["triangles"], g["e"], V, details=det)
    nxt.setflags(write=False)
    return nxt, det


def call_lists(m, V, min_len, cap_l, cap_v, n_lines=True):
    """mof_streamlines itself: (rc, totals, n_lines, off, vtx)."""
    V = np.ascontiguousarray(V, dtype=np.float64)
    K = len(V)
    totals = np.full(2, -7, dtype=np.int64)
    nl = np.full(K, -7, dtype=np.int64)
    off = np.full(cap_l + 1, -7, dtype=np.int64)
    vtx = np.full(max(cap_v, 1), -7, dtype=np.int32)
    with m.lock():
        rc = L.lib().mof_streamlines(m.handle(), L.ptr(V), K, min_len, 0, None, cap_l, cap_v, L.ptr(totals),
                                     L.ptr(nl) if n_lines else None, L.ptr(off), L.ptr(vtx))
    return rc, totals, nl, off, vtx


@pytest.mark.parametrize("name", MESHES)
def test_parity_with_reference(g9, meshes, name):
    g, m = meshes(name)
    V = g9[name + "_V"]
    nxt, length = streamline_map(m, V)
    assert nxt.dtype == np.int32 and length.dtype == np.int32
    assert np.array_equal(nxt, g9[name + "_next"])
    assert np.array_equal(length, g9[name + "_length"])
    print(name, "terminal", (nxt < 0).sum(axis=1), "max length", length.max(axis=1))
    if name + "_lines20_off" not in g9:
        return
    # the reference's lists at the default length, and its functions' coordinates
    off, vtx = g9[name + "_lines20_off"], g9[name + "_lines20_vtx"]
    (o, v), = streamline_lists(m, V[0])
    assert np.array_equal(o, off) and np.array_equal(v, vtx)
    res = track_static_vectorfields_over_time(m, V, 0, 1)
    assert list(res) == ["0"] and len(res["0"]) == len(off) - 1
    pts = g["coordinates"]
    for q, line in enumerate(res["0"]):
        assert line.dtype == pts.dtype and np.array_equal(line, pts[vtx[off[q]:off[q + 1]]])
    first = extract_static_streamline_dot_product(pts[vtx[off[1]]], V[0], m)
    assert np.array_equal(np.array(first), pts[vtx[off[1]:off[2]]])
    short = int(np.argmin(g9[name + "_length"][0]))
    if g9[name + "_length"][0, short] < 20:
        assert extract_static_streamline_dot_product(pts[short], V[0], m) == []


def test_every_walk_ends_on_a_repeat(g9, meshes):
    """G1 field 0 has no terminal vertex: each walk stops at a vertex already
    on its path, so its length is tail + cycle."""
    _, m = meshes("G1_ico642")
    V = g9["G1_ico642_V"][:1]
    nxt, length = streamline_map(m, V)
    assert (nxt >= 0).all()
    assert np.array_equal(length, streamline_ref.lengths(nxt, V))
    assert length.min() >= 2 and length.max() == 164


def test_terminal_vertices(g9, meshes, g2ref):
    """G2: walks end at failed boundary-edge tests and at d <= 0."""
    _, m = meshes("G2_cap641")
    ref, det = g2ref
    nxt, _ = streamline_map(m, g9["G2_cap641_V"])
    assert np.array_equal(nxt, ref)
    by_test = det["tested"] & (det["top"] > 0)
    by_sign = ~(det["top"] > 0)
    assert by_test.any() and by_sign.any()
    assert (nxt[by_test] == -1).all() and (nxt[by_sign] == -1).all()
    assert ((nxt < 0) == (by_test | by_sign)).all()


def test_zero_vectors(g9, meshes, g2ref):
    """V exactly 0 at a few vertices: the seeds are skipped (length 0) and the
    vertices are terminal when a walk reaches them."""
    g, m = meshes("G2_cap641")
    V = g9["G2_cap641_V"][:1].copy()
    base = g2ref[0][0]
    zeroed = [int(base[5]), int(base[base[300]]), 17, 640]  # two of them successors of other vertices
    V[0, zeroed] = 0.0
    expect = base.copy()
    expect[zeroed] = streamline_ref.successor_map(g["coordinates"], g["triangles"], g["e"], V, vertices=zeroed)[0]
    assert (expect[zeroed] == -1).all()
    nxt, length = streamline_map(m, V)
    assert np.array_equal(nxt[0], expect)
    assert np.array_equal(length, streamline_ref.lengths(expect[None], V))
    assert (length[0, zeroed] == 0).all() and (np.delete(length[0], zeroed) >= 1).all()
    assert length[0, 5] == 2  # 5 -> its zeroed successor, which ends the walk
    (off, vtx), = streamline_lists(m, V, 1)
    assert len(off) - 1 == 641 - len(zeroed) and not np.isin(vtx[off[:-1]], zeroed).any()


def test_nan_field(meshes):
    """A NaN-filled field (a failed solve): every vertex terminal, every line its seed alone."""
    _, m = meshes("G1_ico642")
    V = np.full((2, 642, 3), np.nan)
    V[1, :, 1:] = 1.0  # one NaN component is enough
    nxt, length = streamline_map(m, V)
    assert (nxt == -1).all() and (length == 1).all()


def test_min_length_extremes(g9, meshes):
    _, m = meshes("G2_cap641")
    V = g9["G2_cap641_V"]
    length = g9["G2_cap641_length"].astype(np.int64)
    res = streamline_lists(m, V, 1)
    for k, (off, vtx) in enumerate(res):
        assert np.array_equal(np.diff(off), length[k]) and len(vtx) == length[k].sum()
        assert np.array_equal(vtx[off[:-1]], np.arange(641))
    for off, vtx in streamline_lists(m, V, int(length.max()) + 1):
        assert list(off) == [0] and len(vtx) == 0
    longest = streamline_lists(m, V, int(length.max()))
    assert sum(len(off) - 1 for off, _ in longest) == int((length == length.max()).sum())


def test_vertex_order_with_tied_maxima(meshes):
    """G1's solved field has exactly tied maxima at some vertices (the
    unjittered icosphere). The smallest caller's id wins whatever the
    handle's internal vertex order is."""
    g, m = meshes("G1_ico642")
    _, m0 = meshes("G1_ico642", reorder=False)
    N = 642
    V = g["V_k"][:2, :N, None] * g["e"][None, :, 0] + g["V_k"][:2, N:, None] * g["e"][None, :, 1]
    a, b = streamline_map(m, V), streamline_map(m0, V)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    la, lb = streamline_lists(m, V, 5), streamline_lists(m0, V, 5)
    for (oa, va), (ob, vb) in zip(la, lb):
        assert np.array_equal(oa, ob) and np.array_equal(va, vb)


@pytest.fixture
def pass_fields():
    def set_(n):
        assert L.lib().mof_test_streamline_pass(n) == L.MOF_OK
    yield set_
    L.lib().mof_test_streamline_pass(0)


def test_fields_and_passes(g9, meshes, pass_fields):
    """K = 5 in one call, in passes of 2 and 3 fields, and as five calls of K = 1."""
    _, m = meshes("G2_cap641")
    V = np.concatenate([g9["G2_cap641_V"], -g9["G2_cap641_V"][:2]])
    full = streamline_map(m, V)
    lists = streamline_lists(m, V, 10)
    assert np.array_equal(full[0][:3], g9["G2_cap641_next"])
    for k in range(5):
        one = streamline_map(m, V[k])
        assert np.array_equal(one[0][0], full[0][k]) and np.array_equal(one[1][0], full[1][k])
    for n in (2, 3):
        pass_fields(n)
        part = streamline_map(m, V)
        assert np.array_equal(part[0], full[0]) and np.array_equal(part[1], full[1])
        for (oa, va), (ob, vb) in zip(streamline_lists(m, V, 10), lists):
            assert np.array_equal(oa, ob) and np.array_equal(va, vb)
    pass_fields(0)
    for k, (off, vtx) in enumerate(lists):
        o, v = streamline_ref.line_lists(full[0][k], full[1][k], 10)
        assert np.array_equal(off, o) and np.array_equal(vtx, v)


def test_output_selection(g9, meshes):
    _, m = meshes("G3_ico642_f32")
    V = np.ascontiguousarray(g9["G3_ico642_f32_V"])
    full = streamline_map(m, V)
    fn, h = L.lib().mof_streamline_map, m.handle()
    for k in (0, 1):
        out = np.full((2, 642), -7, dtype=np.int32)
        args = [None, None]
        args[k] = L.ptr(out)
        assert fn(h, L.ptr(V), 2, 0, None, *args) == L.MOF_OK
        assert np.array_equal(out, full[k])


def test_device_pointers(g9, meshes, pass_fields):
    import torch
    _, m = meshes("G2_cap641")
    V = g9["G2_cap641_V"]
    host = streamline_map(m, V)
    dev = torch.device("cuda", 0)
    Vd = torch.from_numpy(V.copy()).to(dev)
    for n in (0, 2):
        pass_fields(n)
        outs = [torch.full((3, 641), -7, dtype=torch.int32, device=dev) for _ in range(2)]
        torch.cuda.synchronize()
        streamline_map_device(m, Vd.data_ptr(), 3, next_ptr=outs[0].data_ptr(), length_ptr=outs[1].data_ptr())
        assert np.array_equal(outs[0].cpu().numpy(), host[0]) and np.array_equal(outs[1].cpu().numpy(), host[1])
        only = torch.full((3, 641), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        streamline_map_device(m, Vd.data_ptr(), 3, length_ptr=only.data_ptr())
        assert np.array_equal(only.cpu().numpy(), host[1])
    # the lists from fields resident on the device
    totals = np.zeros(2, dtype=np.int64)
    nl = np.zeros(3, dtype=np.int64)
    ref = streamline_lists(m, V, 20)
    cap_l, cap_v = sum(len(o) - 1 for o, _ in ref), sum(len(v) for _, v in ref)
    off, vtx = np.zeros(cap_l + 1, dtype=np.int64), np.zeros(cap_v, dtype=np.int32)
    with m.lock():
        rc = L.lib().mof_streamlines(m.handle(), ctypes.c_void_p(Vd.data_ptr()), 3, 20, L.MOF_IO_DEVICE, None,
                                     cap_l, cap_v, L.ptr(totals), L.ptr(nl), L.ptr(off), L.ptr(vtx))
    assert rc == L.MOF_OK and list(totals) == [cap_l, cap_v]
    assert list(nl) == [len(o) - 1 for o, _ in ref]
    assert np.array_equal(vtx, np.concatenate([v for _, v in ref]))
    assert np.array_equal(np.diff(off), np.concatenate([np.diff(o) for o, _ in ref]))


def test_caps(g9, meshes):
    """A cap one short: MOF_E_ARG with the right totals; the retry sized by them succeeds."""
    _, m = meshes("G2_cap641")
    V = g9["G2_cap641_V"]
    length = g9["G2_cap641_length"].astype(np.int64)
    keep = length >= 20
    nl, nv = int(keep.sum()), int(length[keep].sum())
    for cap_l, cap_v in ((nl - 1, nv), (nl, nv - 1), (0, 0)):
        rc, totals, _, _, _ = call_lists(m, V, 20, cap_l, cap_v)
        assert rc == L.MOF_E_ARG and list(totals) == [nl, nv]
        assert b"cap" in L.lib().mof_last_error()
    rc, totals, n_lines, off, vtx = call_lists(m, V, 20, nl, nv)
    assert rc == L.MOF_OK and list(totals) == [nl, nv]
    assert np.array_equal(n_lines, keep.sum(axis=1))
    assert off[0] == 0 and off[-1] == nv and np.array_equal(np.diff(off), length[keep])
    assert np.array_equal(vtx[off[:-1]], np.nonzero(keep)[1])
    rc, _, n2, off2, vtx2 = call_lists(m, V, 20, nl + 3, nv + 5, n_lines=False)  # room to spare, no n_lines
    assert rc == L.MOF_OK and np.array_equal(off2[:nl + 1], off) and np.array_equal(vtx2[:nv], vtx)
    assert (n2 == -7).all() and (off2[nl + 1:] == -7).all() and (vtx2[nv:] == -7).all()


def test_argument_errors(g9, meshes):
    _, m = meshes("G1_ico642")
    V = np.ascontiguousarray(g9["G1_ico642_V"])
    out = np.empty((2, 642), dtype=np.int32)
    fn, h, err = L.lib().mof_streamline_map, m.handle(), L.lib().mof_last_error
    assert fn(None, L.ptr(V), 2, 0, None, L.ptr(out), None) == L.MOF_E_ARG and b"mesh" in err()
    assert fn(h, None, 2, 0, None, L.ptr(out), None) == L.MOF_E_ARG and b"V_coord" in err()
    assert fn(h, L.ptr(V), 0, 0, None, L.ptr(out), None) == L.MOF_E_ARG and b"K" in err()
    assert fn(h, L.ptr(V), 2, 0, None, None, None) == L.MOF_E_ARG and b"output" in err()
    assert fn(h, L.ptr(V), 2, 0, None, L.ptr(out), None) == L.MOF_OK
    fn = L.lib().mof_streamlines
    totals = np.zeros(2, dtype=np.int64)
    off, vtx = np.zeros(2 * 642 + 1, dtype=np.int64), np.zeros(2 * 642 * 200, dtype=np.int32)
    tail = (L.ptr(totals), None, L.ptr(off), L.ptr(vtx))
    assert fn(None, L.ptr(V), 2, 20, 0, None, 1284, len(vtx), *tail) == L.MOF_E_ARG and b"mesh" in err()
    assert fn(h, None, 2, 20, 0, None, 1284, len(vtx), *tail) == L.MOF_E_ARG and b"V_coord" in err()
    assert fn(h, L.ptr(V), 0, 20, 0, None, 1284, len(vtx), *tail) == L.MOF_E_ARG and b"K" in err()
    assert fn(h, L.ptr(V), 2, 20, 0, None, -1, len(vtx), *tail) == L.MOF_E_ARG and b"capacity" in err()
    assert fn(h, L.ptr(V), 2, 20, 0, None, 1284, -1, *tail) == L.MOF_E_ARG and b"capacity" in err()
    assert fn(h, L.ptr(V), 2, 20, 0, None, 1284, len(vtx), None, None, L.ptr(off), L.ptr(vtx)) == L.MOF_E_ARG
    assert b"output" in err()
    assert fn(h, L.ptr(V), 2, 20, 0, None, 1284, len(vtx), L.ptr(totals), None, None, L.ptr(vtx)) == L.MOF_E_ARG
    assert fn(h, L.ptr(V), 2, 20, 0, None, 1284, len(vtx), *tail) == L.MOF_OK
    assert totals[0] == 642 + int((g9["G1_ico642_length"][1] >= 20).sum())


def test_solver_unaffected(g9, meshes):
    g, m = meshes("G1_ico642")
    I, tk, lam = g["I"][:4], g["t_k"][:4], float(g["lambda_"])
    V0, _ = m.solve_range(I, tk, 0, 3, lam, precision="mixed", precond="amg")
    streamline_map(m, g9["G1_ico642_V"])
    streamline_lists(m, g9["G1_ico642_V"])
    V1, _ = m.solve_range(I, tk, 0, 3, lam, precision="mixed", precond="amg")
    assert np.array_equal(V0, V1)


@pytest.mark.slow
def test_160k_sample():
    """C3 (163,842 vertices: many slices, a ragged last one, long walks), more
    fields than one pass holds: next at every 97th vertex against
    streamline_ref run on that vertex's ring, length for those seeds against a
    host walk of the GPU's own next."""
    from mofhip import synth
    p, t, n, a = synth.mesh_for_config("C3")
    m = DeviceMesh(p, n, t, a)
    e, _, _ = m.geometry()
    N = len(p)
    K = (2 << 20) // N // 4 * 4 + 1  # one field more than a pass of the library's choice
    nrm = n / np.linalg.norm(n, axis=1, keepdims=True)
    V = np.empty((K, N, 3))
    for k in range(K):
        w = np.cross(np.array([0.31, -0.23, 0.17]) * (1 + 0.3 * k), p) + np.array([0.7, 0.2, -1.1]) + 0.25 * k \
            + 0.05 * np.sin(p @ np.array([0.9, -0.4, 0.6]) + k)[:, None] * np.array([0.2, 1.0, -0.5])
        V[k] = w - (w * nrm).sum(axis=1, keepdims=True) * nrm
    nxt, length = streamline_map(m, V)
    m.close()
    sample = list(range(0, N, 97))
    det = {}
    ks = [0, K - 2, K - 1]
    ref = streamline_ref.successor_map(p, t, e, V[ks], vertices=sample, details=det)
    # the input's own condition (no decision within rounding of a tie), then every sampled vertex
    print("min margin / max|V| %.3g" % (det["margin"].min() / np.abs(V[ks]).max()), "max length", int(length.max()))
    assert det["margin"].min() >= 1e-9 * np.abs(V[ks]).max()
    assert np.array_equal(nxt[ks][:, sample], ref)
    assert ((nxt >= -1) & (nxt < N)).all()
    assert np.array_equal(length[ks][:, sample], streamline_ref.lengths(nxt[ks], V[ks], seeds=sample))
