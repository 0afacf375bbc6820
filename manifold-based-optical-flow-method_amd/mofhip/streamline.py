"""Streamlines on the mesh: the reference's ``S6_streamline.py`` on the GPU.

The reference starts a greedy vertex walk from every vertex of every frame and
rescans the whole path at each step, in Python (S6:17-49). Its choice of the
next vertex depends on (frame, vertex) alone, so the result is a successor map
``next[k, i]`` per field plus a walk along it from each seed to the first
vertex that is terminal or already on the path. ``mof_streamline_map`` returns
the two arrays that hold all of it (``next``, ``length``: 8 B per vertex and
field); ``mof_streamlines`` returns the reference's lists, compacted on the
device, on a :class:`~mofhip.mesh.DeviceMesh` handle.

Vertices are compared by id where the reference compares coordinates
(S6:44): the same thing on a mesh without duplicate points. Equal maxima of
the dot products go to the smallest vertex id (the reference takes VTK's
neighbour order there). The functions named like the reference's take a
``DeviceMesh`` where it takes its pyvista ``surface``.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib as L
from .mesh import DeviceMesh


def _fields(mesh, V_k_coord):
    V = np.asarray(V_k_coord)
    if V.dtype.kind not in "fiu":
        raise ValueError("V_k_coord must be a real array, not %s" % V.dtype)
    if V.ndim == 2:
        V = V[None]
    if V.ndim != 3 or V.shape[1:] != (mesh.N, 3) or V.shape[0] < 1:
        raise ValueError("V_k_coord must be (K, N, 3) with K >= 1 and N = %d, not %s" % (mesh.N, V.shape))
    return np.ascontiguousarray(V, dtype=np.float64)


def streamline_map(mesh: DeviceMesh, V_k_coord, device=None):
    """``(next, length)``, both (K, N) int32 in the caller's vertex order, for
    the fields V_k_coord (K, N, 3) (one field: (N, 3), K = 1). ``next[k, i]``:
    the vertex the walk steps to from i, -1 where it stops; ``length[k, s]``:
    the vertices of the line from seed s, 0 where the seed is skipped because
    its vector is zero (S6:29)."""
    V = _fields(mesh, V_k_coord)
    K = len(V)
    nxt = np.empty((K, mesh.N), dtype=np.int32)
    length = np.empty((K, mesh.N), dtype=np.int32)
    h = mesh.handle(device)
    with mesh.lock(device):
        L.check(L.lib().mof_streamline_map(h, L.ptr(V), K, 0, None, L.ptr(nxt), L.ptr(length)))
    return nxt, length


def streamline_map_device(mesh: DeviceMesh, V_ptr: int, K: int, device=None, stream=None, next_ptr=None,
                          length_ptr=None):
    """Device-pointer form: V (K, N, 3) f64 and the int32 outputs (either may
    be None) are already in HBM on the handle's device (``stream``: a
    hipStream_t or None); returns when done."""
    if not V_ptr or int(K) < 1 or not (next_ptr or length_ptr):
        raise ValueError("streamline_map_device needs V, K >= 1 and at least one output")
    h = mesh.handle(device)
    with mesh.lock(device):
        L.check(L.lib().mof_streamline_map(h, ctypes.c_void_p(V_ptr), int(K), L.MOF_IO_DEVICE, stream,
                                           ctypes.c_void_p(next_ptr) if next_ptr else None,
                                           ctypes.c_void_p(length_ptr) if length_ptr else None))


def streamline_lists(mesh: DeviceMesh, V_k_coord, min_streamline_length=20, device=None):
    """Per field ``(offsets, vertex_ids)`` of the lines with at least
    ``min_streamline_length`` vertices, seeds ascending: line q of a field is
    ``vertex_ids[offsets[q]:offsets[q + 1]]``. The lists are compacted on the
    device; a first call sized by a guess is repeated once, sized, when they
    do not fit."""
    V = _fields(mesh, V_k_coord)
    min_len = int(min_streamline_length)
    if min_len != min_streamline_length or not -2 ** 31 <= min_len < 2 ** 31:
        raise ValueError("min_streamline_length must be an int32 value")
    K = len(V)
    totals = np.zeros(2, dtype=np.int64)
    n_lines = np.zeros(K, dtype=np.int64)
    h = mesh.handle(device)
    cap_l, cap_v = K * mesh.N, 32 * K * mesh.N
    with mesh.lock(device):
        for attempt in (0, 1):
            off = np.empty(cap_l + 1, dtype=np.int64)
            vtx = np.empty(max(cap_v, 1), dtype=np.int32)
            rc = L.lib().mof_streamlines(h, L.ptr(V), K, min_len, 0, None, cap_l, cap_v, L.ptr(totals),
                                         L.ptr(n_lines), L.ptr(off), L.ptr(vtx))
            if rc == L.MOF_E_ARG and attempt == 0 and (totals[0] > cap_l or totals[1] > cap_v):
                cap_l, cap_v = int(totals[0]), int(totals[1])
                continue
            L.check(rc)
            break
    out, l0 = [], 0
    for k in range(K):
        l1 = l0 + int(n_lines[k])
        o = off[l0:l1 + 1]
        out.append((o - o[0], vtx[o[0]:o[-1]].copy()))
        l0 = l1
    return out


def _points(mesh):
    return mesh._xyz.astype(np.float32) if mesh.f32_points else mesh._xyz


def track_static_vectorfields_over_time(mesh: DeviceMesh, V_k_coord, start_time_idx=50, end_time_idx=60,
                                        min_streamline_length=20):
    """``track_static_vectorfields_over_time(surface, V_k_coord, ...)``
    (S6:17-37): ``{str(t): [coordinates[ids] (L, 3), ...]}`` for the frames
    ``start_time_idx <= t < end_time_idx``, with the reference's progress
    print per frame."""
    frames = range(int(start_time_idx), int(end_time_idx))
    V = np.asarray(V_k_coord)
    if len(frames) and not (0 <= frames[0] and frames[-1] < len(V)):
        raise ValueError("frames [%d, %d) outside V_k_coord's %d" % (frames[0], frames[-1] + 1, len(V)))
    pts = _points(mesh)
    res = {}
    lists = streamline_lists(mesh, V[frames[0]:frames[-1] + 1], min_streamline_length) if len(frames) else []
    for t, (off, ids) in zip(frames, lists):
        res[str(t)] = [pts[ids[off[q]:off[q + 1]]] for q in range(len(off) - 1)]
        print(f"{t} has been finished.")
    return res


def extract_static_streamline_dot_product(point, V_now, mesh: DeviceMesh, min_streamline_length=20):
    """``extract_static_streamline_dot_product(point, V_now, surface, ...)``
    (S6:51-138): the line from the vertex nearest to ``point`` (the lowest id
    among equally near ones) as a list of coordinates, or ``[]`` when it has
    fewer than ``min_streamline_length`` vertices. Like the reference's, it
    does not look at whether the seed's vector is zero."""
    V = _fields(mesh, V_now)
    if len(V) != 1:
        raise ValueError("V_now must be one field (N, 3)")
    point = np.asarray(point, dtype=np.float64)
    if point.shape != (3,):
        raise ValueError("point must be (3,)")
    pts = _points(mesh)
    seed = int(np.argmin(((mesh._xyz - point) ** 2).sum(axis=1)))
    nxt = np.empty((1, mesh.N), dtype=np.int32)
    h = mesh.handle(None)
    with mesh.lock(None):
        L.check(L.lib().mof_streamline_map(h, L.ptr(V), 1, 0, None, L.ptr(nxt), None))
    ids, seen = [seed], {seed}
    while True:
        j = int(nxt[0, ids[-1]])
        if j < 0 or j in seen:
            break
        ids.append(j)
        seen.add(j)
    return list(pts[ids]) if len(ids) >= min_streamline_length else []
