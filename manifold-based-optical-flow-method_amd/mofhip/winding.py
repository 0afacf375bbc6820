"""Winding numbers on the mesh: the reference's ``S7_winding_line.py`` on the GPU.

For each singular point the reference reports a type (+1 node / focus, -1
saddle) and the number of consecutive neighbour rings over which the velocity
field keeps that winding number (``calculate_winding_numbers``, S7:120-165).
Which vertices form ring l around a centre, their positions in the centre's
tangent basis and their polar order do not depend on the frame: they are a
ring table per distinct centre (``mof_winding_rings``), built once and shared
by all frames, and a cheap evaluation per (frame, centre) along it
(``mof_winding_levels``). Level 0 at every vertex of every field
(``mof_winding_map``) is the Poincare index of the one-ring: a second
detector, topological and free of ``eps``, beside ``mof_singularities``.

Equal polar keys go to the smaller vertex id (the reference's stable sort
keeps VTK's ring order there). A ring that is empty because the mesh is
exhausted ends the evaluation like a failed check; the reference raises
IndexError there. Level 0 does not stop the loop: level 1 is evaluated even
when level 0 set no type. The functions named like the reference's take a
``DeviceMesh`` where it takes its pyvista ``surf``.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib as L
from .mesh import DeviceMesh
from .streamline import _fields


def _max_level(max_level):
    ml = int(max_level)
    if ml != max_level or not 1 <= ml < 2 ** 15:
        raise ValueError("max_level must be an integer in [1, 32768), not %r" % (max_level,))
    return ml


def _ids(name, a, hi):
    a = np.asarray(a)
    if a.dtype.kind not in "iu" or a.ndim != 1 or a.size < 1:
        raise ValueError("%s must be a non-empty 1-D integer array" % name)
    if a.min() < 0 or a.max() >= hi:
        raise ValueError("%s outside [0, %d)" % (name, hi))
    return np.ascontiguousarray(a, dtype=np.int32)


def _points(points):
    p = np.asarray(points)
    if p.dtype.kind not in "fiu" or p.size == 0 or p.ndim not in (1, 2) or p.shape[-1] != 3:
        raise ValueError("points must be (Q, 3) or (3,) real numbers")
    return np.ascontiguousarray(p.reshape(-1, 3), dtype=np.float64)


def winding_map(mesh: DeviceMesh, V_k_coord, device=None):
    """``(wn0, index)``: the level-0 winding number (K, N) float64 and its type
    (K, N) int8 (+1 / -1 / 0; NaN gives 0) at every vertex of the fields
    V_k_coord (K, N, 3) (one field: (N, 3), K = 1)."""
    V = _fields(mesh, V_k_coord)
    K = len(V)
    wn0 = np.empty((K, mesh.N), dtype=np.float64)
    index = np.empty((K, mesh.N), dtype=np.int8)
    h = mesh.handle(device)
    with mesh.lock(device):
        L.check(L.lib().mof_winding_map(h, L.ptr(V), K, 0, None, L.ptr(wn0), L.ptr(index)))
    return wn0, index


def winding_map_device(mesh: DeviceMesh, V_ptr: int, K: int, device=None, stream=None, wn0_ptr=None, index_ptr=None):
    """Device-pointer form: V (K, N, 3) f64 and the outputs wn0 (K, N) f64 and
    index (K, N) int8 (either may be None) are already in HBM on the handle's
    device (``stream``: a hipStream_t or None); returns when done."""
    if not V_ptr or int(K) < 1 or not (wn0_ptr or index_ptr):
        raise ValueError("winding_map_device needs V, K >= 1 and at least one output")
    h = mesh.handle(device)
    with mesh.lock(device):
        L.check(L.lib().mof_winding_map(h, ctypes.c_void_p(V_ptr), int(K), L.MOF_IO_DEVICE, stream,
                                        ctypes.c_void_p(wn0_ptr) if wn0_ptr else None,
                                        ctypes.c_void_p(index_ptr) if index_ptr else None))


def winding_levels_device(mesh: DeviceMesh, V_ptr: int, K: int, frame_ptr: int, centre_ptr: int, Q: int,
                          max_level=25, all_levels=False, device=None, stream=None, wn_ptr=None, count_ptr=None,
                          type_ptr=None):
    """Device-pointer form of :func:`winding_levels`: V (K, N, 3) f64, frame
    and centre (Q,) int32 and the outputs wn (Q, max_level) f64, count (Q,)
    int32, type (Q,) int8 (any may be None, not all) in HBM; returns when
    done. The library checks the ids after copying them to the host."""
    ml = _max_level(max_level)
    if not (V_ptr and frame_ptr and centre_ptr) or int(K) < 1 or int(Q) < 1 or not (wn_ptr or count_ptr or type_ptr):
        raise ValueError("winding_levels_device needs V, frame, centre, K >= 1, Q >= 1 and at least one output")
    h = mesh.handle(device)
    with mesh.lock(device):
        L.check(L.lib().mof_winding_levels(
            h, ctypes.c_void_p(V_ptr), int(K), ctypes.c_void_p(frame_ptr), ctypes.c_void_p(centre_ptr), int(Q), ml,
            L.MOF_IO_DEVICE | (L.MOF_WIND_ALL_LEVELS if all_levels else 0), stream,
            ctypes.c_void_p(wn_ptr) if wn_ptr else None, ctypes.c_void_p(count_ptr) if count_ptr else None,
            ctypes.c_void_p(type_ptr) if type_ptr else None))


def winding_timing():
    """Milliseconds the last ring-table or levels call spent in the host
    search, the sort kernel and the evaluation kernel."""
    ms = np.zeros(3)
    L.check(L.lib().mof_winding_timing(L.ptr(ms)))
    return {"host_bfs_ms": float(ms[0]), "sort_kernel_ms": float(ms[1]), "levels_kernel_ms": float(ms[2])}


def winding_levels(mesh: DeviceMesh, V_k_coord, frame, centre, max_level=25, all_levels=False, device=None):
    """``(wn, count, type)`` of the queries (frame[q], centre[q]): wn
    (Q, max_level) float64 per level (NaN: not evaluated), count (Q,) int32
    and type (Q,) int8. ``all_levels``: evaluate every non-empty level
    whatever the checks say; count and type are unchanged."""
    V = _fields(mesh, V_k_coord)
    ml = _max_level(max_level)
    f = _ids("frame", frame, len(V))
    c = _ids("centre", centre, mesh.N)
    if f.shape != c.shape:
        raise ValueError("frame and centre differ in length")
    Q = len(f)
    wn = np.empty((Q, ml), dtype=np.float64)
    count = np.empty(Q, dtype=np.int32)
    typ = np.empty(Q, dtype=np.int8)
    h = mesh.handle(device)
    with mesh.lock(device):
        L.check(L.lib().mof_winding_levels(h, L.ptr(V), len(V), L.ptr(f), L.ptr(c), Q, ml,
                                           L.MOF_WIND_ALL_LEVELS if all_levels else 0, None, L.ptr(wn), L.ptr(count),
                                           L.ptr(typ)))
    return wn, count, typ


def winding_rings(mesh: DeviceMesh, centres, max_level=25, device=None):
    """``(level_off, ring_vtx)``: ring l of centre q, in polar order, is
    ``ring_vtx[level_off[q, l]:level_off[q, l + 1]]`` (level_off
    (C, max_level + 1) int64). A first call sized by a guess is repeated once,
    sized, when the table does not fit."""
    c = _ids("centres", centres, mesh.N)
    ml = _max_level(max_level)
    total = ctypes.c_int64(0)
    off = np.empty((len(c), ml + 1), dtype=np.int64)
    cap = 8 * len(c) * ml * (ml + 1)
    h = mesh.handle(device)
    with mesh.lock(device):
        for attempt in (0, 1):
            vtx = np.empty(max(cap, 1), dtype=np.int32)
            rc = L.lib().mof_winding_rings(h, L.ptr(c), len(c), ml, cap, ctypes.byref(total), L.ptr(off), L.ptr(vtx))
            if rc == L.MOF_E_ARG and attempt == 0 and total.value > cap:
                cap = int(total.value)
                continue
            L.check(rc)
            break
    return off, vtx[:total.value].copy()


def closest_vertices(mesh: DeviceMesh, points, device=None):
    """``surf.find_closest_point`` for points (Q, 3): the vertex minimising
    ``(dx dx + dy dy) + dz dz`` in float64, the lowest id on ties; (Q,) int32."""
    p = _points(points)
    out = np.empty(len(p), dtype=np.int32)
    h = mesh.handle(device)
    with mesh.lock(device):
        L.check(L.lib().mof_closest_vertices(h, L.ptr(p), len(p), 0, None, L.ptr(out)))
    return out


def calculate_winding_numbers(mesh: DeviceMesh, singularity_points, V_now, e=None, points=None, max_level=25):
    """``calculate_winding_numbers(surf, singularity_points, V_now, e, points,
    max_level)`` (S7:120-165): ``(counts, types)``, one count per point and
    one type per point whose level 0 passed, in the points' order. ``e`` and
    ``points`` are the handle's own; the arguments are accepted for the
    reference's signature and only their shapes are checked."""
    V = _fields(mesh, V_now)
    if len(V) != 1:
        raise ValueError("V_now must be one field (N, 3)")
    ml = _max_level(max_level)
    if e is not None and np.shape(e) != (mesh.N, 2, 3):
        raise ValueError("e must be (N, 2, 3)")
    if points is not None and np.shape(points) != (mesh.N, 3):
        raise ValueError("points must be (N, 3)")
    if len(singularity_points) == 0:
        return [], []
    c = closest_vertices(mesh, np.asarray(singularity_points))
    _, count, typ = winding_levels(mesh, V, np.zeros(len(c), dtype=np.int32), c, ml)
    return [int(x) for x in count], [int(t) for t in typ if t != 0]


def winding_lines(mesh: DeviceMesh, singularity_points_per_frame, V_k_coord, max_level=25):
    """The dict S7's ``__main__`` builds (S7:234-256): ``{str(t): [[point,
    count, type], ...]}`` over the frames with singular points, the points
    with count 0 dropped. One library call for all frames."""
    V = _fields(mesh, V_k_coord)
    ml = _max_level(max_level)
    if len(singularity_points_per_frame) > len(V):
        raise ValueError("%d frames of singular points for %d fields" % (len(singularity_points_per_frame), len(V)))
    frames, pts = [], []
    for t, sp in enumerate(singularity_points_per_frame):
        for p in sp:
            frames.append(t)
            pts.append(p)
    res = {}
    if not pts:
        return res
    c = closest_vertices(mesh, np.asarray(pts))
    _, count, typ = winding_levels(mesh, V, np.asarray(frames, dtype=np.int32), c, ml)
    for q, t in enumerate(frames):
        line = res.setdefault(str(t), [])
        if count[q]:
            line.append([pts[q], int(count[q]), int(typ[q])])
    return res
