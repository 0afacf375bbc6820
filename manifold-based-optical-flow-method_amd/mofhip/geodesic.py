"""Geodesic distances on the mesh and the reference's error score on the GPU.

``surface.geodesic_distance`` of pyvista is Dijkstra's algorithm on the edge
graph with Euclidean edge lengths; the reference calls it once per (true
point, detected point) pair per frame (``compute_displacement_difference``,
utils/find_singularity_point.py:608-672). ``mof_geodesic`` (include/mof.h)
computes the same distances for many sources at once: d(s, v) is the minimum
over all edge paths of the fp64 sum of ``sqrt((dx dx + dy dy) + dz dz)`` folded
from s, +inf where no path exists, bit for bit what
``scipy.sparse.csgraph.dijkstra`` returns on those lengths. ``d(a, b)`` and
``d(b, a)`` may differ in the last bits; the source is the first argument, as
in the reference (the true point). Parity with VTK's own implementation is
unpinned.

The functions named like the reference's take a ``DeviceMesh`` where it takes
its pyvista ``surface``.
"""
from __future__ import annotations

import ctypes
import statistics  # noqa: F401  (compute_err_for_all_Vk raises its StatisticsError)

import numpy as np

from . import _lib as L
from .winding import _ids, closest_vertices


def _limit(limit):
    lim = float(limit)
    if not lim > 0.0:
        raise ValueError("limit must be positive (it may be inf), not %r" % (limit,))
    return lim


def geodesic_distances(mesh, sources, targets=None, limit=np.inf, device=None):
    """Distances (S, Q) float64 from the vertices ``sources`` to the vertices
    ``targets``, or (S, N) to every vertex when ``targets`` is None. Sources may
    repeat and be unsorted. With a finite ``limit`` every distance above it is
    +inf and the others are unchanged."""
    s = _ids("sources", sources, mesh.N)
    t = None if targets is None else _ids("targets", targets, mesh.N)
    lim = _limit(limit)
    out = np.empty((len(s), mesh.N if t is None else len(t)), dtype=np.float64)
    h = mesh.handle(device)
    with mesh.lock(device):
        L.check(L.lib().mof_geodesic(h, L.ptr(s), len(s), None if t is None else L.ptr(t), 0 if t is None else len(t),
                                     lim, 0, None, L.ptr(out)))
    return out


def _i32_tensor(name, x):
    import torch
    if not isinstance(x, torch.Tensor) or x.dtype != torch.int32 or x.dim() != 1 or x.numel() < 1 or not x.is_cuda:
        raise ValueError("%s must be a non-empty 1-D int32 tensor on the GPU" % name)
    return x.contiguous()


def geodesic_distances_device(mesh, sources, targets=None, limit=np.inf, device=None, stream=None, out=None):
    """:func:`geodesic_distances` on torch tensors in HBM on the handle's
    device: ``sources`` (S,) and ``targets`` (Q,) int32; returns (or fills
    ``out``) a float64 tensor (S, Q) or (S, N). The library checks the ids
    after copying them to the host; returns when done."""
    import torch
    s = _i32_tensor("sources", sources)
    t = None if targets is None else _i32_tensor("targets", targets)
    lim = _limit(limit)
    shape = (s.numel(), mesh.N if t is None else t.numel())
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=s.device)
    elif out.dtype != torch.float64 or tuple(out.shape) != shape or not out.is_contiguous() or not out.is_cuda:
        raise ValueError("out must be a contiguous float64 GPU tensor of shape %r" % (shape,))
    torch.cuda.current_stream(s.device).synchronize()  # the inputs are written
    h = mesh.handle(device)
    with mesh.lock(device):
        L.check(L.lib().mof_geodesic(h, ctypes.c_void_p(s.data_ptr()), shape[0],
                                     None if t is None else ctypes.c_void_p(t.data_ptr()),
                                     0 if t is None else shape[1], lim, L.MOF_IO_DEVICE, stream,
                                     ctypes.c_void_p(out.data_ptr())))
    return out


def geodesic_distance(mesh, a, b, device=None):
    """``surface.geodesic_distance(a, b)``: the distance from vertex a to
    vertex b, a float."""
    return float(geodesic_distances(mesh, [int(a)], [int(b)], device=device)[0, 0])


def geodesic_edges(mesh, device=None):
    """``(edges (E, 2) int32, lengths (E,) float64)``: the mesh's edges
    (a < b, ascending) and their lengths as the distances use them."""
    total = ctypes.c_int64(0)
    h = mesh.handle(device)
    with mesh.lock(device):
        lib = L.lib()
        rc = lib.mof_geodesic_edges(h, 0, ctypes.byref(total), None, None, None)
        if not (rc == L.MOF_E_ARG and total.value > 0):
            L.check(rc)
        n = int(total.value)
        a, b, w = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.float64)
        if n:
            L.check(lib.mof_geodesic_edges(h, n, ctypes.byref(total), L.ptr(a), L.ptr(b), L.ptr(w)))
    return np.stack([a, b], axis=1), w


def geodesic_timing():
    """Milliseconds the last :func:`geodesic_distances` call spent building the
    edge and tile tables (0 when they existed), relaxing and gathering."""
    ms = np.zeros(3)
    L.check(L.lib().mof_geodesic_timing(L.ptr(ms)))
    return {"build_ms": float(ms[0]), "relax_ms": float(ms[1]), "gather_ms": float(ms[2])}


def geodesic_counters():
    """What the last call did: passes, tile-kernel launches, tile executions,
    rounds, whether the edge table was built, tiles, tile and pass size."""
    c = np.zeros(8, dtype=np.int64)
    L.check(L.lib().mof_geodesic_counters(L.ptr(c)))
    keys = ("passes", "launches", "tile_executions", "rounds", "built", "tiles", "tile", "pass")
    return {k: int(v) for k, v in zip(keys, c)}


def _match(threshold, D, n_true, n_det, i, id):
    """The matching of compute_displacement_difference on the distances D
    (n_true, n_det): true points in order, the first minimum wins."""
    err, err_list, matched_num, spare, missed = 0, [], 0, 0, 0
    flag = [False] * n_det
    if n_det == 0:
        missed = n_true
    elif i < id:
        for t in range(n_true):
            j = int(np.argmin(D[t]))  # the first of equal minima, as list.index(min(...))
            min_diff = float(D[t, j])
            if min_diff <= threshold and flag[j] is False:
                err_list.append(min_diff)
                err += min_diff
                flag[j] = True
            else:
                missed += 1
        matched_num = flag.count(True) + 1
        spare = max(n_det - matched_num - 1, 0)
    else:
        missed = 2
        matched_num = 1
    return err, err_list, matched_num, spare, missed


def _pairwise(surface, true_v, det_v):
    """Distances (len(true_v), len(det_v)) from one library call with the
    distinct true vertices as sources and the distinct detected ones as targets."""
    if len(true_v) == 0 or len(det_v) == 0:
        return np.empty((len(true_v), len(det_v)))
    us, si = np.unique(true_v, return_inverse=True)
    ut, ti = np.unique(det_v, return_inverse=True)
    d = geodesic_distances(surface, us.astype(np.int32), ut.astype(np.int32))
    return d[np.ix_(si, ti)]


def compute_displacement_difference(threshold, singularity_points, true_singularity_points, surface, i, id):
    """``compute_displacement_difference(threshold, singularity_points,
    true_singularity_points, surface, i, id)`` (:608-672) with a ``DeviceMesh``
    as ``surface``: ``(err, err_list, matched_num, spare_singularity_points_num,
    missed_singularity_points_num)``.

    Kept from the reference: every point is snapped to its closest vertex; with
    no detected point every true point is missed; for ``i < id`` each true
    point, in order, takes the detected point at the smallest geodesic
    distance from it (the first of equal minima), matches when that distance is
    <= threshold and the detected point is still free, and is missed otherwise
    -- the minimum is taken before the threshold, so a nearer taken point hides
    a farther free one; ``matched_num = flag.count(True) + 1`` and
    ``spare = max(n_detected - matched_num - 1, 0)``; for ``i >= id`` the fixed
    ``(missed, matched) = (2, 1)`` with no error. ``err`` is summed in the
    reference's order (the int 0 when nothing matched)."""
    n_true, n_det = len(true_singularity_points), len(singularity_points)
    tv = closest_vertices(surface, np.asarray(true_singularity_points)) if n_true else np.empty(0, np.int32)
    dv = closest_vertices(surface, np.asarray(singularity_points)) if n_det else np.empty(0, np.int32)
    D = _pairwise(surface, tv, dv) if (n_det and i < id) else None
    return _match(threshold, D, n_true, n_det, i, id)


def compute_err_for_all_Vk(true_singularity_points, singularity_points, threshold, surface, turning_point):
    """``compute_err_for_all_Vk(true_singularity_points, singularity_points,
    threshold, surface, turning_point)`` (:675-720) with a ``DeviceMesh`` as
    ``surface``: ``(err, err_max, err_min, err_stdev,
    spare_singularity_points_num, missed_singularity_points_num, matched_num)``.

    All points of all frames are snapped with one ``closest_vertices`` call and
    all distances come from one ``mof_geodesic`` call (distinct true vertices
    as sources, distinct detected vertices as targets, no limit: the reference
    takes the minimum before it compares with the threshold); the matching of
    :func:`compute_displacement_difference`, quirks included, then runs per
    frame on the host and the totals are added in frame order. As in the
    reference, ``max`` / ``min`` raise ValueError when no point matched in any
    frame and ``statistics.stdev`` raises StatisticsError on fewer than two
    matches; frames beyond the shorter of the two lists are ignored (``zip``)."""
    frames = list(zip(singularity_points, true_singularity_points))
    pts = [p for det, true in frames for p in list(true) + list(det)]
    verts = closest_vertices(surface, np.asarray(pts)) if pts else np.empty(0, np.int32)
    tvs, dvs, at = [], [], 0
    for det, true in frames:
        tvs.append(verts[at:at + len(true)])
        at += len(true)
        dvs.append(verts[at:at + len(det)])
        at += len(det)
    use = [i for i in range(len(frames)) if i < turning_point and len(dvs[i]) and len(tvs[i])]
    if use:
        us = np.unique(np.concatenate([tvs[i] for i in use]))
        ut = np.unique(np.concatenate([dvs[i] for i in use]))
        dist = geodesic_distances(surface, us.astype(np.int32), ut.astype(np.int32))
    err, err_list, matched_num, spare, missed = 0, [], 0, 0, 0
    for i in range(len(frames)):
        D = None
        if i in use:
            D = dist[np.ix_(np.searchsorted(us, tvs[i]), np.searchsorted(ut, dvs[i]))]
        elif len(dvs[i]) and i < turning_point:
            D = np.empty((0, len(dvs[i])))
        e, el, m, s, ms = _match(threshold, D, len(tvs[i]), len(dvs[i]), i, turning_point)
        err += e
        err_list.extend(el)
        matched_num += m
        spare += s
        missed += ms
    err_max = max(err_list)
    err_min = min(err_list)
    err_stdev = statistics.stdev(err_list)
    return err, err_max, err_min, err_stdev, spare, missed, matched_num
