"""numpy / scipy checker of the geodesic distances (mof_geodesic, include/mof.h)
and of the reference's error score built on them
(utils/find_singularity_point.py:608-720); pinned to the reference's own
outputs in tests/golden/G11_geodesic.npz by tests/test_geodesic.py.

The distance is Dijkstra's on the mesh's edge graph with the lengths
``sqrt((dx dx + dy dy) + dz dz)`` of the fp64 coordinates: scipy's
``csgraph.dijkstra`` relaxes ``d[u] + w`` in fp64 exactly as the definition
folds a path's lengths from the source, so the comparison with the library is
``np.array_equal``.
"""
from __future__ import annotations

import statistics

import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import dijkstra


def mesh_edges(triangles):
    """The undirected edges (a < b), ascending by (a, b): (E, 2) int32."""
    t = np.asarray(triangles, dtype=np.int64)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    return np.unique(e, axis=0).astype(np.int32)


def edge_lengths(points, edges):
    p = np.asarray(points).astype(np.float64)  # float32 points are widened first
    d = p[edges[:, 0]] - p[edges[:, 1]]
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def graph(n, a, b, w):
    """The symmetric csr graph of the edges (a[k], b[k]) with lengths w[k]."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    w = np.asarray(w, dtype=np.float64)
    assert (w > 0).all()  # scipy drops explicit zeros
    return csr_matrix((np.concatenate([w, w]), (np.concatenate([a, b]), np.concatenate([b, a]))), shape=(n, n))


def distances(g, sources, limit=np.inf):
    """(S, N) rows of the sources in their order; beyond ``limit``: +inf."""
    src = np.asarray(sources, dtype=np.int64).reshape(-1)
    uniq, back = np.unique(src, return_inverse=True)
    d = dijkstra(g, directed=False, indices=uniq)
    if np.isfinite(limit):
        d = np.where(d <= limit, d, np.inf)
    return d[back]


def closest_vertices(points, query):
    p = np.asarray(points, dtype=np.float64)
    out = np.empty(len(query), dtype=np.int32)
    for q, x in enumerate(np.asarray(query, dtype=np.float64).reshape(-1, 3)):
        d = p - x
        out[q] = np.argmin((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return out


def displacement_difference(threshold, det_vertices, true_vertices, dist, i, turning_point):
    """compute_displacement_difference (:608-672) from snapped vertices;
    ``dist(a, b)`` is the geodesic distance from a (a true vertex) to b."""
    err, err_list, matched, spare, missed = 0, [], 0, 0, 0
    flag = [False] * len(det_vertices)
    if len(det_vertices) == 0:
        missed = len(true_vertices)
    elif i < turning_point:
        for tv in true_vertices:
            diff = [dist(tv, v) for v in det_vertices]
            mn = min(diff)
            j = diff.index(mn)
            if mn <= threshold and flag[j] is False:
                err_list.append(mn)
                err += mn
                flag[j] = True
            else:
                missed += 1
        matched = flag.count(True) + 1
        spare = max(len(det_vertices) - matched - 1, 0)
    else:
        missed, matched = 2, 1
    return err, err_list, matched, spare, missed


def err_for_all(true_vertices, det_vertices, threshold, dist, turning_point):
    """compute_err_for_all_Vk (:675-720) from per-frame snapped vertices."""
    err, err_list, matched, spare, missed = 0, [], 0, 0, 0
    for i, (dv, tv) in enumerate(zip(det_vertices, true_vertices)):
        e, el, m, s, ms = displacement_difference(threshold, dv, tv, dist, i, turning_point)
        err += e
        err_list.extend(el)
        matched += m
        spare += s
        missed += ms
    return err, max(err_list), min(err_list), statistics.stdev(err_list), spare, missed, matched


def split_frames(values, frame, n_frames):
    """The per-frame lists of a flat array and its frame index."""
    return [list(values[frame == t]) for t in range(n_frames)]
