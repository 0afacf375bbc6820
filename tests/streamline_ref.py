"""CPU checker of the streamline path: S6_streamline.py restated in numpy as
a successor map plus a walk to the first repeat.

The reference's choice of the next vertex at vertex i depends on (field, i)
alone, never on the path walked so far, so its greedy walk from every seed
(S6:17-37, 51-138) is ``next[i]`` per field and, from a seed s,
``s, next[s], next[next[s]], ...`` up to the first vertex that is terminal
or already on the path. ``successor_map`` keeps the reference's operations and
their order at each vertex (the same numpy calls on the same operands), the
boundary-edge test of S6:100-133 included, vertex *indices* where it passes
indices. Neighbours and incident triangles are taken in ascending id, so the
first of equal maxima is the smallest vertex id. tests/test_streamline.py pins
all of it to tests/golden/G9_streamlines.npz, derived from the reference's own
output.

Line numbers: S6_streamline.py of the reference.
"""
from __future__ import annotations

import numpy as np


class Adjacency:
    """Incident triangles (ascending) and neighbours (ascending) per vertex."""

    def __init__(self, triangles, N):
        tri = np.asarray(triangles, dtype=np.int64)
        flat = tri.ravel()
        order = np.argsort(flat, kind="stable")
        self.tri = tri
        self.cell_ptr = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=N))])
        self.cell_ids = order // 3  # stable sort of the flattened corners: ascending triangle ids

    def cells(self, i):
        return self.cell_ids[self.cell_ptr[i]:self.cell_ptr[i + 1]]

    def neighbours(self, i):
        v = np.unique(self.tri[self.cells(i)])
        return v[v != i]


def unit_directions(coordinates, e_i, i, nbrs):
    """The normalised tangent-plane projections of p_j - p_i (S6:69-75);
    float32 points give a float32 difference, the rest is float64."""
    e1, e2 = e_i
    n = np.cross(e1, e2)
    vectors = coordinates[nbrs] - coordinates[i]
    out = []
    for v in vectors:
        vt = v - np.dot(v, n) * n / np.dot(n, n)
        out.append(vt / np.linalg.norm(vt))
    return out


def _position_diff(A, B, e1, e2):
    # position_diff_on_basis_with_origin (S6:173-182), called with vertex ids
    rel = B - A
    n = np.cross(e1, e2)
    proj = rel - np.dot(rel, n) * n / np.dot(n, n)
    return np.dot(proj, e1), np.dot(proj, e2)


def _cross2(a, b):
    return a[0] * b[1] - a[1] * b[0]


def boundary_edge_test(tri_row, i, e_i, V_i):
    """S6:100-128 for the one triangle ``tri_row`` that i shares with its
    chosen neighbour: True when the walk may go on. The 2-D triangle is built
    from differences of vertex *ids* (S6:115-116), so its corners are
    multiples of one vector up to rounding."""
    e1, e2 = e_i
    A, B, C = (int(v) for v in tri_row)
    if A == i:
        pass
    elif B == i:
        B, A = A, i
    elif C == i:
        C, A = A, i
    p1 = _position_diff(A, B, e1, e2)
    p2 = _position_diff(C, A, e1, e2)
    a, b, c = (0, 0), p1, p2
    cross = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])  # clockwise (S6:204-219)
    if cross > 0:
        pass
    elif cross < 0:
        b, c = c, b
    else:
        return False
    p = (np.dot(V_i, e1) / np.dot(e1, e1), np.dot(V_i, e2) / np.dot(e2, e2))  # express_vector_on_basis
    a, b, c, p = (np.array(x, dtype=np.float64) for x in (a, b, c, p))
    # inTri (S6:184-202) == 1
    return bool(_cross2(b - a, p - a) > 0 and _cross2(c - b, p - b) > 0 and _cross2(a - c, p - c) > 0)


def successor_map(coordinates, triangles, e, V, vertices=None, details=None):
    """next (K, len(vertices)) int32 for the fields V (K, N, 3): the vertex the
    reference steps to from each vertex (path checks aside), or -1 where it
    stops: not ``d > 0`` at the best neighbour (S6:43), or a failed
    boundary-edge test (S6:129). ``details``: a dict that receives ``margin``
    (K, n) = min(top - second, |top|) of the dot products, ``top`` (K, n) the
    largest one, ``tested`` (K, n) whether the boundary-edge test ran, and
    ``boundary_tests`` (K,) = tests run, ``boundary_passed`` (K,)."""
    V = np.asarray(V, dtype=np.float64)
    if V.ndim == 2:
        V = V[None]
    N = len(coordinates)
    adj = Adjacency(triangles, N)
    verts = range(N) if vertices is None else vertices
    out = np.full((len(V), len(verts)), -1, dtype=np.int32)
    margin = np.zeros(out.shape)
    tops = np.zeros(out.shape)
    tested = np.zeros(out.shape, dtype=bool)
    ntest = np.zeros(len(V), dtype=np.int64)
    npass = np.zeros(len(V), dtype=np.int64)
    for q, i in enumerate(verts):
        nbrs = adj.neighbours(i)
        cells_i = adj.cells(i)
        unit = unit_directions(coordinates, e[i], i, nbrs)
        for k in range(len(V)):
            dots = np.sum(unit * V[k, i], axis=1)
            idx = int(np.argmax(dots))
            top = dots[idx]
            rest = np.delete(dots, idx)
            with np.errstate(invalid="ignore"):
                margin[k, q] = min(top - rest.max(), abs(top)) if len(rest) else abs(top)
            tops[k, q] = top
            ok = bool(top > 0)
            if len(cells_i) < 6:
                common = np.intersect1d(cells_i, adj.cells(int(nbrs[idx])))
                if len(common) < 2:
                    ntest[k] += 1
                    tested[k, q] = True
                    passed = boundary_edge_test(adj.tri[common[0]], i, e[i], V[k, i])
                    npass[k] += passed
                    ok = ok and passed
            if ok:
                out[k, q] = nbrs[idx]
    if details is not None:
        details.update(margin=margin, top=tops, tested=tested, boundary_tests=ntest, boundary_passed=npass)
    return out


def walk(next_row, seed):
    """The vertex ids of the reference's line from ``seed``: it ends before the
    first vertex that is terminal-exited or already on the path. The reference
    compares coordinates (S6:44); on a mesh without duplicate points that is
    the comparison of ids."""
    path, seen = [int(seed)], {int(seed)}
    while True:
        j = int(next_row[path[-1]])
        if j < 0 or j in seen:
            return path
        path.append(j)
        seen.add(j)


def lengths(next_rows, V, seeds=None):
    """length (K, n): vertices of the line from each seed, 0 where the seed is
    skipped because its vector is zero (S6:29)."""
    V = np.asarray(V, dtype=np.float64)
    if V.ndim == 2:
        V, next_rows = V[None], np.asarray(next_rows)[None]
    N = V.shape[1]
    seeds = range(N) if seeds is None else seeds
    out = np.zeros((len(V), len(seeds)), dtype=np.int32)
    for k in range(len(V)):
        for q, s in enumerate(seeds):
            if np.linalg.norm(V[k, s]) != 0:
                out[k, q] = len(walk(next_rows[k], s))
    return out


def line_lists(next_row, length_row, min_streamline_length=20):
    """(offsets, vertex ids) of one field's kept lines, seeds ascending
    (S6:28-32, 135-138)."""
    off, ids = [0], []
    for s in range(len(next_row)):
        if length_row[s] > 0 and length_row[s] >= min_streamline_length:
            ids.extend(walk(next_row, s))
            off.append(len(ids))
    return np.asarray(off, dtype=np.int64), np.asarray(ids, dtype=np.int32)
