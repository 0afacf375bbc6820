"""numpy checker of the winding numbers (S7_winding_line.py), operation by
operation as the reference writes them; tests/test_winding.py pins it to the
reference's own values in tests/golden/G10_winding.npz.

For a centre c with e1, e2 = e[c], n = e1 x e2 (S7:26-57, 120-165):
  ring l          the vertices at edge distance l + 1 from c, ascending ids;
  polar key       atan2(v, u), (u, v) = (proj . e1, proj . e2),
                  proj = w - (w . n) n / (n . n), w = p_j - p_c formed in the
                  points' own dtype (float32 points: a float32 difference);
                  keys ascending, equal keys to the smaller id;
  field           Vt = V_j - (V_j . n) n / (n . n),
                  (a, b) = (Vt . e1 / e1 . e1, Vt . e2 / e2 . e2);
  winding number  sum of the signed angles between consecutive unit vectors
                  of the sorted cyclic sequence (arccos of the clamped dot,
                  negated when the 2-D cross product is < 0), in sequence
                  order, divided by 2 pi.
An empty ring ends the evaluation as a failed check (the reference raises
IndexError there). Dots of 3-vectors are (a0 b0 + a1 b1) + a2 b2.
"""
from __future__ import annotations

import numpy as np

TWO_PI = 2 * np.pi


def adjacency(tri, N):
    nb = [set() for _ in range(N)]
    for t in np.asarray(tri).tolist():
        for v in t:
            nb[v].update(t)
    return [np.array(sorted(s - {i}), dtype=np.int64) for i, s in enumerate(nb)]


def rings(adj, c, max_level):
    """Ring l = vertices at edge distance l + 1 from c, ascending; stops after
    the last non-empty ring (at most max_level rings)."""
    seen = np.zeros(len(adj), dtype=bool)
    seen[c] = True
    front, out = np.array([c]), []
    for _ in range(max_level):
        nxt = np.unique(np.concatenate([adj[i] for i in front])) if len(front) else front
        nxt = nxt[~seen[nxt]]
        if len(nxt) == 0:
            break
        seen[nxt] = True
        out.append(nxt)
        front = nxt
    return out


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _basis(e, c):
    e1, e2 = np.asarray(e[c, 0], dtype=np.float64), np.asarray(e[c, 1], dtype=np.float64)
    n = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]])
    return e1, e2, n, _dot(n, n)


def polar_keys(points, e, c, ids):
    e1, e2, n, nn = _basis(e, c)
    w = (points[ids] - points[c]).astype(np.float64)  # in the points' dtype, as points[x] - points[index]
    proj = w - _dot(w, n)[:, None] * n / nn
    return np.arctan2(_dot(proj, e2), _dot(proj, e1))


def sort_ring(points, e, c, ids):
    """ids (ascending) in polar order: keys ascending, equal keys by id."""
    ids = np.asarray(ids)
    return ids[np.lexsort((ids, polar_keys(points, e, c, ids)))]


def ring_table(points, tri, e, centres, max_level, adj=None):
    """(level_off (C, max_level + 1), ring_vtx) of mof_winding_rings."""
    adj = adjacency(tri, len(points)) if adj is None else adj
    off = np.zeros((len(centres), max_level + 1), dtype=np.int64)
    vtx, tot = [], 0
    for q, c in enumerate(centres):
        rs = rings(adj, int(c), max_level)
        for l in range(max_level):
            off[q, l] = tot
            if l < len(rs):
                vtx.append(sort_ring(points, e, int(c), rs[l]))
                tot += len(rs[l])
        off[q, max_level] = tot
    return off, (np.concatenate(vtx) if vtx else np.zeros(0, dtype=np.int64)).astype(np.int32)


def ring_angles(V, e, c, ring):
    """The signed angles (S7:59-74) along the sorted ring, V (N, 3)."""
    e1, e2, n, nn = _basis(e, c)
    Vj = np.asarray(V, dtype=np.float64)[ring]
    with np.errstate(all="ignore"):
        Vt = Vj - _dot(Vj, n)[:, None] * n / nn
        a, b = _dot(Vt, e1) / _dot(e1, e1), _dot(Vt, e2) / _dot(e2, e2)
        r = np.sqrt(a * a + b * b)
        ux, uy = a / r, b / r
        vx, vy = np.roll(ux, -1), np.roll(uy, -1)
        d = ux * vx + uy * vy
        d = np.where(d > 1, 1.0, np.where(d < -1, -1.0, d))
        ang = np.arccos(d)
        return np.where(ux * vy - uy * vx < 0, -ang, ang)


def winding_number(V, e, c, ring):
    acc = 0.0
    for x in ring_angles(V, e, c, ring).tolist():  # in sequence order
        acc += x
    return acc / TWO_PI


def wn_bound(n_ring):
    """|wn - any reordering of the same operations|: arccos near +-1 turns one
    rounding of the dot into sqrt(8 * 2^-52) of angle at worst, per pair."""
    return n_ring * np.sqrt(8 * 2.0 ** -52) / TWO_PI


def level0_type(wn):
    if -1.01 <= wn <= -0.99:
        return -1
    if 0.99 <= wn <= 1.01:
        return 1
    return 0


def check_property(wn, flag):
    if flag == 1:
        return 0.999 <= wn <= 1.001
    if flag == -1:
        return -1.001 <= wn <= -0.999
    return False


def levels(points, e, V, c, sorted_rings, max_level, all_levels=False):
    """(wn (max_level,), count, type, ring sizes) of one query (S7:133-164).
    sorted_rings: the centre's non-empty rings in polar order."""
    wn = np.full(max_level, np.nan)
    count = flag = 0
    live = True
    for l in range(max_level):
        if l >= len(sorted_rings):
            break  # an empty ring: the reference raises IndexError
        if not live and not all_levels:
            break
        wn[l] = winding_number(V, e, c, sorted_rings[l])
        if not live:
            continue
        if l == 0:
            flag = level0_type(wn[0])
            count = 1 if flag else 0
        elif check_property(wn[l], flag):
            count += 1
        else:
            live = False
    return wn, count, flag


def centre_rings(points, tri, e, c, max_level, adj=None):
    adj = adjacency(tri, len(points)) if adj is None else adj
    return [sort_ring(points, e, c, r) for r in rings(adj, c, max_level)]


def winding_map(points, tri, e, V, adj=None):
    """Level 0 at every vertex of every field: (wn0 (K, N), index (K, N) int8)."""
    V = np.asarray(V, dtype=np.float64)
    adj = adjacency(tri, len(points)) if adj is None else adj
    K, N = V.shape[:2]
    wn0 = np.full((K, N), np.nan)
    idx = np.zeros((K, N), dtype=np.int8)
    for c in range(N):
        if len(adj[c]) == 0:
            continue
        ring = sort_ring(points, e, c, adj[c])
        for k in range(K):
            wn0[k, c] = winding_number(V[k], e, c, ring)
            idx[k, c] = level0_type(wn0[k, c])
    return wn0, idx


def closest_vertices(points, q):
    """argmin of (dx dx + dy dy) + dz dz in fp64, the lowest id on ties."""
    p = np.asarray(points, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    out = np.empty(len(q), dtype=np.int32)
    for i, x in enumerate(q):
        d = p - x
        out[i] = np.argmin((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return out


def calculate_winding_numbers(points, tri, e, singularity_points, V_now, max_level=25, adj=None):
    """(counts, types) with the reference's list shapes."""
    adj = adjacency(tri, len(points)) if adj is None else adj
    counts, types = [], []
    for c in closest_vertices(points, singularity_points).tolist():
        _, cnt, flag = levels(points, e, V_now, c, centre_rings(points, tri, e, c, max_level, adj), max_level)
        counts.append(cnt)
        if flag:
            types.append(flag)
    return counts, types
