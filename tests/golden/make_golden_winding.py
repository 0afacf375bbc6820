"""Capture the winding-number golden vectors from the reference itself
(container-only tool, like make_golden_streamlines.py).

Imports ``S7_winding_line.py`` from ``/root/reference`` (read-only; bytecode
writing disabled; ``pyvista``, ``yaml`` and ``utils.draw_optical_flow_field``,
used only by the script's ``__main__``, replaced by empty modules where they
are missing) and runs ``calculate_winding_numbers`` with a small stand-in for
the pyvista surface: ``points``, ``find_closest_point`` (argmin of
``(dx dx + dy dy) + dz dz``, lowest id) and ``point_neighbors_levels`` (a BFS
over the mesh edges yielding each ring's ids ascending, nothing after the last
non-empty ring). The reference's values are recorded by wrapping its
``winding_number`` and ``sort_by_polar_angle_anticlockwise`` from the outside.

Where the rings run out before a check fails the reference raises IndexError
(S7:135, reachable: the 642-vertex meshes are exhausted after 20-24 rings);
the point is then called on its own, the error caught, and its count formed
from the recorded winding numbers with the reference's own ``check_property``.

Meshes: ``W1`` = G1's icosphere with a seeded 0.5 % radial jitter, normals
and areas recomputed (stored here: the unjittered sphere has exactly tied
polar keys beyond level 8); G2, the cap; G3 (float32 points), 8 levels only.
Fields per mesh: the two generic tangent fields of G9 and the tangential part
of a rotated grad(xy) (saddles as well as nodes); on G2 also the solved
``V_k[0]``.

Asserted here, from the reference's own operations: on every ring evaluated,
the failing one included, adjacent polar keys differ by >= 1e-9 and
pi - |angle| >= 1e-6 for every consecutive pair (no vertex or query is
excluded); ``e`` equals ``compute_orthonormal_basis`` bit for bit; and
tests/winding_ref.py reproduces the ring tables, counts and types exactly and
the winding numbers within its bound.

Stored in ``G10_winding.npz`` (keys prefixed with the fixture's name):
  coordinates, normals, areas, e   W1 only (triangles are G1's)
  V                   (K, N, 3) the fields
  wn0, index          (K, N) the reference's level-0 winding number and type
                      at every vertex
  sp_points (P, 3), sp_field (P,), sp_centre (P,)   the singular points of
                      every field (find_singularity_points, eps 1e-3), the
                      field each belongs to, its closest vertex
  sp_count25 / sp_type25 / sp_wn25 (P, 25), and the same at 8
                      the reference's counts, types (0: level 0 failed) and
                      winding numbers per level (NaN: not evaluated)
  sp_ring_off (P, L + 1), sp_ring_vtx   the sorted rings of those centres
  ref_seconds_per_point   the reference's seconds per singular point
Only data is stored: inputs and the reference's outputs.

Run:  python tests/golden/make_golden_winding.py
"""
from __future__ import annotations

import contextlib
import io
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import winding_ref  # noqa: E402
from make_golden_streamlines import solved_field, tangent_field  # noqa: E402

EPS = 1e-3


def load_reference():
    sys.dont_write_bytecode = True
    for name in ("pyvista", "yaml"):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    utils = types.ModuleType("utils")
    utils.draw_optical_flow_field = types.ModuleType("utils.draw_optical_flow_field")
    sys.modules["utils"] = utils
    sys.modules["utils.draw_optical_flow_field"] = utils.draw_optical_flow_field
    sys.path.insert(0, REF)
    import importlib
    s7 = importlib.import_module("S7_winding_line")
    del sys.modules["utils"], sys.modules["utils.draw_optical_flow_field"]
    fsp = importlib.import_module("utils.find_singularity_point")
    sys.path.remove(REF)
    return s7, fsp


class Surface:
    """What the reference takes from its pyvista surface."""

    def __init__(self, points, triangles):
        self.points = points
        self._p64 = np.asarray(points, dtype=np.float64)
        self.adj = winding_ref.adjacency(triangles, len(points))

    def find_closest_point(self, point):
        d = self._p64 - np.asarray(point, dtype=np.float64)
        return int(np.argmin((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))

    def point_neighbors_levels(self, index, n_levels):
        seen = {index}
        front = [index]
        for _ in range(n_levels):
            nxt = sorted({int(j) for i in front for j in self.adj[i]} - seen)
            if not nxt:
                return
            seen.update(nxt)
            yield nxt
            front = nxt


def saddle_field(points, normals):
    """Tangential part of grad(x' y'), p' = R p."""
    a, b = 0.4, -0.7
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    R = Rz @ Rx
    p = np.asarray(points, dtype=np.float64) @ R.T
    g = np.stack([p[:, 1], p[:, 0], np.zeros(len(p))], axis=1) @ R
    n = np.asarray(normals, dtype=np.float64)
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    return g - (g * n).sum(axis=1, keepdims=True) * n


def jittered_sphere(coords, tri):
    rng = np.random.default_rng(20261020)
    p = coords * (1 + 0.005 * rng.uniform(-1, 1, size=(len(coords), 1)))
    a, b, c = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
    fn = np.cross(b - a, c - a)
    areas = 0.5 * np.linalg.norm(fn, axis=1)
    nrm = np.zeros_like(p)
    for k in range(3):
        np.add.at(nrm, tri[:, k], fn)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return p, nrm, areas


class Recorder:
    """The reference's sort and winding_number, wrapped from the outside."""

    def __init__(self, s7):
        self.s7 = s7
        self.sort0, self.wn0 = s7.sort_by_polar_angle_anticlockwise, s7.winding_number
        self.orders, self.wns = [], []
        self.min_gap = self.min_pi = np.inf

    def __enter__(self):
        def sort(point, x, y, vx=None, vy=None):
            res = self.sort0(point, x, y, vx, vy)
            keys = np.sort(np.arctan2(y, x))
            if len(keys) > 1:
                gaps = np.append(np.diff(keys), keys[0] + 2 * np.pi - keys[-1]) if len(keys) > 2 else np.diff(keys)
                self.min_gap = min(self.min_gap, float(np.min(gaps)))
            self.orders.append(np.asarray(res[0]))
            return res

        def wn(vx, vy):
            n = len(vx)
            for i in range(n):
                ang = self.s7.angle_between_vectors([vx[i], vy[i]], [vx[(i + 1) % n], vy[(i + 1) % n]])
                self.min_pi = min(self.min_pi, float(np.pi - abs(ang)))
            val = self.wn0(vx, vy)
            self.wns.append(float(val))
            return val

        self.s7.sort_by_polar_angle_anticlockwise, self.s7.winding_number = sort, wn
        return self

    def __exit__(self, *exc):
        self.s7.sort_by_polar_angle_anticlockwise, self.s7.winding_number = self.sort0, self.wn0

    def take(self):
        o, w = self.orders, self.wns
        self.orders, self.wns = [], []
        return o, w


def one_point(s7, rec, surf, point, V, e, points, max_level):
    """The reference on one singular point: (count, type, wn list, orders)."""
    rec.take()
    try:
        counts, typs = s7.calculate_winding_numbers(surf, [point], V, e, points, max_level)
        orders, wns = rec.take()
        return counts[0], (typs[0] if typs else 0), wns, orders
    except IndexError:  # the rings ran out (S7:135)
        orders, wns = rec.take()
        orders = orders[:len(wns)]
        flag = -1 if -1.01 <= wns[0] <= -0.99 else (1 if 0.99 <= wns[0] <= 1.01 else 0)
        count = 1 if flag else 0
        for w in wns[1:]:
            assert s7.check_property(w, flag), "the rings ran out after a failed check"
            count += 1
        return count, flag, wns, orders


def main():
    s7, fsp = load_reference()
    out = {}
    load = lambda n: np.load(os.path.join(HERE, n + ".npz"), allow_pickle=False)  # noqa: E731
    for name, src, levels in (("W1", "G1_ico642", (25, 8)), ("G2_cap641", "G2_cap641", (25, 8)),
                              ("G3_ico642_f32", "G3_ico642_f32", (8,))):
        with load(src) as z:
            coords, nrm, tri, e, V_k = z["coordinates"], z["normals"], z["triangles"], z["e"], z["V_k"]
        if name == "W1":
            coords, nrm, areas = jittered_sphere(coords, tri)
            e = np.array([s7.compute_orthonormal_basis(n) for n in nrm])
            out.update(W1_coordinates=coords, W1_normals=nrm, W1_areas=areas, W1_e=e)
        N = len(coords)
        for i in range(N):
            e1, e2 = s7.compute_orthonormal_basis(nrm[i])
            assert np.array_equal(e1, e[i, 0]) and np.array_equal(e2, e[i, 1]) and e.dtype == np.float64
        fields = [tangent_field(coords, nrm, 0), tangent_field(coords, nrm, 1), saddle_field(coords, nrm)]
        if name == "G2_cap641":
            fields.append(solved_field(V_k[0], e))
        V = np.array(fields)
        K = len(V)
        surf = Surface(coords, tri)
        adj = surf.adj
        with Recorder(s7) as rec, contextlib.redirect_stdout(io.StringIO()):
            # level 0 at every vertex of every field
            wn0 = np.empty((K, N))
            index = np.zeros((K, N), dtype=np.int8)
            for k in range(K):
                counts, typs = s7.calculate_winding_numbers(surf, list(coords), V[k], e, coords, max_level=1)
                orders, wns = rec.take()
                wn0[k] = wns
                index[k, np.array(counts) == 1] = typs
                for c in range(N):
                    assert np.array_equal(adj[c][orders[c]], winding_ref.sort_ring(coords, e, c, adj[c]))
            dense = (rec.min_gap, rec.min_pi)
            rec.min_gap = rec.min_pi = np.inf
            # the singular points of every field
            pts, fld = [], []
            for k in range(K):
                sv, si, _ = fsp.find_singularity_points(coords, tri, V[k], EPS)
                for p in [v[1] for v in sv] + [t[1] for t in si]:
                    pts.append(np.asarray(p, dtype=np.float64))
                    fld.append(k)
            P = len(pts)
            cen = np.array([surf.find_closest_point(p) for p in pts], dtype=np.int32)
            res = {}
            secs = 0.0
            for L in levels:
                cnt, typ, wn = np.zeros(P, np.int32), np.zeros(P, np.int8), np.full((P, L), np.nan)
                roff, rvtx = np.zeros((P, L + 1), dtype=np.int32), []
                for q in range(P):
                    t0 = time.perf_counter()
                    cnt[q], typ[q], w, orders = one_point(s7, rec, surf, pts[q], V[fld[q]], e, coords, L)
                    if L == levels[0]:
                        secs += time.perf_counter() - t0
                    wn[q, :len(w)] = w
                    rings = list(surf.point_neighbors_levels(int(cen[q]), L))
                    chk = winding_ref.centre_rings(coords, tri, e, int(cen[q]), L, adj)
                    for l in range(L):
                        roff[q, l] = len(rvtx)
                        if l < len(rings):
                            assert np.array_equal(chk[l], winding_ref.sort_ring(coords, e, int(cen[q]), rings[l]))
                            if l < len(orders):  # the reference's own order where it evaluated the ring
                                assert np.array_equal(np.asarray(rings[l])[orders[l]], chk[l]), (name, q, l)
                            rvtx.extend(chk[l].tolist())
                    roff[q, L] = len(rvtx)
                    # the checker against the reference
                    w2, c2, t2 = winding_ref.levels(coords, e, V[fld[q]], int(cen[q]), chk, L)
                    assert c2 == cnt[q] and t2 == typ[q], (name, q, c2, cnt[q], t2, typ[q])
                    assert np.array_equal(np.isnan(w2), np.isnan(wn[q]))
                    for l in np.flatnonzero(~np.isnan(w2)):
                        assert abs(w2[l] - wn[q, l]) <= winding_ref.wn_bound(len(chk[l]))
                res[L] = (cnt, typ, wn, roff, np.asarray(rvtx, dtype=np.int16))
        wc, ic = winding_ref.winding_map(coords, tri, e, V, adj)
        assert np.array_equal(ic, index)
        assert (np.abs(wc - wn0) <= winding_ref.wn_bound(np.array([len(a) for a in adj]))).all()
        print(name, "dense level 0: min key gap %.3g, min pi - |angle| %.3g" % dense)
        print(name, "sparse rings: min key gap %.3g, min pi - |angle| %.3g" % (rec.min_gap, rec.min_pi))
        assert min(dense[0], rec.min_gap) >= 1e-9 and min(dense[1], rec.min_pi) >= 1e-6
        out[name + "_V"] = V
        out[name + "_wn0"] = wn0
        out[name + "_index"] = index
        out[name + "_sp_points"] = np.array(pts).reshape(-1, 3)
        out[name + "_sp_field"] = np.array(fld, dtype=np.int32)
        out[name + "_sp_centre"] = cen
        for L in levels:
            cnt, typ, wn, roff, rvtx = res[L]
            out["%s_sp_count%d" % (name, L)] = cnt
            out["%s_sp_type%d" % (name, L)] = typ
            out["%s_sp_wn%d" % (name, L)] = wn
            print(name, "max_level", L, "fields", fld, "centres", cen.tolist(), "counts", cnt.tolist(), "types",
                  typ.tolist(), "largest ring", int(np.diff(roff, axis=1).max()) if P else 0)
        out[name + "_sp_ring_off"] = res[levels[0]][3]
        out[name + "_sp_ring_vtx"] = res[levels[0]][4]
        out[name + "_ref_seconds_per_point"] = np.array(secs / max(P, 1))
        print(name, "index counts (+1, -1):", (index == 1).sum(axis=1), (index == -1).sum(axis=1),
              "reference seconds per singular point %.3g" % (secs / max(P, 1)))
    path = os.path.join(HERE, "G10_winding.npz")
    np.savez_compressed(path, **out)
    print("G10_winding", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
