"""Capture the streamline golden vectors from the reference itself
(container-only tool, like make_golden_wave.py).

Imports ``S6_streamline.py`` from ``/root/reference`` (read-only; bytecode
writing disabled; ``pyvista`` and ``utils.draw_optical_flow_field``, used only
by the script's ``__main__`` and plotting, replaced by empty modules) and runs
``track_static_vectorfields_over_time`` on the meshes of G1, G2 and G3 with a
small stand-in for the pyvista surface: ``points``, ``point_normals``,
``faces``, ``find_closest_point``, ``point_cell_ids`` and ``point_neighbors``,
the last two returning ascending ids.

Fields per mesh (K = 3 on G2, 2 on G1 and G3): fields 0 and 1 are the
tangential part of ``a_k x p + b_k + 0.05 sin(c . p + k) d``; on G2 field 2 is
the mesh's own solved ``V_k[0]`` as vectors (process_V_k). G1's and G3's
solved fields are not used: on the unjittered icosphere some 2.5 % of their
vertices have exactly tied maxima, where the reference's choice follows VTK's
neighbour order.

Asserted here: at every vertex and field ``min(top - second, |top|)`` of the
reference's own dot products is at least 1e-6 max|V| (so decisions compare
exactly, no vertex excluded); the handle's ``e`` equals the reference's
``compute_orthonormal_basis(point_normals[i])`` bit for bit; and the
reference's lines equal tests/streamline_ref.py's "successor map + walk to the
first repeat", vertex for vertex.

Stored in ``G9_streamlines.npz`` (keys prefixed with the fixture's name):
  V                     (K, N, 3) the fields
  next, length          (K, N) int16, from the reference's lines at
                        min_streamline_length = 1: next[s] is the second
                        vertex of the line from s (-1: the line is s alone)
  lines20_off / _vtx    field 0 of G1 and G2: the reference's lines at the
                        default 20, offsets (int32) + vertex ids (int16)
  boundary_tests        (K,) boundary-edge tests the successor map runs
  ref_seconds_per_frame the reference's measured seconds per frame
Only data is stored: inputs and the reference's outputs.

Run:  python tests/golden/make_golden_streamlines.py
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
MESHES = ("G1_ico642", "G2_cap641", "G3_ico642_f32")
sys.path.insert(0, os.path.dirname(HERE))
import streamline_ref  # noqa: E402


def load_reference():
    sys.dont_write_bytecode = True
    sys.modules.setdefault("pyvista", types.ModuleType("pyvista"))
    utils = types.ModuleType("utils")
    utils.draw_optical_flow_field = types.ModuleType("utils.draw_optical_flow_field")
    sys.modules.setdefault("utils", utils)
    sys.modules.setdefault("utils.draw_optical_flow_field", utils.draw_optical_flow_field)
    sys.path.insert(0, REF)
    import importlib
    mod = importlib.import_module("S6_streamline")
    sys.path.remove(REF)
    return mod


class Surface:
    """What the reference takes from its pyvista surface."""

    def __init__(self, points, normals, triangles):
        self.points = points
        self.point_normals = normals
        tri = np.asarray(triangles, dtype=np.int64)
        self.faces = np.hstack([np.full((len(tri), 1), 3, dtype=np.int64), tri]).reshape(-1)
        self._cells = [[] for _ in range(len(points))]
        nb = [set() for _ in range(len(points))]
        for q, t in enumerate(tri.tolist()):
            for v in t:
                self._cells[v].append(q)
                nb[v].update(t)
        self._nbrs = [sorted(s - {i}) for i, s in enumerate(nb)]
        self._index = {tuple(p.tolist()): i for i, p in reversed(list(enumerate(points)))}
        assert len(self._index) == len(points), "duplicate points"

    def find_closest_point(self, point):
        return self._index[tuple(np.asarray(point).tolist())]

    def point_cell_ids(self, index):
        return self._cells[index]

    def point_neighbors(self, index):
        return self._nbrs[index]


def tangent_field(points, normals, k):
    p = np.asarray(points, dtype=np.float64)
    n = np.asarray(normals, dtype=np.float64)
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    a = np.array([0.31, -0.23, 0.17]) * (1 + 0.3 * k)
    b = np.array([0.7, 0.2, -1.1]) + 0.25 * k
    c = np.array([0.9, -0.4, 0.6])
    d = np.array([0.2, 1.0, -0.5])
    w = np.cross(a, p) + b + 0.05 * np.sin(p @ c + k)[:, None] * d
    return w - (w * n).sum(axis=1, keepdims=True) * n


def solved_field(V_k_row, e):
    N = len(e)
    return V_k_row[:N, None] * e[:, 0] + V_k_row[N:, None] * e[:, 1]  # process_V_k


def ids_of(surf, line):
    return [surf.find_closest_point(p) for p in line]


def main():
    ref = load_reference()
    out = {}
    for name in MESHES:
        with np.load(os.path.join(HERE, name + ".npz"), allow_pickle=False) as z:
            coords, nrm, tri, e, V_k = z["coordinates"], z["normals"], z["triangles"], z["e"], z["V_k"]
        N = len(coords)
        surf = Surface(coords, nrm, tri)
        for i in range(N):
            e1, e2 = ref.compute_orthonormal_basis(nrm[i])
            assert np.array_equal(e1, e[i, 0]) and np.array_equal(e2, e[i, 1]) and e1.dtype == np.float64
        fields = [tangent_field(coords, nrm, 0), tangent_field(coords, nrm, 1)]
        if name == "G2_cap641":
            fields.append(solved_field(V_k[0], e))
        V = np.array(fields)
        K = len(V)
        # the condition, from the reference's own operations
        det = {}
        nxt_chk = streamline_ref.successor_map(coords, tri, e, V, details=det)
        for k in range(K):
            for i in (0, N // 2, N - 1):  # the checker's dots are the reference's
                nb = surf.point_neighbors(i)
                vt = [ref.project_vector_to_plane(v, e[i, 0], e[i, 1]) for v in coords[nb] - coords[i]]
                dots = np.sum([v / np.linalg.norm(v) for v in vt] * V[k, i], axis=1)
                srt = np.sort(dots)
                assert det["margin"][k, i] == min(srt[-1] - srt[-2], abs(srt[-1]))
            cond = det["margin"][k].min() / np.abs(V[k]).max()
            print(name, "field", k, "min margin / max|V| %.3g" % cond)
            assert cond >= 1e-6
        secs = []
        nxt = np.full((K, N), -1, dtype=np.int32)
        length = np.zeros((K, N), dtype=np.int32)
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.perf_counter()
            res = ref.track_static_vectorfields_over_time(surf, V, 0, K, min_streamline_length=1)
            secs.append((time.perf_counter() - t0) / K)
        for k in range(K):
            lines = res[str(k)]
            assert len(lines) == N  # no zero vectors: one line per seed
            for s, line in enumerate(lines):
                ids = ids_of(surf, line)
                assert ids[0] == s
                assert ids == streamline_ref.walk(nxt_chk[k], s), (name, k, s)
                length[k, s] = len(ids)
                if len(ids) > 1:
                    nxt[k, s] = ids[1]
        assert np.array_equal(nxt, nxt_chk)
        out[name + "_V"] = V
        out[name + "_next"] = nxt.astype(np.int16)
        out[name + "_length"] = length.astype(np.int16)
        out[name + "_boundary_tests"] = det["boundary_tests"]
        assert not det["boundary_passed"].any()
        print(name, "boundary tests", det["boundary_tests"], "terminal", (nxt < 0).sum(axis=1),
              "max length", length.max(axis=1))
        if name != "G3_ico642_f32":
            with contextlib.redirect_stdout(io.StringIO()):
                t0 = time.perf_counter()
                res = ref.track_static_vectorfields_over_time(surf, V, 0, 1)
                secs.append(time.perf_counter() - t0)
            off, vtx = [0], []
            for line in res["0"]:
                vtx.extend(ids_of(surf, line))
                off.append(len(vtx))
            o2, v2 = streamline_ref.line_lists(nxt[0], length[0], 20)
            assert np.array_equal(off, o2) and np.array_equal(vtx, v2)
            out[name + "_lines20_off"] = np.asarray(off, dtype=np.int32)
            out[name + "_lines20_vtx"] = np.asarray(vtx, dtype=np.int16)
            print(name, "lines at 20:", len(off) - 1, "vertices", len(vtx))
        out[name + "_ref_seconds_per_frame"] = np.array(secs)
        print(name, "reference seconds per frame", secs)
    path = os.path.join(HERE, "G9_streamlines.npz")
    np.savez_compressed(path, **out)
    print("G9_streamlines", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
