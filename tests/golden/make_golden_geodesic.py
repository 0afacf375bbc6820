"""Capture the error-score golden vectors from the reference itself
(container-only tool, like make_golden_winding.py).

Imports ``utils/find_singularity_point.py`` from the read-only reference
checkout as make_golden_winding.load_reference does (bytecode writing disabled;
``pyvista`` and ``yaml`` replaced by empty modules where they are missing) and
runs its
``compute_displacement_difference`` and ``compute_err_for_all_Vk`` with a
small stand-in for the pyvista surface: ``find_closest_point`` (argmin of
``(dx dx + dy dy) + dz dz``, lowest id, the winding maker's) and
``geodesic_distance(a, b)`` = scipy's Dijkstra from ``a`` on the edge lengths
``sqrt((dx dx + dy dy) + dz dz)`` (tests/geodesic_ref.py; the definition in
include/mof.h), one search per distinct ``a``, cached.

Meshes: ``W1`` (G1's icosphere with the winding maker's seeded jitter, stored
in G10_winding.npz: the unjittered sphere has exactly tied distances) and G2,
the open cap. Detected points: the singular points ``find_singularity_points``
found in the G10 fields, field ``t % K`` in frame t of 12. True points: the
detected ones displaced by seeded vectors of up to 3.5 (W1) or 6 (G2)
(thresholds 2.0 and 1.0; the stand-in snaps them back to the surface's
vertices), shuffled; frame 3 has no detected point, frame 5 three extra
detected points, frame 6 one true point less, frame 7 no true point. The turning point is 9: frames 9-11 take the fixed
branch.

Asserted here: in no frame before the turning point are two detected vertices
equidistant from a true vertex (no tie in ``min``), and no minimum lies within
1e-9 of the threshold; both branches of the matching (matched; missed because
beyond the threshold) occur.

Stored in ``G11_geodesic.npz`` (keys prefixed with the fixture's name):
  threshold, turning_point, n_frames
  det_points (P, 3), det_frame (P,), det_vertex (P,)     detected, frame order
  true_points (R, 3), true_frame (R,), true_vertex (R,)  true, frame order
  frame_err (F,), frame_matched / frame_spare / frame_missed (F,)
  err_list, err_list_frame    the per-match errors of every frame, flat
  total (4,) err, err_max, err_min, err_stdev; total_int (3,) spare, missed, matched
  src_vertex (U,), src_rows (U, N)   the distance rows the stand-in used
  ref_seconds_per_frame
Only data is stored: inputs and the reference's outputs.

Run:  python tests/golden/make_golden_geodesic.py
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import geodesic_ref as G  # noqa: E402
from make_golden_winding import load_reference  # noqa: E402

THRESHOLD = {"W1": 2.0, "G2_cap641": 1.0}
TURNING = 9
FRAMES = 12


class Surface:
    """What the reference's score takes from its pyvista surface."""

    def __init__(self, points, triangles):
        self.points = points
        self._p64 = np.asarray(points, dtype=np.float64)
        e = G.mesh_edges(triangles)
        self.graph = G.graph(len(points), e[:, 0], e[:, 1], G.edge_lengths(points, e))
        self.rows = {}

    def find_closest_point(self, point):
        d = self._p64 - np.asarray(point, dtype=np.float64)
        return int(np.argmin((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))

    def geodesic_distance(self, a, b):
        if a not in self.rows:
            self.rows[a] = G.distances(self.graph, [a])[0]
        return float(self.rows[a][b])


def frames_for(name, sp, fld, K):
    rng = np.random.default_rng({"W1": 20261021, "G2_cap641": 20261022}[name])
    reach = {"W1": 3.5, "G2_cap641": 6.0}[name]
    det, true = [], []
    for t in range(FRAMES):
        d = [np.array(p) for p in sp[fld == t % K]]
        tr = []
        for p in d:
            v = rng.normal(size=3)
            tr.append(p + v / np.linalg.norm(v) * rng.uniform(0.0, reach))
        order = rng.permutation(len(tr))
        tr = [tr[i] for i in order]
        if t == 3:
            d = []
        if t == 5:
            d = d + [d[0] + np.array([0.0, 3.0, -2.0]), d[-1] + np.array([2.5, 0.0, 1.0]), d[0] * 0.9 + d[-1] * 0.1]
        if t == 6:
            tr = tr[:-1]
        if t == 7:
            tr = []
        det.append(d)
        true.append(tr)
    return det, true


def main():
    _, fsp = load_reference()
    out = {}
    load = lambda n: np.load(os.path.join(HERE, n + ".npz"), allow_pickle=False)  # noqa: E731
    with load("G10_winding") as z:
        g10 = {k: z[k] for k in z.files}
    for name, src in (("W1", "G1_ico642"), ("G2_cap641", "G2_cap641")):
        thr = THRESHOLD[name]
        with load(src) as z:
            coords, tri = z["coordinates"], z["triangles"]
        if name == "W1":
            coords = g10["W1_coordinates"]
        sp, fld, K = g10[name + "_sp_points"], g10[name + "_sp_field"], len(g10[name + "_V"])
        det, true = frames_for(name, sp, fld, K)
        surf = Surface(coords, tri)
        per, el_flat, el_frame = [], [], []
        t0 = time.perf_counter()
        for t in range(FRAMES):
            r = fsp.compute_displacement_difference(thr, det[t], true[t], surf, t, TURNING)
            per.append(r)
            el_flat.extend(r[1])
            el_frame.extend([t] * len(r[1]))
        secs = (time.perf_counter() - t0) / FRAMES
        tot = fsp.compute_err_for_all_Vk(true, det, thr, surf, TURNING)
        # no tie in min, no minimum at the threshold; both outcomes occur
        dv = [[surf.find_closest_point(p) for p in d] for d in det]
        tv = [[surf.find_closest_point(p) for p in d] for d in true]
        gap, margin, n_far = np.inf, np.inf, 0
        for t in range(TURNING):
            for a in tv[t]:
                if not dv[t]:
                    continue
                row = np.sort([surf.geodesic_distance(a, b) for b in dv[t]])
                if len(row) > 1:
                    gap = min(gap, row[1] - row[0])
                margin = min(margin, abs(row[0] - thr))
                n_far += row[0] > thr
        print(name, "min gap between the two nearest detected vertices %.3g, min |minimum - threshold| %.3g, "
              "%d minima beyond the threshold" % (gap, margin, n_far))
        assert gap > 0 and margin >= 1e-9 and n_far > 0 and len(el_flat) > 2
        # the checker reproduces the reference exactly
        for t in range(FRAMES):
            assert G.displacement_difference(thr, dv[t], tv[t], surf.geodesic_distance, t, TURNING) == per[t]
        assert G.err_for_all(tv, dv, thr, surf.geodesic_distance, TURNING) == tot
        src_v = np.array(sorted(surf.rows), dtype=np.int32)
        flat = lambda ll: np.array([p for l in ll for p in l], dtype=np.float64).reshape(-1, 3)  # noqa: E731
        fr = lambda ll: np.array([t for t, l in enumerate(ll) for _ in l], dtype=np.int32)  # noqa: E731
        out.update({
            name + "_threshold": np.array(thr), name + "_turning_point": np.array(TURNING),
            name + "_n_frames": np.array(FRAMES),
            name + "_det_points": flat(det), name + "_det_frame": fr(det),
            name + "_det_vertex": np.array([v for l in dv for v in l], dtype=np.int32),
            name + "_true_points": flat(true), name + "_true_frame": fr(true),
            name + "_true_vertex": np.array([v for l in tv for v in l], dtype=np.int32),
            name + "_frame_err": np.array([float(r[0]) for r in per]),
            name + "_frame_matched": np.array([r[2] for r in per], dtype=np.int32),
            name + "_frame_spare": np.array([r[3] for r in per], dtype=np.int32),
            name + "_frame_missed": np.array([r[4] for r in per], dtype=np.int32),
            name + "_err_list": np.array(el_flat, dtype=np.float64),
            name + "_err_list_frame": np.array(el_frame, dtype=np.int32),
            name + "_total": np.array([float(x) for x in tot[:4]]),
            name + "_total_int": np.array(tot[4:], dtype=np.int32),
            name + "_src_vertex": src_v, name + "_src_rows": np.array([surf.rows[int(v)] for v in src_v]),
            name + "_ref_seconds_per_frame": np.array(secs),
        })
        print(name, "frames", [(len(d), len(t)) for d, t in zip(det, true)], "matched", [r[2] for r in per], "spare",
              [r[3] for r in per], "missed", [r[4] for r in per], "totals", tot, "sources", len(src_v),
              "reference seconds per frame %.3g" % secs)
    path = os.path.join(HERE, "G11_geodesic.npz")
    np.savez_compressed(path, **out)
    print("G11_geodesic", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
