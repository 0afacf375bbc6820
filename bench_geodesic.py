#!/usr/bin/env python3
"""bench_geodesic.py -- measurement of the geodesic-distance row (mof_geodesic:
pyvista's surface.geodesic_distance and the reference's error score on a mesh
handle) on MI355X.

Configuration: the C3 mesh (163,842 vertices), seeded random sources, ids and
output resident in HBM. Warm-up calls, then timed repetitions bracketed by HIP
events on the stream the library runs on (every call ends in a stream
synchronise and looks at its counters once per 8 rounds, so the events also see
the host's gaps; the wall clock is printed beside them).

One JSON line:
  value            sources/s at S = 1024, full rows (S, N)
  cases            per case (S = 64 and S = 1024 full rows, S = 1024 with
                   Q = 1024 targets; each also with limit = 5 % of the sphere's
                   diameter 2 r): ms per call (events and wall), sources/s,
                   passes, rounds and tile executions per pass, the library's
                   own clocks (relaxation, gather), and achieved bytes against
                   the floor: one write (the fill) and one read of each pass's
                   block N x 64 x 8 B, the output, and one read of a tile's
                   edges (12 B each) per tile execution -- as a share of the
                   8 TB/s nominal HBM peak, which nobody has measured here
  score            compute_err_for_all_Vk on 1,535 frames x 3 points: seconds
                   per call (wall), distinct sources and targets
  edge_table       host milliseconds of the first call's edge and tile tables
  cpu_baseline     scipy.sparse.csgraph.dijkstra on the same lengths on this
                   box, 64 of the same sources (sampled): one process, and a pool
                   of 16 processes; the reference's own seconds per frame on the
                   642-vertex fixture (tests/golden/G11_geodesic.npz)

    python bench_geodesic.py [--reps 3] [--warmup 1] [--config C3] [--no-cpu]
"""
import argparse
import json
import multiprocessing as mp
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, "manifold-based-optical-flow-method_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
HBM_PEAK_GBS = 8000.0
LANES = 64  # sources per pass (csrc/mof_geodesic.hip kGeoLanes)

_graph = None


def _pool_init(n, a, b, w):
    global _graph
    import geodesic_ref as G
    _graph = G.graph(n, a, b, w)


def _pool_rows(src):
    from scipy.sparse.csgraph import dijkstra
    return float(dijkstra(_graph, directed=False, indices=src).sum())


def cpu_baseline(points, triangles, sources):
    """Before the GPU is initialised: the pool forks."""
    import geodesic_ref as G
    from scipy.sparse.csgraph import dijkstra
    e = G.mesh_edges(triangles)
    w = G.edge_lengths(points, e)
    g = G.graph(len(points), e[:, 0], e[:, 1], w)
    src = np.asarray(sources[:64], dtype=np.int64)
    t0 = time.perf_counter()
    rows = dijkstra(g, directed=False, indices=src)
    one = time.perf_counter() - t0
    with mp.get_context("fork").Pool(16, initializer=_pool_init, initargs=(len(points), e[:, 0], e[:, 1], w)) as pool:
        pool.map(_pool_rows, [src[i:i + 1] for i in range(16)])  # start the workers
        t0 = time.perf_counter()
        pool.map(_pool_rows, [src[i::16] for i in range(16)])
        many = time.perf_counter() - t0
    with np.load(os.path.join(REPO, "tests", "golden", "G11_geodesic.npz"), allow_pickle=False) as z:
        ref = float(z["W1_ref_seconds_per_frame"])
    return rows, {"kind": "scipy.sparse.csgraph.dijkstra, sampled on 64 of the sources", "sources": 64,
                  "one_process": {"seconds": round(one, 4), "sources_per_s": round(64 / one, 1)},
                  "pool_16": {"seconds": round(many, 4), "sources_per_s": round(64 / many, 1)},
                  "reference_seconds_per_frame_642_vertices": round(ref, 6)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--frames", type=int, default=1535)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()

    from mofhip import synth
    p, t, n, a = synth.mesh_for_config(args.config)
    N = len(p)
    rng = np.random.default_rng(0)
    src_all = rng.choice(N, 1024, replace=False).astype(np.int32)
    tgt_all = rng.choice(N, 1024, replace=False).astype(np.int32)
    cpu_rows, cpu = (None, None) if args.no_cpu else cpu_baseline(p, t, src_all)

    import torch  # after the pool: the library then shares torch's HIP runtime
    if not torch.cuda.is_available():
        raise SystemExit("bench_geodesic.py needs a GPU")
    torch.cuda.init()
    from mofhip import DeviceMesh
    from mofhip.geodesic import (compute_err_for_all_Vk, geodesic_counters, geodesic_distances_device,
                                 geodesic_edges, geodesic_timing)

    mesh = DeviceMesh(p, n, t, a)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    edges, _ = geodesic_edges(mesh)
    E2 = 2 * len(edges)
    radius = float(np.linalg.norm(p, axis=1).mean())
    limit5 = 0.05 * 2 * radius

    def case(S, Q, limit, first=False):
        sd = torch.from_numpy(src_all[:S]).to(dev)
        td = None if Q is None else torch.from_numpy(tgt_all[:Q]).to(dev)
        out = torch.empty((S, N if Q is None else Q), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        run = lambda: geodesic_distances_device(mesh, sd, td, limit, stream=stream.cuda_stream, out=out)  # noqa: E731
        w0 = time.perf_counter()
        run()
        first_s = time.perf_counter() - w0
        build = geodesic_timing()["build_ms"] if first else None
        for _ in range(max(0, args.warmup - 1)):
            run()
        reps = args.reps if first_s < 2.0 else 1
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        parts = []
        w0 = time.perf_counter()
        ev0.record(stream)
        for _ in range(reps):
            run()
            parts.append(geodesic_timing())
        ev1.record(stream)
        ev1.synchronize()
        sec, wall = ev0.elapsed_time(ev1) * 1e-3 / reps, (time.perf_counter() - w0) / reps
        c = geodesic_counters()
        floor = c["passes"] * 2.0 * N * LANES * 8 + out.numel() * 8.0 + c["tile_executions"] * 12.0 * E2 / c["tiles"]
        res = {"S": S, "Q": Q, "limit": None if np.isinf(limit) else round(limit, 4), "reps": reps,
               "ms_per_call": round(sec * 1e3, 3), "ms_per_call_wall": round(wall * 1e3, 3),
               "sources_per_s": round(S / sec, 1), "passes": c["passes"],
               "rounds_per_pass": round(c["rounds"] / c["passes"], 1),
               "launches_per_pass": round(c["launches"] / c["passes"], 1),
               "tile_executions_per_pass": round(c["tile_executions"] / c["passes"], 1), "tiles": c["tiles"],
               "relax_ms": round(float(np.median([x["relax_ms"] for x in parts])), 3),
               "gather_ms": round(float(np.median([x["gather_ms"] for x in parts])), 3),
               "roofline": {"bound": "hbm", "floor_bytes": floor, "achieved": round(floor / sec / 1e9, 1),
                            "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(floor / sec / 1e9 / HBM_PEAK_GBS, 4)}}
        print("bench_geodesic:", json.dumps(res), file=sys.stderr, flush=True)
        return res, out, build

    cases = []
    first, out64, build_ms = case(64, None, np.inf, first=True)
    cases.append(first)
    same = None if cpu_rows is None else bool(np.array_equal(out64.cpu().numpy(), cpu_rows))
    cases.append(case(64, None, limit5)[0])
    for Q in (None, 1024):
        for lim in (np.inf, limit5):
            cases.append(case(1024, Q, lim)[0])

    # the error score: 1,535 frames x 3 detected points at random vertices, the
    # true points displaced by up to 2 % of the radius; threshold 5 % of the diameter
    F = args.frames
    det_v = rng.integers(0, N, (F, 3))
    det = [list(p[v]) for v in det_v]
    true = [list(p[v] + rng.normal(size=(3, 3)) * 0.02 * radius) for v in det_v]
    compute_err_for_all_Vk(true[:8], det[:8], limit5, mesh, F)
    w0 = time.perf_counter()
    tot = compute_err_for_all_Vk(true, det, limit5, mesh, F)
    score_s = time.perf_counter() - w0
    c = geodesic_counters()
    score = {"frames": F, "points_per_frame": 3, "seconds_per_call_wall": round(score_s, 4),
             "frames_per_s": round(F / score_s, 1), "passes": c["passes"],
             "relax_ms": round(geodesic_timing()["relax_ms"], 2), "matched": int(tot[6]), "missed": int(tot[5]),
             "err": float(tot[0])}

    full = [x for x in cases if x["S"] == 1024 and x["Q"] is None and x["limit"] is None][0]
    res = {"row": "geodesic distances (surface.geodesic_distance, compute_err_for_all_Vk)", "config": args.config,
           "N": N, "edges": int(len(edges)), "sources_per_pass": LANES, "rounds_per_counter_look": 8,
           "value": full["sources_per_s"], "unit": "sources/s", "cases": cases, "score": score,
           "edge_table": {"build_ms": round(build_ms, 3)}, "limit_5_percent_of_diameter": round(limit5, 4),
           "first_64_rows_identical_to_scipy": same}
    if cpu is not None:
        res["cpu_baseline"] = cpu
        res["speedup_vs_scipy_pool_16"] = round(full["sources_per_s"] / cpu["pool_16"]["sources_per_s"], 2)
        res["speedup_vs_scipy_one_process"] = round(full["sources_per_s"] / cpu["one_process"]["sources_per_s"], 2)
        res["score_speedup_vs_reference_seconds_per_frame_642_vertices"] = round(
            cpu["reference_seconds_per_frame_642_vertices"] * F / score_s, 2)
    mesh.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
