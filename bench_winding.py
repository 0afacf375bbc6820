#!/usr/bin/env python3
"""bench_winding.py -- measurement of the winding-number row (mof_winding_map,
mof_winding_levels: S7_winding_line.py on a mesh handle) on MI355X.

Configuration: the C3 mesh (163,842 vertices), K = 32 synthetic tangent fields
resident in HBM. Warm-up calls, then timed repetitions bracketed by HIP events
on the stream the library runs on (every call ends in a stream synchronise, so
the events also see the host's launch gaps; the wall clock is printed beside
them).

One JSON line:
  value            fields/s of the dense map (K * reps / event time), wn0 + index
  map              ms per call and achieved GB/s against the floor
                   K N (24 read + 9 written) B plus one read of the polar-ordered
                   neighbour table (4 B per SELL position) per pass
  sparse           64 queries per frame (seeded random centres) at max_level 25,
                   ids and outputs in HBM: ms per call (events and wall), and
                   from the library's own clocks (mof_winding_timing) the host
                   breadth-first search, the sort kernel and the evaluation
                   kernel, each the median of the repetitions; the same with
                   MOF_WIND_ALL_LEVELS (random centres fail at level 1, so the
                   default call evaluates two rings per query); ring entries
                   and the largest ring
  cpu_baseline     tests/winding_ref.py timed on this box on the singular
                   points of the 642-vertex W1 fixture at max_level 25, seconds
                   per point; and the reference's own seconds per singular
                   point there, recorded in tests/golden/G10_winding.npz when
                   the fixture was made

    python bench_winding.py [--K 32] [--reps 20] [--warmup 3] [--config C3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, "manifold-based-optical-flow-method_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
HBM_PEAK_GBS = 8000.0
WIND_F = 4            # fields per thread of the map kernel (csrc/mof_winding.hip kWindF)
PASS_ELEMS = 2 << 20  # its automatic pass size in (field, vertex) pairs (kWindPassElems)


def tangent_fields(p, n, K):
    nrm = n / np.linalg.norm(n, axis=1, keepdims=True)
    V = np.empty((K, len(p), 3))
    for k in range(K):
        w = (np.cross(np.array([0.31, -0.23, 0.17]) * (1 + 0.3 * k), p) + np.array([0.7, 0.2, -1.1]) + 0.25 * k
             + 0.05 * np.sin(p @ np.array([0.9, -0.4, 0.6]) + k)[:, None] * np.array([0.2, 1.0, -0.5]))
        V[k] = w - (w * nrm).sum(axis=1, keepdims=True) * nrm
    return V


def auto_fields(N, K):  # wind_pass_fields of csrc/mof_winding.hip
    kp = max(1, PASS_ELEMS // N)
    if kp > WIND_F:
        kp = kp // WIND_F * WIND_F
    return min(kp, K)


def cpu_baseline():
    import winding_ref as W
    load = lambda n: np.load(os.path.join(REPO, "tests", "golden", n + ".npz"), allow_pickle=False)  # noqa: E731
    with load("G10_winding") as z, load("G1_ico642") as g:
        pts, e, tri, V = z["W1_coordinates"], z["W1_e"], g["triangles"], z["W1_V"]
        sp, fld = z["W1_sp_points"], z["W1_sp_field"]
        ref = float(z["W1_ref_seconds_per_point"])
    adj = W.adjacency(tri, len(pts))
    t0 = time.perf_counter()
    for k in np.unique(fld):
        W.calculate_winding_numbers(pts, tri, e, sp[fld == k], V[k], 25, adj)
    s = (time.perf_counter() - t0) / len(sp)
    return {"value": round(1.0 / s, 2), "unit": "points/s", "cores": 1, "kind": "port",
            "seconds_per_point": round(s, 5),
            "sample": "tests/winding_ref.py on the %d singular points of W1 (642 vertices), max_level 25" % len(sp),
            "reference_seconds_per_point_642_vertices": round(ref, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--queries-per-frame", type=int, default=64)
    ap.add_argument("--max-level", type=int, default=25)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()

    import torch  # first: the library then shares torch's HIP runtime
    if not torch.cuda.is_available():
        raise SystemExit("bench_winding.py needs a GPU")
    torch.cuda.init()
    from mofhip import DeviceMesh, synth
    from mofhip.winding import (winding_levels, winding_levels_device, winding_map, winding_map_device,
                                winding_rings, winding_timing)

    p, t, n, a = synth.mesh_for_config(args.config)
    N, K, Lv = len(p), args.K, args.max_level
    mesh = DeviceMesh(p, n, t, a)
    info = mesh.info()
    V = tangent_fields(p, n, K)
    dev = torch.device("cuda", 0)
    Vd = torch.from_numpy(V).to(dev)
    wn0 = torch.empty((K, N), dtype=torch.float64, device=dev)
    index = torch.empty((K, N), dtype=torch.int8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()

    def timed(run, after=None):
        for _ in range(max(1, args.warmup)):  # the first map call also builds the neighbour table
            run()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        w0 = time.perf_counter()
        ev0.record(stream)
        for _ in range(args.reps):
            run()
            if after:
                after()
        ev1.record(stream)
        ev1.synchronize()
        return ev0.elapsed_time(ev1) * 1e-3 / args.reps, (time.perf_counter() - w0) / args.reps

    sec_map, wall_map = timed(lambda: winding_map_device(mesh, Vd.data_ptr(), K, stream=stream.cuda_stream,
                                                         wn0_ptr=wn0.data_ptr(), index_ptr=index.data_ptr()))
    hw, hi = winding_map(mesh, V[:2])  # the device result against a host-pointer call on two fields
    same = bool(np.array_equal(wn0[:2].cpu().numpy(), hw, equal_nan=True) and np.array_equal(index[:2].cpu().numpy(), hi))
    idx = index.cpu().numpy()
    kp = auto_fields(N, K)
    passes = -(-K // kp)
    floor = K * N * 33.0 + passes * 4.0 * info["sell_blocks"]

    # the sparse path
    rng = np.random.default_rng(0)
    Q = K * args.queries_per_frame
    frame = np.repeat(np.arange(K, dtype=np.int32), args.queries_per_frame)
    centre = rng.integers(0, N, Q).astype(np.int32)
    fd, cd = torch.from_numpy(frame).to(dev), torch.from_numpy(centre).to(dev)
    wn = torch.empty((Q, Lv), dtype=torch.float64, device=dev)
    cnt = torch.empty(Q, dtype=torch.int32, device=dev)
    typ = torch.empty(Q, dtype=torch.int8, device=dev)
    torch.cuda.synchronize()
    sparse = {"queries": Q, "queries_per_frame": args.queries_per_frame, "max_level": Lv,
              "distinct_centres": int(len(np.unique(centre)))}
    for label, all_levels in (("until_a_check_fails", False), ("all_levels", True)):
        parts = []
        sec, wall = timed(lambda: winding_levels_device(mesh, Vd.data_ptr(), K, fd.data_ptr(), cd.data_ptr(), Q, Lv,
                                                        all_levels=all_levels, stream=stream.cuda_stream,
                                                        wn_ptr=wn.data_ptr(), count_ptr=cnt.data_ptr(),
                                                        type_ptr=typ.data_ptr()),
                          after=lambda: parts.append(winding_timing()))
        med = {k: round(float(np.median([x[k] for x in parts])), 4) for k in parts[0]}
        evaluated = int((~torch.isnan(wn)).sum().item())
        sparse[label] = dict(ms_per_call=round(sec * 1e3, 4), ms_per_call_wall=round(wall * 1e3, 4),
                             rings_evaluated=evaluated, **med)
    off, vtx = winding_rings(mesh, np.unique(centre), Lv)
    sparse["ring_entries"] = int(len(vtx))
    sparse["largest_ring"] = int(np.diff(off, axis=1).max())
    hq = slice(0, 8)
    hwn, hc, ht = winding_levels(mesh, V, frame[hq], centre[hq], Lv, all_levels=True)
    sparse["first_queries_identical_to_host_call"] = bool(
        np.array_equal(wn[hq].cpu().numpy(), hwn, equal_nan=True) and np.array_equal(cnt[hq].cpu().numpy(), hc)
        and np.array_equal(typ[hq].cpu().numpy(), ht))
    b = sparse["all_levels"]
    sparse["host_bfs_share_of_call"] = round(b["host_bfs_ms"] / b["ms_per_call_wall"], 3)

    res = {"row": "winding numbers (S7_winding_line.py)", "config": args.config, "N": N, "K": K,
           "outputs": ["wn0", "index"], "fields_per_thread": WIND_F, "fields_per_pass": kp, "passes": passes,
           "reps": args.reps, "value": round(K / sec_map, 1), "unit": "fields/s",
           "map": {"ms_per_call": round(sec_map * 1e3, 4), "ms_per_call_wall": round(wall_map * 1e3, 4),
                   "index_plus": int((idx == 1).sum()), "index_minus": int((idx == -1).sum()),
                   "roofline": {"bound": "hbm", "floor_bytes": floor, "achieved": round(floor / sec_map / 1e9, 1),
                                "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                "frac": round(floor / sec_map / 1e9 / HBM_PEAK_GBS, 3)}},
           "sparse": sparse, "first_fields_identical_to_host_call": same}
    if not args.no_cpu:
        res["cpu_baseline"] = cpu_baseline()
        per_point = sparse["until_a_check_fails"]["ms_per_call_wall"] * 1e-3 / Q
        res["sparse_seconds_per_point"] = per_point
        res["speedup_vs_reference_per_point"] = round(
            res["cpu_baseline"]["reference_seconds_per_point_642_vertices"] / per_point, 1)
    mesh.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
