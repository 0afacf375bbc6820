#!/usr/bin/env python3
"""bench_streamline.py -- measurement of the streamline row (SURVEY.md §8(f)6,
mof_streamline_map: S6_streamline.py on a mesh handle) on MI355X.

Configuration: the C3 mesh (163,842 vertices), K = 32 synthetic tangent fields
resident in HBM, ``next`` and ``length`` as device outputs. Warm-up calls, then
timed repetitions bracketed by HIP events on the stream the library runs on
(every call ends in a stream synchronise, so the events also see the host's
launch gaps between passes; the wall clock is printed beside them). The map
kernel is timed by calls that ask for ``next`` alone; the walk is the
difference to the calls that ask for both.

One JSON line:
  value            fields/s (K * reps / event time), next + length
  map              the successor-map kernel alone: ms per call, and its
                   achieved GB/s against the floor K N (24 read + 8 written) B
                   plus one read of the direction table (24 B of u_j, 4 B of
                   neighbour id per SELL position) per pass
  walk             the lengths alone: ms per call, line vertices per second
                   (the sum of the lengths the reference would walk, not the
                   pointer steps taken: pointer jumping takes about
                   2 N log2 N per field), mean and max length. A pointer chase
                   in a table that fits in L2 has no byte floor: none is given
  cpu_baseline     tests/streamline_ref.py (the reference's operations per
                   vertex, then a walk with a visited set -- so linear where
                   the reference rescans its path) timed on this box on a
                   642-vertex icosphere and scaled by N / 642; and the
                   reference's own seconds per frame on the 642-vertex G1,
                   recorded in tests/golden/G9_streamlines.npz when the
                   fixture was made (not scaled: its cost grows faster than N)

    python bench_streamline.py [--K 32] [--reps 20] [--warmup 3] [--config C3]
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
STREAM_F = 4                # fields per thread of the map kernel (csrc/mof_streamline.hip kStreamF)
PASS_ELEMS = 2 << 20        # its automatic pass size in (field, vertex) pairs (kStreamPassElems)
WALK = "pointer jumping"    # the committed build's lengths (MOF_STREAM_WALK 1; 0: one Brent walk per seed)


def tangent_fields(p, n, K):
    nrm = n / np.linalg.norm(n, axis=1, keepdims=True)
    V = np.empty((K, len(p), 3))
    for k in range(K):
        w = (np.cross(np.array([0.31, -0.23, 0.17]) * (1 + 0.3 * k), p) + np.array([0.7, 0.2, -1.1]) + 0.25 * k
             + 0.05 * np.sin(p @ np.array([0.9, -0.4, 0.6]) + k)[:, None] * np.array([0.2, 1.0, -0.5]))
        V[k] = w - (w * nrm).sum(axis=1, keepdims=True) * nrm
    return V


def auto_fields(N, K):  # stream_pass_fields of csrc/mof_streamline.hip
    kp = max(1, PASS_ELEMS // N)
    if kp > STREAM_F:
        kp = kp // STREAM_F * STREAM_F
    return min(kp, K, 65535)


def cpu_baseline(N):
    import streamline_ref
    from mofhip import synth
    p, t = synth.icosphere(8, 10.0)
    n = synth.vertex_normals(p, t)
    e = np.zeros((len(p), 2, 3))
    for i, ni in enumerate(n):  # any orthonormal tangent basis serves the timing
        e1 = np.array([-ni[1], ni[0], 0.0]) if (ni[0] or ni[1]) else np.array([0.0, -ni[2], ni[1]])
        e[i][0], e[i][1] = e1 / np.linalg.norm(e1), np.cross(ni, e1) / np.linalg.norm(np.cross(ni, e1))
    V = tangent_fields(p, n, 1)
    t0 = time.perf_counter()
    nxt = streamline_ref.successor_map(p, t, e, V)
    streamline_ref.lengths(nxt, V)
    s = time.perf_counter() - t0
    scaled = s * N / len(p)
    res = {"value": round(1.0 / scaled, 4), "unit": "fields/s", "cores": 1, "kind": "port",
           "seconds_per_field_scaled": round(scaled, 2),
           "sample": "tests/streamline_ref.py on %d vertices x 1 field: %.3f s, scaled by N / %d"
                     % (len(p), s, len(p))}
    g9 = os.path.join(REPO, "tests", "golden", "G9_streamlines.npz")
    with np.load(g9, allow_pickle=False) as z:
        res["reference_seconds_per_frame_642_vertices"] = [round(float(x), 2) for x in
                                                           z["G1_ico642_ref_seconds_per_frame"]]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--walk", default=WALK, help="label of the length algorithm of the library under MOFHIP_LIB")
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()

    import torch  # first: the library then shares torch's HIP runtime
    if not torch.cuda.is_available():
        raise SystemExit("bench_streamline.py needs a GPU")
    torch.cuda.init()
    from mofhip import DeviceMesh, synth
    from mofhip.streamline import streamline_map, streamline_map_device

    p, t, n, a = synth.mesh_for_config(args.config)
    N, K = len(p), args.K
    mesh = DeviceMesh(p, n, t, a)
    info = mesh.info()
    V = tangent_fields(p, n, K)
    dev = torch.device("cuda", 0)
    Vd = torch.from_numpy(V).to(dev)
    nxt = torch.empty((K, N), dtype=torch.int32, device=dev)
    length = torch.empty((K, N), dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()

    def timed(with_length):
        def run():
            streamline_map_device(mesh, Vd.data_ptr(), K, stream=stream.cuda_stream, next_ptr=nxt.data_ptr(),
                                  length_ptr=length.data_ptr() if with_length else None)
        for _ in range(max(1, args.warmup)):  # the first call also builds the direction table
            run()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        w0 = time.perf_counter()
        ev0.record(stream)
        for _ in range(args.reps):
            run()
        ev1.record(stream)
        ev1.synchronize()
        return ev0.elapsed_time(ev1) * 1e-3 / args.reps, (time.perf_counter() - w0) / args.reps

    sec_map, wall_map = timed(False)
    sec, wall = timed(True)
    sec_walk = max(sec - sec_map, 1e-12)
    ln = length.cpu().numpy()
    hn, hl = streamline_map(mesh, V[:2])  # the device result against a host-pointer call on two fields
    same = bool(np.array_equal(nxt[:2].cpu().numpy(), hn) and np.array_equal(ln[:2], hl))
    kp = auto_fields(N, K)
    passes = -(-K // kp)
    floor = K * N * 32.0 + passes * 28.0 * info["sell_blocks"]
    res = {"row": "(f)6 streamlines (S6_streamline.py)", "config": args.config, "N": N, "K": K,
           "outputs": ["next", "length"], "fields_per_thread": STREAM_F, "fields_per_pass": kp, "passes": passes,
           "reps": args.reps, "value": round(K / sec, 1), "unit": "fields/s", "ms_per_call": round(sec * 1e3, 4),
           "ms_per_call_wall": round(wall * 1e3, 4),
           "map": {"ms_per_call": round(sec_map * 1e3, 4), "ms_per_call_wall": round(wall_map * 1e3, 4),
                   "roofline": {"bound": "hbm", "floor_bytes": floor, "achieved": round(floor / sec_map / 1e9, 1),
                                "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                "frac": round(floor / sec_map / 1e9 / HBM_PEAK_GBS, 3)}},
           "walk": {"algorithm": args.walk, "ms_per_call": round(sec_walk * 1e3, 4),
                    "line_vertices_per_s": round(float(ln.sum()) / sec_walk, 1),
                    "mean_length": round(float(ln.mean()), 2), "max_length": int(ln.max()),
                    "terminal_vertices": int((nxt.cpu().numpy() < 0).sum()), "roofline": None,
                    "note": "a pointer chase in a 4 N byte table per field: no byte floor"},
           "first_fields_identical_to_host_call": same}
    if not args.no_cpu:
        res["cpu_baseline"] = cpu_baseline(N)
        res["speedup_vs_cpu_baseline"] = round(res["value"] / res["cpu_baseline"]["value"], 1)
    mesh.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
