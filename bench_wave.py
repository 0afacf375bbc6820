#!/usr/bin/env python3
"""bench_wave.py -- measurement of the wave-speed row (SURVEY.md §8(f)5,
mof_wave_speed: S5_compute_wave_v.py on a mesh handle) on MI355X.

Configuration: the C3 mesh (163,842 vertices), T = 256 frames of a wrapped
travelling phase resident in HBM, phase mode, the speed as the only output.
Warm-up calls, then timed repetitions bracketed by HIP events on the stream
the library runs on (every call ends in a stream synchronise, so the events
also see the host's launch gaps between passes; the wall clock is printed
beside them).

One JSON line:
  value            frames/s (T * reps / event time)
  roofline         achieved GB/s and its fraction of the HBM peak against the
                   floor bytes T N (8 read + 8 written) plus one read of the
                   coefficient table (16 B per SELL position) per pass
  cpu_baseline     tests/wave_ref.py -- the reference's loops restated in
                   numpy, frames vectorised, so a lower bound of the
                   reference's own time -- timed on a 642-vertex icosphere
                   with 6 frames and scaled by (T N) / (6 * 642): the
                   reference's cost is its two nests, triangles x frames and
                   vertices x frames, both proportional to T N on one mesh
                   family

    python bench_wave.py [--T 256] [--reps 20] [--warmup 3] [--frames-per-pass 0] [--config C3]
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
WAVE_F = 4                  # frames per thread of the hot kernel (csrc/mof_wave.hip kWaveF)
PASS_ELEMS = 11 << 20       # its automatic pass size in (frame, vertex) values (kWavePassElems)


def wrapped_phase(p, T):
    theta = p @ np.array([0.31, -0.23, 0.17]) + 0.9
    return np.mod(theta[None, :] - 0.7 * np.arange(T)[:, None] + np.pi, 2 * np.pi) - np.pi


def auto_frames(N, T):  # wave_auto_frames of csrc/mof_wave.hip
    fpp, grp = PASS_ELEMS // N, 8 * WAVE_F
    fpp = fpp // grp * grp if fpp >= grp else max(WAVE_F, fpp // WAVE_F * WAVE_F)
    return min(fpp, T)


def cpu_baseline(T, N):
    import wave_ref
    from mofhip import synth
    p, t = synth.icosphere(8, 10.0)
    n, a = synth.vertex_normals(p, t), synth.triangle_areas(p, t)
    e = np.zeros((len(p), 2, 3))
    for i, ni in enumerate(n):  # any orthonormal tangent basis serves the timing
        e1 = np.array([-ni[1], ni[0], 0.0]) if (ni[0] or ni[1]) else np.array([0.0, -ni[2], ni[1]])
        e[i][0], e[i][1] = e1 / np.linalg.norm(e1), np.cross(ni, e1) / np.linalg.norm(np.cross(ni, e1))
    X = wrapped_phase(p, 6)
    t0 = time.perf_counter()
    wave_ref.wave_speed(p, t, a, e, X, 1.0 / 512)
    s = time.perf_counter() - t0
    scaled = s * (T * N) / (6.0 * len(p))
    return {"value": round(T / scaled, 4), "unit": "frames/s", "cores": 1, "kind": "port",
            "seconds_scaled": round(scaled, 1),
            "sample": "tests/wave_ref.py (the reference's loops, frames vectorised) on %d vertices x 6 frames: "
                      "%.3f s, scaled by T N / (6 * %d)" % (len(p), s, len(p))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames-per-pass", type=int, default=0)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--mode", default="phase", choices=("phase", "amp"))
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()

    import torch  # first: the library then shares torch's HIP runtime
    if not torch.cuda.is_available():
        raise SystemExit("bench_wave.py needs a GPU")
    torch.cuda.init()
    from mofhip import DeviceMesh, synth
    from mofhip.wave import wave_speed, wave_speed_device

    p, t, n, a = synth.mesh_for_config(args.config)
    N, T = len(p), args.T
    mesh = DeviceMesh(p, n, t, a)
    info = mesh.info()
    X = wrapped_phase(p, T)
    if args.mode == "amp":
        X = np.cos(X)
    dev = torch.device("cuda", 0)
    Xd = torch.from_numpy(X).to(dev)
    out = torch.empty((T, N), dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    phase = args.mode == "phase"

    def run():
        wave_speed_device(mesh, Xd.data_ptr(), T, 1.0 / 512, phase=phase, frames_per_pass=args.frames_per_pass,
                          stream=stream.cuda_stream, speed_ptr=out.data_ptr())

    for _ in range(max(1, args.warmup)):  # the first call also builds the coefficient table
        run()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    w0 = time.perf_counter()
    ev0.record(stream)
    for _ in range(args.reps):
        run()
    ev1.record(stream)
    ev1.synchronize()
    wall = (time.perf_counter() - w0) / args.reps
    sec = ev0.elapsed_time(ev1) * 1e-3 / args.reps

    # the device result against a host-pointer call on the first frames (of a
    # shorter sequence: its frames before the last are the long one's)
    k = min(T - 1, 4)
    same = bool(np.array_equal(out[:k].cpu().numpy(), wave_speed(mesh, X[:k + 2], 1.0 / 512, phase=phase)[:k],
                               equal_nan=True))
    fpp = args.frames_per_pass or auto_frames(N, T)
    passes = -(-T // fpp)
    floor = T * N * 16.0 + passes * 16.0 * info["sell_blocks"]
    res = {"row": "(f)5 wave speed (S5_compute_wave_v.py)", "config": args.config, "N": N, "T": T,
           "mode": args.mode, "outputs": ["speed"], "frames_per_thread": WAVE_F, "frames_per_pass": fpp,
           "passes": passes, "reps": args.reps,
           "value": round(T / sec, 1), "unit": "frames/s", "ms_per_call": round(sec * 1e3, 4),
           "ms_per_call_wall": round(wall * 1e3, 4),
           "roofline": {"bound": "hbm", "floor_bytes": floor, "achieved": round(floor / sec / 1e9, 1),
                        "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(floor / sec / 1e9 / HBM_PEAK_GBS, 3)},
           "first_frames_bit_identical_to_host_call": same}
    if not args.no_cpu:
        res["cpu_baseline"] = cpu_baseline(T, N)
        res["speedup_vs_cpu_baseline"] = round(res["value"] / res["cpu_baseline"]["value"], 1)
    mesh.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
