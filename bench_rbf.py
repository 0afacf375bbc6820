#!/usr/bin/env python3
"""bench_rbf.py -- measurement of the electrode-interpolation row (SURVEY.md
§8(f)9, mof_rbf_eval: the reference's S2_interpolate.py and
S2_interpolate_phases.py) on MI355X.

Configurations: C3's N = 163,842 and S1's N = 160,801 vertices, E = 62 and 126
electrodes (a jittered 8 x 8 / 8 x 16 grid on the radius-70 sphere without its
stimulated pair, the vertices on the same sphere over the grid), T = 1536
frames of weights resident in HBM, real data; for C3 / 62 also the phase
script's complex data to the angle. Each is the whole library call between HIP
events on the stream the library runs on -- so the span holds the call's own
hipMalloc / hipFree of the padded weights and its final stream synchronise,
not the kernels alone: the rates are those of the call, a lower bound of the
kernel's. No target rate is fixed in advance.

One JSON line:
  value            frames/s of the first configuration (C3, E = 62)
  configs[]        ms (the best of the timed calls; the worst beside it),
                   frames/s, FLOP/s = 2 T N E / t (x 2 for the two planes of
                   the angle) and its fraction of AMD's published
                   78.6 TFLOP/s fp64 matrix peak -- a data-sheet figure nobody
                   has measured on this machine --, output GB/s against the
                   8 TB/s HBM peak
  parity           check 2 of tests/test_gpu_interp.py (against a
                   np.longdouble sum, (E + 1) u S) on a slice of the first
                   configuration's output, and check 4 (interpolation(...) on
                   the golden's raw inputs against the reference's fields)
  s1s              the reference's own size (N = 3,249, 97 frames, E = 62):
                   interpolation(...) from host arrays, wall clock, against
                   scipy's per-frame Rbf loop timed in full -- the one claim:
                   the call beats it
  cpu_baseline     the same loop on a few frames at the large N, scaled by
                   the frame count (sampled)

    python bench_rbf.py [--T 1536] [--reps 10] [--warmup 1] [--no-cpu]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, "manifold-based-optical-flow-method_amd"))
HBM_PEAK_GBS = 8000.0
F64_MATRIX_PEAK_TF = 78.6  # AMD's data sheet; not measured here
U = 2.0 ** -53
SIZES = (("C3", 163842), ("S1", 160801))


def electrodes(n_cols, seed=0, spacing=10.0, jitter=0.15, radius=70.0):
    """An 8 x n_cols jittered grid on the sphere without two neighbouring
    electrodes (the stimulated pair): 62 for 8, 126 for 16."""
    rng = np.random.default_rng(seed)
    gx = (np.arange(8) - 3.5) * spacing
    gy = (np.arange(n_cols) - 0.5 * (n_cols - 1)) * spacing * (1.0 if n_cols == 8 else 0.5)
    x, y = np.meshgrid(gx, gy, indexing="ij")
    xy = np.stack([x.ravel(), y.ravel()], axis=1)
    xy += jitter * spacing * rng.uniform(-1.0, 1.0, size=xy.shape)
    z = np.sqrt(radius ** 2 - (xy ** 2).sum(axis=1)) - radius
    return np.delete(np.column_stack([xy, z]), (27, 28), axis=0)


def vertices(N, seed=1, half=40.0, radius=70.0):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-half, half, size=(N, 2))
    return np.column_stack([xy, np.sqrt(radius ** 2 - (xy ** 2).sum(axis=1)) - radius])


def frames(xi, T, complex_=False):
    t = np.arange(T)[:, None]
    s = np.sin(0.05 * xi[:, 0] + 0.03 * xi[:, 1] - 0.3 * t)
    return np.exp(1j * 2.0 * np.arcsin(s)) if complex_ else 1e-4 * s


def scipy_loop(pts, data, xi):
    """The scripts' loop, statement by statement; seconds and the array."""
    from scipy.interpolate import Rbf
    t0 = time.perf_counter()
    out = []
    for frame in data:
        rbf = Rbf(xi[:, 0], xi[:, 1], xi[:, 2], frame)
        out.append(rbf(pts[:, 0], pts[:, 1], pts[:, 2]))
    return time.perf_counter() - t0, np.array(out)


def parity_slice(interp, pts, xi, eps, W, out_rows, rows, cols):
    """Check 2 on out[rows][:, cols] of a timed configuration."""
    E = len(xi)
    phi = interp.rbf_phi(pts[cols], xi, eps)
    Ws = W[rows]
    exact = Ws.astype(np.longdouble) @ phi.astype(np.longdouble).T
    S = np.abs(Ws) @ phi.T
    e = (np.abs(out_rows[:, cols] - exact) / ((E + 1) * U * S)).astype(np.float64).max()
    return {"frames": len(rows), "vertices": len(cols), "err_over_bar": float(e), "bar": "(E + 1) u S",
            "ok": bool(e <= 1)}


def parity_golden(interp):
    """Check 4 on the golden's raw real frames."""
    with np.load(os.path.join(REPO, "tests", "golden", "G12_rbf.npz"), allow_pickle=False) as z:
        g = {k: z[k] for k in z.files}
    pts, xi = g["points"], g["electrodes"]
    E = len(xi)
    a, b = int(g["real_start"]), int(g["real_stop"])
    out = interp.interpolation(pts, g["real_data"], xi, a, b)
    W = interp.rbf_weights(xi, g["real_data"][a:b])
    phi = interp.rbf_phi(pts, xi, interp.rbf_epsilon(xi))
    chain = (phi @ W.T).T
    ref = g["real_field"]
    bar = np.abs(chain - ref) + 2 * (E + 1) * U * (np.abs(W) @ phi.T)
    e = np.abs(out - ref)
    return {"err_over_max_ref": float(e.max() / np.abs(ref).max()), "err_over_bar": float((e / bar).max()),
            "bar": "|numpy chain - ref| + 2 (E + 1) u S", "ok": bool((e <= bar).all())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=1536)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()

    import torch  # first: the library then shares torch's HIP runtime
    if not torch.cuda.is_available():
        raise SystemExit("bench_rbf.py needs a GPU")
    torch.cuda.init()
    from mofhip import interp

    T = args.T
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)  # noqa: E731

    def timed(fn):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for i in range(args.warmup + args.reps):
            ev0.record(stream)
            fn()
            ev1.record(stream)
            ev1.synchronize()
            if i >= args.warmup:
                ms.append(ev0.elapsed_time(ev1))
        return min(ms), max(ms)

    configs, parity, first = [], {}, None
    runs = [(name, N, nc, False) for name, N in SIZES for nc in (8, 16)] + [("C3", SIZES[0][1], 8, True)]
    for name, N, n_cols, phase in runs:
        xi, pts = electrodes(n_cols), vertices(N)
        E = len(xi)
        eps = float(interp.rbf_epsilon(xi))
        W = interp.rbf_weights(xi, frames(xi, T, phase))
        dp, dx, dwr = up(pts), up(xi), up(W.real)
        dwi = up(W.imag) if phase else None
        dout = torch.empty((T, N), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        def call():
            interp.rbf_eval_device(dp.data_ptr(), N, dx.data_ptr(), E, eps, dwr.data_ptr(), T, dout.data_ptr(),
                                   W_im_ptr=dwi.data_ptr() if phase else None, angle=phase,
                                   stream=stream.cuda_stream)

        ms, ms_worst = timed(call)
        flop = 2.0 * T * N * E * (2 if phase else 1)
        tf = flop / (ms * 1e-3) / 1e12
        gbs = T * N * 8.0 / (ms * 1e-3) / 1e9
        configs.append({"config": name, "N": N, "E": E, "T": T, "data": "complex to angle" if phase else "real",
                        "ms": round(ms, 3), "ms_worst_of_reps": round(ms_worst, 3), "frames_per_s": round(T / (ms * 1e-3), 1), "flop": flop,
                        "tflops": round(tf, 2), "frac_of_peak_tflops": round(tf / F64_MATRIX_PEAK_TF, 3),
                        "out_gbs": round(gbs, 1), "frac_of_peak_gbs": round(gbs / HBM_PEAK_GBS, 3)})
        if first is None:
            first = configs[-1]
            rows, cols = np.arange(0, T, max(1, T // 24)), np.arange(0, N, 41)
            parity["check2_slice"] = parity_slice(interp, pts, xi, eps, W, dout[torch.from_numpy(rows).to(dev)]
                                                  .cpu().numpy(), rows, cols)
        del dout, dp, dx, dwr, dwi
    parity["check4_golden"] = parity_golden(interp)

    # the reference's own size, from host arrays, against the scripts' loop in full
    xi, pts = electrodes(8), vertices(3249, seed=2)
    data = frames(xi, 97)
    interp.interpolation(pts, data, xi, 0, 97)
    wall = []
    for _ in range(5):
        t0 = time.perf_counter()
        out = interp.interpolation(pts, data, xi, 0, 97)
        wall.append(time.perf_counter() - t0)
    s1s = {"N": 3249, "frames": 97, "E": len(xi), "ms_interpolation": round(min(wall) * 1e3, 3)}
    res = {"row": "(f)9 electrode interpolation (S2_interpolate*)", "value": first["frames_per_s"],
           "unit": "frames/s", "config": "C3, E = 62, T = %d, real data" % T, "reps": args.reps,
           "peak_tflops": F64_MATRIX_PEAK_TF, "peak_gbs": HBM_PEAK_GBS,
           "peak_note": "AMD's published fp64 matrix and HBM peaks; neither measured on this machine",
           "timed_span": "the whole library call between HIP events: its workspace hipMalloc / hipFree and final "
                         "stream synchronise are inside, so the rates are lower bounds of the kernel's",
           "configs": configs, "parity": parity}
    if not args.no_cpu:
        secs, ref = scipy_loop(pts, data, xi)
        s1s.update(ms_scipy_loop=round(secs * 1e3, 3), ms_scipy_per_frame=round(secs * 1e3 / 97, 3),
                   call_beats_scipy_loop=bool(min(wall) < secs),
                   max_abs_diff_over_max_ref=float(np.abs(out - ref).max() / np.abs(ref).max()))
        name, N = SIZES[0]
        big, ns = vertices(N), 3
        secs, _ = scipy_loop(big, frames(xi, ns), xi)
        res["cpu_baseline"] = {"value": round(ns / secs, 2), "unit": "frames/s", "kind": "sampled",
                               "cores": min(os.cpu_count() or 1, int(os.environ.get("OMP_NUM_THREADS", "16"))),
                               "sample": "scipy's per-frame Rbf loop on %d frames at N = %d, E = %d: %.3f s per frame"
                                         % (ns, N, len(xi), secs / ns)}
        res["speedup_vs_cpu_baseline"] = round(res["value"] / res["cpu_baseline"]["value"], 1)
    res["s1s"] = s1s
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
