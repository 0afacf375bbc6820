#!/usr/bin/env python3
"""bench_modes.py -- measurement of the spatiotemporal-mode row (SURVEY.md
§8(f)8, mof_modes_gram / mof_modes_project: the reference's two
S4_spatiotemporal_decomposition_* scripts by the method of snapshots) on
MI355X.

Configuration: C3's N = 163,842 vertices with K = 1536 fields resident in HBM
(seeded: eight decaying rank-one terms plus noise), kind "complex", r = 4.
The three steps are timed apart: the Gram pass and the projection by HIP
events on the stream the library runs on, recorded around the blocking library
call -- so each span holds the call's own hipMalloc and hipFree of its
workspace (up to 256 MiB) and its final stream synchronise, not the kernels
alone: the rates below are those of the call, a lower bound of the kernels' --
the K x K eigh by the host's wall clock.

One JSON line:
  value            fields/s through the three steps (K / their summed time)
  gram             ms, FLOP/s = (K (K + 1) / 2 * 2N + K^2 N) * 2 / t and its
                   fraction of AMD's published 78.6 TFLOP/s fp64 matrix peak --
                   a data-sheet figure nobody has measured on this machine
  project          ms, GB/s against one read of V at the 8 TB/s HBM peak
  parity           checks 2-3 of tests/test_gpu_modes.py against
                   np.linalg.svd on a K = 64 slice
  s1s              the reference's own size (K = 96, N = 3,249): the three
                   steps' wall time against np.linalg.svd(full_matrices=False)
                   timed in full on the host's cores -- the one claim: the
                   three steps together beat it
  cpu_baseline     the same svd on a K = 256 slice of the fields, scaled by
                   K^2 N (sampled: the full one is minutes)

    python bench_modes.py [--K 1536] [--N 163842] [--reps 3] [--warmup 1] [--kind complex] [--no-cpu]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, "manifold-based-optical-flow-method_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
HBM_PEAK_GBS = 8000.0
F64_MATRIX_PEAK_TF = 78.6  # AMD's data sheet; not measured here


def make_fields(torch, K, N, dev, seed=0):
    """(K, 2N) f64 on the device: sum_j 0.6^j t_j x_j^T + 1e-3 noise."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    T = torch.randn((K, 8), generator=g, dtype=torch.float64, device=dev)
    T *= 0.6 ** torch.arange(8, dtype=torch.float64, device=dev)
    X = torch.randn((8, 2 * N), generator=g, dtype=torch.float64, device=dev)
    V = T @ X
    for k0 in range(0, K, 128):  # the noise in slabs: no second (K, 2N) temporary
        V[k0:k0 + 128] += 1e-3 * torch.randn((min(128, K - k0), 2 * N), generator=g, dtype=torch.float64, device=dev)
    return V


def svd_seconds(X):
    t0 = time.perf_counter()
    out = np.linalg.svd(X, full_matrices=False)
    return time.perf_counter() - t0, out


def sign_rule(U, VT):
    neg = np.mean(np.real(U), axis=0) < 0
    U[:, neg] = -U[:, neg]
    VT[neg] = -VT[neg]


def parity(torch, V, N, kind):
    """Checks 2-3 on V's first 64 rows against numpy."""
    import modes_ref as R
    from mofhip.modes import velocity_modes_device
    K = 64
    Vh = V[:K].cpu().numpy()
    X = R.complex_Y(Vh) if kind == "complex" else Vh
    _, (U0, Sg0, VT0) = svd_seconds(X)
    sign_rule(U0, VT0)
    dS = torch.empty((K, K), dtype=torch.float64, device=V.device)
    dA = torch.empty((K, K), dtype=torch.float64, device=V.device)
    from mofhip import _lib as L
    fl = (L.MOF_MODES_COMPLEX if kind == "complex" else 0) | L.MOF_IO_DEVICE
    torch.cuda.synchronize()
    L.check(L.lib().mof_modes_gram(0, ctypes.c_void_p(V.data_ptr()), K, N, fl, None, ctypes.c_void_p(dS.data_ptr()),
                                   ctypes.c_void_p(dA.data_ptr())))
    S, A = dS.cpu().numpy(), dA.cpu().numpy()
    bound = R.gram_bound(Vh)
    eS = float((np.abs(S - Vh @ Vh.T) / bound).max())
    eA = float((np.abs(A - (Vh[:, N:] @ Vh[:, :N].T - Vh[:, :N] @ Vh[:, N:].T)) / bound).max()) if kind == "complex" \
        else 0.0
    res = velocity_modes_device(V.data_ptr(), K, N, 4, kind)
    eta, g2 = R.eta(K, N), R.gap2(Sg0)[:4]
    bars, bar_v = eta * Sg0[0] ** 2 / Sg0, 4 * eta * Sg0[0] / g2
    dSg = np.abs(res["Sigma"] - Sg0)
    d_sr = np.abs(res["sigma_r"] - Sg0[:4])
    r1 = R.rank_one_errors(kind, res["U"], res["Y"], U0, Sg0, VT0)
    ok = bool(eS <= 1 and eA <= 1 and np.array_equal(S, S.T) and (kind != "complex" or np.array_equal(A, -A.T))
              and (dSg <= bars).all() and (d_sr <= bar_v).all() and (r1 <= bar_v).all())
    return {"K": K, "ok": ok, "gram_S_err_over_bound": eS, "gram_A_err_over_bound": eA,
            "Sigma_err_over_bar": float((dSg / bars).max()), "sigma_r_rel_err": float((d_sr / Sg0[:4]).max()),
            "rank_one_err_over_sigma1": float((r1 / Sg0[0]).max()), "rank_one_bar_over_sigma1": float((bar_v / Sg0[0]).max()),
            "gap2_min": float(g2.min())}


def s1s(torch, dev, kind, no_cpu):
    """K = 96, N = 3,249: the three steps' wall time against the full svd."""
    import modes_ref as R
    from mofhip.modes import velocity_modes_device
    K, N = 96, 3249
    V = make_fields(torch, K, N, dev, seed=1)
    torch.cuda.synchronize()
    velocity_modes_device(V.data_ptr(), K, N, 4, kind)
    best = None
    for _ in range(5):
        tm = {}
        velocity_modes_device(V.data_ptr(), K, N, 4, kind, timings=tm)
        if best is None or sum(tm.values()) < sum(best.values()):
            best = tm
    out = {"K": K, "N": N, "ms_gram": round(best["ms_gram"], 3), "ms_eigh": round(best["ms_eigh"], 3),
           "ms_project": round(best["ms_project"], 3), "ms_three_steps": round(sum(best.values()), 3)}
    if not no_cpu:
        Vh = V.cpu().numpy()
        X = R.complex_Y(Vh) if kind == "complex" else Vh
        svd_seconds(X)
        secs = min(svd_seconds(X)[0] for _ in range(3))
        out["ms_numpy_svd"] = round(secs * 1e3, 3)
        out["three_steps_beat_svd"] = bool(out["ms_three_steps"] < out["ms_numpy_svd"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=1536)
    ap.add_argument("--N", type=int, default=163842)
    ap.add_argument("--r", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kind", default="complex", choices=("complex", "concat"))
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()

    import torch  # first: the library then shares torch's HIP runtime
    if not torch.cuda.is_available():
        raise SystemExit("bench_modes.py needs a GPU")
    torch.cuda.init()
    import modes_ref as R
    from mofhip import _lib as L
    from mofhip.modes import gram_eig

    K, N, r, kind = args.K, args.N, args.r, args.kind
    cplx = kind == "complex"
    dev = torch.device("cuda", 0)
    V = make_fields(torch, K, N, dev)
    f64 = dict(dtype=torch.float64, device=dev)
    dS, dA = torch.empty((K, K), **f64), torch.empty((K, K), **f64)
    dY, dsig = torch.empty((r, 2 * N), **f64), torch.empty(r, **f64)
    stream = torch.cuda.Stream(device=dev)
    fl = (L.MOF_MODES_COMPLEX if cplx else 0) | L.MOF_IO_DEVICE
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    torch.cuda.synchronize()

    def gram():
        L.check(L.lib().mof_modes_gram(0, p(V), K, N, fl, stream.cuda_stream, p(dS), p(dA) if cplx else None))

    def project(dP, dQ):
        L.check(L.lib().mof_modes_project(0, p(V), K, N, p(dP), p(dQ) if cplx else None, r, fl, stream.cuda_stream,
                                          p(dY), p(dsig)))

    def timed(fn, *a):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        best = None
        for i in range(args.warmup + args.reps):
            ev0.record(stream)
            fn(*a)
            ev1.record(stream)
            ev1.synchronize()
            if i >= args.warmup:
                ms = ev0.elapsed_time(ev1)
                best = ms if best is None else min(best, ms)
        return best

    ms_gram = timed(gram)
    S = dS.cpu().numpy()
    A = dA.cpu().numpy() if cplx else None
    t0 = time.perf_counter()
    Sigma, W = gram_eig(S, A)
    ms_eigh = (time.perf_counter() - t0) * 1e3
    U = W[:, :r]
    dP = torch.from_numpy(np.ascontiguousarray(U.real)).to(dev)
    dQ = torch.from_numpy(np.ascontiguousarray(U.imag)).to(dev)
    torch.cuda.synchronize()
    ms_proj = timed(project, dP, dQ)
    sig = dsig.cpu().numpy()

    flop = (K * (K + 1) / 2 * 2 * N + (K * K * N if cplx else 0)) * 2.0
    tf = flop / (ms_gram * 1e-3) / 1e12
    vbytes = K * 2.0 * N * 8
    gbs = vbytes / (ms_proj * 1e-3) / 1e9
    total = (ms_gram + ms_eigh + ms_proj) * 1e-3
    res = {"row": "(f)8 spatiotemporal modes (S4_spatiotemporal_decomposition_*)", "config": "C3", "N": N, "K": K,
           "kind": kind, "r": r, "reps": args.reps, "value": round(K / total, 1), "unit": "fields/s",
           "ms_total": round(total * 1e3, 3),
           "gram": {"ms": round(ms_gram, 3), "flop": flop, "tflops": round(tf, 2), "peak_tflops": F64_MATRIX_PEAK_TF,
                    "frac": round(tf / F64_MATRIX_PEAK_TF, 3),
                    "peak_note": "AMD's published fp64 matrix peak; not measured on this machine"},
           "eigh": {"ms_host_wall": round(ms_eigh, 3)},
           "project": {"ms": round(ms_proj, 3), "bytes": vbytes, "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS,
                       "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 3)},
           "timed_span": "each device step is the whole library call between HIP events: its workspace hipMalloc / "
                         "hipFree and final stream synchronise are inside, so the rates are lower bounds of the kernels'",
           "sigma_r_over_Sigma_max_rel": float(np.abs(sig / Sigma[:r] - 1).max()),
           "parity": parity(torch, V, N, kind),
           "s1s": s1s(torch, dev, kind, args.no_cpu)}
    if not args.no_cpu:
        Ks = min(256, K)
        Vh = V[:Ks].cpu().numpy()
        secs, _ = svd_seconds(R.complex_Y(Vh) if cplx else Vh)
        scaled = secs * (K / Ks) ** 2
        res["cpu_baseline"] = {"value": round(K / scaled, 2), "unit": "fields/s", "kind": "sampled",
                               "cores": min(os.cpu_count() or 1, int(os.environ.get("OMP_NUM_THREADS", "16"))),
                               "seconds_scaled": round(scaled, 1),
                               "sample": "np.linalg.svd(full_matrices=False) on a K = %d slice: %.2f s, scaled by "
                                         "K^2 N" % (Ks, secs)}
        res["speedup_vs_cpu_baseline"] = round(res["value"] / res["cpu_baseline"]["value"], 1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
