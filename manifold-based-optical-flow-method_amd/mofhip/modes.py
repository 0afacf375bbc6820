"""The spatiotemporal modes of the velocity fields: the reference's two
``S4_spatiotemporal_decomposition_*`` scripts.

Both scripts take ``np.linalg.svd`` of the K fields -- of the complex
``K x N`` matrix ``X = V1 + i V2`` (ComplexMatrices) or of the real ``K x 2N``
matrix ``[V1 | V2]`` (ConcatMatrices) -- keep the first four modes, flip signs
by ``mean(real(U), axis=0) < 0``, print ``calculate_percentages(Sigma)`` and
turn ``sigma * vt`` into 3-D vectors. With ``K << N`` this is the method of
snapshots, two N-long device passes around one small eigenproblem:

1. ``mof_modes_gram``: ``S = V V^T`` (and ``A = V2 V1^T - V1 V2^T``), the Gram
   matrix ``X X^H = S + i A`` or ``S``, on the fp64 matrix cores;
2. ``numpy.linalg.eigh`` of it on the host, ``O(K^3)``: ``U`` and
   ``Sigma = sqrt(max(lambda, 0))``, descending;
3. ``mof_modes_project``: ``Y = U[:, :r]^H X`` in V's planar layout, one read
   of V, with the row norms ``sigma_r``. ``Y_j`` is the scripts'
   ``sigma * vt`` and ``VT[j] = Y_j / sigma_r[j]``.

The 3-D mode vectors are ``mof_velocity_vectors`` of ``Y``. Nothing ``N x N``
is ever formed (the scripts' ``full_matrices=1`` asks for one).

Accuracy: the Gram matrix carries an error of ``eta |G|``, ``eta = 4 K N u``,
so ``|Sigma_j - sigma_j| <= eta sigma_1^2 / sigma_j``: modes below about
``1e-6 sigma_1`` are not resolved.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib as L
from .epilogue import velocity_vectors, velocity_vectors_device

KINDS = ("complex", "concat")


# ---- the scripts' helpers, vectorised, bit-identical ---------------------
def process_V_k_to_complex(V_k):
    """``(K, N)`` complex: ``complex(V[k][i], V[k][i + N])``."""
    V = np.asarray(V_k, dtype=np.float64)
    n = V.shape[1] // 2
    out = np.empty((V.shape[0], n), dtype=complex)
    out.real = V[:, :n]
    out.imag = V[:, n:2 * n]
    return out


def calculate_V_k_from_complex(V_k_coord_complex, e):
    """``v.real * e[i][0] + v.imag * e[i][1]`` per vertex: ``(N, 3)`` (the
    scripts return the same rows as a list)."""
    v = np.asarray(V_k_coord_complex)
    e = np.asarray(e)
    return v.real[:, None] * e[:, 0] + v.imag[:, None] * e[:, 1]


def calculate_percentages(Sigma):
    """``(percentages, percentages_squared)``: each singular value's share of
    their sum, and each square's share of the sum of squares, in per cent
    rounded to two decimals."""
    sv = np.asarray(Sigma)
    sq = sv * sv
    return np.round(sv / sv.sum() * 100, 2), np.round(sq / sq.sum() * 100, 2)


# ---- the C calls ---------------------------------------------------------
def _flags(kind):
    if kind not in KINDS:
        raise ValueError("kind must be 'complex' or 'concat'")
    return L.MOF_MODES_COMPLEX if kind == "complex" else 0


def _planar(V_k):
    V = np.ascontiguousarray(np.asarray(V_k, dtype=np.float64))
    if V.ndim != 2 or V.shape[0] < 1 or V.shape[1] < 2 or V.shape[1] % 2:
        raise ValueError("need V_k (K, 2N) with K >= 1 and N >= 1")
    return V


def modes_gram(V_k, kind="complex", device: int = 0):
    """``(S, A)`` of V_k (K, 2N): ``S = V V^T``, ``A = V2 V1^T - V1 V2^T``
    (None for ``kind="concat"``)."""
    fl = _flags(kind)
    V = _planar(V_k)
    K, N = V.shape[0], V.shape[1] // 2
    S = np.empty((K, K))
    A = np.empty((K, K)) if fl else None
    L.check(L.lib().mof_modes_gram(int(device), L.ptr(V), K, N, fl, None, L.ptr(S), L.ptr(A) if fl else None))
    return S, A


def modes_project(V_k, W, kind="complex", device: int = 0):
    """``(Y (r, 2N), sigma_r (r,))``: ``Y = W^H X`` in planar form for the
    columns of W (K, r) -- complex for ``kind="complex"``, real for concat."""
    fl = _flags(kind)
    V = _planar(V_k)
    K, N = V.shape[0], V.shape[1] // 2
    W = np.asarray(W)
    if W.ndim != 2 or W.shape[0] != K or not 1 <= W.shape[1] <= K:
        raise ValueError("need W (K, r) with 1 <= r <= K")
    r = W.shape[1]
    P = np.ascontiguousarray(W.real, dtype=np.float64)
    Q = np.ascontiguousarray(W.imag, dtype=np.float64) if fl else None
    Y = np.empty((r, 2 * N))
    sig = np.empty(r)
    L.check(L.lib().mof_modes_project(int(device), L.ptr(V), K, N, L.ptr(P), L.ptr(Q) if fl else None, r, fl, None,
                                      L.ptr(Y), L.ptr(sig)))
    return Y, sig


# ---- the eigen step and the scripts' conventions -------------------------
def _check_frames(S):
    bad = np.flatnonzero(~np.isfinite(np.diagonal(S)))
    if bad.size:
        raise ValueError("V_k holds non-finite values (a solve that did not converge?) in frame(s) %s"
                         % ", ".join(str(int(k)) for k in bad))


def gram_eig(S, A=None):
    """``(Sigma (K,), W (K, K))`` of the Gram matrix ``S + i A`` (or ``S``):
    eigenvalues descending, ``Sigma = sqrt(max(lambda, 0))``."""
    _check_frames(S)
    lam, W = np.linalg.eigh(S + 1j * A if A is not None else S)
    order = np.argsort(lam)[::-1]
    return np.sqrt(np.maximum(lam[order], 0.0)), np.ascontiguousarray(W[:, order])


def _finish(kind, N, Sigma, U, Y, sigma_r):
    """The sign rule on U, VT and Y together; VT; the percentages."""
    neg = np.mean(np.real(U), axis=0) < 0
    U = U.copy()
    U[:, neg] = -U[:, neg]
    Y[neg, :] = -Y[neg, :]
    # a mode of norm 0 (V_k of rank below nmodes) has no direction: its VT row is 0
    VT = np.divide(Y, sigma_r[:, None], out=np.zeros_like(Y), where=sigma_r[:, None] > 0)
    if kind == "complex":
        VT = process_V_k_to_complex(VT)
    pct, pct2 = calculate_percentages(Sigma)
    return {"U": U, "Sigma": Sigma, "sigma_r": sigma_r, "VT": VT, "Y": Y, "percentages": pct,
            "percentages_squared": pct2}


def _nmodes(nmodes, K):
    r = int(nmodes)
    if not 1 <= r <= K:
        raise ValueError("nmodes must lie in 1 .. K = %d" % K)
    return r


def velocity_modes(V_k, nmodes=4, kind="complex", device: int = 0):
    """The leading ``r = nmodes`` modes of V_k (K, 2N) as a dict:
    ``U (K, r)``, ``Sigma (K,)`` (all of them: the percentages need them),
    ``sigma_r (r,)`` (the row norms of Y: Sigma[:r] to rounding), ``VT`` --
    ``(r, N)`` complex or ``(r, 2N)`` real --, ``Y (r, 2N)`` (planar
    ``sigma * vt``), ``percentages`` and ``percentages_squared`` (K,). The
    scripts' sign rule is applied to U, VT and Y together. A frame with a
    non-finite value raises ValueError naming the frames. Where V_k has rank
    below nmodes (duplicated or all-zero frames) a mode with ``sigma_r == 0``
    gets a zero VT row -- the svd returns an arbitrary unit vector there."""
    _flags(kind)
    V = _planar(V_k)
    K, N = V.shape[0], V.shape[1] // 2
    r = _nmodes(nmodes, K)
    S, A = modes_gram(V, kind, device)
    Sigma, W = gram_eig(S, A)
    U = W[:, :r]
    Y, sigma_r = modes_project(V, U, kind, device)
    return _finish(kind, N, Sigma, U, Y, sigma_r)


def spatiotemporal_modes(V_k, e, nmodes=4, kind="complex", device: int = 0):
    """:func:`velocity_modes` plus ``mode_vectors (r, N, 3)``: the scripts'
    ``calculate_V_k_from_complex(sigma * vt, e)`` for each mode, by
    ``mof_velocity_vectors`` of Y."""
    res = velocity_modes(V_k, nmodes, kind, device)
    res["mode_vectors"], _ = velocity_vectors(res["Y"], e, device=device, want_speed=False)
    return res


def velocity_modes_device(V_ptr: int, K: int, N: int, nmodes=4, kind="complex", device: int = 0, stream=None,
                          e_ptr: int | None = None, timings: dict | None = None):
    """:func:`velocity_modes` for fields still in HBM: V (K, 2N) f64 at the
    device pointer ``V_ptr`` on ``device`` (``mof_solve_range``'s V_out with
    MOF_IO_DEVICE). Only the K x K matrices and the results cross to the host.
    With ``e_ptr`` (e (N, 2, 3) f64 in HBM) the dict also holds
    ``mode_vectors``. ``timings`` (a dict) receives the wall milliseconds of
    the three steps (each call returns when its work is done)."""
    import time

    import torch
    fl = _flags(kind)
    K, N = int(K), int(N)
    if not V_ptr or K < 1 or N < 1:
        raise ValueError("velocity_modes_device needs V, K >= 1 and N >= 1")
    r = _nmodes(nmodes, K)
    dev = torch.device("cuda", int(device))
    dptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    f64 = dict(dtype=torch.float64, device=dev)
    V_ptr = ctypes.c_void_p(V_ptr)
    t0 = time.perf_counter()
    dS = torch.empty((K, K), **f64)
    dA = torch.empty((K, K), **f64) if fl else None
    torch.cuda.synchronize(dev)
    L.check(L.lib().mof_modes_gram(int(device), V_ptr, K, N, fl | L.MOF_IO_DEVICE, stream, dptr(dS),
                                   dptr(dA) if fl else None))
    S = dS.cpu().numpy()
    A = dA.cpu().numpy() if fl else None
    t1 = time.perf_counter()
    Sigma, W = gram_eig(S, A)
    U = W[:, :r]
    t2 = time.perf_counter()
    dP = torch.from_numpy(np.ascontiguousarray(U.real)).to(dev)
    dQ = torch.from_numpy(np.ascontiguousarray(U.imag)).to(dev) if fl else None
    dY = torch.empty((r, 2 * N), **f64)
    dsig = torch.empty(r, **f64)
    torch.cuda.synchronize(dev)
    L.check(L.lib().mof_modes_project(int(device), V_ptr, K, N, dptr(dP), dptr(dQ) if fl else None, r,
                                      fl | L.MOF_IO_DEVICE, stream, dptr(dY), dptr(dsig)))
    t3 = time.perf_counter()
    res = _finish(kind, N, Sigma, U, dY.cpu().numpy(), dsig.cpu().numpy())
    if e_ptr:
        Yd = torch.from_numpy(res["Y"]).to(dev)  # after the sign rule
        dc = torch.empty((r, N, 3), **f64)
        torch.cuda.synchronize(dev)
        velocity_vectors_device(ctypes.c_void_p(e_ptr), dptr(Yd), N, r, dptr(dc), None, device=device, stream=stream)
        res["mode_vectors"] = dc.cpu().numpy()
    if timings is not None:
        timings.update(ms_gram=(t1 - t0) * 1e3, ms_eigh=(t2 - t1) * 1e3, ms_project=(t3 - t2) * 1e3)
    return res
