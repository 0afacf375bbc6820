"""numpy restatement of the spatiotemporal-mode passes (mofhip/modes.py,
csrc/mof_modes.hip), for the tests: the Gram matrix in column chunks, the
eigen step, the projection and the scripts' conventions -- and the error bars
the tests hold the device path to.

Bars (u = 2^-53, eta = 4 K N u). Two differently ordered sums of the same 2N
products differ by at most 2 (2N) u sum|products| (each is within (2N) u of
the exact sum, to first order). Against the reference's SVD the computed Gram
matrix is G + E with |E| <= eta |G| in norm (2N-term sums, K entries per row;
the factor 4 covers numpy's own eigh backward error, a few K u |G|), hence
  Weyl:          |lambda_j - ref| <= eta sigma_1^2, i.e.
                 |Sigma_j - sigma_j| <= eta sigma_1^2 / sigma_j
                 (sqrt is 1 / (2 sigma_j)-Lipschitz there; where the bar
                 exceeds sigma_j the value is unresolved and the bar says so);
  Davis-Kahan:   |u_j - ref| <= 2 |E| / gap(lambda) = 2 eta / gap2_j in units
                 of sigma_1^2, gap2_j = min_{i != j} |lambda_j - lambda_i| /
                 lambda_1; the tests use 4 eta / gap2_j for the vectors and
                 4 eta sigma_1 / gap2_j for sigma_r and the rank-one terms
                 U_j Y_j (a projector: invariant to the unit phase LAPACK
                 leaves on a complex vector).
"""
from __future__ import annotations

import numpy as np

U_ROUND = 2.0 ** -53
CHUNK = 2048  # csrc/mof_modes.hip kModesChunk


def split(V):
    V = np.asarray(V, dtype=np.float64)
    N = V.shape[1] // 2
    return V[:, :N], V[:, N:]


def gram(V, kind="complex", chunk=CHUNK):
    """(S, A): per chunk of N columns the products of both halves, chunks
    added in ascending order; A is None for concat."""
    V1, V2 = split(V)
    K, N = V1.shape
    S = np.zeros((K, K))
    A = np.zeros((K, K)) if kind == "complex" else None
    for c in range(0, N, chunk):
        a, b = V1[:, c:c + chunk], V2[:, c:c + chunk]
        S += a @ a.T + b @ b.T
        if A is not None:
            A += b @ a.T - a @ b.T
    S = np.triu(S) + np.triu(S, 1).T
    if A is not None:
        A = np.triu(A, 1) - np.triu(A, 1).T
    return S, A


def gram_bound(V):
    """Elementwise bar of the Gram matrices: 2 (2N) u (|V| |V|^T)."""
    a = np.abs(np.asarray(V, dtype=np.float64))
    return 2 * a.shape[1] * U_ROUND * (a @ a.T)


def eig(S, A=None):
    lam, W = np.linalg.eigh(S + 1j * A if A is not None else S)
    order = np.argsort(lam)[::-1]
    return np.sqrt(np.maximum(lam[order], 0.0)), W[:, order]


def project(V, W, kind="complex"):
    """(Y (r, 2N) planar, sigma_r)."""
    V1, V2 = split(V)
    if kind == "complex":
        P, Q = W.real, W.imag
        Y = np.concatenate([P.T @ V1 + Q.T @ V2, P.T @ V2 - Q.T @ V1], axis=1)
    else:
        Y = W.real.T @ np.asarray(V, dtype=np.float64)
    return Y, np.sqrt((Y * Y).sum(axis=1))


def modes(V, r=4, kind="complex", chunk=CHUNK):
    """Passes 1-3 and the scripts' sign rule: the dict of mofhip.velocity_modes."""
    S, A = gram(V, kind, chunk)
    Sigma, W = eig(S, A)
    U = W[:, :r].copy()
    Y, sigma_r = project(V, U, kind)
    neg = np.mean(np.real(U), axis=0) < 0
    U[:, neg] = -U[:, neg]
    Y[neg] = -Y[neg]
    VT = Y / sigma_r[:, None]
    N = Y.shape[1] // 2
    if kind == "complex":
        VT = VT[:, :N] + 1j * VT[:, N:]
    return {"U": U, "Sigma": Sigma, "sigma_r": sigma_r, "VT": VT, "Y": Y}


# ---- the bars ------------------------------------------------------------
def eta(K, N):
    return 4.0 * K * N * U_ROUND


def gap2(Sigma_ref):
    """gap2_j over all K reference singular values."""
    lam = (np.asarray(Sigma_ref) / Sigma_ref[0]) ** 2
    d = np.abs(lam[:, None] - lam[None, :])
    np.fill_diagonal(d, np.inf)
    return d.min(axis=1)


def complex_Y(Y):
    N = Y.shape[1] // 2
    return Y[:, :N] + 1j * Y[:, N:]


def rank_one_errors(kind, U, Y, U_ref, Sigma_ref, VT_ref):
    """max |U_j Y_j - sigma_j u_j v_j^H(ref)| per mode (Y planar)."""
    Yc = complex_Y(Y) if kind == "complex" else Y
    return np.array([np.abs(np.outer(U[:, j], Yc[j]) - Sigma_ref[j] * np.outer(U_ref[:, j], VT_ref[j])).max()
                     for j in range(U.shape[1])])


def percent_boundary_clear(Sigma_ref, bars, r=4):
    """True where the reference's unrounded percentages of the first r modes
    keep further from a rounding boundary (x.xx5) than the Sigma bars can
    move them."""
    ok = np.ones(r, dtype=bool)
    s1, s2 = Sigma_ref.sum(), (Sigma_ref ** 2).sum()
    for j in range(r):
        for val, dval in ((Sigma_ref[j] / s1 * 100, (bars[j] + bars.sum() * Sigma_ref[j] / s1) / s1 * 100),
                          (Sigma_ref[j] ** 2 / s2 * 100,
                           (2 * Sigma_ref[j] * bars[j] + 2 * (Sigma_ref * bars).sum() * Sigma_ref[j] ** 2 / s2) / s2
                           * 100)):
            frac = (val * 100) % 1.0
            if abs(frac - 0.5) <= dval * 100:
                ok[j] = False
    return ok
