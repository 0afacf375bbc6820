"""CPU checker of the inner PCG and the refinement step (csrc/mof_pcg.hip:
k_pcg_init, k_pcg_tol, k_pcg_spmv, k_pcg_update, k_pcg_conv_early, pcg<V>(),
k_outer_update, k_outer_check): one iteration restated in fp64 with numpy,
stage by stage, on the values the device stage read, each with its rounding
bound.

The device's iteration k (k_pcg_spmv k, then k_pcg_update k), u the unit
roundoff of the working type (2^-24 float, 2^-53 double), every vector over the
2 N dofs of one system:
  SpMV k     x_k = x_{k-1} + alpha_{k-1} p_{k-1}   (the update deferred from k - 1)
             beta_k = fl(rz_k / rz_{k-1})          (k = 0, FIRST: p = z, q = A z)
             p_k = z_k + beta_k p_{k-1}
             q_k = A z_k + beta_k q_{k-1}          (= A p_k up to rounding: the
                                                   product is taken of z, not of p)
             pq_k = sum_owned p_k q_k
  update k   alpha_k = fl(rz_k / pq_k)
             r_{k+1} = r_k - alpha_k q_k           (0 on rows >= nown)
             z_{k+1} = D^-1 r_{k+1}                (block Jacobi; the multigrid: the
                                                   V-cycle, x0 = w D0^-1 r_{k+1})
             rz_{k+1} = sum_owned r z, rr_{k+1} = sum_owned r r
A system whose rr_k <= TOL2 stops in SpMV k after the deferred x update alone.

Scalars. alpha and beta are quotients of the device's own fp64 sums rounded
once to the working type: reproduced exactly (``quot``), no tolerance.

Bounds (``U``: u of the working type).
  axpy       a + b c, two roundings (the product, the sum; one if fused):
             2 u (|a| + |b c|).
  row        y = A z summed in the working type from 2 w products, w the row's
             stored blocks (a padding slot adds an exact 0), then y + beta q:
             (2 w + 3) u (sum |a| |z| + |beta q|): 2 w for the products and
             their sums, 3 for beta q, the add and one spare.
  jacobi     d0 r0 + d1 r1: 3 u sum |d| |r|.
  sum        an fp64 sum of n products. Of floats: every product is exact in
             fp64 (24 + 24 bits), so only the n - 1 adds round, in any order:
             n 2^-53 sum |term|. Of doubles (the fp64 solve) each product
             rounds once more, or is fused: (n + 1) 2^-53 sum |term|.
The accumulated bound of the true-residual invariant (``Drift``): with
g_k = q_k - A p_k and e_k = (b - A x_k) - r_k,
  g_k = beta_k g_{k-1} + dq_k - A dp_k,  e_{k+1} = e_k + alpha_k g_k - A dx_{k+1} + dr_{k+1},
dq, dp, dx, dr the stages' own rounding errors, so with their bounds bq, bp,
bx, br:  G_k = |beta_k| G_{k-1} + bq_k + |A| bp_k,
         E_{k+1} = E_k + |alpha_k| G_k + |A| bx_{k+1} + br_{k+1},
         E_0 = u |b| (r_0 = fl(b), x_0 = 0), G_{-1} = 0.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

import amg_ref as R

U24 = 2.0 ** -24
U53 = 2.0 ** -53


def unit(dtype):
    return U24 if np.dtype(dtype) == np.float32 else U53


def quot(a, b, dtype):
    """fl(a / b): the fp64 quotient rounded once to the working type (alpha, beta)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.dtype(dtype).type(np.float64(a) / np.float64(b)))


# ---- the operator ------------------------------------------------------------------

def level0(sell_off, sell_col, mirror, n, sym):
    """The level dict amg_ref.sell_to_csr takes, from the level-0 SELL tables.
    sym: the row kernels read every lower block as its upper twin transposed
    (the mirror table); otherwise every block at its own position."""
    sell_off = np.asarray(sell_off)
    nb = int(sell_off[-1])
    row = np.zeros(nb, dtype=np.int64)
    for s in range(len(sell_off) - 1):
        q = np.arange(sell_off[s], sell_off[s + 1])
        row[q] = 64 * s + (q - sell_off[s]) % 64
    mirror = np.asarray(mirror)
    if not sym:
        mirror = np.where(mirror >= 0, np.arange(nb), -1).astype(mirror.dtype)
    return {"n": int(n), "bs": 2, "sell_row": row, "sell_col": np.asarray(sell_col), "mirror": mirror}


def untranspose_one(level, blocks):
    """The negative control: the mirror entry of one lower block whose upper
    twin is not symmetric loses its transpose bit. Returns the new level."""
    m = level["mirror"]
    blocks = np.asarray(blocks, dtype=np.float64).reshape(-1, 2, 2)
    cand = np.flatnonzero((m >= 0) & ((m & R.MIR_T) != 0))
    twin = blocks[m[cand] & R.MIR_POS]
    k = cand[np.argmax(np.abs(twin[:, 0, 1] - twin[:, 1, 0]))]
    m2 = m.copy()
    m2[k] = m[k] & R.MIR_POS
    return dict(level, mirror=m2)


class Op:
    """One system's operator as the row product reads it."""

    def __init__(self, level, blocks):
        self.A = R.sell_to_csr(level, np.asarray(blocks, dtype=np.float64).reshape(-1, 2, 2))
        self.Aabs = abs(self.A)
        stored = R.stored_positions(level)
        w = np.bincount(level["sell_row"][stored], minlength=level["n"])[:level["n"]]
        self.w = np.repeat(w, 2).astype(np.float64)  # stored blocks of each dof's row
        self.n = 2 * level["n"]


# ---- the stages: (exact value, bound) on the values the device stage read ---------------

def axpy(a, b, c, U):
    a, c = np.asarray(a, dtype=np.float64), np.asarray(c, dtype=np.float64)
    return a + b * c, 2 * U * (np.abs(a) + np.abs(b * c))


def x_step(x, alpha, p, U):
    return axpy(x, alpha, p, U)


def r_step(r, alpha, q, U, nown=None):
    e, beta = axpy(r, -alpha, q, U)
    if nown is not None:
        e[2 * nown:] = 0.0
        beta[2 * nown:] = 0.0
    return e, beta


def p_step(z, beta, p, U):
    return axpy(z, beta, p, U)


def q_step(op, z, beta, q_old, U):
    z = np.asarray(z, dtype=np.float64)
    bq = beta * np.asarray(q_old, dtype=np.float64)
    return op.A @ z + bq, (2 * op.w + 3) * U * (op.Aabs @ np.abs(z) + np.abs(bq))


def jacobi_z(dinv, r, U):
    """dinv (N, 2, 2), r (2 N,)."""
    d = np.asarray(dinv, dtype=np.float64)
    r2 = np.asarray(r, dtype=np.float64).reshape(-1, 2)
    e = np.einsum("nij,nj->ni", d, r2).ravel()
    return e, 3 * U * np.einsum("nij,nj->ni", np.abs(d), np.abs(r2)).ravel()


def dot(a, b, nown=None, rows=None, exact_products=True):
    """sum over the owned dofs (rows: an explicit dof index list instead -- the
    negative control that lets a row past the owned ones in)."""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    if rows is None:
        rows = np.arange(len(a) if nown is None else 2 * nown)
    t = a[rows] * b[rows]
    n = len(t) + (0 if exact_products else 1)
    return float(t.sum()), n * U53 * float(np.abs(t).sum())


def within(got, e, beta):
    """(all within the bound, largest error / bound); a zero bound demands equality."""
    got, e, beta = np.asarray(got, dtype=np.float64), np.asarray(e, dtype=np.float64), np.asarray(beta, np.float64)
    err = np.abs(got - e)
    bad = ~np.isfinite(err)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(beta > 0, err / np.where(beta > 0, beta, 1.0), np.where(err > 0, np.inf, 0.0))
    ratio = np.where(bad, np.inf, ratio)
    return bool((ratio <= 1.0).all()), float(ratio.max()) if ratio.size else 0.0


# ---- the stop rule ----------------------------------------------------------------------

K_ERR_SAFETY = 2.0   # mof_pcg.hip kErrSafety


def inner_tol(rtol, outer_rtol, etol, ff, rr, est, xmax):
    """k_pcg_tol's t: rtol, or with outer_rtol > 0 what the system's outer
    residual still needs, 0.3 outer_rtol |f| / |r64|, no looser than the error
    estimate needs, within [rtol, 0.5]."""
    t = rtol
    if outer_rtol > 0.0 and ff > 0.0 and rr > 0.0:
        need = 0.3 * outer_rtol * np.sqrt(ff / rr)
        if etol > 0.0 and est > 0.0:
            need = min(need, 0.5 * etol * xmax / (K_ERR_SAFETY * est))
        t = max(rtol, min(0.5, need))
    return float(t)


def tol2(t, rr0):
    return t * t * rr0


def conv_step(rr, tol2_):
    """SI_CONV: the first step whose own |r|^2 is <= TOL2 (None: none of them)."""
    for k, v in enumerate(rr):
        if v <= tol2_:
            return k
    return None


def best(rr):
    """SD_BEST, SI_BEST_IT after the SpMV launches 0 .. len(rr) - 1 of a running
    system: k_pcg_tol starts at (rr_0, 0), a launch takes a strictly smaller one."""
    b, it = rr[0], 0
    for k, v in enumerate(rr):
        if v < b:
            b, it = v, k
    return b, it


def outer_check(rr, ff, dmax, xmax, rr_prev, first, rtol, etol):
    """k_outer_check from its inputs: rel, est, met, retired."""
    rel = np.sqrt(rr / ff) if ff > 0.0 else (np.inf if rr > 0.0 else 0.0)
    prev = ff if first else rr_prev
    est = dmax * np.sqrt(rr / prev) if prev > 0.0 else 0.0
    met = bool(rel <= rtol)
    retired = met and (etol <= 0.0 or K_ERR_SAFETY * est <= etol * xmax)
    return float(rel), float(est), met, bool(retired)


# ---- the iteration as a whole (exact arithmetic; test_pcg_ref.py) ------------------------

def start(op, b, precond, dtype=np.float64, nown=None):
    """The state k_pcg_init, k_pcg_tol and the first preconditioner leave."""
    r = np.asarray(b, dtype=np.float64).astype(dtype).astype(np.float64)
    if nown is not None:
        r[2 * nown:] = 0.0
    z = precond(r)
    return {"k": 0, "x": np.zeros(op.n), "r": r, "z": z, "p": None, "q": None, "rz": dot(r, z, nown)[0],
            "rr": dot(r, r, nown)[0], "pq": None, "rz_old": None, "alpha_old": None}


def iterate(op, st, precond, dtype=np.float64, nown=None):
    """SpMV k and update k in the device's order, every stage's exact value,
    alpha and beta rounded to dtype: the state before SpMV k + 1."""
    U = unit(dtype)
    s = dict(st)
    if s["k"] == 0:
        s["p"], s["q"], beta = s["z"].copy(), op.A @ s["z"], 0.0
    else:
        s["x"] = x_step(s["x"], s["alpha_old"], s["p"], U)[0]
        beta = quot(s["rz"], s["rz_old"], dtype)
        s["q"] = q_step(op, s["z"], beta, s["q"], U)[0]
        s["p"] = p_step(s["z"], beta, s["p"], U)[0]
    s["pq"] = dot(s["p"], s["q"], nown)[0]
    alpha = quot(s["rz"], s["pq"], dtype)
    s["r"] = r_step(s["r"], alpha, s["q"], U, nown)[0]
    s["z"] = precond(s["r"])
    s["rz_old"], s["alpha_old"], s["beta"] = s["rz"], alpha, beta
    s["rz"], s["rr"] = dot(s["r"], s["z"], nown)[0], dot(s["r"], s["r"], nown)[0]
    s["k"] += 1
    return s


def finish(st):
    """The check launch: the deferred x update alone."""
    s = dict(st)
    if s["k"] > 0:
        s["x"] = s["x"] + s["alpha_old"] * s["p"]
    return s


def textbook_pcg(A, b, Minv, steps):
    """Dense preconditioned CG in fp64 (Hestenes-Stiefel): the iterates x_1 .. x_steps."""
    x = np.zeros(len(b))
    r = b.copy()
    z = Minv @ r
    p = z.copy()
    out = []
    for _ in range(steps):
        Ap = A @ p
        a = (r @ z) / (p @ Ap)
        x = x + a * p
        rn = r - a * Ap
        zn = Minv @ rn
        p = zn + ((rn @ zn) / (r @ z)) * p
        r, z = rn, zn
        out.append((x.copy(), r.copy()))
    return out


# ---- the true-residual invariant's accumulated bound ---------------------------------------

class Drift:
    """E_k of the module docstring for one system, fed the per-step bounds the
    reference formed."""

    def __init__(self, op, b, U):
        self.op, self.U = op, U
        self.E = U * np.abs(np.asarray(b, dtype=np.float64))
        self.G = np.zeros(op.n)

    def spmv(self, beta, bq, bp, bx):
        """SpMV k: its x, p, q stage bounds (k = 0: bp = bx = 0, bq the row product's)."""
        self.E = self.E + self.op.Aabs @ bx
        self.G = abs(beta) * self.G + bq + self.op.Aabs @ bp

    def update(self, alpha, br):
        """update k: the x update it owes is charged with its alpha here, its
        rounding when the next SpMV (or the check launch) applies it."""
        self.E = self.E + abs(alpha) * self.G + br

    def final_x(self, bx):
        return self.E + self.op.Aabs @ bx


def true_residual_gap(op, b, x, r):
    """|(b - A x) - r| per dof, A x in fp64 from the read-back blocks."""
    return np.abs((np.asarray(b, dtype=np.float64) - op.A @ np.asarray(x, dtype=np.float64)) - np.asarray(r, np.float64))


# ---- a system's state after a capped solve, and the checks between two of them ----------------
#
# A state is what the hook leaves for one system after cap K: a dict of the flat
# fp64-widened vectors "x", "r", "z", "p", "q" (2 N,), "scal" (2 slots, 3: r.z,
# |r|^2, p.q; step k's are in slot k & 1), "conv" (SI_CONV) and "tol2".

def from_csr(A):
    """An Op from a matrix of 2 x 2 blocks (the CPU tests)."""
    A = sp.csr_matrix(A)
    op = Op.__new__(Op)
    op.A, op.Aabs, op.n = A, abs(A), A.shape[0]
    # (a copy of indptr: sum_duplicates compacts it in place, and A keeps its own)
    blk = sp.csr_matrix((np.ones(A.nnz), A.indices // 2, A.indptr.copy()), shape=(A.shape[0], A.shape[1] // 2))
    blk.sum_duplicates()
    op.w = np.diff(blk.indptr).astype(np.float64)
    return op


def check_first(op, b, S, dtype, dinv=None, nown=None):
    """The state after cap 0 (k_pcg_init, the preconditioner, SpMV 0 -- the FIRST
    instance) of a system that did not stop at step 0: [(stage, ok, error / bound)]
    and the q bound (the drift's G_0). dinv None: z is not checked here (the
    multigrid's is the V-cycle's own output)."""
    U = unit(dtype)
    r0 = np.asarray(b, dtype=np.float64).astype(dtype).astype(np.float64)
    if nown is not None:
        r0[2 * nown:] = 0.0
    out = [("r0 = fl(b)", bool(np.array_equal(S["r"], r0)), 0.0),
           ("x0 = 0", bool((S["x"] == 0).all()), 0.0),
           ("p0 = z0", bool(np.array_equal(S["p"], S["z"])), 0.0)]
    if dinv is not None:
        out.append(("z = D^-1 r",) + within(S["z"], *jacobi_z(dinv, S["r"], U)))
    e, bq = q_step(op, S["z"], 0.0, np.zeros(op.n), U)
    out.append(("q = A z",) + within(S["q"], e, bq))
    ex = np.dtype(dtype) == np.float32
    out.append(("r.z",) + within(S["scal"][0][0], *dot(S["r"], S["z"], nown, exact_products=ex)))
    out.append(("r.r",) + within(S["scal"][0][1], *dot(S["r"], S["r"], nown, exact_products=ex)))
    out.append(("p.q",) + within(S["scal"][0][2], *dot(S["p"], S["q"], nown, exact_products=ex)))
    return out, bq


def check_step(op, S0, S1, K, dtype, dinv=None, nown=None, control=None):
    """The transition cap K -> cap K + 1 (update K, the preconditioner, SpMV
    K + 1) of a system still running at K, every stage on what it read:
    [(stage, ok, error / bound)] and the dict of alpha, beta and the stage
    bounds bx, br, bp, bq the drift takes. control: a reference wrong in one
    thing -- "beta_slot" (beta from the swapped slots), "drop_x" (the deferred x
    update left out), "pq_row" (one row past the owned ones summed into p.q)."""
    U = unit(dtype)
    ex = np.dtype(dtype) == np.float32
    cur, nxt = K & 1, (K + 1) & 1
    rz, _, pq = S0["scal"][cur]
    out = [("step K's scalars kept", bool(np.array_equal(S1["scal"][cur][:2], S0["scal"][cur][:2])), 0.0)]
    alpha = quot(rz, pq, dtype)
    e, br = r_step(S0["r"], alpha, S0["q"], U, nown)
    out.append(("r -= alpha q",) + within(S1["r"], e, br))
    if dinv is not None:
        out.append(("z = D^-1 r",) + within(S1["z"], *jacobi_z(dinv, S1["r"], U)))
        out.append(("r.z",) + within(S1["scal"][nxt][0], *dot(S1["r"], S1["z"], nown, exact_products=ex)))
    out.append(("r.r",) + within(S1["scal"][nxt][1], *dot(S1["r"], S1["r"], nown, exact_products=ex)))
    e, bx = x_step(S0["x"], 0.0 if control == "drop_x" else alpha, S0["p"], U)
    out.append(("x += alpha p",) + within(S1["x"], e, bx))
    info = {"alpha": alpha, "beta": 0.0, "bx": bx, "br": br, "bp": np.zeros(op.n), "bq": np.zeros(op.n),
            "stopped": S1["scal"][nxt][1] <= S1["tol2"]}
    if info["stopped"]:  # SpMV K + 1 applied the x update and left: p, q as they were
        out.append(("p, q kept", bool(np.array_equal(S1["p"], S0["p"]) and np.array_equal(S1["q"], S0["q"])), 0.0))
        return out, info
    if dinv is None:  # the multigrid's r.z comes with its z (k_post0_ns), of a running system only
        out.append(("r.z",) + within(S1["scal"][nxt][0], *dot(S1["r"], S1["z"], nown, exact_products=ex)))
    rz1 = S1["scal"][nxt][0]
    beta = quot(rz, rz1, dtype) if control == "beta_slot" else quot(rz1, rz, dtype)
    e, bp = p_step(S1["z"], beta, S0["p"], U)
    out.append(("p = z + beta p",) + within(S1["p"], e, bp))
    e, bq = q_step(op, S1["z"], beta, S0["q"], U)
    out.append(("q = A z + beta q",) + within(S1["q"], e, bq))
    rows = None
    if control == "pq_row":
        n = op.n if nown is None else 2 * nown
        rows = np.concatenate([np.arange(n), [n % op.n, (n + 1) % op.n]])  # the row after the last owned one
    out.append(("p.q",) + within(S1["scal"][nxt][2], *dot(S1["p"], S1["q"], nown, rows=rows, exact_products=ex)))
    info.update(beta=beta, bp=bp, bq=bq)
    return out, info


def failing(recs):
    return {k for k, ok, _ in recs if not ok}
