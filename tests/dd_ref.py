"""CPU restatement of the decomposed solve (csrc/mof_dd_plan.cpp, mof_dd.hip,
pcg() of mof_pcg.hip over the parts) in fp64 numpy: the halo plan from its definition, the
halo exchange and the gather as copies, and the lockstep PCG iteration over
the parts. tests/test_dd_ref.py checks it on the CPU, tests/test_gpu_dd_kernels.py
holds the device to it.

The plan. Part p owns the vertices v with part[v] = p; the order of its owned
rows is the library's one free choice (the global RCM position) and is taken
as given (``own_order``). Everything else follows:
  local triangles  every triangle with a corner owned by p, in caller order;
  ghosts           their other corners, sorted by (owner part, the owner's
                   local row) -- so grouped by owner, one contiguous range per
                   neighbour, ghost_src ascending inside a range;
  neighbours       the owners of the ghosts, ascending; recv_off their ranges;
  send lists       part q sends p the rows p's ghost range for q names, in
                   that order; q's segments are ordered by neighbour;
  packed segment   for an exchange of B systems segment k of a part holds
                   [B][cnt_k][2] values at element offset 2 B send_off[k] of
                   the part's region (``pack`` / ``unpack``).

The lockstep iteration (``start`` / ``iterate``): pcg_ref's stages per part
with nown -- ghost r is 0, ghost z is replaced by the owner's before each row
product, ghost p follows from ghost z and the global beta (the same
expression on the same values as on the owner), and r.z, |r|^2, p.q are sums
over the owned rows of all parts, part by part. The iteration's checks use
pcg_ref's bounds (axpy, row, jacobi, sum) and vcycle_ref's; two bounds are
derived here, where no reference had one: the fp32 assembly's (``a32_bound``)
and the fp64 residual's (``residual_bound``), both counts of roundings on the
magnitudes of the terms, restated from the geometry (``a1_terms``).
"""
from __future__ import annotations

import numpy as np

import pcg_ref as P


# ---- the plan -------------------------------------------------------------------------------

def restated_plan(tri, N, part, own_order):
    """own_order: per part the caller vertices it owns, in local row order.
    Returns per part a dict of l2g, n_own, n_ghost, ghost_owner, ghost_src,
    nbr, recv_off, send_off, send_idx, n_tri."""
    tri = np.asarray(tri)
    part = np.asarray(part)
    nparts = len(own_order)
    g2l = np.full(N, -1, dtype=np.int64)
    for p, own in enumerate(own_order):
        own = np.asarray(own)
        assert sorted(own.tolist()) == np.flatnonzero(part == p).tolist(), "own_order is not the part's vertex set"
        g2l[own] = np.arange(len(own))
    tp = part[tri]                                    # (M, 3) owner of every corner
    out = []
    for p in range(nparts):
        local = (tp == p).any(axis=1)
        corners = tri[local].ravel()
        ghosts = sorted({int(v) for v in corners if part[v] != p}, key=lambda v: (int(part[v]), int(g2l[v])))
        owner = [int(part[v]) for v in ghosts]
        nbr = sorted(set(owner))
        recv_off = [0] + [sum(o <= q for o in owner) for q in nbr]
        out.append({"l2g": np.array(list(own_order[p]) + ghosts, dtype=np.int64), "n_own": len(own_order[p]),
                    "n_ghost": len(ghosts), "ghost_owner": np.array(owner, dtype=np.int64),
                    "ghost_src": g2l[ghosts] if ghosts else np.zeros(0, dtype=np.int64),
                    "nbr": np.array(nbr, dtype=np.int64), "recv_off": np.array(recv_off, dtype=np.int64),
                    "n_tri": int(local.sum())})
    for q in range(nparts):
        send, off = [], [0]
        for p in out[q]["nbr"]:                       # the neighbour relation is symmetric
            R = out[int(p)]
            k = R["nbr"].tolist().index(q)
            send += R["ghost_src"][R["recv_off"][k]:R["recv_off"][k + 1]].tolist()
            off.append(len(send))
        out[q]["send_idx"] = np.array(send, dtype=np.int64)
        out[q]["send_off"] = np.array(off, dtype=np.int64)
    return out


def plan_of_handles(parts):
    """The same dicts from what mof_dd_test_part returned (PartHandle)."""
    keys = ("l2g", "n_own", "n_ghost", "ghost_owner", "ghost_src", "nbr", "recv_off", "send_off", "send_idx", "n_tri")
    return [{k: getattr(p, k) for k in keys} for p in parts]


def plan_mismatches(got, want):
    """Every field of every part that differs, exactly."""
    bad = []
    for p, (g, w) in enumerate(zip(got, want)):
        for k in w:
            if not np.array_equal(np.asarray(g[k]), np.asarray(w[k])):
                bad.append((p, k))
    return bad


def ghost_positions(plan):
    """{(receiver p, ghost g): [(sender q, position in q's send list)]}: where
    each ghost appears in the send lists, and the position the receiver expects
    (q's segment for p, offset g - recv_off)."""
    seen = {}
    for q, Q in enumerate(plan):
        for k, p in enumerate(Q["nbr"]):
            R = plan[int(p)]
            kk = R["nbr"].tolist().index(q)
            for e in range(int(Q["send_off"][k]), int(Q["send_off"][k + 1])):
                g = int(R["recv_off"][kk]) + e - int(Q["send_off"][k])
                seen.setdefault((int(p), g), []).append((q, e))
    return seen


# ---- halo and gather: copies ------------------------------------------------------------------

def halo(plan, vecs, wrong_row=None, stale=()):
    """Every ghost row of every part takes its owner's value; owned rows are
    untouched. vecs: per part (B, n_loc, 2) or flat (2 n_loc,) arrays.
    Negative controls: stale (parts whose ghosts are left as they are),
    wrong_row = (part, ghost): that ghost is taken from the owner's next row."""
    flat = vecs[0].ndim == 1
    src = [v.reshape(1, -1, 2) if flat else v for v in vecs]
    out = [v.copy() for v in src]
    for p, D in enumerate(plan):
        if p in stale:
            continue
        for g in range(D["n_ghost"]):
            q, row = int(D["ghost_owner"][g]), int(D["ghost_src"][g])
            if wrong_row == (p, g):
                row = (row + 1) % plan[q]["n_own"]
            out[p][:, D["n_own"] + g] = src[q][:, row]
    return [v.reshape(-1) for v in out] if flat else out


def pack(D, vec):
    """A part's send region for its (B, n_loc, 2) vector: segment k as
    [B][cnt_k][2] at element offset 2 B send_off[k]."""
    B = vec.shape[0]
    buf = np.zeros(2 * B * len(D["send_idx"]), dtype=vec.dtype)
    for k in range(len(D["nbr"])):
        a, b = int(D["send_off"][k]), int(D["send_off"][k + 1])
        buf[2 * B * a:2 * B * b] = vec[:, D["send_idx"][a:b]].ravel()
    return buf


def halo_staged(plan, vecs):
    """The same exchange through the packed segments: pack, copy q's segment
    for p into p's receive segment for q, unpack into the ghost range."""
    B = vecs[0].shape[0]
    sent = [pack(D, v) for D, v in zip(plan, vecs)]
    out = [v.copy() for v in vecs]
    for p, D in enumerate(plan):
        for k, q in enumerate(D["nbr"]):
            Q = plan[int(q)]
            kk = Q["nbr"].tolist().index(p)
            a, b = int(Q["send_off"][kk]), int(Q["send_off"][kk + 1])
            g0, g1 = int(D["recv_off"][k]), int(D["recv_off"][k + 1])
            assert b - a == g1 - g0
            seg = sent[int(q)][2 * B * a:2 * B * b].reshape(B, b - a, 2)
            out[p][:, D["n_own"] + g0:D["n_own"] + g1] = seg
    return out


def gather(plan, N, x64, failed=None):
    """Planar V (B, 2 N) from the owned rows; a failed system is all NaN. Also
    returns how often each caller vertex was written (all 1)."""
    B = x64[0].shape[0]
    V = np.zeros((B, 2 * N))
    hits = np.zeros(N, dtype=np.int64)
    for D, x in zip(plan, x64):
        own = D["l2g"][:D["n_own"]]
        V[:, own] = x[:, :D["n_own"], 0]
        V[:, N + own] = x[:, :D["n_own"], 1]
        hits[own] += 1
    if failed is not None:
        V[np.asarray(failed, dtype=bool)] = np.nan
    return V, hits


def coded(plan, B, shift=0):
    """Per part a (B, n_loc, 2) array of small integers, each value unique over
    (part, system, row, component) and exact in fp32 (< 2^24)."""
    out, base = [], 1 + shift
    for D in plan:
        n = B * len(D["l2g"]) * 2
        out.append(np.arange(base, base + n, dtype=np.float64).reshape(B, len(D["l2g"]), 2))
        base += n
    assert base < 2 ** 24
    return out


# ---- the lockstep iteration ------------------------------------------------------------------

def owned_sum(plan, a, b, drop_part=None, ghost_part=None):
    """sum over the owned rows of all parts, part by part (pcg_ref.dot per part).
    Negative controls: drop_part (a part's records left out), ghost_part (that
    part's ghost rows summed too). Returns (sum, pcg_ref.dot's bound of the whole)."""
    tot = 0.0
    cat_a, cat_b = [], []
    for p, D in enumerate(plan):
        if p == drop_part:
            continue
        n = None if p == ghost_part else D["n_own"]
        s, _ = P.dot(a[p], b[p], n)
        tot += s
        cat_a.append(np.asarray(a[p], dtype=np.float64).ravel()[:2 * D["n_own"]])
        cat_b.append(np.asarray(b[p], dtype=np.float64).ravel()[:2 * D["n_own"]])
    return tot, P.dot(np.concatenate(cat_a), np.concatenate(cat_b))[1]


def start(plan, ops, b, precond, dtype=np.float64):
    """ops: per part a pcg_ref.Op of its local matrix; b: per part the flat
    (2 n_loc,) right-hand side; precond(p, r) -> z of part p (its ghost rows are
    never read)."""
    r = []
    for D, bp in zip(plan, b):
        v = np.asarray(bp, dtype=np.float64).astype(dtype).astype(np.float64)
        v[2 * D["n_own"]:] = 0.0
        r.append(v)
    z = [precond(p, v) for p, v in enumerate(r)]
    return {"k": 0, "x": [np.zeros(o.n) for o in ops], "r": r, "z": z, "p": None, "q": None,
            "rz": owned_sum(plan, r, z)[0], "rr": owned_sum(plan, r, r)[0], "pq": None, "rz_old": None,
            "alpha_old": None}


def iterate(plan, ops, st, precond, dtype=np.float64, control=None):
    """SpMV k (after the halo of z) and update k on every part, alpha and beta
    global. control = (name, part[, ghost]) for this step: "stale" (that part's
    ghosts are not refreshed), "wrong_row" (one ghost from the owner's next row),
    "pq_ghost" (ghost rows in p.q), "drop_part" (its records left out of p.q)."""
    U = P.unit(dtype)
    name = control[0] if control else None
    s = dict(st)
    z = halo(plan, s["z"], stale=(control[1],) if name == "stale" else (),
             wrong_row=tuple(control[1:3]) if name == "wrong_row" else None)
    n = len(plan)
    if s["k"] == 0:
        s["p"], s["q"], beta = [v.copy() for v in z], [ops[p].A @ z[p] for p in range(n)], 0.0
    else:
        s["x"] = [P.x_step(s["x"][p], s["alpha_old"], s["p"][p], U)[0] for p in range(n)]
        beta = P.quot(s["rz"], s["rz_old"], dtype)
        s["q"] = [P.q_step(ops[p], z[p], beta, s["q"][p], U)[0] for p in range(n)]
        s["p"] = [P.p_step(z[p], beta, s["p"][p], U)[0] for p in range(n)]
    s["z"] = z
    s["pq"] = owned_sum(plan, s["p"], s["q"], drop_part=control[1] if name == "drop_part" else None,
                        ghost_part=control[1] if name == "pq_ghost" else None)[0]
    alpha = P.quot(s["rz"], s["pq"], dtype)
    s["r"] = [P.r_step(s["r"][p], alpha, s["q"][p], U, plan[p]["n_own"])[0] for p in range(n)]
    s["z"] = [precond(p, v) for p, v in enumerate(s["r"])]
    s["rz_old"], s["alpha_old"], s["beta"] = s["rz"], alpha, beta
    s["rz"], s["rr"] = owned_sum(plan, s["r"], s["z"])[0], owned_sum(plan, s["r"], s["r"])[0]
    s["k"] += 1
    return s


def finish(st):
    """The check launch: the deferred x update alone."""
    s = dict(st)
    if s["k"] > 0:
        s["x"] = [x + s["alpha_old"] * p for x, p in zip(s["x"], s["p"])]
    return s


def to_global(plan, N, vecs):
    """The owned rows of per-part flat vectors as one (2 N,) vector, dofs
    interleaved by caller vertex."""
    out = np.zeros((N, 2))
    for D, v in zip(plan, vecs):
        out[D["l2g"][:D["n_own"]]] = np.asarray(v).reshape(-1, 2)[:D["n_own"]]
    return out.ravel()


def local_matrix(A, D, couple_ghost=None):
    """Part D's local matrix from the global one (2 x 2 blocks, scipy CSR): the
    owned rows over the local columns, the ghost rows decoupled (identity).
    couple_ghost: the negative control -- that ghost row keeps its coupling."""
    import scipy.sparse as sp
    idx = np.stack([2 * D["l2g"], 2 * D["l2g"] + 1], axis=1).ravel()
    L = sp.lil_matrix(sp.csr_matrix(A)[idx][:, idx])
    for g in range(D["n_own"], len(D["l2g"])):
        if couple_ghost == g - D["n_own"]:
            continue
        for c in (0, 1):
            L[2 * g + c, :] = 0.0
            L[2 * g + c, 2 * g + c] = 1.0
    return sp.csr_matrix(L)


# ---- device-side checks built on pcg_ref's ---------------------------------------------------------

SUMS = ("r.z", "r.r", "p.q")


def part_state(o, scal, b):
    """System b's state of one part of a hook run, in pcg_ref's format (the sums are the shared ones)."""
    f = lambda a: a[b].astype(np.float64).ravel()  # noqa: E731
    return {"x": f(o["x"]), "r": f(o["r"]), "z": f(o["z"]), "p": f(o["p"]), "q": f(o["q"]),
            "scal": scal[:, b, :].copy(), "conv": int(o["sys"]["CONV"][b]), "tol2": float(o["sys"]["TOL2"][b])}


def jacobi_owned(dinv, S, nown, U):
    """z = D^-1 r on the owned rows (the ghost rows hold the owner's z after the halo)."""
    e, beta = P.jacobi_z(dinv[:nown], S["r"][:2 * nown], U)
    return ("z = D^-1 r",) + P.within(S["z"][:2 * nown], e, beta)


def global_sums(plan, S, slot, exact_products, which=SUMS, **control):
    """The three shared sums of a step against the fp64 sums over the owned rows of all parts."""
    pairs = {"r.z": ("r", "z", 0), "r.r": ("r", "r", 1), "p.q": ("p", "q", 2)}
    out = []
    for name in which:
        a, b, i = pairs[name]
        s, bound = owned_sum(plan, [v[a] for v in S], [v[b] for v in S], **control)
        if not exact_products:
            n = sum(2 * D["n_own"] for D in plan)
            bound *= (n + 1) / n
        out.append((name,) + P.within(S[0]["scal"][slot][i], s, bound))
    return out


# ---- the fp32 assembly's bound, from the geometry ---------------------------------------------

def a1_terms(tri, areas, grad_w, e, I0):
    """a1 restated per (triangle, corner pair), planar dofs (component * N +
    vertex): block (i, j) = sum_T c_T (E_i g_T)(E_j g_T)^T, g_T = grad_M I0 on
    T, c_T = area / 6 on the diagonal block and area / 12 elsewhere. Returns the
    value, the sum of the terms' magnitude bounds c_T (|E_i| |g_T|)(|E_j| |g_T|)^T
    (it dominates every way of grouping the products) as CSR (2 N, 2 N), and
    the triangles shared by each vertex pair as CSR (N, N)."""
    import scipy.sparse as sp
    tri = np.asarray(tri, dtype=np.int64)
    N = len(e)
    g = np.einsum("tc,tcd->td", np.asarray(I0, dtype=np.float64)[tri], np.asarray(grad_w, dtype=np.float64))
    rows, cols, val, mag, vr, vc = [], [], [], [], [], []
    for a in range(3):
        for b in range(3):
            i, j = tri[:, a], tri[:, b]
            c = np.asarray(areas, dtype=np.float64) / np.where(i == j, 6.0, 12.0)
            ui, uj = np.einsum("tkd,td->tk", e[i], g), np.einsum("tkd,td->tk", e[j], g)
            mi, mj = np.einsum("tkd,td->tk", np.abs(e[i]), np.abs(g)), np.einsum("tkd,td->tk", np.abs(e[j]), np.abs(g))
            for al in range(2):
                for be in range(2):
                    rows.append(al * N + i)
                    cols.append(be * N + j)
                    val.append(c * ui[:, al] * uj[:, be])
                    mag.append(c * mi[:, al] * mj[:, be])
            vr.append(i)
            vc.append(j)
    cat = np.concatenate
    shape = (2 * N, 2 * N)
    value = sp.coo_matrix((cat(val), (cat(rows), cat(cols))), shape=shape).tocsr()
    bound = sp.coo_matrix((cat(mag), (cat(rows), cat(cols))), shape=shape).tocsr()
    shared = sp.coo_matrix((np.ones(9 * len(tri)), (cat(vr), cat(vc))), shape=(N, N)).tocsr()
    return value, bound, shared


# The fp32 assembly of one entry, a1 folded from t triangles plus lambda a2: each term carries at most
# 13 + t roundings -- g twice, E_i, E_j and the weight rounded to fp32 (5), the outer product (1), the fold
# over the t triangles (t), the two 3-term projections (3 + 3) and the add of lambda a2 (1); lambda a2 is
# rounded once and added once (2). The older per-incidence fold has fewer (7 + t) on smaller magnitudes.
def a32_bound(mag, shared_t, a2_abs, U=2.0 ** -24):
    k = 13.0 + shared_t
    return k * U / (1.0 - k * U) * mag + 2.0 * U * a2_abs


# The fp64 residual f - A x of one dof, the operator applied block by block (lambda a2) and triangle by
# triangle (a1, re-formed from the geometry): per a1 term at most 24 roundings (the two tangent projections
# of g, the 6-term inner product, the weight, the outer factor) plus the fold over the row's t <= w
# triangles; the w blocks of lambda a2 2 w + 1; the subtraction from f 1.
def residual_bound(w, mag_x, a2_abs_x, f_abs, U=2.0 ** -53):
    return (3.0 * w + 26.0) * U * (mag_x + a2_abs_x + f_abs)
