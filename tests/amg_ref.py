"""CPU checker of the multigrid's per-timestep setup (csrc/mof_amg.hip,
amg_setup_batch): the storage formats decoded, and the Galerkin product
A_{l+1} = P^T A_l P restated in fp64 with numpy and scipy.

A "level" here is one entry of ``mofhip.mesh.amg_levels(mesh)["levels"]`` (the
export mof_test_amg_levels): the SELL-64 tables of the level and, for the
transition to the next one, the prolongator as stored (CSR ``pptr`` / ``pcol``
over the fine nodes with block k's bs x 3 float32 entries in ``Q[k]``) and the
gather lists ``gptr`` / ``gent`` the product kernels fold.

Formats (mof_rowkern.h, mof_amg.hip):
  bf16            the upper 16 bits of a float32, rounded to nearest even;
  level-0 block   h0_st: 8 B, the words a00 | a01 << 16 and a10 | a11 << 16;
  D^-1            st_h9: 16 B of bf16 entries 0..7 (row-major) and entry 8 apart;
  sweep copy      st_a9: 8 B of int8 codes 0..7 in offset binary (q + 128),
                  then code 8 and the block's bf16 scale (max |a| / 127).
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

MIR_T = 1 << 30          # a mirror / level-0 gather entry: read the block transposed
MIR_POS = MIR_T - 1
U24 = 2.0 ** -24         # unit roundoff of float32


# ---- bf16 -------------------------------------------------------------------

def bf16_bits(x):
    """float32 -> bf16 bit patterns (uint16), round to nearest even (bf16_bits)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(h):
    """bf16 bit patterns -> float32 (bf16_lo)."""
    return (np.ascontiguousarray(h, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_ulp(x):
    """The spacing of bf16 numbers at |x| (8 significand bits), 0 at 0."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    out = np.zeros_like(x)
    nz = x > 0
    out[nz] = 2.0 ** (np.floor(np.log2(x[nz])) - 7)
    return out


# ---- level-0 blocks (h0_st / h0_dec) ------------------------------------------

def h0_enc(blocks):
    """(nb, 2, 2) float32 -> (nb,) uint64, one 8-byte block per position."""
    h = bf16_bits(np.asarray(blocks, dtype=np.float32).reshape(-1, 4))
    return np.ascontiguousarray(h).view("<u8").reshape(-1)


def h0_dec(words):
    """(nb,) uint64 (or (nb, 2) uint32) -> (nb, 2, 2) float64: a00, a01 in the
    first word, a10, a11 in the second."""
    h = np.ascontiguousarray(words).view("<u2").reshape(-1, 4)
    return bf16_value(h).astype(np.float64).reshape(-1, 2, 2)


# ---- D^-1 (st_h9) --------------------------------------------------------------

def h9_enc(blocks):
    """(n, 3, 3) float32 -> Dh (n, 4) uint32, Dh22 (n,) uint16."""
    h = bf16_bits(np.asarray(blocks, dtype=np.float32).reshape(-1, 9))
    return np.ascontiguousarray(h[:, :8]).view("<u4").reshape(-1, 4), np.ascontiguousarray(h[:, 8])


def h9_bits(Dh, Dh22):
    """Dh (n, 4) uint32, Dh22 (n,) uint16 -> the 9 bf16 bit patterns (n, 3, 3)."""
    h = np.ascontiguousarray(Dh).view("<u2").reshape(-1, 8)
    return np.concatenate([h, np.asarray(Dh22, dtype=np.uint16).reshape(-1, 1)], axis=1).reshape(-1, 3, 3)


def h9_dec(Dh, Dh22):
    """-> (n, 3, 3) float64."""
    return bf16_value(h9_bits(Dh, Dh22)).astype(np.float64)


# ---- sweep copy (st_a9) --------------------------------------------------------

def a9_enc(blocks):
    """(nb, 3, 3) float32 -> Ah (nb, 2) uint32, Ah22 (nb, 2) uint16, in float32
    arithmetic as st_a9: scale = bf16(max |a| / 127), code = rint(a / scale)
    clamped to +-127, + 128; a block of zeros gets scale 0 and codes 128."""
    c = np.asarray(blocks, dtype=np.float32).reshape(-1, 9)
    sb = bf16_bits(np.abs(c).max(axis=1) / np.float32(127.0))
    sc = bf16_value(sb)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where(sc[:, None] > 0, np.rint(c / sc[:, None]), np.float32(0.0))
    u = (np.clip(v, -127.0, 127.0) + 128.0).astype(np.uint8)
    Ah = np.ascontiguousarray(u[:, :8]).view("<u4").reshape(-1, 2)
    Ah22 = np.stack([u[:, 8].astype(np.uint16), sb], axis=1)
    return Ah, Ah22


def a9_dec(Ah, Ah22):
    """-> codes (nb, 3, 3) int64 in 0..255 and the scales (nb,) float32; the
    block's entries are (codes - 128) * scale."""
    u = np.ascontiguousarray(Ah).view(np.uint8).reshape(-1, 8)
    h = np.asarray(Ah22, dtype=np.uint16).reshape(-1, 2)
    codes = np.concatenate([u, (h[:, :1] & 0xFF).astype(np.uint8)], axis=1).astype(np.int64).reshape(-1, 3, 3)
    return codes, bf16_value(h[:, 1])


# ---- SELL blocks -> matrix -------------------------------------------------------

def stored_positions(level):
    """Mask of the SELL positions that hold a block of the matrix (the rest is
    padding): level 0 by its mirror table, levels >= 1 by the layout's rule
    (a padding position of row i names column i away from the diagonal's)."""
    row, col = level["sell_row"], level["sell_col"]
    if level["mirror"].size:
        return level["mirror"] >= 0
    ok = row < level["n"]
    r = np.where(ok, row, 0)
    return ok & ((col != row) | (np.arange(len(row)) == level["diag_pos"][r]))


def sell_to_csr(level, blocks):
    """The fp64 block matrix of one system from its SELL blocks (sell_nb, bs,
    bs). Level 0 honours the mirror table: a position flagged MIR_T reads the
    named position's block transposed (all the assembly writes under
    symmetric reads)."""
    bs, n = level["bs"], level["n"]
    blocks = np.asarray(blocks, dtype=np.float64)
    pos = np.flatnonzero(stored_positions(level))
    if level["mirror"].size:
        m = level["mirror"][pos]
        b = blocks[m & MIR_POS]
        b = np.where(((m & MIR_T) != 0)[:, None, None], b.transpose(0, 2, 1), b)
    else:
        b = blocks[pos]
    I, J = level["sell_row"][pos].astype(np.int64), level["sell_col"][pos].astype(np.int64)
    r = (bs * I)[:, None, None] + np.arange(bs)[None, :, None] + np.zeros((1, 1, bs), dtype=np.int64)
    c = (bs * J)[:, None, None] + np.arange(bs)[None, None, :] + np.zeros((1, bs, 1), dtype=np.int64)
    return sp.coo_matrix((b.ravel(), (r.ravel(), c.ravel())), shape=(bs * n, bs * n)).tocsr()


def prolongator(level, n_coarse):
    """P (bs n x 3 n_coarse) from the exported float32 entries widened to fp64."""
    bs, n = level["bs"], level["n"]
    Q = level["Q"].astype(np.float64)
    node = np.repeat(np.arange(n, dtype=np.int64), np.diff(level["pptr"]))
    J = level["pcol"].astype(np.int64)
    r = (bs * node)[:, None, None] + np.arange(bs)[None, :, None] + np.zeros((1, 1, 3), dtype=np.int64)
    c = (3 * J)[:, None, None] + np.arange(3)[None, None, :] + np.zeros((1, bs, 1), dtype=np.int64)
    return sp.coo_matrix((Q.ravel(), (r.ravel(), c.ravel())), shape=(bs * n, 3 * n_coarse)).tocsr()


def galerkin_ref(P, A, dead):
    """P^T A P plus 1.0 on the diagonal of every dead dof (dead: (n_coarse, 3))."""
    return (P.T @ A @ P + sp.diags(np.asarray(dead, dtype=np.float64).ravel())).tocsr()


def csr_blocks(C, I, J):
    """The 3 x 3 blocks (I[k], J[k]) of a CSR matrix as (len(I), 3, 3); entries
    outside its pattern are 0."""
    C = C.tocsr()
    r = (3 * np.asarray(I, dtype=np.int64))[:, None, None] + np.arange(3)[None, :, None] + np.zeros((1, 1, 3), np.int64)
    c = (3 * np.asarray(J, dtype=np.int64))[:, None, None] + np.arange(3)[None, None, :] + np.zeros((1, 3, 1), np.int64)
    return np.asarray(C[r.ravel(), c.ravel()]).reshape(-1, 3, 3)


def galerkin_lists(level, blocks, drop=None):
    """The exported gather lists evaluated term by term in fp64: per coarse
    SELL position p the sum over its terms g in [gptr[p], gptr[p+1]) of
    Q[ii]^T a Q[jj] with a the fine block gent[g, 0] names (level 0: a mirror
    entry, transposed under MIR_T; -1 / -2: a decomposed part's identity /
    zero ghost block). Returns (C, S, K): the sums (npos, 3, 3), the sums of
    the absolute values of the scalar products a_kl q_kr q_lc that enter each
    entry, and their number per entry (npos,). drop: a term index left out
    (the negative control of the tests)."""
    bs = level["bs"]
    blocks = np.asarray(blocks, dtype=np.float64)
    gptr, gent = level["gptr"].astype(np.int64), level["gent"]
    Q = level["Q"].astype(np.float64)
    npos = len(gptr) - 1
    owner = np.repeat(np.arange(npos), np.diff(gptr))
    C = np.zeros((npos, 3, 3))
    S = np.zeros((npos, 3, 3))
    for g0 in range(0, len(gent), 1 << 16):  # in chunks: 9 bs^2 doubles per term
        g1 = min(len(gent), g0 + (1 << 16))
        fp = gent[g0:g1, 0].astype(np.int64)
        ghost = fp < 0
        a = blocks[np.where(ghost, 0, fp & MIR_POS)]
        a = np.where((((fp & MIR_T) != 0) & ~ghost)[:, None, None], a.transpose(0, 2, 1), a)
        if ghost.any():
            a[ghost] = np.where((fp[ghost] == -1)[:, None, None], np.eye(bs)[None], 0.0)
        qi, qj = Q[gent[g0:g1, 1]], Q[gent[g0:g1, 2]]
        # every scalar product on its own, so the sums of absolute values are the same products'
        prod = qi[:, :, None, :, None] * a[:, :, :, None, None] * qj[:, None, :, None, :]  # (g, k, l, r, c)
        if drop is not None and g0 <= drop < g1:
            prod[drop - g0] = 0.0
        np.add.at(C, owner[g0:g1], prod.sum(axis=(1, 2)))
        np.add.at(S, owner[g0:g1], np.abs(prod).sum(axis=(1, 2)))
    return C, S, np.diff(gptr) * bs * bs


def sweep_inverse(M):
    """k_coarse_inverse's algorithm in fp64: the symmetric sweep operator, pivot
    by pivot, with row k standing in for column k as the multipliers (a_ik is
    read as a_ki). The inverse of a symmetric M; on a matrix that is not quite
    symmetric it is off by about cond(M) times the asymmetry."""
    a = np.array(M, dtype=np.float64)
    for k in range(len(a)):
        rowk = a[k].copy()
        ip = 1.0 / rowk[k]
        akc = rowk * ip
        new = a - np.outer(rowk, akc)
        new[:, k] = a[:, k] * ip
        new[k, :] = akc
        new[k, k] = -ip
        a = new
    return -a


def mid_list_term(level, blocks):
    """A gather term from the middle of a list of >= 3 terms -- of all such
    middle terms the one with the largest entry: (position, term index)."""
    gptr = level["gptr"].astype(np.int64)
    cnt = np.diff(gptr)
    pos = np.flatnonzero(cnt >= 3)
    mid = gptr[pos] + cnt[pos] // 2
    one = dict(level, gptr=np.arange(len(mid) + 1), gent=level["gent"][mid])  # each middle term alone
    T, _, _ = galerkin_lists(one, blocks)
    k = int(np.abs(T).max(axis=(1, 2)).argmax())
    return int(pos[k]), int(mid[k])
