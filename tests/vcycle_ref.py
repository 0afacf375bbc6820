"""CPU checker of the multigrid V-cycle (csrc/mof_amg.hip, amg_vcycle): the
cycle restated in fp64 with numpy and scipy, stage by stage, on what the
device holds for one system, with the rounding bound of each stage.

A ``Cycle`` holds, for levels 0 .. L - 1 (level 0 with 2 dofs per node, the
others with 3; vectors are flat dof arrays, or (dofs, columns) matrices):
  A[l]      the operator the sweeps of level l read (level 0: the decoded bf16
            copy A0h; coarse levels: the decoded int8 copy; the coarsest's is
            never read by the cycle),
  Dinv[l]   the smoother's block-diagonal D^-1 (level 0: the inverse of A0h's
            diagonal blocks, which the kernels solve with in place; coarse
            levels: the decoded bf16 Dh), l < L - 1,
  P[l]      the prolongator l + 1 -> l, l < L - 1,
  cinvT     the coarsest solve y = cinvT b (k_subcycle reads cinv by columns),
  w, w1     the damping on level 0 and on the coarse levels,
  ring, sweeps   the dofs of the boundary ring's rows and the Jacobi sweeps on
            them per side (k_bsweep; none on a closed surface).

The cycle (one symmetric V(1,1)):
  x0 = w D0^-1 r; ring sweeps; r1 = r - A0 x0; b1 = P0^T r1;
  per coarse level l < L - 1: x_l = w1 D_l^-1 b_l, r_l = b_l - A_l x_l,
      b_{l+1} = P_l^T r_l;
  y_{L-1} = cinvT b_{L-1};
  back up: x_l += P_l y_{l+1}, y_l = x_l + w1 D_l^-1 (b_l - A_l x_l);
  level 0: x = x0 + P0 y_1; ring sweeps; z = x + w D0^-1 (r - A0 x).

Bounds. A value summed in fp32 from k products whose absolute values sum to S
lies within (k + c) 2^-24 S of the exact value, c counting the other
roundings on the path; every bound_* below states its k and c. A stage that
reads a value the device no longer holds (the coarse pre-smoothed x, a ring
sweep's previous iterate) adds the propagated bound of that value.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

import amg_ref as R

U24 = R.U24


class Cycle:
    def __init__(self, A, Dinv, P, cinvT, w, w1, ring=None, sweeps=0):
        self.A = [None if a is None else sp.csr_matrix(a) for a in A]
        self.Dinv = [sp.csr_matrix(d) for d in Dinv]
        self.P = [sp.csr_matrix(p) for p in P]
        self.cinvT = np.asarray(cinvT, dtype=np.float64)
        self.w, self.w1 = float(w), float(w1)
        self.ring = None if ring is None or sweeps == 0 else np.asarray(ring, dtype=np.int64)
        self.sweeps = int(sweeps) if self.ring is not None else 0
        self.L = len(self.P) + 1
        assert len(self.A) == self.L and len(self.Dinv) == self.L - 1

    def omega(self, l):
        return self.w if l == 0 else self.w1

    def copy(self, **kw):
        c = Cycle.__new__(Cycle)
        c.__dict__.update(self.__dict__)
        c.__dict__.update(kw)
        return c


def block_diag(blocks):
    """(n, bs, bs) -> the block-diagonal CSR matrix."""
    blocks = np.asarray(blocks, dtype=np.float64)
    n = len(blocks)
    return sp.bsr_matrix((blocks, np.arange(n), np.arange(n + 1))).tocsr()


def _abs(M):
    return abs(sp.csr_matrix(M))


# ---- the stages, each on the vectors it reads -----------------------------------

def pre_smooth(c, l, b):
    """x = w D^-1 b."""
    return c.omega(l) * (c.Dinv[l] @ b)


def residual(c, l, b, x):
    """r = b - A x."""
    return b - c.A[l] @ x


def restrict(c, l, r):
    """b_{l+1} = P^T r_l."""
    return c.P[l].T @ r


def coarsest(c, b):
    """y = cinv b on the coarsest level."""
    return c.cinvT @ b


def prolong(c, l, x, y):
    """x_l + P y_{l+1}."""
    return x + c.P[l] @ y


def post_smooth(c, l, b, x):
    """y = x + w D^-1 (b - A x)."""
    return x + c.omega(l) * (c.Dinv[l] @ (b - c.A[l] @ x))


def ring_sweeps(c, r, x, sweeps=None):
    """`sweeps` damped block-Jacobi sweeps of level 0 on the ring rows alone;
    every other row keeps its x."""
    sweeps = c.sweeps if sweeps is None else sweeps
    x = np.array(x, dtype=np.float64)
    for _ in range(sweeps):
        full = post_smooth(c, 0, r, x)
        x = x.copy()
        x[c.ring] = full[c.ring]
    return x


def cycle(c, r, post=True):
    """z = M r: the stages composed with no rounding anywhere; r (dofs,) or
    (dofs, columns). post = False leaves every post-smoothing (and the ring
    sweeps after the correction) out: the negative control of the symmetry
    check."""
    r = np.asarray(r, dtype=np.float64)
    b, x = [r], []
    for l in range(c.L - 1):
        xl = pre_smooth(c, l, b[l])
        if l == 0 and c.sweeps:
            xl = ring_sweeps(c, r, xl)
        x.append(xl)
        b.append(restrict(c, l, residual(c, l, b[l], xl)))
    y = coarsest(c, b[-1])
    for l in range(c.L - 2, -1, -1):
        xl = prolong(c, l, x[l], y)
        if not post:
            y = xl
            continue
        if l == 0 and c.sweeps:
            xl = ring_sweeps(c, r, xl)
        y = post_smooth(c, l, b[l], xl)
    return y


def M_ref(c, post=True):
    """The cycle as a dense matrix."""
    return cycle(c, np.eye(c.A[0].shape[0]), post=post)


def asymmetry(M):
    """|M - M^T| / |M| in the Frobenius norm."""
    return float(np.linalg.norm(M - M.T) / np.linalg.norm(M))


def is_symmetric(M, tol=1e-12):
    return asymmetry(M) <= tol


# ---- the rounding bound of each stage ---------------------------------------------

def _k_rows(M):
    return np.diff(sp.csr_matrix(M).indptr).astype(np.float64)


def _col(k, v):
    return k if np.ndim(v) == 1 else k[:, None]


def bound_pre_smooth(c, l, b):
    """Level 0 (bf16_diag_solve: the determinant of bf16 entries -- exact
    products, one subtraction --, 1 / det, two products and a subtraction per
    row, the multiply by 1 / det and by w): k = 2, c = 6. Coarse levels (three
    products per row of the stored D^-1, the multiply by w1): k = 3, c = 1."""
    kc = 8 if l == 0 else 4
    return kc * U24 * c.omega(l) * (_abs(c.Dinv[l]) @ np.abs(b))


def bound_residual(c, l, b, x, beta_x=0.0):
    """k = the scalar products of the row (bs per stored block), c = 1 (the
    subtraction from b); + |A| beta_x where x itself is only known to beta_x."""
    k = _col(_k_rows(c.A[l]), b)
    Aa = _abs(c.A[l])
    out = (k + 1) * U24 * (np.abs(b) + Aa @ np.abs(x))
    return out + Aa @ beta_x if np.ndim(beta_x) else out


def bound_restrict(c, l, r):
    """k = the products of the coarse dof's column of P (bs per member or list
    entry), c = 1."""
    Pt = sp.csr_matrix(c.P[l].T)
    return (_col(_k_rows(Pt), r) + 1) * U24 * (_abs(Pt) @ np.abs(r))


def bound_coarsest(c, b):
    """k = nc products, c = 4: the partial sums of the four k ranges added."""
    return (len(c.cinvT) + 4) * U24 * (np.abs(c.cinvT) @ np.abs(b))


def bound_prolong(c, l, x, y, beta_x=0.0):
    """k = 3 per P block of the row, c = 2 (each block's sum added to x)."""
    k = _col(_k_rows(c.P[l]), x)
    return (k + 2) * U24 * (np.abs(x) + _abs(c.P[l]) @ np.abs(y)) + beta_x


def bound_post_smooth(c, l, b, x, beta_x=0.0):
    """The residual (k = the row's products, c = 1), D^-1 applied to it (level
    0: c = 5 as in bound_pre_smooth without w; coarse: k = 3), the multiply by
    w and the add to x (c = 2): w |D^-1| ((k + 8) u S + |A| beta_x) + beta_x
    + 2 u (|x| + w |D^-1| S) with S = |b| + |A| |x|."""
    k = _col(_k_rows(c.A[l]), b)
    Aa, Da, w = _abs(c.A[l]), _abs(c.Dinv[l]), c.omega(l)
    S = np.abs(b) + Aa @ np.abs(x)
    prop = Aa @ beta_x if np.ndim(beta_x) else 0.0
    return w * (Da @ ((k + 8) * U24 * S + prop)) + beta_x + 2 * U24 * (np.abs(x) + w * (Da @ S))


def bound_ring_sweeps(c, r, x, sweeps=None):
    """The sweeps' bounds chained: a sweep reads the previous one's fp32
    iterate, known to that sweep's bound on the ring rows and exactly
    elsewhere. Returns the bound of the last iterate (0 off the ring)."""
    sweeps = c.sweeps if sweeps is None else sweeps
    x = np.array(x, dtype=np.float64)
    beta = np.zeros_like(x)
    for _ in range(sweeps):
        full = post_smooth(c, 0, r, x)
        bfull = bound_post_smooth(c, 0, r, x, beta)
        x, beta = x.copy(), beta.copy()
        x[c.ring] = full[c.ring]
        beta[c.ring] = bfull[c.ring]
    return beta


# ---- comparing a stored value with its exact one ----------------------------------

def bf16_round(x):
    """fp64 -> the nearest bf16 value (through float32: both roundings are
    monotone, which is all the window needs)."""
    return R.bf16_value(R.bf16_bits(np.asarray(x, dtype=np.float64).astype(np.float32))).astype(np.float64)


def check_bf16(got, e, beta):
    """A value stored as bf16 whose fp32 original lies within beta of e must lie
    between bf16(e - beta) and bf16(e + beta): a flipped rounding and nothing
    more. Returns (ok mask, fraction of windows that span two bf16 values,
    largest |got - e| / (beta + half a bf16 ulp of e))."""
    got = np.asarray(got, dtype=np.float64)
    lo, hi = bf16_round(e - beta), bf16_round(e + beta)
    ok = (got >= lo) & (got <= hi)
    den = beta + 0.5 * R.bf16_ulp(e)
    ratio = np.where(den > 0, np.abs(got - e) / np.where(den > 0, den, 1.0), np.where(got != e, np.inf, 0.0))
    return ok, float((lo != hi).mean()) if lo.size else 0.0, float(ratio.max()) if ratio.size else 0.0


def check_f32(got, e, beta):
    """A value stored as fp32: |got - e| <= beta (the final rounding is one of
    the bound's c). Returns (ok mask, 0.0, largest error / bound)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - e)
    ratio = np.where(beta > 0, err / np.where(beta > 0, beta, 1.0), np.where(err > 0, np.inf, 0.0))
    return err <= beta, 0.0, float(ratio.max()) if ratio.size else 0.0
