"""tests/vcycle_ref.py (the fp64 restatement of the multigrid V-cycle the GPU
tests compare the kernels with) checked on the CPU: on a small SPD block
matrix with hand-made aggregates the stages compose to M_ref, the cycle is the
textbook two-grid / V(1,1) error propagation, and it is symmetric exactly when
the post-smoothing mirrors the pre-smoothing."""
import numpy as np
import scipy.sparse as sp

import amg_ref as R
import vcycle_ref as V


def block_inverse(A, bs):
    n = A.shape[0] // bs
    D = np.stack([A[bs * i:bs * i + bs, bs * i:bs * i + bs].toarray() for i in range(n)])
    return V.block_diag(np.linalg.inv(D))


def hierarchy(levels=3, ring=False):
    """A 6 x 6 grid of nodes with 2 dofs each, an SPD operator (a graph
    Laplacian plus a mass term, times a 2 x 2 SPD block, plus a random
    symmetric perturbation), 2 x 2-node aggregates with three coarse dofs each
    (the two constants and a rotation-like mode), then the nine coarse nodes
    in three aggregates of three. Exact Galerkin operators and coarse solve."""
    rng = np.random.default_rng(7)
    g = 6
    idx = np.arange(g * g).reshape(g, g)
    e = np.concatenate([np.column_stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()]),
                        np.column_stack([idx[:-1, :].ravel(), idx[1:, :].ravel()])])
    W = sp.coo_matrix((rng.uniform(0.5, 1.5, len(e)), (e[:, 0], e[:, 1])), shape=(g * g, g * g))
    W = W + W.T
    Lap = sp.diags(np.asarray(W.sum(axis=1)).ravel() + 0.3) - W
    A0 = sp.kron(Lap, np.array([[2.0, 0.5], [0.5, 1.0]])).tocsr()
    K = sp.kron(abs(Lap) > 0, np.ones((2, 2))).multiply(sp.random(2 * g * g, 2 * g * g, 1.0, random_state=3))
    A0 = (A0 + 0.02 * (K + K.T)).tocsr()
    assert np.linalg.eigvalsh(A0.toarray()).min() > 0
    agg0 = ((np.arange(g * g) // g) // 2) * 3 + (np.arange(g * g) % g) // 2  # 2 x 2 squares
    xy = np.column_stack([np.arange(g * g) // g, np.arange(g * g) % g]).astype(np.float64)
    rows, cols, vals = [], [], []
    for i in range(g * g):
        d = xy[i] - xy[agg0 == agg0[i]].mean(axis=0)
        blk = np.array([[1.0, 0.0, -d[1]], [0.0, 1.0, d[0]]]) * 0.5
        for r in range(2):
            for k in range(3):
                rows.append(2 * i + r), cols.append(3 * agg0[i] + k), vals.append(blk[r, k])
    P0 = sp.coo_matrix((vals, (rows, cols)), shape=(2 * g * g, 27)).tocsr()
    A1 = (P0.T @ A0 @ P0).tocsr()
    if levels == 2:
        A, P = [A0, A1], [P0]
    else:
        agg1 = np.arange(9) // 3
        rows, cols, vals = [], [], []
        for i in range(9):
            blk = np.eye(3) / np.sqrt(3.0) + 0.1 * rng.standard_normal((3, 3))
            for r in range(3):
                for k in range(3):
                    rows.append(3 * i + r), cols.append(3 * agg1[i] + k), vals.append(blk[r, k])
        P1 = sp.coo_matrix((vals, (rows, cols)), shape=(27, 9)).tocsr()
        A, P = [A0, A1, (P1.T @ A1 @ P1).tocsr()], [P0, P1]
    Dinv = [block_inverse(a, 2 if l == 0 else 3) for l, a in enumerate(A[:-1])]
    rg = None
    if ring:  # the grid's outer two rings of nodes
        on = (np.minimum(xy, g - 1 - xy).min(axis=1) <= 1)
        rg = np.flatnonzero(np.repeat(on, 2))
    return V.Cycle(A, Dinv, P, np.linalg.inv(A[-1].toarray()).T, 0.7, 1.1, ring=rg, sweeps=2 if ring else 0)


def by_hand(c, r):
    """The cycle of a three-level hierarchy written out stage by stage."""
    x0 = V.pre_smooth(c, 0, r)
    if c.sweeps:
        x0 = V.ring_sweeps(c, r, x0)
    b1 = V.restrict(c, 0, V.residual(c, 0, r, x0))
    x1 = V.pre_smooth(c, 1, b1)
    b2 = V.restrict(c, 1, V.residual(c, 1, b1, x1))
    y2 = V.coarsest(c, b2)
    y1 = V.post_smooth(c, 1, b1, V.prolong(c, 1, x1, y2))
    x = V.prolong(c, 0, x0, y1)
    if c.sweeps:
        x = V.ring_sweeps(c, r, x)
    return V.post_smooth(c, 0, r, x)


def test_stages_compose_to_M_ref():
    rng = np.random.default_rng(1)
    for ring in (False, True):
        c = hierarchy(3, ring)
        M = V.M_ref(c)
        r = rng.standard_normal((M.shape[0], 5))
        z = by_hand(c, r)
        assert np.abs(z - M @ r).max() <= 1e-12 * np.abs(z).max()
        assert np.abs(by_hand(c, r[:, 0]) - z[:, 0]).max() <= 1e-12 * np.abs(z).max()  # a single vector too


def test_two_grid_error_propagation():
    """I - M A = (I - w D^-1 A)(I - P (P^T A P)^-1 P^T A)(I - w D^-1 A)."""
    c = hierarchy(2)
    A = c.A[0].toarray()
    P = c.P[0].toarray()
    n = len(A)
    S = np.eye(n) - c.w * c.Dinv[0].toarray() @ A
    C = np.eye(n) - P @ np.linalg.inv(P.T @ A @ P) @ P.T @ A
    E = np.eye(n) - V.M_ref(c) @ A
    assert np.abs(E - S @ C @ S).max() <= 1e-12 * np.abs(E).max()


def test_three_level_error_propagation():
    """The same with the coarse solve replaced by level 1's own cycle M1 (its
    damping w1 on both of its levels): I - M A = S (I - P M1 P^T A) S."""
    c = hierarchy(3)
    c1 = V.Cycle(c.A[1:], c.Dinv[1:], c.P[1:], c.cinvT, c.w1, c.w1)
    A, P = c.A[0].toarray(), c.P[0].toarray()
    n = len(A)
    S = np.eye(n) - c.w * c.Dinv[0].toarray() @ A
    E = np.eye(n) - V.M_ref(c) @ A
    want = S @ (np.eye(n) - P @ V.M_ref(c1) @ P.T @ A) @ S
    assert np.abs(E - want).max() <= 1e-12 * np.abs(E).max()
    assert np.abs(np.linalg.eigvals(E)).max() < 1  # and it contracts


def test_M_ref_is_symmetric_positive_definite():
    for levels, ring in ((2, False), (3, False), (3, True)):
        M = V.M_ref(hierarchy(levels, ring))
        assert V.is_symmetric(M), V.asymmetry(M)
        assert np.linalg.eigvalsh(0.5 * (M + M.T)).min() > 0


def test_symmetry_check_notices_a_dropped_post_smoothing():
    for ring in (False, True):
        c = hierarchy(3, ring)
        M = V.M_ref(c, post=False)
        assert V.asymmetry(M) > 1e-3 and not V.is_symmetric(M)
    # ... and one ring sweep before against two after
    c = hierarchy(3, True)
    r = np.eye(c.A[0].shape[0])
    x0 = V.ring_sweeps(c, r, V.pre_smooth(c, 0, r), sweeps=1)
    M2 = V.cycle(c, r)
    assert V.is_symmetric(M2)
    b1 = V.restrict(c, 0, V.residual(c, 0, r, x0))
    c1 = V.Cycle(c.A[1:], c.Dinv[1:], c.P[1:], c.cinvT, c.w1, c.w1)
    x = V.ring_sweeps(c, r, V.prolong(c, 0, x0, V.cycle(c1, b1)))
    assert not V.is_symmetric(V.post_smooth(c, 0, r, x))


def test_bf16_window():
    """check_bf16 admits a flipped rounding and nothing more."""
    e = np.array([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8, 3.0, 0.0])     # a tie between 1 and 1 + 2^-7
    got = R.bf16_value(R.bf16_bits(np.array([1.0, 1.0 + 2.0 ** -7, 3.0, 0.0], dtype=np.float32)))
    beta = np.array([1e-6, 1e-6, 1e-6, 0.0])
    ok, two, _ = V.check_bf16(got, e, beta)
    assert ok.all() and two == 0.5
    ok, _, _ = V.check_bf16(got + np.array([0.0, 2.0 ** -7, 2.0 ** -6, 2.0 ** -126]), e, beta)
    assert ok.tolist() == [True, False, False, False]
    ok, _, ratio = V.check_f32(np.array([1.0, 2.0]), np.array([1.0 + 1e-7, 2.0]), np.array([2e-7, 0.0]))
    assert ok.all() and abs(ratio - 0.5) < 1e-6
