"""tests/pcg_ref.py checked on the CPU: its exact iteration against a textbook
dense PCG, its bounds against a float32 emulation of the device's order of
operations, the stop rule and the outer check against hand-worked values, and
the negative controls of tests/test_gpu_pcg.py on the emulated states."""
import numpy as np
import pytest
import scipy.sparse as sp

import amg_ref as R
import pcg_ref as P

N = 70  # two SELL slices, the second with 6 rows


def ring_level(n=N, seed=3):
    """A ring graph (row i holds i - 1, i, i + 1) in SELL-64 with symmetric
    reads: the diagonal and upper blocks stored, every lower position a mirror
    entry of its upper twin. Returns (level tables, blocks, dense SPD matrix)."""
    rng = np.random.default_rng(seed)
    ns = (n + 63) // 64
    off = np.arange(ns + 1) * 3 * 64
    nb = int(off[-1])
    col = np.zeros(nb, dtype=np.int32)
    mir = np.full(nb, -1, dtype=np.int32)
    blocks = np.zeros((nb, 2, 2))
    pos = {}
    for i in range(n):
        s, l = divmod(i, 64)
        for t, j in enumerate(sorted({(i - 1) % n, i, (i + 1) % n})):
            q = off[s] + t * 64 + l
            col[q] = j
            pos[i, j] = q
    dense = np.zeros((2 * n, 2 * n))
    for (i, j), q in pos.items():
        if j > i:
            blocks[q] = 0.3 * rng.standard_normal((2, 2))
        elif j == i:
            a = rng.standard_normal((2, 2))
            blocks[q] = 3.0 * np.eye(2) + 0.2 * (a + a.T)
    for (i, j), q in pos.items():
        if j >= i:
            mir[q] = q
            dense[2 * i:2 * i + 2, 2 * j:2 * j + 2] = blocks[q]
        else:
            mir[q] = pos[j, i] | R.MIR_T
            dense[2 * i:2 * i + 2, 2 * j:2 * j + 2] = blocks[pos[j, i]].T
    return {"sell_off": off, "sell_col": col, "mirror": mir, "n": n}, blocks, dense


@pytest.fixture(scope="module")
def ring():
    t, blocks, dense = ring_level()
    lev = P.level0(t["sell_off"], t["sell_col"], t["mirror"], t["n"], sym=True)
    op = P.Op(lev, blocks)
    dinv = np.linalg.inv(np.stack([dense[2 * i:2 * i + 2, 2 * i:2 * i + 2] for i in range(N)]))
    b = np.random.default_rng(5).standard_normal(2 * N)
    return {"tables": t, "lev": lev, "blocks": blocks, "dense": dense, "op": op, "dinv": dinv, "b": b}


def test_operator_from_sell(ring):
    op, dense = ring["op"], ring["dense"]
    assert np.array_equal(op.A.toarray(), dense) and np.array_equal(dense, dense.T)
    assert np.linalg.eigvalsh(dense).min() > 0
    assert (op.w == 3).all() and op.n == 2 * N
    # plain reads: every block at its own position, the lower ones stored transposed there
    t, blocks = ring["tables"], ring["blocks"].copy()
    low = (t["mirror"] >= 0) & ((t["mirror"] & R.MIR_T) != 0)
    blocks[low] = blocks[t["mirror"][low] & R.MIR_POS].transpose(0, 2, 1)
    plain = P.Op(P.level0(t["sell_off"], t["sell_col"], t["mirror"], N, sym=False), blocks)
    assert np.array_equal(plain.A.toarray(), dense)
    # one lower block left untransposed: no longer symmetric, one block differs
    bad = P.Op(P.untranspose_one(ring["lev"], ring["blocks"]), ring["blocks"]).A.toarray()
    assert (bad != dense).sum() in (1, 2) and not np.array_equal(bad, bad.T)
    assert np.array_equal(P.from_csr(sp.csr_matrix(dense)).w, op.w)


def test_exact_iteration_is_textbook_pcg(ring):
    """The reference's iteration, stage after stage with no rounding, against
    dense Hestenes-Stiefel PCG with the same preconditioner: 1e-12 relative."""
    op, dinv, b, dense = ring["op"], ring["dinv"], ring["b"], ring["dense"]
    Minv = np.zeros_like(dense)
    for i in range(N):
        Minv[2 * i:2 * i + 2, 2 * i:2 * i + 2] = dinv[i]
    pre = lambda r: P.jacobi_z(dinv, r, P.U53)[0]  # noqa: E731
    want = P.textbook_pcg(dense, b, Minv, 12)
    st = P.start(op, b, pre)
    for k in range(12):
        st = P.iterate(op, st, pre)
        x = P.finish(st)["x"]
        assert np.linalg.norm(x - want[k][0]) <= 1e-12 * np.linalg.norm(want[k][0]), k
        assert np.linalg.norm(st["r"] - want[k][1]) <= 1e-12 * np.linalg.norm(b), k
    assert np.linalg.norm(b - dense @ x) < 1e-6 * np.linalg.norm(b)


def emulate(op, dinv, b, cap, tol2=None, rtol=1e-3, dtype=np.float32, drop_last_x=False, nown=None):
    """The device's inner solve in its own order and the working type (sums in
    fp64): the state pcg() leaves after cap iterations and the check launch."""
    T = np.dtype(dtype).type
    A = op.A.astype(dtype)
    d = np.asarray(dinv, dtype=dtype)
    n_own = op.n if nown is None else 2 * nown
    r = np.asarray(b, dtype=np.float64).astype(dtype)
    r[n_own:] = 0

    def pre(v):
        v2 = v.reshape(-1, 2)
        return np.stack([d[:, 0, 0] * v2[:, 0] + d[:, 0, 1] * v2[:, 1], d[:, 1, 0] * v2[:, 0] + d[:, 1, 1] * v2[:, 1]],
                        axis=1).ravel().astype(dtype)

    def dot(u, v):
        return float((u[:n_own].astype(np.float64) * v[:n_own].astype(np.float64)).sum())

    x, z = np.zeros(op.n, dtype=dtype), pre(r)
    p, q = np.zeros(op.n, dtype=dtype), np.zeros(op.n, dtype=dtype)
    scal = np.zeros((2, 3))
    scal[0, :2] = dot(r, z), dot(r, r)
    if tol2 is None:
        tol2 = rtol * rtol * scal[0, 1]
    conv, alpha = -1, T(0)
    for it in range(cap + 1):
        cur, old = scal[it & 1], scal[(it + 1) & 1]
        if it > 0:
            alpha = T(old[0] / old[2])
        if cur[1] <= tol2:
            if it > 0 and not drop_last_x:
                x = x + alpha * p
            conv = it
            break
        if it == 0:
            p, q = z.copy(), (A @ z).astype(dtype)
        else:
            beta = T(cur[0] / old[0])
            q = ((A @ z).astype(dtype) + beta * q).astype(dtype)
            if not (drop_last_x and it == cap):
                x = (x + alpha * p).astype(dtype)
            p = (z + beta * p).astype(dtype)
        cur[2] = dot(p, q)
        if it == cap:
            break
        a = T(cur[0] / cur[2])
        r = (r - a * q).astype(dtype)
        r[n_own:] = 0
        z = pre(r)
        scal[(it + 1) & 1, :2] = dot(r, z), dot(r, r)
    f = lambda v: v.astype(np.float64)  # noqa: E731
    return {"x": f(x), "r": f(r), "z": f(z), "p": f(p), "q": f(q), "scal": scal.copy(), "conv": conv, "tol2": tol2}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_stage_bounds_hold_on_the_emulation(ring, dtype):
    """Every stage check of the chain passes on states computed in the working
    type in the device's order, with error / bound below 1, and the drift's
    accumulated bound holds at every cap -- at the step a system stops too."""
    op, dinv, b = ring["op"], ring["dinv"], ring["b"]
    rtol = 1e-3 if dtype == np.float32 else 1e-9
    S = [emulate(op, dinv, b, K, rtol=rtol, dtype=dtype) for K in range(40)]
    conv = S[-1]["conv"]
    assert 3 < conv < 38 and all(s["conv"] == (-1 if k < conv else conv) for k, s in enumerate(S))
    recs, bq = P.check_first(op, b, S[0], dtype, dinv)
    assert not P.failing(recs), recs
    worst = max(r for _, _, r in recs)
    drift = P.Drift(op, b, P.unit(dtype))
    drift.spmv(0.0, bq, np.zeros(op.n), np.zeros(op.n))
    for K in range(conv):
        recs, info = P.check_step(op, S[K], S[K + 1], K, dtype, dinv)
        assert not P.failing(recs), (K, recs)
        worst = max([worst] + [r for _, _, r in recs])
        drift.update(info["alpha"], info["br"])
        drift.spmv(info["beta"], info["bq"], info["bp"], info["bx"])
        gap = P.true_residual_gap(op, b, S[K + 1]["x"], S[K + 1]["r"])
        assert (gap <= drift.E).all(), (K, float((gap / drift.E).max()))
        assert info["stopped"] == (K + 1 == conv)
    assert worst <= 1.0 and (worst > 0.0 or dtype == np.float64)  # in fp64 numpy rounds as the reference does
    for s in S[conv + 1:]:  # a stopped system's state is final
        assert all(np.array_equal(s[k], S[conv][k]) for k in "xrzpq")
    assert P.conv_step([s["scal"][k & 1][1] for k, s in enumerate(S[:conv + 1])], S[0]["tol2"]) == conv


def test_negative_controls_on_the_emulation(ring):
    """Each way the reference can be wrong is reported by its own stage."""
    op, dinv, b, dt = ring["op"], ring["dinv"], ring["b"], np.float32
    S = [emulate(op, dinv, b, K, tol2=0.0) for K in range(6)]
    K = 3
    good, info = P.check_step(op, S[K], S[K + 1], K, dt, dinv)
    assert not P.failing(good)
    assert P.failing(P.check_step(op, S[K], S[K + 1], K, dt, dinv, control="beta_slot")[0]) == \
        {"p = z + beta p", "q = A z + beta q"}
    assert P.failing(P.check_step(op, S[K], S[K + 1], K, dt, dinv, control="drop_x")[0]) == {"x += alpha p"}
    assert P.failing(P.check_step(op, S[K], S[K + 1], K, dt, dinv, control="pq_row")[0]) == {"p.q"}
    bad = P.Op(P.untranspose_one(ring["lev"], ring["blocks"]), ring["blocks"])
    assert P.failing(P.check_step(bad, S[K], S[K + 1], K, dt, dinv)[0]) == {"q = A z + beta q"}
    assert P.failing(P.check_first(bad, b, S[0], dt, dinv)[0]) == {"q = A z"}
    # the invariant: a state whose last deferred x update was lost
    drift = P.Drift(op, b, P.U24)
    drift.spmv(0.0, P.check_first(op, b, S[0], dt, dinv)[1], np.zeros(op.n), np.zeros(op.n))
    for k in range(5):
        _, info = P.check_step(op, S[k], S[k + 1], k, dt, dinv)
        drift.update(info["alpha"], info["br"])
        drift.spmv(info["beta"], info["bq"], info["bp"], info["bx"])
    assert (P.true_residual_gap(op, b, S[5]["x"], S[5]["r"]) <= drift.E).all()
    lost = emulate(op, dinv, b, 5, tol2=0.0, drop_last_x=True)
    assert np.array_equal(lost["r"], S[5]["r"]) and not np.array_equal(lost["x"], S[5]["x"])
    gap = P.true_residual_gap(op, b, lost["x"], lost["r"])
    assert (gap > drift.E).any() and (gap / drift.E).max() > 100.0


def test_ghost_rows_are_not_summed(ring):
    """nown < N: r is 0 on the rows past it and the three sums leave them out."""
    op, dinv, b = ring["op"], ring["dinv"], ring["b"]
    nown = N - 5
    S = [emulate(op, dinv, b, K, tol2=0.0, nown=nown) for K in range(4)]
    assert (S[3]["r"][2 * nown:] == 0).all() and (S[3]["q"][2 * nown:] != 0).any()
    assert not P.failing(P.check_first(op, b, S[0], np.float32, dinv, nown=nown)[0])
    for K in range(3):
        assert not P.failing(P.check_step(op, S[K], S[K + 1], K, np.float32, dinv, nown=nown)[0])
        # a reference that updates r on the ghost rows too disagrees there (their z and p stay 0, so
        # the sums cannot tell)
        assert "r -= alpha q" in P.failing(P.check_step(op, S[K], S[K + 1], K, np.float32, dinv)[0])


def test_bound_helpers():
    rng = np.random.default_rng(11)
    a, c = rng.standard_normal(4000), rng.standard_normal(4000)
    f = np.float32
    got = (a.astype(f) + f(0.37) * c.astype(f)).astype(np.float64)
    e, beta = P.axpy(a.astype(f), float(f(0.37)), c.astype(f), P.U24)
    ok, ratio = P.within(got, e, beta)
    assert ok and 0 < ratio <= 1.0
    assert not P.within(got + 3 * beta, e, beta)[0]
    assert P.within(np.array([1.0]), np.array([1.0]), np.array([0.0])) == (True, 0.0)
    assert P.within(np.array([1.0 + 1e-16 * 8]), np.array([1.0]), np.array([0.0]))[0] is False
    assert not P.within(np.array([np.nan]), np.array([1.0]), np.array([1.0]))[0]
    # an fp64 sum of float products in a scrambled order
    af, cf = a.astype(f).astype(np.float64), c.astype(f).astype(np.float64)
    e, beta = P.dot(af, cf)
    perm = rng.permutation(4000)
    acc = 0.0
    for t in (af * cf)[perm]:
        acc += t
    assert abs(acc - e) <= beta and beta < 1e-11 * np.abs(af * cf).sum()
    assert P.dot(af, cf, nown=1000)[0] == (af[:2000] * cf[:2000]).sum()
    assert P.dot(af, cf, exact_products=False)[1] > beta
    # alpha, beta: one rounding of the fp64 quotient
    assert P.quot(1.0, 3.0, np.float32) == float(np.float32(1.0 / 3.0)) and P.quot(1.0, 3.0, np.float64) == 1.0 / 3.0
    d = rng.standard_normal((50, 2, 2)).astype(f)
    r = rng.standard_normal(100).astype(f)
    got = np.stack([d[:, 0, 0] * r[0::2] + d[:, 0, 1] * r[1::2], d[:, 1, 0] * r[0::2] + d[:, 1, 1] * r[1::2]], 1).ravel()
    ok, ratio = P.within(got.astype(np.float64), *P.jacobi_z(d, r, P.U24))
    assert ok and 0 < ratio <= 1.0


def test_stop_rule():
    # k_pcg_tol
    assert P.inner_tol(1e-4, 0.0, 1e-7, 1.0, 1e-6, 1.0, 1.0) == 1e-4                   # the first step
    assert P.inner_tol(1e-4, 1e-8, 0.0, 1.0, 1e-12, 0.0, 0.0) == pytest.approx(3e-3)   # 0.3 rtol |f| / |r|
    assert P.inner_tol(1e-4, 1e-8, 0.0, 1.0, 1e-18, 0.0, 0.0) == 0.5                   # capped
    assert P.inner_tol(1e-4, 1e-8, 0.0, 1.0, 1e-6, 0.0, 0.0) == 1e-4                   # never below rtol
    assert P.inner_tol(1e-4, 1e-8, 1e-7, 1.0, 1e-14, 1e-5, 2.0) == pytest.approx(0.5 * 1e-7 * 2.0 / (2.0 * 1e-5))
    assert P.inner_tol(1e-4, 1e-8, 1e-7, 0.0, 1e-12, 1e-5, 2.0) == 1e-4                # |f| = 0: rtol
    assert P.tol2(0.5, 8.0) == 2.0
    # SI_CONV, SD_BEST / SI_BEST_IT
    assert P.conv_step([4.0, 2.0, 1.0, 0.5], 1.0) == 2 and P.conv_step([4.0, 2.0], 1.0) is None
    assert P.conv_step([0.0], 0.0) == 0
    assert P.best([4.0, 5.0, 3.0, 3.0, 3.5]) == (3.0, 2) and P.best([4.0]) == (4.0, 0)
    # k_outer_check
    rel, est, met, ret = P.outer_check(1e-18, 1.0, 1e-3, 2.0, 0.0, True, 1e-8, 1e-7)
    assert rel == pytest.approx(1e-9) and est == pytest.approx(1e-12) and met and ret
    rel, est, met, ret = P.outer_check(1e-18, 1.0, 1e-3, 2.0, 1e-14, False, 1e-8, 1e-7)
    assert est == pytest.approx(1e-5) and met and not ret      # the residual met, the error estimate not
    assert P.outer_check(1e-18, 1.0, 1e-3, 2.0, 1e-14, False, 1e-8, 0.0)[3]   # no error control
    assert P.outer_check(1e-14, 1.0, 1e-3, 2.0, 1e-10, False, 1e-8, 1e-7)[2:] == (False, False)
    assert P.outer_check(0.0, 0.0, 0.0, 0.0, 0.0, True, 1e-8, 1e-7) == (0.0, 0.0, True, True)   # f = 0
    assert P.outer_check(1.0, 0.0, 0.0, 0.0, 0.0, True, 1e-8, 1e-7)[0] == np.inf
