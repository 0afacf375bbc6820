"""tests/dd_ref.py checked on the CPU: the restated plan against the library's
host plan (counts) and against its own definition, the packed exchange against
the plain copy, the lockstep iteration in exact arithmetic against dense
textbook PCG with the matching preconditioner (1e-12 relative over 10 steps,
test_pcg_ref.py's bar), and every negative control of
tests/test_gpu_dd_kernels.py against the bound of the check it belongs to."""
import numpy as np
import pytest
import scipy.sparse as sp

import dd_ref as D
import pcg_ref as P
from mofhip import plan_info, synth

NPARTS = 3
STEPS = 10


def build_case():
    """A small SPD matrix of 2 x 2 blocks on the vertex graph of a mesh (A =
    G^T G + I, G one block row per edge), a random 3-way vertex partition, the
    parts' local matrices with decoupled ghost rows."""
    pts, tri = synth.icosphere(3)
    N = len(pts)
    rng = np.random.default_rng(17)
    edges = sorted({tuple(sorted((int(t[a]), int(t[b])))) for t in tri for a, b in ((0, 1), (1, 2), (0, 2))})
    G = sp.lil_matrix((2 * len(edges), 2 * N))
    for e, (i, j) in enumerate(edges):
        G[2 * e:2 * e + 2, 2 * i:2 * i + 2] = rng.standard_normal((2, 2))
        G[2 * e:2 * e + 2, 2 * j:2 * j + 2] = rng.standard_normal((2, 2))
    A = sp.csr_matrix(G.T @ G + sp.identity(2 * N))
    part = rng.integers(0, NPARTS, N).astype(np.int32)
    own = [np.flatnonzero(part == p) for p in range(NPARTS)]
    plan = D.restated_plan(tri, N, part, own)
    ops = [P.from_csr(D.local_matrix(A, d)) for d in plan]
    b = rng.standard_normal(2 * N)
    bl = [np.stack([b[2 * d["l2g"]], b[2 * d["l2g"] + 1]], axis=1).ravel() for d in plan]
    return {"tri": tri, "N": N, "A": A, "dense": A.toarray(), "part": part, "plan": plan, "ops": ops, "b": b, "bl": bl}


@pytest.fixture(scope="module")
def case():
    return build_case()


def test_plan_restatement(case):
    """The restated counts are the library's host plan's; every ghost appears in
    exactly one send list at the position its receiver expects; ghosts are
    grouped by owner with ascending source rows; a ghost's owner row is the same
    caller vertex."""
    plan, tri, N, part = case["plan"], case["tri"], case["N"], case["part"]
    info = plan_info(tri, N, part)
    assert np.array_equal(info["n_own"], [d["n_own"] for d in plan])
    assert np.array_equal(info["n_ghost"], [d["n_ghost"] for d in plan])
    assert np.array_equal(info["n_nbr"], [len(d["nbr"]) for d in plan])
    assert np.array_equal(info["n_tri"], [d["n_tri"] for d in plan])
    assert np.array_equal(info["n_send"], [len(d["send_idx"]) for d in plan])
    pos = D.ghost_positions(plan)
    assert sorted(pos) == [(p, g) for p, d in enumerate(plan) for g in range(d["n_ghost"])]
    for (p, g), where in pos.items():
        assert len(where) == 1
        q, e = where[0]
        d = plan[p]
        assert q == d["ghost_owner"][g] and plan[q]["send_idx"][e] == d["ghost_src"][g]
        assert plan[q]["l2g"][d["ghost_src"][g]] == d["l2g"][d["n_own"] + g]
    for d in plan:
        key = list(zip(d["ghost_owner"].tolist(), d["ghost_src"].tolist()))
        assert key == sorted(key) and len(set(key)) == len(key)
    assert not D.plan_mismatches(plan, plan)
    other = [dict(d) for d in plan]
    other[1]["ghost_src"] = np.roll(other[1]["ghost_src"], 1)
    assert D.plan_mismatches(other, plan) == [(1, "ghost_src")]


@pytest.mark.parametrize("B", [1, 3])
def test_packed_exchange_is_the_copy(case, B):
    plan = case["plan"]
    vecs = D.coded(plan, B)
    a, b = D.halo(plan, vecs), D.halo_staged(plan, vecs)
    for d, v, x, y in zip(plan, vecs, a, b):
        assert np.array_equal(x, y) and np.array_equal(x[:, :d["n_own"]], v[:, :d["n_own"]])
        for g in range(d["n_ghost"]):
            assert np.array_equal(x[:, d["n_own"] + g], vecs[d["ghost_owner"][g]][:, d["ghost_src"][g]])
    # all values distinct and exact in float32: a wrong row cannot pass for the right one
    allv = np.concatenate([v.ravel() for v in vecs])
    assert len(np.unique(allv)) == allv.size and np.array_equal(allv.astype(np.float32).astype(np.float64), allv)
    # segment k of a part starts at element 2 B send_off[k]
    d = plan[0]
    buf = D.pack(d, vecs[0])
    for k in range(len(d["nbr"])):
        a0, a1 = d["send_off"][k], d["send_off"][k + 1]
        assert np.array_equal(buf[2 * B * a0:2 * B * a1].reshape(B, a1 - a0, 2), vecs[0][:, d["send_idx"][a0:a1]])
    V, hits = D.gather(plan, case["N"], vecs, failed=[True] + [False] * (B - 1))
    assert (hits == 1).all() and np.isnan(V[0]).all() and not np.isnan(V[1:]).any()


def preconditioners(case):
    """Block Jacobi (D^-1) and the part-multigrid model: each part's exact solve
    on its owned rows, block diagonal over the parts."""
    plan, dense, N = case["plan"], case["dense"], case["N"]
    dinv = np.stack([np.linalg.inv(dense[2 * i:2 * i + 2, 2 * i:2 * i + 2]) for i in range(N)])
    Mj = np.zeros_like(dense)
    for i in range(N):
        Mj[2 * i:2 * i + 2, 2 * i:2 * i + 2] = dinv[i]
    jac = lambda p, r: P.jacobi_z(dinv[plan[p]["l2g"]], r, P.U53)[0]  # noqa: E731
    Mb = np.zeros_like(dense)
    inv = []
    for d in plan:
        own = d["l2g"][:d["n_own"]]
        idx = np.stack([2 * own, 2 * own + 1], axis=1).ravel()
        inv.append(np.linalg.inv(dense[np.ix_(idx, idx)]))
        Mb[np.ix_(idx, idx)] = inv[-1]

    def blk(p, r):
        z = np.full(len(r), np.nan)   # the cycle's ghost rows are never read: the halo replaces them
        z[:2 * plan[p]["n_own"]] = inv[p] @ r[:2 * plan[p]["n_own"]]
        return z
    return {"jacobi": (jac, Mj), "part solve": (blk, Mb)}


@pytest.mark.parametrize("which", ["jacobi", "part solve"])
def test_lockstep_iteration_is_textbook_pcg(case, which):
    plan, ops, N = case["plan"], case["ops"], case["N"]
    pre, Minv = preconditioners(case)[which]
    want = P.textbook_pcg(case["dense"], case["b"], Minv, STEPS)
    st = D.start(plan, ops, case["bl"], pre)
    for k in range(STEPS):
        st = D.iterate(plan, ops, st, pre)
        x = D.to_global(plan, N, D.finish(st)["x"])
        r = D.to_global(plan, N, st["r"])
        assert np.linalg.norm(x - want[k][0]) <= 1e-12 * np.linalg.norm(want[k][0]), k
        assert np.linalg.norm(r - want[k][1]) <= 1e-12 * np.linalg.norm(case["b"]), k
        for d, rp in zip(plan, st["r"]):
            assert (rp[2 * d["n_own"]:] == 0).all()
        # ghost p is the owner's p, from ghost z and the global beta alone
        ph = D.halo(plan, st["p"])
        assert all(np.array_equal(a, b) for a, b in zip(ph, st["p"])), k


def test_negative_controls_exceed_their_bounds(case):
    """Each control changes what its check compares by more than the check's
    fp32 bound (pcg_ref's row, sum), from a state three steps in."""
    plan, ops = case["plan"], case["ops"]
    pre, _ = preconditioners(case)["jacobi"]
    st = D.start(plan, ops, case["bl"], pre, np.float32)
    for _ in range(3):
        st = D.iterate(plan, ops, st, pre, np.float32)
    good = D.iterate(plan, ops, st, pre, np.float32)
    z = D.halo(plan, st["z"])
    beta = good["beta"]
    p = 1
    bq = P.q_step(ops[p], z[p], beta, st["q"][p], P.U24)[1]
    # stale ghosts for one step / one ghost from the neighbouring owner row: the row product
    for control in (("stale", p), ("wrong_row", p, 0)):
        bad = D.iterate(plan, ops, st, pre, np.float32, control=control)
        assert (np.abs(bad["q"][p] - good["q"][p]) > bq).any(), control
        assert all(np.array_equal(bad["q"][o], good["q"][o]) for o in range(NPARTS) if o != p)
    # ghost rows in p.q / a part's records left out: the sum
    pq, bound = D.owned_sum(plan, good["p"], good["q"])
    assert pq == good["pq"]
    for kw in ({"ghost_part": p}, {"drop_part": p}):
        assert abs(D.owned_sum(plan, good["p"], good["q"], **kw)[0] - pq) > bound, kw
    for control in (("pq_ghost", p), ("drop_part", p)):
        assert D.iterate(plan, ops, st, pre, np.float32, control=control)["pq"] != good["pq"]
    # a ghost block left coupled: the part's preconditioner is no longer the owned rows' Dirichlet
    # problem, and the iterate leaves textbook PCG's by far more than the 1e-12 the right one is held to
    _, Mb = preconditioners(case)["part solve"]
    want = P.textbook_pcg(case["dense"], case["b"], Mb, 2)

    def solve_with(couple):
        loc = [D.local_matrix(case["A"], d, couple_ghost=0 if couple and k == p else None).toarray()
               for k, d in enumerate(plan)]
        pre2 = lambda k, r: np.linalg.solve(loc[k], r)  # noqa: E731
        s = D.start(plan, ops, case["bl"], pre2)
        for _ in range(2):
            s = D.iterate(plan, ops, s, pre2)
        return D.to_global(plan, case["N"], D.finish(s)["x"])
    ref = np.linalg.norm(want[1][0])
    assert np.linalg.norm(solve_with(False) - want[1][0]) <= 1e-12 * ref
    assert np.linalg.norm(solve_with(True) - want[1][0]) > 1e-6 * ref
