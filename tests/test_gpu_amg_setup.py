"""The multigrid's per-timestep setup (amg_setup_batch: the Galerkin products,
st_pair, D^-1, the int8 sweep copy, the coarsest inverse) against the fp64
checker tests/amg_ref.py, level by level.

Every case builds a handle, runs one multigrid solve of exactly one batch and
reads back what the setup left for a few systems of it (mof_test_amg_readback)
beside the host hierarchy the handle was built from (mof_test_amg_levels).
Each level is checked against the input its kernel really read -- level 0's
read-back A0h (bf16) or A32, level l's read-back fp32 A for the product
l -> l + 1 -- so a fault is pinned to one kernel and nothing is carried along.

The Galerkin bound is derived, not tuned: an entry summed in fp32 (no
contraction) from k scalar products a q q whose absolute values sum to S is
within (k + 8) 2^-24 S of the exact sum in any order. Largest error / bound
seen on an MI355X over the blocks each kernel computes (the diagonal and upper
positions; test_galerkin_product prints them, -s):
  k_galerkin_ent<2> 0.237   k_galerkin_ns<2> 0.237   k_galerkin_sys<2> fp32 0.281
  k_galerkin_sys<2> bf16 0.217   k_galerkin_sys<3> 0.091   k_galerkin_ent<3> 0.125
  k_galerkin_ns<3> 0.125   k_galerkin3_big 0.006
The lower twins meet the same bound with the same figures, and the coarsest
inverse is within 0.79 .. 0.97 of its bound against numpy's. Both needed the
operators symmetric to the bit (these tests caught it, hull3000 / hull_chain
and every curved mesh): the level-0 gather lists now read every lower block as
its upper twin transposed on plain-read meshes too, and a product's diagonal
block keeps its upper entries for both halves (sym3); before, the twins of the
plain-read hulls missed the bound at level 0 -> 1 (3.52 and 1.25) and the
coarsest inverse missed its by 10 .. 460 (a sweep that takes row k for column
k, on a matrix symmetric only to fp32 rounding).

icosphere(32, jitter=0.005) has no coarse gather list past kGalBig = 128 terms
(the longest has 56: its two coarse products are all k_galerkin_ent<3>'s, nbig = 0): k_galerkin3_big is
checked where it does run -- G2_cap641, the smoothed G1_ico642, hull3000, S1s.
"""
import functools
import os

import numpy as np
import pytest

import amg_ref as R
from conftest import load_golden
from mofhip import DeviceMesh, synth
from mofhip.mesh import (GALERKIN_KERNELS, amg_levels, amg_readback, assembly_readback, force_galerkin_ns,
                         galerkin_launches)

pytestmark = pytest.mark.gpu

K_SUB_NODES = 512   # mof_amg.h kSubNodes: larger level 1s of a smoothed level 0 take the slab chain
K_GAL_BIG = 128     # mof_amg.hip kGalBig: positions with more terms go to k_galerkin3_big

# the smallest random hull (seed 3, in steps of 50 vertices) whose level 1 has more
# than kSubNodes nodes: levels of 4150 / 519 / 24 nodes (4100: 508 on level 1)
HULL_N = 4150

# case -> (mesh, batch, systems read back, MOF_AMG_SMOOTH, forced _ns, kernels that must have run)
CASES = {
    "G1_ico642": ("G1_ico642", 5, (0, 3, 4), None, False, ("galerkin0_ent", "galerkin3_ent")),
    "G2_cap641": ("G2_cap641", 5, (0, 4), None, False, ("galerkin_sys2_f32", "galerkin3_big")),
    "G1_ico642_smoothed": ("G1_ico642", 5, (0, 4), "1", False, ("galerkin_sys2_bf16", "galerkin3_big")),
    "hull3000": ("hull3000", 66, (0, 63, 64, 65), None, False, ("galerkin_sys2_f32", "galerkin3_big")),
    "hull_chain": ("hull_chain", 3, (0, 2), None, False, ("galerkin_sys2_f32", "galerkin_sys3")),
    "S1s": ("S1s", 3, (0, 2), None, False, ("galerkin_sys2_f32", "galerkin3_big")),
    "ico32": ("ico32", 3, (0, 2), None, False, ("galerkin0_ent", "galerkin3_ent")),
    "flat7": ("flat7", 3, (0, 2), None, False, ("galerkin_sys2_f32",)),
    "G1_ico642_ns": ("G1_ico642", 5, (0, 3, 4), None, True, ("galerkin0_ns", "galerkin3_ns")),
    "ico32_ns": ("ico32", 3, (0, 2), None, True, ("galerkin0_ns", "galerkin3_ns")),
}
DEFAULT_CASES = [c for c, v in CASES.items() if not v[4]]


def flat_patch(n):
    """An n x n grid of unit squares in the plane z = 0, two triangles each
    (normals towards +z): every tangent frame spans the same plane, so each
    aggregate's near-null block has rank 2 and its third coarse dof is dead."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    p = np.column_stack([i.ravel(), j.ravel(), np.zeros(n * n)]).astype(np.float64)
    a = (i[:-1, :-1] * n + j[:-1, :-1]).ravel()
    t = np.concatenate([np.column_stack([a, a + n, a + 1]), np.column_stack([a + n, a + n + 1, a + 1])])
    return p, t.astype(np.int32)


def mesh_and_fields(name, T):
    if name.startswith("G"):
        g = load_golden(name)
        assert len(g["I"]) >= T
        return (g["coordinates"], g["normals"], g["triangles"], g["areas"]), g["I"][:T], g["t_k"][:T], float(g["lambda_"])
    if name == "S1s":
        p, t, n, a = synth.mesh_for_config("S1s")
        return (p, n, t, a), synth.config_wave("S1s", p, T), np.arange(float(T)), 0.01
    if name == "ico32":
        p, t = synth.icosphere(32, jitter=0.005)
    elif name.startswith("flat"):
        p, t = flat_patch(int(name[4:]))
    else:
        p, t = synth.random_sphere(3000 if name == "hull3000" else HULL_N, 10.0, seed=3)
    return (p, synth.vertex_normals(p, t), t, synth.triangle_areas(p, t)), synth.travelling_wave(p, T), \
        np.arange(float(T)), 0.01


@functools.lru_cache(maxsize=None)
def run(case):
    """One batch solved, then everything the checks need copied to the host."""
    name, B, systems, smooth, ns, _ = CASES[case]
    (p, n, t, a), I, tk, lam = mesh_and_fields(name, B + 1)
    old = os.environ.get("MOF_AMG_SMOOTH")
    if smooth is not None:
        os.environ["MOF_AMG_SMOOTH"] = smooth  # read when the handle's hierarchy is built
    try:
        before = galerkin_launches()
        m = DeviceMesh(p, n, t, a)
        if ns:
            with force_galerkin_ns():
                V, st = m.solve_range(I, tk, 0, B, lam, precision="mixed", precond="amg", batch=B)
        else:
            V, st = m.solve_range(I, tk, 0, B, lam, precision="mixed", precond="amg", batch=B)
        after = galerkin_launches()
    finally:
        if smooth is not None:
            if old is None:
                del os.environ["MOF_AMG_SMOOTH"]
            else:
                os.environ["MOF_AMG_SMOOTH"] = old
    assert V.shape[0] == B and st["failed"] == st["recovered"] == 0, st  # a recovery pass re-runs the setup
    H = amg_levels(m)
    lv = H["levels"]
    assert H["cap"] >= B and len(lv) >= 2 and H["nc"] == 3 * lv[-1]["n"]
    out = {"H": H, "info": m.info(), "ran": {k: after[k] - before[k] for k in GALERKIN_KERNELS}, "sys": {}}
    for s in systems:
        a0 = assembly_readback(m, s)
        # what level 0's product read: the fp32 A on an irregular mesh's slab, the bf16 copy otherwise
        fp32 = lv[0]["smoothed"] and not H["regular"]
        lev = [{"A": a0["A32"].astype(np.float64).reshape(-1, 2, 2) if fp32 else R.h0_dec(a0["A0h"])}]
        for l in range(1, len(lv)):
            lev.append(amg_readback(m, l, s, lv[l]["n"], lv[l]["sell_nb"], lv[l]["has_Ah"],
                                    H["nc"] if l + 1 == len(lv) else 0))
        out["sys"][s] = lev
    with pytest.raises(Exception):
        amg_readback(m, 1, H["cap"], lv[1]["n"], lv[1]["sell_nb"], False)  # a system past the capacity
    m.close()
    return out


def kernel_of(H, l, ns, nterms):
    """The kernel amg_setup_batch gives the product l -> l + 1 (per coarse
    position for the by-entry pair of the coarse levels)."""
    lv = H["levels"]
    slab = lv[0]["smoothed"]
    if l == 0:
        if slab:
            return "galerkin_sys2_bf16" if H["regular"] else "galerkin_sys2_f32"
        return "galerkin0_ns" if ns else "galerkin0_ent"
    if l == 1 and slab and len(lv) >= 3 and lv[1]["n"] > K_SUB_NODES:
        return "galerkin_sys3"
    if ns:
        return "galerkin3_ns"
    return np.where(nterms > K_GAL_BIG, "galerkin3_big", "galerkin3_ent")


def blocks33(r):
    """A level's read-back A (sell_nb, 3, 4) float32 -> (sell_nb, 3, 3) float64."""
    return r["A"][:, :, :3].astype(np.float64)


def product_check(F, C, fine_blocks, coarse):
    """Device A of level l + 1 against P^T A_l P at every stored position of
    the coarse level: (positions, error, bound, position is a lower twin)."""
    P = R.prolongator(F, C["n"])
    ref = R.galerkin_ref(P, R.sell_to_csr(F, fine_blocks), C["dead"])
    Cl, S, K = R.galerkin_lists(F, fine_blocks)
    upper = np.flatnonzero(np.diff(F["gptr"]) > 0)  # the diagonal and upper blocks: the positions with terms
    tw = C["twin"][upper]
    # a lower twin's entry: its upper block's products, transposed
    lower = tw[tw >= 0]
    S[lower] = S[upper[tw >= 0]].transpose(0, 2, 1)
    K[lower] = K[upper[tw >= 0]]
    pos = np.flatnonzero(R.stored_positions(C))
    assert np.array_equal(np.sort(np.concatenate([upper, lower])), pos)  # diagonal + upper + their twins: every block
    I, J = C["sell_row"][pos], C["sell_col"][pos]
    dg = (pos == C["diag_pos"][I])[:, None, None] * np.eye(3)[None] * C["dead"][I][:, :, None]  # the dead dofs' + 1
    want = R.csr_blocks(ref, I, J)
    S = S[pos] + dg
    # the host-built lists give the triple product (they cover the diagonal and upper blocks)
    up = np.isin(pos, upper)
    assert (np.abs(Cl[pos] + dg - want)[up] <= 1e-13 * S[up]).all()
    bound = (K[pos][:, None, None] + 8) * R.U24 * S
    return pos, np.abs(coarse[pos] - want), bound, ~up


RATIOS = {False: {}, True: {}}  # largest error / bound per kernel: upper blocks, lower twins


def galerkin_product(case, lower_twins):
    d = run(case)
    H, lv, ns = d["H"], d["H"]["levels"], CASES[case][4]
    for k in CASES[case][5]:
        assert d["ran"][k] > 0, (k, d["ran"])
    if case == "S1s":
        assert d["info"]["blocks_read"] < d["info"]["nblocks"] and lv[0]["sym"]  # symmetric reads chosen
    for s, lev in d["sys"].items():
        for l in range(len(lv) - 1):
            F, C = lv[l], lv[l + 1]
            fine = lev[l]["A"] if l == 0 else blocks33(lev[l])
            coarse = blocks33(lev[l + 1])
            pos, err, bound, low = product_check(F, C, fine, coarse)
            pos, err, bound = pos[low == lower_twins], err[low == lower_twins], bound[low == lower_twins]
            names = np.broadcast_to(kernel_of(H, l, ns, upper_terms(F, C)[pos]), pos.shape)
            ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
            for k in np.unique(names):
                assert d["ran"][k] > 0, (k, d["ran"])
                r = float(ratio[names == k].max())
                RATIOS[lower_twins][str(k)] = max(RATIOS[lower_twins].get(str(k), 0.0), r)
                print("%s system %d level %d -> %d %s: max error / bound %.3f over %d %s blocks"
                      % (case, s, l, l + 1, k, r, int((names == k).sum()), "lower" if lower_twins else "upper"))
            assert (err <= bound).all(), (case, s, l, float(ratio.max()))
    print("largest error / bound so far (%s):" % ("lower" if lower_twins else "upper"),
          {k: round(v, 3) for k, v in sorted(RATIOS[lower_twins].items())})


@pytest.mark.parametrize("case", list(CASES))
def test_galerkin_product(case):
    """The blocks the product kernels compute -- the diagonal and upper
    positions, every one with gather terms -- against P^T A_l P."""
    galerkin_product(case, False)


@pytest.mark.parametrize("case", list(CASES))
def test_galerkin_product_lower_twins(case):
    """The lower positions (st_pair's transposes) against P^T A_l P's own
    lower blocks, to the same bound: A_l is symmetric to the bit on every
    level (level 0 as the gather lists read it, through the exported mirror
    table), so the twins carry their upper blocks' errors."""
    galerkin_product(case, True)


def upper_terms(F, C):
    """Gather terms of the product that writes each coarse position: its own,
    or for a lower twin its upper block's."""
    n = np.diff(F["gptr"]).copy()
    up = np.flatnonzero(C["twin"] >= 0)
    n[C["twin"][up]] = n[up]
    return n


@pytest.mark.parametrize("case", ["G1_ico642", "hull3000", "ico32"])
def test_galerkin_bound_bites(case):
    """Without one mid-list gather term in the reference, the comparison of
    test_galerkin_product fails (at that term's position)."""
    d = run(case)
    lv = d["H"]["levels"]
    s, lev = next(iter(d["sys"].items()))
    for l in range(len(lv) - 1):
        F, C = lv[l], lv[l + 1]
        fine = lev[l]["A"] if l == 0 else blocks33(lev[l])
        p, g = R.mid_list_term(F, fine)
        _, S, K = R.galerkin_lists(F, fine)  # the bound of the full lists
        Cl, _, _ = R.galerkin_lists(F, fine, drop=g)
        dead = (p == C["diag_pos"][C["sell_row"][p]]) * np.diag(C["dead"][C["sell_row"][p]].astype(np.float64))
        err = np.abs(blocks33(lev[l + 1])[p] - (Cl[p] + dead))
        assert (err > (K[p] + 8) * R.U24 * (S[p] + dead)).any(), (case, l, p, g)


@pytest.mark.parametrize("case", DEFAULT_CASES)
def test_symmetric_to_the_bit(case):
    """Every upper block's lower twin is its exact transpose (st_pair), in A
    and in the sweep copy, and every diagonal block its own; what no product
    writes stays zero."""
    d = run(case)
    lv = d["H"]["levels"]
    for s, lev in d["sys"].items():
        for l in range(1, len(lv)):
            C, r = lv[l], lev[l]
            A = r["A"]
            up = np.flatnonzero(C["twin"] >= 0)
            assert len(up) > 0 and (C["sell_col"][up] > C["sell_row"][up]).all()
            assert A[C["twin"][up], :, :3].tobytes() == np.ascontiguousarray(
                A[up, :, :3].transpose(0, 2, 1)).tobytes(), (case, s, l)
            D = A[C["diag_pos"], :, :3]  # a diagonal block is its own transpose (sym3)
            assert D.tobytes() == np.ascontiguousarray(D.transpose(0, 2, 1)).tobytes(), (case, s, l)
            assert (A[:, :, 3].view(np.uint32) == 0).all()  # the rows' padding float
            written = np.zeros(C["sell_nb"], dtype=bool)
            written[R.stored_positions(C)] = True
            assert written[up].all() and written[C["twin"][up]].all()
            assert (A[~written].view(np.uint32) == 0).all(), (case, s, l)
            if C["has_Ah"]:
                codes, scale = R.a9_dec(r["Ah"], r["Ah22"])
                assert np.array_equal(scale[C["twin"][up]].view(np.uint32), scale[up].view(np.uint32))
                assert np.array_equal(codes[C["twin"][up]], codes[up].transpose(0, 2, 1))
                assert (r["Ah"][~written] == 0).all() and (r["Ah22"][~written] == 0).all()


def test_some_case_has_a_dead_dof():
    """The + 1 on a dead dof's diagonal (checked entry by entry in
    test_galerkin_product) is exercised: some case has one, and its diagonal
    block is the unit row and column."""
    found = 0
    for case in DEFAULT_CASES:
        d = run(case)
        lv = d["H"]["levels"]
        for l in range(1, len(lv)):
            for I, c in zip(*np.nonzero(lv[l]["dead"])):
                found += 1
                for lev in d["sys"].values():
                    blk = blocks33(lev[l])[lv[l]["diag_pos"][I]]
                    unit = np.eye(3)[c]
                    assert np.array_equal(blk[c], unit) and np.array_equal(blk[:, c], unit), (case, l, I, c)
        print(case, "levels", [v["n"] for v in lv], "dead dofs", [int(v["dead"].sum()) for v in lv])
    assert found > 0


@pytest.mark.parametrize("case", DEFAULT_CASES)
def test_block_jacobi_inverse(case):
    """Dh = bf16(float32(inverse of the diagonal block)), the inverse taken in
    fp64 from the stored fp32 block; one bf16 ulp of slack per entry for
    inv3's cofactors against numpy's LU."""
    d = run(case)
    lv = d["H"]["levels"]
    for s, lev in d["sys"].items():
        for l in range(1, len(lv)):
            D = blocks33(lev[l])[lv[l]["diag_pos"]]
            want = R.bf16_value(R.bf16_bits(np.linalg.inv(D).astype(np.float32))).astype(np.float64)
            got = R.h9_dec(lev[l]["Dh"], lev[l]["Dh22"])
            slack = R.bf16_ulp(np.maximum(np.abs(want), np.abs(got)))
            assert (np.abs(got - want) <= slack).all(), (case, s, l, float(np.abs(got - want).max()))


@pytest.mark.parametrize("case", DEFAULT_CASES)
def test_sweep_copy(case):
    """The int8 sweep copy of a level's A: scale = bf16(max |a| / 127) of the
    fp32 block, each code within 1 of rint(a / scale) + 128 clamped to +-127."""
    d = run(case)
    lv = d["H"]["levels"]
    seen = 0
    for s, lev in d["sys"].items():
        for l in range(1, len(lv)):
            assert lv[l]["has_Ah"] == (l + 1 < len(lv))  # every level but the coarsest
            if not lv[l]["has_Ah"]:
                continue
            pos = np.flatnonzero(R.stored_positions(lv[l]))
            A = np.ascontiguousarray(lev[l]["A"][pos, :, :3])
            codes, scale = R.a9_dec(lev[l]["Ah"][pos], lev[l]["Ah22"][pos])
            m = np.abs(A).reshape(-1, 9).max(axis=1)
            assert np.array_equal(R.bf16_bits(scale), R.bf16_bits(m / np.float32(127.0))), (case, s, l)
            assert (scale > 0).all()
            want = np.clip(np.rint(A.astype(np.float64) / scale.astype(np.float64)[:, None, None]), -127, 127) + 128
            assert (np.abs(codes - want) <= 1).all(), (case, s, l)
            seen += 1
    assert seen > 0 or len(lv) == 2


def coarsest_inverse(case, reference):
    """cinv of every system read back against reference(M) of the dense matrix
    M its coarsest level's read-back A gives, entry by entry to 2^-24 |x_ij| +
    nc^2 cond(M) 2^-53 max |x| (the fp32 store, and fp64 elimination without
    pivoting of an SPD matrix); the neighbouring system's matrix must fail it."""
    d = run(case)
    H, lv = d["H"], d["H"]["levels"]
    nc, Lc = H["nc"], lv[-1]
    ref = {}
    for s, lev in d["sys"].items():
        M = R.sell_to_csr(Lc, blocks33(lev[-1])).toarray()
        assert M.shape == (nc, nc) and np.array_equal(M, M.T)
        ref[s] = (reference(M), np.linalg.cond(M))

    def ratio(cinv, s):
        X, kappa = ref[s]
        return float((np.abs(cinv - X) / (R.U24 * np.abs(X) + nc * nc * kappa * 2.0 ** -53 * np.abs(X).max())).max())
    systems = list(d["sys"])
    worst = 0.0
    for k, s in enumerate(systems):
        cinv = d["sys"][s][-1]["cinv"].astype(np.float64)
        other = ratio(cinv, systems[(k + 1) % len(systems)])
        worst = max(worst, ratio(cinv, s))
        print("%s system %d coarsest inverse (%s): error / bound %.3g, against the neighbour's matrix %.3g"
              % (case, s, reference.__name__, ratio(cinv, s), other))
        assert other > 1, (case, s)  # system s's inverse belongs to system s
    assert worst <= 1, (case, worst)


@pytest.mark.parametrize("case", DEFAULT_CASES)
def test_coarsest_inverse(case):
    """cinv against numpy.linalg.inv of the coarsest level's read-back matrix
    (symmetric to the bit, which k_coarse_inverse's sweep relies on: it takes
    row k for column k): 0.79 .. 0.97 of the bound on an MI355X."""
    coarsest_inverse(case, np.linalg.inv)


@pytest.mark.parametrize("case", DEFAULT_CASES)
def test_coarsest_inverse_replays_sweep(case):
    """cinv against the kernel's own algorithm replayed in fp64 on the read-back
    matrix (amg_ref.sweep_inverse), to the same bound: 0.79 .. 0.97 of it on an
    MI355X (the fp32 store's half ulp), 1e6 .. 4e8 against the neighbour's."""
    coarsest_inverse(case, R.sweep_inverse)


@pytest.mark.parametrize("case", ["G1_ico642", "ico32"])
def test_per_position_products_equal_by_entry(case):
    """k_galerkin_ns<2> / k_galerkin_ns<3> (forced on a fresh handle) leave the
    bytes of the by-entry kernels on every level: A, D^-1, the sweep copy and
    the coarsest inverse."""
    d0, d1 = run(case), run(case + "_ns")
    assert d1["ran"]["galerkin0_ns"] > 0 and d1["ran"]["galerkin3_ns"] > 0
    assert d1["ran"]["galerkin0_ent"] == d1["ran"]["galerkin3_ent"] == d1["ran"]["galerkin3_big"] == 0
    assert d0["ran"]["galerkin0_ns"] == d0["ran"]["galerkin3_ns"] == 0 and d0["ran"]["galerkin0_ent"] > 0
    assert galerkin_launches() and not _hook_left_on()
    assert list(d0["sys"]) == list(d1["sys"])
    for s in d0["sys"]:
        assert np.array_equal(d0["sys"][s][0]["A"], d1["sys"][s][0]["A"])  # the same level-0 input
        for l in range(1, len(d0["H"]["levels"])):
            a, b = d0["sys"][s][l], d1["sys"][s][l]
            assert sorted(a) == sorted(b)
            for k in a:
                assert a[k].tobytes() == b[k].tobytes(), (case, s, l, k)


def _hook_left_on():
    """A fresh handle outside force_galerkin_ns takes the by-entry kernels again."""
    g = load_golden("G1_ico642")
    before = galerkin_launches()
    m = DeviceMesh(g["coordinates"], g["normals"], g["triangles"], g["areas"])
    m.solve_range(g["I"][:3], g["t_k"][:3], 0, 2, float(g["lambda_"]), precision="mixed", precond="amg")
    m.close()
    after = galerkin_launches()
    return after["galerkin0_ns"] > before["galerkin0_ns"] or after["galerkin0_ent"] == before["galerkin0_ent"]
