"""The decomposed solve (config C5) below V: the halo plan, the halo and gather
kernels of csrc/mof_dd.hip, the parts' operators, the lockstep inner iteration
(pcg() of csrc/mof_pcg.hip over the parts) and the refinement step, against tests/dd_ref.py
(the plan, copies, cross-part sums) and the derived bounds of tests/pcg_ref.py.
Every assertion is byte equality or error / bound <= 1.0 of a derived bound:
pcg_ref's and vcycle_ref's, and dd_ref's two for the fp32 assembly and the fp64
residual (counts of roundings on the terms' magnitudes, from the geometry).

Cases (B = 3 systems):
  a   icosphere(8), RCB, P = 3
  b   icosphere(8), a random part, P = 4: nearly every row has ghosts, a part
      has 3 neighbours
  c   icosphere(8), hand-made parts of 436 / 200 / 6 owned vertices (the last
      one vertex and its ring): the parts have 2 / 1 / 1 row blocks, so the
      shared records have a tail. The smallest part's local mesh (16 rows) is
      below the multigrid's 42-vertex floor, so the library runs block Jacobi
      on every part there; the multigrid variant runs on a and b only.
  e   icosphere(8), parts of 392 / 200 / 50 owned vertices by height: 2 / 2 /
      1 row blocks and every part above the floor -- the part multigrid with
      tail records in the shared arrays
  d   two disjoint icospheres(4), P = 2 by component: no ghost, no neighbour
  cap G2_cap641 (open, boundary sweeps), RCB, P = 3
  rnd random_sphere(1500), RCB, P = 3: every part reads plain (asserted)

mof_dd_test_pcg_inner runs the production pcg() capped at K = 0, 1, ...: runs
are bit-reproducible (asserted), so the state at cap K is the input of the
transition cap K + 1 shows. Per part, pcg_ref.check_first / check_step run
with nown; the three sums are shared by all parts and are checked once, over
the owned rows of all parts (dd_ref.global_sums); z = D^-1 r is checked on the
owned rows (after the halo the ghost rows hold the owner's z). The smallest
part of case c has no hierarchy to export its level-0 tables from, so its row
product is not restated; its other stages are.
"""
import functools

import numpy as np
import pytest

import amg_ref as R
import dd_ref as D
import oracle
import pcg_ref as P
import test_gpu_vcycle as TV
import vcycle_ref as VR
from conftest import load_golden
from mofhip import DecomposedMesh, MofError, partition_rcb, synth
from mofhip.decomp import dd_gather, dd_halo, dd_launches, dd_parts, dd_pcg_inner
from mofhip.mesh import (amg_levels, amg_readback, amg_vcycle, amg_vcycle_tables, assembly_readback, outer_readback,
                         pcg_launches, vcycle_launches)

pytestmark = pytest.mark.gpu

B = 3
LAM = 0.01
SENTINEL = 0x7FC0BEEF            # a quiet NaN no kernel produces
PREFILL = 0x7FF8DEADBEEF0001     # a NaN the gather never writes (its own is the default quiet NaN)
RTOL = {"amg": 1e-4, "jacobi": 0.03}   # as tests/test_gpu_pcg.py
KMAX_CAP = 40
ROWS_PER_WG = 256


def uneven_part50(p):
    """392 / 200 / 50 by height: every part's local mesh is above the multigrid's floor."""
    order = np.argsort(p[:, 2], kind="stable")
    part = np.zeros(len(p), dtype=np.int32)
    part[order[50:250]] = 1
    part[order[:50]] = 2
    return part


def uneven_part(p, t):
    """436 / 200 / 6: part 2 is vertex 0 and its ring, part 1 the 200 lowest of the rest."""
    ring = sorted({int(v) for tri in t if 0 in tri for v in tri})
    part = np.zeros(len(p), dtype=np.int32)
    rest = np.array([v for v in np.argsort(p[:, 2], kind="stable") if v not in set(ring)])
    part[rest[:200]] = 1
    part[ring] = 2
    return part


@functools.lru_cache(maxsize=None)
def mesh_of(case):
    """(p, n, t, a), I (B + 1, N), t_k, lambda, part (or None: RCB), P."""
    if case == "cap":
        g = load_golden("G2_cap641")
        return (g["coordinates"], g["normals"], g["triangles"], g["areas"]), g["I"][:B + 1], g["t_k"][:B + 1], \
            float(g["lambda_"]), None, 3
    if case == "rnd":
        p, t = synth.random_sphere(1500, 10.0, seed=3)
        part, nparts = None, 3
    elif case == "d":
        p0, t0 = synth.icosphere(4)
        p, t = np.concatenate([p0, p0 + [3.0, 0.0, 0.0]]), np.concatenate([t0, t0 + len(p0)])
        part, nparts = np.repeat([0, 1], len(p0)).astype(np.int32), 2
    else:
        p, t = synth.icosphere(8)
        part, nparts = {"a": (None, 3), "b": (np.random.default_rng(5).integers(0, 4, len(p)).astype(np.int32), 4),
                        "c": (uneven_part(p, t), 3), "e": (uneven_part50(p), 3)}[case]
    return (p, synth.vertex_normals(p, t), t, synth.triangle_areas(p, t)), synth.travelling_wave(p, B + 1), \
        np.arange(float(B + 1)), LAM, part, nparts


def open_case(case, staged, batch=B, **opts):
    """A handle that has solved one batch (so its workspaces hold `batch` systems), its parts and the plan."""
    (p, n, t, a), I, tk, lam, part, nparts = mesh_of(case)
    d = DecomposedMesh(p, n, t, a, nparts, part=part, staged=staged)
    V, st = d.solve_range(I, tk, 0, batch, lam, batch=batch, **opts)
    assert st["failed"] == st["recovered"] == 0, st
    parts = dd_parts(d)
    return d, parts, D.plan_of_handles(parts), V


def delta(c0):
    c1 = dd_launches()
    return {k: c1[k] - c0[k] for k in c0 if c1[k] != c0[k]}


# ---- the plan ---------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["a", "b", "c", "d", "cap", "rnd"])
def test_plan_against_its_definition(case):
    """Everything mof_dd_test_part returns equals the restatement, exactly: the
    ghosts' owners and owner rows (the same caller vertex), the neighbour ranges,
    the send lists in the receiver's ghost order; and what each case is for."""
    (p, n, t, a), _, _, _, part, nparts = mesh_of(case)
    d = DecomposedMesh(p, n, t, a, nparts, part=part)
    parts = dd_parts(d)
    d.close()
    got = D.plan_of_handles(parts)
    if part is None:
        part = partition_rcb(p, nparts)
    assert len(parts) == nparts == parts[0].nparts and [h.part for h in parts] == list(range(nparts))
    want = D.restated_plan(t, len(p), part, [g["l2g"][:g["n_own"]] for g in got])
    assert D.plan_mismatches(got, want) == []
    pos = D.ghost_positions(got)
    assert sorted(pos) == [(q, g) for q, h in enumerate(parts) for g in range(h.n_ghost)]
    for (q, g), where in pos.items():
        assert len(where) == 1, (q, g, where)
        o, e = where[0]
        assert o == got[q]["ghost_owner"][g] and got[o]["send_idx"][e] == got[q]["ghost_src"][g]
        assert got[o]["l2g"][got[q]["ghost_src"][g]] == got[q]["l2g"][got[q]["n_own"] + g]
    assert sorted(np.concatenate([g["l2g"][:g["n_own"]] for g in got]).tolist()) == list(range(len(p)))
    assert parts[0].n_halo == sum(h.n_ghost for h in parts)
    nblk = [-(-h.N // ROWS_PER_WG) for h in parts]
    nbrs = [len(h.nbr) for h in parts]
    print(case, "owned", [h.n_own for h in parts], "ghosts", [h.n_ghost for h in parts], "row blocks", nblk,
          "neighbours", nbrs)
    if case == "a":
        assert max(nblk) >= 2 and all(k == 2 for k in nbrs)
    if case == "b":
        assert max(nbrs) == 3 and all(h.n_ghost > 0.9 * h.n_own for h in parts)
    if case == "c":
        assert [h.n_own for h in parts] == [436, 200, 6] and nblk == [2, 1, 1] and parts[2].N == 16
    if case == "d":
        assert nbrs == [0, 0] and parts[0].n_halo == 0 and all(h.n_ghost == 0 for h in parts)


# ---- halo and gather ----------------------------------------------------------------------------

def halo_and_gather(case, staged, batch):
    """Every (which, f32) exchange and the gather at each B <= batch on one handle; host data only."""
    d, parts, plan, _ = open_case(case, staged, batch=batch, precision="mixed")
    N = d.N
    out = {"plan": plan, "N": N, "runs": [], "cap": parts[0].cap}
    before = [outer_readback(h, batch) for h in parts]
    for Bv in range(batch, 0, -1):
        for which, f32 in ((0, True), (0, False), (1, False)):
            vecs = D.coded(plan, Bv, shift=7 * Bv + which)
            c0 = dd_launches()
            got = dd_halo(d, parts, vecs, which, f32, sentinel=SENTINEL)
            out["runs"].append(("halo", Bv, which, f32, vecs, got, delta(c0)))
        x = D.coded(plan, Bv, shift=3)
        failed = np.array([0, 1, 0][:Bv], dtype=np.uint8)
        c0 = dd_launches()
        V = dd_gather(d, parts, x, failed, PREFILL)
        out["runs"].append(("gather", Bv, x, failed, V, delta(c0)))
    # the hooks put back what they replaced: every part's x64 and per-system rows read as before them
    # (z is scratch of the inner solve; no hook reads it back outside one)
    after = [outer_readback(h, batch) for h in parts]
    out["restored"] = all(x["x64"].tobytes() == y["x64"].tobytes() and
                          all(x["sys"][k].tobytes() == y["sys"][k].tobytes() for k in x["sys"])
                          for x, y in zip(before, after))
    d.close()
    return out


@pytest.mark.parametrize("case,batch", [("a", 3), ("a", 1), ("b", 3), ("c", 3), ("d", 3)])
def test_halo_and_gather_are_copies(case, batch):
    """After dd_halo every ghost row of every part holds its owner's bytes and
    every owned row is unchanged -- z as floats and doubles, x64 -- in-process and
    through the packed segments, at B = 3, and at B = 2 and 1 on the same handle
    (capacity 3: the region bases use the capacity, the segment offsets B), and
    at B = 1 on a handle of capacity 1. The gather writes every caller vertex
    from its owner, a flagged system all NaN, nothing twice or never (no prefill
    word survives; the owned sets partition the vertices), both paths the same
    bytes. The counters show which kernel instances ran."""
    res = {staged: halo_and_gather(case, staged, batch) for staged in (False, True)}
    plan, N = res[False]["plan"], res[False]["N"]
    nsend = sum(len(g["send_idx"]) > 0 for g in plan)
    nrecv = sum(g["n_ghost"] > 0 for g in plan)
    nhalo = sum(g["n_ghost"] for g in plan)
    for staged, r in res.items():
        assert r["cap"] == batch and r["restored"]
        for run in r["runs"]:
            if run[0] == "halo":
                _, Bv, which, f32, vecs, got, ran = run
                dt = np.float32 if f32 else np.float64
                want = D.halo(plan, vecs)
                for q, (g, w, v) in enumerate(zip(got, want, vecs)):
                    assert g.dtype == dt and g.tobytes() == w.astype(dt).tobytes(), (case, staged, Bv, which, f32, q)
                    no = plan[q]["n_own"]
                    assert np.array_equal(g[:, :no], v[:, :no])
                sfx = "f32" if f32 else "f64"
                if staged:
                    exp = {"halo_pack_" + sfx: nsend, "halo_unpack_" + sfx: nrecv}
                else:
                    exp = {"halo_pull_" + sfx: 1} if nhalo else {}
                assert ran == {k: v for k, v in exp.items() if v}, (case, staged, ran)
            else:
                _, Bv, x, failed, V, ran = run
                want, hits = D.gather(plan, N, x, failed)
                assert (hits == 1).all()
                assert not (V.view(np.uint64) == PREFILL).any(), (case, staged, Bv)
                ok = failed == 0
                assert np.array_equal(V[ok], want[ok]) and np.isnan(V[~ok]).all()
                exp = {"dd_own_pack": len(plan), "dd_own_scatter": 1} if staged else {"dd_scatter": len(plan)}
                assert ran == exp, (case, staged, ran)
    for a, b in zip(res[False]["runs"], res[True]["runs"]):
        if a[0] == "gather":
            assert a[4].tobytes() == b[4].tobytes()
    print(case, "batch", batch, "ghost rows", nhalo, "sending parts", nsend, "receiving parts", nrecv)


RATIOS = {}


def note(key, ratio):
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)


# ---- the parts' operators ---------------------------------------------------------------------------

def part_level(h):
    """A part's level-0 tables (pcg_ref.level0) and hierarchy."""
    H = amg_levels(h)
    l0 = H["levels"][0]
    return H, P.level0(l0["sell_off"], l0["sell_col"], l0["mirror"], l0["n"], sym=l0["sym"])


def ghost_blocks_decoupled(blk, lev, mir, no):
    """The bf16 copy's blocks (nb, 2, 2): the identity on a ghost row's diagonal, zero on every other block
    of a ghost row, zero on an owned row's blocks in ghost columns."""
    row, col = lev["sell_row"], lev["sell_col"]
    stored = np.flatnonzero(mir >= 0)
    gr = stored[row[stored] >= no]
    diag, off = gr[col[gr] == row[gr]], gr[col[gr] != row[gr]]
    gc = stored[(row[stored] < no) & (col[stored] >= no)]
    return bool((blk[diag] == np.eye(2)).all() and (blk[off] == 0).all() and (blk[gc] == 0).all()), off


@functools.lru_cache(maxsize=None)
def operators(case):
    d, parts, plan, _ = open_case(case, False, precision="mixed", precond="amg", rtol=1e-10)
    out = {"plan": plan, "parts": []}
    for h in parts:
        H, lev = part_level(h)
        out["parts"].append({"H": H, "lev": lev, "sym": H["levels"][0]["sym"], "n_own": h.n_own,
                             "A0h": [assembly_readback(h, b)["A0h"] for b in range(B)]})
    (p, n, t, a), I, tk, lam, _, _ = mesh_of(case)
    ones = [np.ones((B, h.N, 2)) for h in parts]
    # a block-Jacobi mixed solve: the fp32 operator, f and the fp32 D^-1 (the multigrid's assembly writes none)
    _, st = d.solve_range(I, tk, 0, B, lam, batch=B, precision="mixed")
    assert st["failed"] == st["recovered"] == 0
    o = dd_pcg_inner(d, parts, ones, 0.5, 0, precision="mixed")
    for q, h in enumerate(parts):
        rb = [assembly_readback(h, b) for b in range(B)]
        out["parts"][q].update(A32=[v["A32"] for v in rb], rhs32=[v["rhs"] for v in rb], dinv32=o["parts"][q]["dinv"])
    _, st = d.solve_range(I, tk, 0, B, lam, batch=B, precision="f64")
    assert st["failed"] == st["recovered"] == 0
    for b in range(B):
        o = dd_pcg_inner(d, parts, ones, 0.5, 0, precision="f64", a_system=b)
        for q, h in enumerate(parts):
            out["parts"][q].setdefault("A64", []).append(o["parts"][q]["A"])
            out["parts"][q].setdefault("rhs", []).append(assembly_readback(h, b)["rhs"])
    d.close()
    return out


@pytest.mark.parametrize("case", ["a", "cap", "rnd"])
def test_part_operators(case):
    """The fp64 solve's owned rows of A and f are the oracle's bit for bit
    (DESIGN.md §10). The mixed solve's f is the same; every stored entry of an
    owned row of its fp32 operator is within dd_ref.a32_bound of the oracle's
    (the fp32 fold's roundings on the magnitudes of its terms, from the
    geometry); its fp32 D^-1 is the fp64 inverse of the stored fp32 diagonal
    block rounded once. The multigrid's bf16 copy holds the identity on a ghost
    row's diagonal and zero on every block of a ghost row or column; on every
    plain-read part its owned-owned lower blocks are their upper twins
    transposed, by bytes (the assembly rounds them on their own). A
    symmetric-read part stores no lower block -- those positions keep what the
    allocation held (597 of 597 differ on case a) and nothing reads them;
    test_part_vcycle holds the copy as it is read there, through the mirror
    table, symmetric to the bit."""
    (p, n, t, a), I, tk, lam, _, _ = mesh_of(case)
    d = operators(case)
    N = len(p)
    a2, gw, e, iw = oracle.geometry(p, n, t, a)
    plain = 0
    for q, (g, o) in enumerate(zip(d["plan"], d["parts"])):
        lev, no = o["lev"], g["n_own"]
        l2g = g["l2g"]
        own = l2g[:no]
        for b in range(B):
            Ao, fo = oracle.step_system(a2, gw, e, iw, t, a, lam, I[b], I[b + 1], tk[b + 1] - tk[b])
            A = P.Op(lev, o["A64"][b]).A.toarray()
            glob = np.stack([l2g, N + l2g], axis=1).ravel()          # local dof -> the oracle's planar dof
            want = Ao[glob[:2 * no]][:, glob].toarray()
            assert np.array_equal(A[:2 * no], want), (case, q, b)
            fw = np.stack([fo[own], fo[N + own]], axis=1)
            assert np.array_equal(o["rhs"][b][:no], fw) and np.array_equal(o["rhs32"][b][:no], fw), (case, q, b)
            # the fp32 operator, every stored entry of the owned rows
            val, mag, shared = D.a1_terms(t, a, gw, e, I[b])
            assert abs(Ao - (val + lam * a2)).max() <= 8 * P.U53 * abs(Ao).max()   # the restated terms are A's
            A32 = P.Op(lev, o["A32"][b]).A.toarray()[:2 * no]
            pat = P.Op(lev, np.ones_like(o["A32"][b])).A.toarray()[:2 * no] != 0
            magl = mag[glob[:2 * no]][:, glob].toarray()
            a2l = abs(lam * a2)[glob[:2 * no]][:, glob].toarray()
            sh = shared[l2g[:no]][:, l2g].toarray()
            bound = D.a32_bound(magl, np.repeat(np.repeat(sh, 2, axis=0), 2, axis=1), a2l)
            ok, ratio = P.within(A32[pat], want[pat], bound[pat])
            note(("operators", "A32 owned rows"), ratio)
            assert ok and pat.sum() >= 4 * no, (case, q, b, ratio)
            # D^-1 of the owned rows: the stored diagonal block's fp64 inverse, rounded once; the fp64
            # adjugate's own roundings (4 of them) are below 2^-53 (|d0 d3| + |d1 d2|) / |det| of an entry
            dg = o["A32"][b].reshape(-1, 2, 2)[o["H"]["levels"][0]["diag_pos"][:no]].astype(np.float64)
            det = dg[:, 0, 0] * dg[:, 1, 1] - dg[:, 0, 1] * dg[:, 1, 0]
            inv = np.stack([dg[:, 1, 1], -dg[:, 0, 1], -dg[:, 1, 0], dg[:, 0, 0]], axis=1).reshape(-1, 2, 2) / det[:, None, None]
            cond = (np.abs(dg[:, 0, 0] * dg[:, 1, 1]) + np.abs(dg[:, 0, 1] * dg[:, 1, 0])) / np.abs(det)
            ok, ratio = P.within(o["dinv32"][b][:no], inv, (P.U24 + 4 * P.U53 * cond[:, None, None]) * np.abs(inv))
            note(("operators", "dinv32 owned rows"), ratio)
            assert ok, (case, q, b, ratio)
        mir = o["H"]["levels"][0]["mirror"]   # built with nown: only owned-owned lower blocks name a twin
        row, col = lev["sell_row"], lev["sell_col"]
        stored = np.flatnonzero(mir >= 0)
        low = stored[(mir[stored] & R.MIR_T) != 0]
        assert len(low) and (row[low] < no).all() and (col[low] < row[low]).all()
        plain += not o["sym"]
        for b in range(B):
            blk = R.h0_dec(o["A0h"][b]).astype(np.float32)
            assert ghost_blocks_decoupled(blk, lev, mir, no)[0], (case, q, b)
            if o["sym"]:   # lower blocks are read through the table: their own positions are never written
                continue
            twin = blk[mir[low] & R.MIR_POS].transpose(0, 2, 1)
            diff = np.flatnonzero((blk[low].reshape(-1, 4).view(np.uint32) !=
                                   np.ascontiguousarray(twin).reshape(-1, 4).view(np.uint32)).any(axis=1))
            ulps = (np.abs(blk[low][diff] - twin[diff]) / np.maximum(R.bf16_ulp(twin[diff]), 1e-300)).max() if len(diff) else 0
            assert len(diff) == 0, (case, q, b, "lower blocks apart from their twins", len(diff), "of", len(low),
                                    "by bf16 ulps:", float(ulps))
    print(case, "plain-read parts", plain, "of", len(d["parts"]), "largest error / bound so far:",
          {k[1]: round(r, 3) for k, r in RATIOS.items() if k[0] == "operators"})
    if case == "rnd":
        assert plain >= 1
    if case == "a":
        assert plain == 0


# ---- the inner iteration ------------------------------------------------------------------------------

VARIANTS = [("a", "jacobi", "mixed"), ("a", "jacobi", "f64"), ("a", "amg", "mixed"),
            ("b", "jacobi", "mixed"), ("b", "jacobi", "f64"), ("b", "amg", "mixed"),
            ("c", "jacobi", "mixed"), ("c", "jacobi", "f64"), ("e", "amg", "mixed")]


@functools.lru_cache(maxsize=None)
def inner(case, precond, precision):
    """Every cap of one variant in-process, a few staged; host data only."""
    out = {}
    for staged in (False, True):
        # the multigrid solve first where there is one: its hierarchy exports the level-0 tables
        # (case c: the library builds the hierarchies up to the part that refuses, then runs block Jacobi)
        d, parts, plan, _ = open_case(case, staged, precision="mixed", precond="amg")
        if not staged:
            levs = []
            for h in parts:
                try:
                    levs.append(part_level(h))
                except MofError:   # no built multigrid: case c's smallest part alone
                    assert case == "c" and h.part == 2
                    levs.append(None)
            out.update(plan=plan, levs=levs, sizes=[None if v is None else [x["n"] for x in v[0]["levels"]]
                                                    for v in levs])
        (p, n, t, a), I, tk, lam, _, _ = mesh_of(case)
        if (precond, precision) != ("amg", "mixed") or case == "c":
            kw = dict(precision=precision) if precond == "jacobi" else dict(precision=precision, precond=precond)
            _, st = d.solve_range(I, tk, 0, B, lam, batch=B, **kw)
            assert st["failed"] == st["recovered"] == 0
        rhs = [np.stack([assembly_readback(h, b)["rhs"] for b in range(B)]) for h in parts]
        for v in rhs:
            v[2] = 0.25 * v[0]
        kw = dict(precond=precond, precision=precision, sentinel=SENTINEL)
        rtol = RTOL[precond]
        if not staged:
            c0 = pcg_launches()
            probe = dd_pcg_inner(d, parts, rhs, rtol, 400, a_system=0, **kw)
            c1 = pcg_launches()
            out["ran_probe"] = {k: c1[k] - c0[k] for k in c0 if c1[k] != c0[k]}
            conv = [int(c) for c in probe["parts"][0]["sys"]["CONV"]]
            assert min(conv) >= 1 and not probe["parts"][0]["sys"]["FAILED"].any(), (case, precond, conv)
            kmax = max(conv) + 1
            assert kmax <= KMAX_CAP, conv
            blocks = [[o["A"] for o in dd_pcg_inner(d, parts, rhs, rtol, 0, a_system=b, **kw)["parts"]]
                      for b in range(B)]
            c0 = pcg_launches()
            caps = [dd_pcg_inner(d, parts, rhs, rtol, 0, **kw)]
            c1 = pcg_launches()
            out["ran_cap0"] = {k: c1[k] - c0[k] for k in c0 if c1[k] != c0[k]}
            caps += [dd_pcg_inner(d, parts, rhs, rtol, K, **kw) for K in range(1, kmax + 1)]
            again = dd_pcg_inner(d, parts, rhs, rtol, 2, **kw)
            cycle = None
            if precond == "amg":   # the production cycle of every part on the r each cap left
                cycle = [[amg_vcycle(h, o["parts"][q]["r"], out["sizes"][q], sentinel=SENTINEL)
                          for q, h in enumerate(parts)] for o in caps]
            out.update(rhs=rhs, probe=probe, conv=conv, kmax=kmax, blocks=blocks, caps=caps, again=again, cycle=cycle,
                       rtol=rtol, dtype=np.float32 if precision == "mixed" else np.float64,
                       nblk=[-(-h.N // ROWS_PER_WG) for h in parts])
        else:
            out["staged"] = {K: dd_pcg_inner(d, parts, rhs, rtol, K, **kw) for K in (0, 1, 2, out["kmax"])}
        d.close()
    return out


def bytes_equal(a, b):
    """Two hook runs left the same bytes on every part, and the same shared records."""
    same = all(x["words"][k].tobytes() == y["words"][k].tobytes() for x, y in zip(a["parts"], b["parts"]) for k in "xrzpq")
    same &= all(np.array_equal(x["sys"][k], y["sys"][k]) for x, y in zip(a["parts"], b["parts"]) for k in x["sys"])
    return same and all(a[k].tobytes() == b[k].tobytes() for k in ("scal", "part_rzrr", "part_pq"))


def dummy_op(n):
    import scipy.sparse as sp
    op = P.Op.__new__(P.Op)
    op.A = op.Aabs = sp.csr_matrix((n, n))
    op.w, op.n = np.zeros(n), n
    return op


def chain(d, b, controls=()):
    """System b's stage checks of every part from cap 0 to its last step:
    [(cap, part, stage, ok, ratio)]. controls: names of reference-side faults
    (dd_ref / pcg_ref), applied at every step."""
    plan, dt, conv = d["plan"], d["dtype"], d["conv"][b]
    U, ex = P.unit(dt), d["dtype"] == np.float32
    jac = d["caps"][0]["parts"][0]["dinv"] is not None
    n = len(plan)
    ops, norow = [], []
    for q in range(n):
        if d["levs"][q] is None:
            ops.append(dummy_op(2 * len(plan[q]["l2g"])))
            norow.append(True)
        else:
            ops.append(P.Op(d["levs"][q][1], d["blocks"][b][q]))
            norow.append(False)
    S = [[D.part_state(o["parts"][q], o["scal"], b) for q in range(n)] for o in d["caps"]]
    recs = []

    def ghosts(K):
        # r is exactly 0 on the ghost rows; z and p there are the owner's bytes
        for key in "zp":
            vec = [s[key] for s in S[K]]
            if "wrong_row" in controls:
                q0 = next(q for q in range(n) if plan[q]["n_ghost"])
                want = D.halo(plan, vec, wrong_row=(q0, 0))
            else:
                want = D.halo(plan, vec)
            recs.append((K, -1, "ghost %s = the owner's" % key,
                         all(np.array_equal(a, w) for a, w in zip(vec, want)), 0.0))
        recs.append((K, -1, "ghost r = 0", all((s["r"][2 * g["n_own"]:] == 0).all() for s, g in zip(S[K], plan)), 0.0))

    def sums(K, slot, which):
        kw = {}
        if "pq_ghost" in controls and "p.q" in which:
            kw = {"ghost_part": next(q for q in range(n) if plan[q]["n_ghost"])}
        if "drop_part" in controls:
            kw = {"drop_part": n - 1}
        for name, ok, r in D.global_sums(plan, S[K], slot, ex, which, **kw):
            recs.append((K, -1, name, ok, r))

    for q in range(n):
        dinv = d["caps"][0]["parts"][q]["dinv"]
        first, _ = P.check_first(ops[q], d["rhs"][q][b].ravel(), S[0][q], dt, None, plan[q]["n_own"])
        recs += [(0, q, k, ok, r) for k, ok, r in first if k not in D.SUMS and not (norow[q] and k.startswith("q ="))]
        if jac:
            recs.append((0, q) + D.jacobi_owned(dinv[b], S[0][q], plan[q]["n_own"], U))
    sums(0, 0, D.SUMS)
    ghosts(0)
    for K in range(conv):
        stopped = None
        for q in range(n):
            dinv = d["caps"][0]["parts"][q]["dinv"]
            step, info = P.check_step(ops[q], S[K][q], S[K + 1][q], K, dt, None, plan[q]["n_own"])
            recs += [(K + 1, q, k, ok, r) for k, ok, r in step
                     if k not in D.SUMS and not (norow[q] and k.startswith("q ="))]
            if jac:
                recs.append((K + 1, q) + D.jacobi_owned(dinv[b], S[K + 1][q], plan[q]["n_own"], U))
            assert stopped in (None, info["stopped"])
            stopped = info["stopped"]
        assert stopped == (K + 1 == conv), (b, K)
        nxt = (K + 1) & 1
        sums(K + 1, nxt, ("r.r",) if stopped and not jac else (("r.z", "r.r") if stopped else D.SUMS))
        ghosts(K + 1)
    return recs


@pytest.mark.parametrize("case,precond,precision", VARIANTS)
def test_runs_reproducible_and_parts_agree(case, precond, precision):
    """Two runs of a cap leave the same bytes; sysi and sysd are byte-identical
    on every part at every cap (the same decisions); the raw records of row
    blocks past a part's own count are exactly 0; the in-process and the staged
    transport leave the same bytes at every cap compared."""
    d = inner(case, precond, precision)
    assert bytes_equal(d["caps"][2], d["again"])
    for K, o in enumerate(d["caps"]):
        s0 = o["parts"][0]["sys"]
        for q, x in enumerate(o["parts"][1:], start=1):
            for k in s0:
                assert s0[k].tobytes() == x["sys"][k].tobytes(), (case, K, q, k)
        for q, nb in enumerate(d["nblk"]):
            assert (o["part_rzrr"][:, q, :, nb:] == 0).all() and (o["part_pq"][:, q, :, nb:] == 0).all(), (case, K, q)
            assert (o["part_pq"][K & 1, q, :, :nb] != 0).any()
    for K, o in d["staged"].items():
        assert bytes_equal(o, d["caps"][K]), (case, precond, K)
    print(case, precond, precision, "steps to stop", d["conv"], "row blocks", d["nblk"], "nmax", d["caps"][0]["nmax"],
          "probe ran", d["ran_probe"], "cap 0 ran", d["ran_cap0"])
    # cap 0: the FIRST instance alone, once per part (the parts' check launch took the other one before)
    spmv0 = {k: n for k, n in d["ran_cap0"].items() if k.startswith("spmv")}
    assert len(spmv0) == 1 and "_first" in next(iter(spmv0)) and sum(spmv0.values()) == len(d["plan"]), spmv0
    assert "update" not in d["ran_cap0"] and "conv_early" not in d["ran_probe"]
    inst = {k for k in d["ran_probe"] if k.startswith("spmv")}
    assert all(("f64" in k) == (precision == "f64") and "_zh" not in k for k in inst), inst
    if case == "c":
        assert d["nblk"] == [2, 1, 1] and d["caps"][0]["nmax"] == 2 and d["levs"][2] is None
    if case == "e":   # the multigrid with a tail in the shared records
        assert d["nblk"] == [2, 2, 1] and d["caps"][0]["nmax"] == 2 and None not in d["levs"]


@pytest.mark.parametrize("case,precond,precision", VARIANTS)
def test_stage_chain(case, precond, precision):
    """Every stage of every step on every part within pcg_ref's bound on the
    input it read; ghost r exactly 0, ghost z and p the owner's bytes; the three
    sums against the fp64 sums over the owned rows of all parts."""
    d = inner(case, precond, precision)
    for b in range(B):
        for cap, q, stage, ok, ratio in chain(d, b):
            note((precision, stage), ratio)
            assert ok, (case, precond, precision, b, cap, q, stage, ratio)
    print("largest error / bound so far:", {"%s %s" % k: round(r, 3) for k, r in sorted(RATIOS.items())})


@pytest.mark.parametrize("case,precond,precision", VARIANTS)
def test_stop_rule_and_final_state(case, precond, precision):
    """SD_TOL2 = rtol^2 rr_0, SI_CONV the first step whose own |r|^2 is <= it,
    SD_BEST / SI_BEST_IT the running minimum (as tests/test_gpu_pcg.py); a
    stopped system's x, r and flags are the same bytes at every later cap, on
    every part, and its ghosts stay the owner's."""
    d = inner(case, precond, precision)
    for b in range(B):
        c = d["conv"][b]
        rr = [float(d["caps"][K]["scal"][K & 1, b, 1]) for K in range(c + 1)]
        sys0 = d["caps"][0]["parts"][0]["sys"]
        assert sys0["TOL2"][b] == P.tol2(d["rtol"], rr[0]) and sys0["RR0"][b] == rr[0]
        assert P.conv_step(rr, sys0["TOL2"][b]) == c
        for K in range(d["kmax"] + 1):
            s = d["caps"][K]["parts"][0]["sys"]
            assert s["CONV"][b] == (c if K >= c else -1) and s["FAILED"][b] == 0
            if K <= c:
                assert (s["BEST"][b], s["BEST_IT"][b]) == P.best(rr[:K + 1] if K < c else rr[:c]), (case, b, K)
            for q, o in enumerate(d["caps"][K]["parts"]):
                if K >= c:
                    for k in "xr":
                        assert o["words"][k][b].tobytes() == d["probe"]["parts"][q]["words"][k][b].tobytes(), (case, b, K, q)
            for key in "zp":
                vec = [o[key][b:b + 1].astype(np.float64) for o in d["caps"][K]["parts"]]
                assert all(np.array_equal(x, y) for x, y in zip(vec, D.halo(d["plan"], vec))), (case, b, K, key)


@pytest.mark.parametrize("case", ["a", "b", "e"])
def test_multigrid_z_is_each_parts_cycle(case):
    """z_K is, on every part's owned rows, the output of mof_test_amg_vcycle on
    that part's r_K, byte for byte, up to the step c a system stops at (pcg()
    launches no k_pcg_conv_early: the cycle still runs on r_c, and SpMV c stops
    the system); after it z never changes again, ghost rows included. The
    cycle's ghost rows are never read: no sentinel word is left in z after the
    halo."""
    d = inner(case, "amg", "mixed")
    for K, (o, cyc) in enumerate(zip(d["caps"], d["cycle"])):
        for q, g in enumerate(d["plan"]):
            no = g["n_own"]
            assert not cyc[q]["zh"]
            for b in range(B):
                c = d["conv"][b]
                z = o["parts"][q]["z_words"][b]
                assert not (z == SENTINEL).any(), (case, K, q, b)
                if K <= c:
                    assert z[:no].tobytes() == cyc[q]["z_words"][b][:no].tobytes(), (case, K, q, b)
                else:
                    assert z.tobytes() == d["caps"][c]["parts"][q]["z_words"][b].tobytes(), (case, K, q, b)


def fails(d, b, *controls):
    return {stage for _, _, stage, ok, _ in chain(d, b, controls) if not ok}


def test_negative_controls():
    """A reference wrong in one thing fails the check it belongs to (the
    device is never perturbed), and the right reference fails none."""
    d = inner("b", "jacobi", "mixed")
    assert not fails(d, 0)
    bad = fails(d, 0, "wrong_row")
    assert bad == {"ghost z = the owner's", "ghost p = the owner's"}, bad
    bad = fails(d, 0, "pq_ghost")
    assert bad == {"p.q"}, bad
    bad = fails(d, 0, "drop_part")
    assert bad == {"r.z", "r.r", "p.q"}, bad
    # one part's ghosts left stale for one step: the row product of step 2 on the z of step 1's ghosts
    plan, q = d["plan"], 0
    op = P.Op(d["levs"][q][1], d["blocks"][0][q])
    S = [D.part_state(o["parts"][q], o["scal"], 0) for o in d["caps"][:3]]
    stale = dict(S[2])
    stale["z"] = S[2]["z"].copy()
    stale["z"][2 * plan[q]["n_own"]:] = S[1]["z"][2 * plan[q]["n_own"]:]
    good = P.failing(P.check_step(op, S[1], S[2], 1, np.float32, None, plan[q]["n_own"])[0]) - set(D.SUMS)
    bad = P.failing(P.check_step(op, S[1], stale, 1, np.float32, None, plan[q]["n_own"])[0]) - set(D.SUMS)
    assert not good and {"q = A z + beta q"} <= bad, (good, bad)
    # a ghost block of A0h left coupled: the bf16 copy's ghost rows are the identity, a coupled one is not
    # test_part_operators' own predicate on a copy with one ghost-row block as the fp32 operator has it
    o = operators("a")["parts"][0]
    lev, mir = o["lev"], o["H"]["levels"][0]["mirror"]
    blk = R.h0_dec(o["A0h"][0])
    ok, off = ghost_blocks_decoupled(blk, lev, mir, o["n_own"])
    assert ok and len(off)
    a32 = o["A32"][0].reshape(-1, 2, 2).astype(np.float64)
    k = off[np.argmax(np.abs(a32[off]).reshape(len(off), -1).max(axis=1))]
    assert np.abs(a32[k]).max() > 0
    coupled = blk.copy()
    coupled[k] = R.bf16_value(R.bf16_bits(a32[k].astype(np.float32))).astype(np.float64)
    assert not ghost_blocks_decoupled(coupled, lev, mir, o["n_own"])[0]


# ---- a part's V-cycle -----------------------------------------------------------------------------------------

CYCLE_SYSTEMS = (0, 2)


@functools.lru_cache(maxsize=None)
def part_cycle(case, q):
    """Part q's operators read back after one multigrid batch and the production cycle on given residuals
    (zero on the ghost rows, as the solver's), in the format of tests/test_gpu_vcycle.py's run()."""
    import scipy.sparse as sp
    d, parts, plan, _ = open_case(case, False, precision="mixed", precond="amg")
    h = parts[q]
    H = amg_levels(h)
    lv = H["levels"]
    T = amg_vcycle_tables(h, len(lv), CYCLE_SYSTEMS[0])
    sizes = [v["n"] for v in lv]
    N = sizes[0]
    out = {"H": H, "T": T, "ops": {}, "n_own": h.n_own}
    rhs = np.stack([assembly_readback(h, b)["rhs"] for b in range(B)])
    for s in CYCLE_SYSTEMS:
        lev = [{"A0h": assembly_readback(h, s)["A0h"]}]
        for l in range(1, len(lv)):
            lev.append(amg_readback(h, l, s, lv[l]["n"], lv[l]["sell_nb"], lv[l]["has_Ah"],
                                    H["nc"] if l + 1 == len(lv) else 0))
        out["ops"][s] = lev
    stored = R.stored_positions(lv[0])
    adj = sp.coo_matrix((np.ones(int(stored.sum())), (lv[0]["sell_row"][stored], lv[0]["sell_col"][stored])),
                        shape=(N, N)).tocsr()
    r, kinds = TV.inputs(B, N, rhs, adj, T["bsw_n"] > 0)
    r[:, h.n_own:] = 0.0
    c0 = vcycle_launches()
    out["full"] = amg_vcycle(h, r, sizes, tuple(range(B)), tap=True, sentinel=SENTINEL)
    c1 = vcycle_launches()
    out.update(r=r, kinds=kinds, ran={k: c1[k] - c0[k] for k in c0})
    d.close()
    return out


@pytest.mark.parametrize("case,q", [("a", 0), ("cap", 0), ("rnd", 1)])
def test_part_vcycle(case, q):
    """The twelve stages of tests/test_gpu_vcycle.py (its checks, its bounds) on
    one part's cycle, run as pcg() runs it on a part: the ghost blocks of the read-back
    level-0 copy are the identity, so the reference's ghost rows are decoupled
    too. The part cycle as a whole operator is symmetric to the level the single
    domain is held to (1e-12 of its norm) and positive definite on the owned
    rows."""
    d = part_cycle(case, q)
    o = d["full"]
    names = TV.kernel_names(d, o, d["ran"])
    print(case, "part", q, "levels", [v["n"] for v in d["H"]["levels"]], "sym", d["H"]["levels"][0]["sym"], "xm",
          o["xm"], "zh", o["zh"], "ring rows", d["T"]["bsw_n"], "launches", {k: v for k, v in d["ran"].items() if v})
    assert not o["zh"]
    assert (o["z"][1] == 0).all() and o["rz"][1] == 0.0   # the zero system
    if case == "rnd":
        assert not d["H"]["levels"][0]["sym"]
    for s in CYCLE_SYSTEMS:
        c = TV.build_cycle(d["H"], d["T"], d["ops"][s])
        for stage, l, k, ok, two, ratio in TV.stage_checks(c, d, o, s, names):
            note(("cycle", "%2d %s" % (stage, k)), ratio)
            assert ok, (case, q, s, stage, l, k, ratio)
            assert two <= TV.TWO_VALUED_CAP, (case, q, s, stage, l, k, two)
        for l, A in enumerate(c.A[:-1]):
            assert abs(A - A.T).max() == 0.0, (case, q, s, "A", l)
        M = VR.M_ref(c)
        no = 2 * d["n_own"]
        asym = VR.asymmetry(M)
        ev = np.linalg.eigvalsh(0.5 * (M + M.T)[:no, :no])
        print("%s part %d system %d: asymmetry %.2e, eig(M) on the owned rows in [%.3e, %.3e]"
              % (case, q, s, asym, ev.min(), ev.max()))
        assert asym <= 1e-12 and ev.min() > 0, (case, q, s, asym, ev.min())
    print("largest error / bound so far:", {k[1]: round(r, 3) for k, r in sorted(RATIOS.items()) if k[0] == "cycle"})


# ---- the refinement step ----------------------------------------------------------------------------------

RTOL_OUT = 1e-8   # the solve's rtol, passed to it


@pytest.mark.parametrize("case,precond", [("a", "amg"), ("b", "jacobi")])
def test_outer_step(case, precond):
    """After a full decomposed solve: x64's ghost rows are the owner's bytes;
    the owned rows of r64 are f - A x64 with the oracle's fp64 A and f, per dof
    within dd_ref.residual_bound, and |f - A V| <= rtol |f| as
    tests/test_gpu_robust.py holds it; SD_RR / SD_FF are the sums over the owned
    rows of all parts; sysd is identical on all parts; V is the owned x64 rows
    exactly."""
    d, parts, plan, V = open_case(case, False, precision="mixed", precond=precond, rtol=RTOL_OUT)
    rd = [outer_readback(h, B) for h in parts]
    rhs = [np.stack([assembly_readback(h, b)["rhs"] for b in range(B)]) for h in parts]
    N = d.N
    d.close()
    (p, n, t, a), I, tk, lam, _, _ = mesh_of(case)
    a2, gw, e, iw = oracle.geometry(p, n, t, a)
    vptr, vcol = oracle.structural_blocks(t, N)
    import scipy.sparse as sp
    sp_blocks = sp.csr_matrix((np.ones(len(vcol)), vcol, vptr), shape=(N, N))
    x64 = [r["x64"] for r in rd]
    assert all(np.array_equal(a, b) for a, b in zip(x64, D.halo(plan, x64)))
    want, hits = D.gather(plan, N, x64)
    assert (hits == 1).all() and V.tobytes() == want.tobytes()
    for r in rd[1:]:
        for k in rd[0]["sys"]:
            assert rd[0]["sys"][k].tobytes() == r["sys"][k].tobytes(), k
    n = sum(2 * g["n_own"] for g in plan)
    for b in range(B):
        own = lambda vs: np.concatenate([v[b, :g["n_own"]].ravel() for v, g in zip(vs, plan)])  # noqa: E731
        r64, f = own([r["r64"] for r in rd]), own(rhs)
        rr, ff = float(r64 @ r64), float(f @ f)
        s = rd[0]["sys"]
        # fp64 sums of n rounded products in another order: (n + 1) 2^-53 of the sum (tests/test_gpu_pcg.py)
        assert abs(s["RR"][b] - rr) <= (n + 1) * P.U53 * rr and abs(s["FF"][b] - ff) <= (n + 1) * P.U53 * ff
        assert s["REL"][b] <= RTOL_OUT
        # r64 against the oracle's system
        Ao, fo = oracle.step_system(a2, gw, e, iw, t, a, lam, I[b], I[b + 1], tk[b + 1] - tk[b])
        val, mag, _ = D.a1_terms(t, a, gw, e, I[b])
        want = fo - Ao @ V[b]
        assert np.linalg.norm(want) <= RTOL_OUT * np.linalg.norm(fo) * 1.01
        w = np.tile(np.diff(sp_blocks.indptr), 2).astype(np.float64)
        bound = D.residual_bound(w, mag @ np.abs(V[b]), abs(lam * a2) @ np.abs(V[b]), np.abs(fo))
        got = np.zeros(2 * N)
        for r, g in zip(rd, plan):
            ownv = g["l2g"][:g["n_own"]]
            got[ownv], got[N + ownv] = r["r64"][b, :g["n_own"], 0], r["r64"][b, :g["n_own"], 1]
        ok, ratio = P.within(got, want, bound)
        note(("outer", "r64 = f - A x64"), ratio)
        assert ok, (case, b, ratio)
    print(case, precond, "largest error / bound:", {k[1]: round(r, 4) for k, r in RATIOS.items() if k[0] == "outer"})
