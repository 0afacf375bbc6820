"""The coarse levels' storage formats: 12-byte vector rows (b, x, r, y at every
level >= 1, three floats per node, system b's rows from word b * n * 3), the
packed fp32 operator of a level only the next product reads (its diagonal and
upper blocks, 9 floats each; the gather lists name a lower block as its upper
twin transposed) and the sweep copy's twins written from one quantisation.

Two meshes, B = 5 (odd: the 2-, 4-, 8- and 16-system groups all run partial,
and where n * 3 floats per system is no multiple of four a system's rows
start off the 16-byte grid; rows of 12 bytes meet every 4-byte phase of it):
  ico24  icosphere(24, jitter 0.005), 5762 vertices, tentative transfers,
         levels of 5762 / 752 / 95 / 11 nodes: level 1 is past kSubNodes, so
         k_res3, k_restrict<3>, k_prolong and k_post3 run as kernels; levels 1
         and 2 are packed;
  cap30  spherical_cap(30, zcut 0.6), 1817 vertices, open: smoothed transfers
         and boundary sweeps, levels of 1817 / 230 / 18 nodes; level 1 runs
         inside k_subcycle (the fused levels' global reads and writes) and is
         packed.
Everything here is bit identity except the Galerkin product against the host
P^T A P, which takes test_gpu_amg_setup's derived bound.
"""
import functools

import numpy as np
import pytest

import amg_ref as R
import test_gpu_amg_setup as S
from mofhip import DeviceMesh, synth
from mofhip.mesh import (amg_levels, amg_readback, amg_vcycle, amg_vcycle_tables, assembly_readback,
                         galerkin_launches, vcycle_launches)

pytestmark = pytest.mark.gpu

B = 5
K_SUB_NODES = 512        # mof_amg.h kSubNodes
SENTINEL = 0x7FC0BEEF    # a quiet NaN no kernel produces
MESHES = {"ico24": lambda: synth.icosphere(24, 10.0, jitter=0.005),
          "cap30": lambda: synth.spherical_cap(30, 10.0, 0.6)}
SPLITS = {"one": (5,), "3+2": (3, 2), "single": (1, 1, 1, 1, 1)}


@functools.lru_cache(maxsize=None)
def fields(case):
    p, t = MESHES[case]()
    return (p, synth.vertex_normals(p, t), t, synth.triangle_areas(p, t)), synth.travelling_wave(p, B + 1), \
        np.arange(float(B + 1))


@functools.lru_cache(maxsize=None)
def solved(case, split):
    """V of the B systems solved in the batches of `split` on a fresh handle."""
    (p, n, t, a), I, tk = fields(case)
    m = DeviceMesh(p, n, t, a)
    V, k = [], 0
    for nb in SPLITS[split]:
        Vb, st = m.solve_range(I, tk, k, k + nb, 0.01, precision="mixed", precond="amg", batch=nb)
        assert st["failed"] == st["recovered"] == 0, (case, split, k, st)
        V.append(Vb)
        k += nb
    m.close()
    assert k == B
    return np.concatenate(V)


@functools.lru_cache(maxsize=None)
def run(case):
    """One batch of B solved, the hierarchy and system B - 1's operators read
    back, then the hook's cycles: all systems, the last alone, its neighbour
    alone."""
    (p, n, t, a), I, tk = fields(case)
    g0, c0 = galerkin_launches(), vcycle_launches()
    m = DeviceMesh(p, n, t, a)
    V, st = m.solve_range(I, tk, 0, B, 0.01, precision="mixed", precond="amg", batch=B)
    g1, c1 = galerkin_launches(), vcycle_launches()
    assert st["failed"] == st["recovered"] == 0, st
    H = amg_levels(m)
    lv = H["levels"]
    T = amg_vcycle_tables(m, len(lv), B - 1)
    out = {"H": H, "T": T, "V": V, "gal": {k: g1[k] - g0[k] for k in g0}, "vc": {k: c1[k] - c0[k] for k in c0}}
    a0 = assembly_readback(m, B - 1)
    fp32 = lv[0]["smoothed"] and not H["regular"]
    lev = [{"A": a0["A32"].astype(np.float64).reshape(-1, 2, 2) if fp32 else R.h0_dec(a0["A0h"])}]
    for l in range(1, len(lv)):
        lev.append(amg_readback(m, l, B - 1, lv[l]["n"], lv[l]["sell_nb"], lv[l]["has_Ah"],
                                H["nc"] if l + 1 == len(lv) else 0))
    out["ops"] = lev
    rng = np.random.default_rng(7)
    r = np.stack([rng.standard_normal((lv[0]["n"], 2)) * np.sqrt((assembly_readback(m, b)["rhs"] ** 2).mean())
                  for b in range(B)]).astype(np.float32)
    sizes = [v["n"] for v in lv]
    everyone = tuple(range(B))
    out["full"] = amg_vcycle(m, r, sizes, everyone, sentinel=SENTINEL)
    out["last"] = amg_vcycle(m, r, sizes, everyone, smap=(B - 1,), sentinel=SENTINEL)
    out["before_last"] = amg_vcycle(m, r, sizes, everyone, smap=(B - 2,), sentinel=SENTINEL)
    m.close()
    return out


@pytest.mark.parametrize("case", list(MESHES))
def test_levels_and_formats(case):
    """The mesh has the levels the other checks rely on, and some level keeps
    the packed operator: every level but the coarsest and but a level whose
    product runs from the system slab."""
    d = run(case)
    H, lv, T = d["H"], d["H"]["levels"], d["T"]
    sizes = [v["n"] for v in lv]
    print(case, "levels", sizes, "packed", [v["packed"] for v in lv], "S", T["S"], "smoothed",
          [v["smoothed"] for v in lv], "launches", {k: v for k, v in d["vc"].items() if v},
          {k: v for k, v in d["gal"].items() if v})
    assert len(lv) >= 3 and lv[2]["n"] > 0  # level 2 exists
    assert not lv[0]["packed"] and not lv[-1]["packed"]  # level 0 is not a 3x3 level; k_coarse_inverse's input
    slab = lv[0]["smoothed"] and lv[1]["n"] > K_SUB_NODES
    for l in range(1, len(lv) - 1):
        assert lv[l]["packed"] == (not (l == 1 and slab)), (case, l)
        assert lv[l]["has_Ah"]
    assert any(v["packed"] for v in lv)
    if case == "ico24":
        assert sizes[0] == 5762 and sizes[1] > K_SUB_NODES and not lv[0]["smoothed"] and T["S"] == 2
        # 12-byte rows start at every 4-byte phase of a 16-byte line; with B odd a level of n * 3 floats
        # per system, no multiple of four, also starts its systems off the 16-byte grid (level 2: 95 nodes)
        assert any((3 * n) % 4 for n in sizes[1:]), sizes
        for k in ("res3", "post3", "restrict3", "prolong3", "subcycle", "restrict2", "prolong0_x1"):
            assert d["vc"][k] > 0, (k, d["vc"])
        assert d["gal"]["galerkin0_ent"] > 0 and d["gal"]["galerkin3_ent"] > 0
    else:
        assert lv[0]["smoothed"] and T["bsw_n"] > 0 and T["S"] == 1  # open: smoothed transfers, boundary sweeps
        for k in ("subcycle", "restrict0_sa2", "prolong0_sa_x2", "bsweep_h", "bsweep_f"):
            assert d["vc"][k] > 0, (k, d["vc"])
        assert d["gal"]["galerkin_sys2_f32"] > 0 and d["gal"]["galerkin3_ent"] + d["gal"]["galerkin3_big"] > 0


@pytest.mark.parametrize("case", list(MESHES))
def test_v_independent_of_the_batch_split(case):
    """V of the B systems byte for byte whether they are solved in one batch,
    as 3 + 2 or one at a time: a wrong per-system stride or a row straddling
    two systems changes a neighbour's bits."""
    one = solved(case, "one")
    assert np.isfinite(one).all()
    assert run(case)["V"].tobytes() == one.tobytes()
    for split in ("3+2", "single"):
        assert solved(case, split).tobytes() == one.tobytes(), (case, split)


def same_system(a, b, s):
    ok = np.array_equal(a["z_words"][s], b["z_words"][s]) and a["rz"][s].tobytes() == b["rz"][s].tobytes()
    ok = ok and np.array_equal(a["sys"][s]["r1"], b["sys"][s]["r1"])
    for la, lb in zip(a["sys"][s]["coarse"][1:], b["sys"][s]["coarse"][1:]):
        for k in la:
            ok = ok and la[k].tobytes() == lb[k].tobytes()
    return bool(ok)


@pytest.mark.parametrize("case", list(MESHES))
def test_cycle_of_one_system_and_the_hook_layout(case):
    """The last system's z, r1 and coarse vectors are the same bits when it
    runs alone; a system the cycle skips keeps the sentinel in every word the
    hook returns (its neighbour's first and last rows included). The hook's
    rows stay 16 bytes: three floats and a fourth word that is 0 on a written
    row and the sentinel on a row still holding it."""
    d = run(case)
    lv = d["H"]["levels"]
    full, last, prev = d["full"], d["last"], d["before_last"]
    assert same_system(full, last, B - 1)
    assert same_system(full, prev, B - 2)
    for o, ran in ((last, B - 1), (prev, B - 2)):
        for s in range(B):
            if s == ran:
                continue
            assert (o["z_words"][s] == SENTINEL).all() and (o["sys"][s]["r1"] == SENTINEL).all() and o["rz"][s] == 0.0
            for lev in o["sys"][s]["coarse"][1:]:
                for k in lev:
                    assert (lev[k].view(np.uint32) == SENTINEL).all(), (case, ran, s, k)
    for s in range(B):
        for l, lev in enumerate(full["sys"][s]["coarse"][1:], start=1):
            for k in lev:
                w = lev[k].view(np.uint32)
                assert w.shape == (lv[l]["n"], 4)
                if l == len(lv) - 1 and k in ("x", "r"):  # the coarsest level has no pre-smoothing and no residual
                    assert (w == SENTINEL).all(), (case, s, l, k)
                else:
                    assert (w[:, 3] == 0).all() and np.isfinite(lev[k][:, :3]).all(), (case, s, l, k)


@pytest.mark.parametrize("case", list(MESHES))
def test_operator_readback(case):
    """The read-back keeps [sell_nb][12] on a packed level: every lower block
    is its upper twin's transpose to the bit, the twin's sweep-copy words hold
    the same scale and the transposed codes, what no product writes is zero,
    and A is P^T A P of the level below within the products' derived bound."""
    d = run(case)
    lv, lev = d["H"]["levels"], d["ops"]
    for l in range(1, len(lv)):
        C, r = lv[l], lev[l]
        A = r["A"]
        up = np.flatnonzero(C["twin"] >= 0)
        assert len(up) > 0 and (C["sell_col"][up] > C["sell_row"][up]).all()
        assert A[C["twin"][up], :, :3].tobytes() == np.ascontiguousarray(A[up, :, :3].transpose(0, 2, 1)).tobytes()
        assert (A[:, :, 3].view(np.uint32) == 0).all()
        written = np.zeros(C["sell_nb"], dtype=bool)
        written[R.stored_positions(C)] = True
        assert written[up].all() and written[C["twin"][up]].all()
        assert (A[~written].view(np.uint32) == 0).all() and np.abs(A[written]).max() > 0
        if C["has_Ah"]:
            codes, scale = R.a9_dec(r["Ah"], r["Ah22"])
            assert np.array_equal(scale[C["twin"][up]].view(np.uint32), scale[up].view(np.uint32))
            assert np.array_equal(codes[C["twin"][up]], codes[up].transpose(0, 2, 1))
            m = np.abs(A[written, :, :3]).reshape(-1, 9).max(axis=1)
            assert np.array_equal(R.bf16_bits(scale[written]), R.bf16_bits(m / np.float32(127.0)))
    for l in range(len(lv) - 1):
        fine = lev[l]["A"] if l == 0 else S.blocks33(lev[l])
        pos, err, bound, low = S.product_check(lv[l], lv[l + 1], fine, S.blocks33(lev[l + 1]))
        ratio = float(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)).max())
        print("%s level %d -> %d (%s source): max error / bound %.3f over %d blocks, %d of them lower twins"
              % (case, l, l + 1, "packed" if lv[l]["packed"] else "unpacked", ratio, len(pos), int(low.sum())))
        assert (err <= bound).all(), (case, l, ratio)
