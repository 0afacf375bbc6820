"""The multigrid V-cycle (amg_vcycle in csrc/mof_amg.hip) against the fp64
checker tests/vcycle_ref.py: every kernel of the cycle on the input it really
read, then the cycle as a whole operator.

Every case builds a handle, runs one multigrid solve of exactly one batch (so
the batch's operators are live), reads back the operators of a few systems
(as tests/test_gpu_amg_setup.py does) and applies the production cycle to
residuals of its own through mof_test_amg_vcycle: the hook uploads r, writes
the pre-smoothed x0 with the PCG's own expression, calls amg_vcycle and reads
back level 0's iterate at four taps, level 0's r1, every coarse vector and z.
Each system gets another r: 0 a seeded normal vector scaled to the system's
right-hand side, 1 zero (z must be exactly zero), 2 the right-hand side
itself (batches of 5, and flat7, whose right-hand side cancels too much in
stage 3: another normal vector), 3 the right-hand side, 4 an impulse at one
vertex (a boundary vertex on an open mesh), 5 and up further normal vectors.

The chain (stage_checks): the taps and the end state lead from r to z without
a gap, every stage's reference is computed from the buffers the previous
stages' checks validated:
   1 x0 = w D0^-1 r (bf16)                       2 the pre-sweep on the ring
   3 r1 = r - A0h x0 (bf16, member order)        4 b_{l+1} = P^T r_l
   5 r_l = b_l - A_l (w1 D_l^-1 b_l)             6 y = cinv b
   7 x_l = w1 D_l^-1 b_l + P y_{l+1}             8 y_l = x_l + w1 D^-1 (b_l - A_l x_l)
   9 x = x0 + P y_1 (bf16 or float2)            10 the post-sweep
  11 z = x + w D0^-1 (r - A0h x)                12 r.z of the kernel's own z
The coarsest level has no pre-smoothing (amg_vcycle: smooth = l + 1 < L - 1).

Bounds (vcycle_ref.bound_*): a value summed in fp32 from k products whose
absolute values sum to S is within (k + c) 2^-24 S of the exact one, S taken
in fp64 from the same inputs:
   1 k = 2 (the two products of a row of the 2 x 2 solve), c = 6 (determinant,
     reciprocal, the subtraction, times 1 / det, times w, one spare);
   3, 5 k = the row's products (bs per stored block), c = 1 (b - A x);
     5 adds |A| beta(x_pre): the pre-smoothed x_l is overwritten by the
     prolongation, so the reference recomputes it (k = 3, c = 1);
   4 k = the products of the coarse dof's column of P, c = 1;
   6 k = nc, c = 4 (the four k ranges' partial sums);
   7, 9 k = 3 per P block of the row, c = 2; 7 adds beta(x_pre);
   8, 11 the residual's k, c = 8 (its subtraction, D^-1 -- a 2 x 2 solve or
     3 products --, w, the add to x), all under w |D^-1|, plus 2 u (|x| + ...)
     for the last add;
   2, 10 stage 11's bound sweep by sweep on the ring rows, the second sweep
     adding w |D^-1| |A| beta(first sweep); rows off the ring bit-identical;
  12 fp64: 2 N 2^-53 sum |r z| (the products of two floats are exact).
A value stored as bf16 must lie between bf16(e - beta) and bf16(e + beta): a
flipped rounding and nothing more; at most 5 % of a stage's windows may span
two bf16 values.

Largest error / bound per kernel instance seen on an MI355X
(test_stage_chain prints them, -s; for a bf16 output error / (bound + half a
bf16 ulp), at most 1 by the window):
  pre-smooth 1.00   k_bsweep<false> 1.00   k_bsweep<true> 0.03
  k_res0_ns 1.00 (plain), 1.00 (packed)   k_restrict<2,2> 0.19   k_restrict<3> 0.13
  k_restrict0_sa<2> 0.12   k_restrict0_sa<3> 0.02   k_res3 0.08   k_post3 0.07
  k_subcycle 0.10 (restriction) 0.11 (residual) 0.11 (coarsest solve)
             0.49 (prolongation) 0.07 (post-smoothing)
  k_prolong 0.44   k_prolong_sa<3,0,8> 0.26   k_prolong0<1> 1.00   k_prolong0<2> 0.46
  k_prolong_sa<2,1,16> 1.00   k_prolong_sa<2,2,16> 0.44
  k_post0_ns with float2 z 0.08 .. 0.14, with bf16 z 1.00 (four instances each)
  r.z partials <= 0.005
and at most 3.1 % of a stage's bf16 windows span two values (stage 3).
Whole operator (test_whole_operator): asymmetry 2 .. 3e-16; G1_ico642 eig(M A)
in [0.265 .. 0.268, 1.0005 .. 1.0015], |z - M r| / |M r| 1.6 .. 1.8e-3;
G2_cap641 [0.355 .. 0.365, 1.025 .. 1.028], 3.5 .. 9.2e-4.

Two faults these tests found, both fixed: the bf16 diagonal block of level 0
stored a01 and a10 rounded separately (G1_ico642's system 4: the cycle
symmetric to 1.6e-7 of its norm only), and on plain-read meshes the bf16
copy's lower blocks rounded apart from their upper twins (hull3000: max
|a_ij - a_ji| 2.4e-7); test_whole_operator and
test_stored_operators_symmetric hold both.

Every instance amg_vcycle can launch runs in some case, and each case
asserts its own (the launch counters, mof_test_vcycle_launches): both
k_res0_ns, k_restrict<2,2>, <3>, k_restrict0_sa<2>, <3>, k_res3, k_subcycle,
k_prolong (counter prolong3), k_prolong_sa<3,0,8> (prolong3_sa), k_prolong0<1>,
<2>, k_prolong_sa<2,1,16>, <2,2,16> (prolong0_sa_x1, _x2), k_post3, both
k_bsweep and all eight k_post0_ns<XM, ZH, 2, PK> (the forced z format gives
each mesh its second one; the unpacked XM = 1 pair needs the 32-bit index
tables forced on a regular mesh, G1_ico642_index32). Two cases fill the
multi-system groups (SysGroup): G1_ico642_smoothed_b17's 17 systems make one
full 16-system prolongation group and two full 8-system restriction groups,
each beside a group of one, hull_chain_b9's 9 one full group of 8 and a group
of one in level 1's smoothed transfers (G1_ico642 records 16 frames: the b17
case takes the golden mesh under the synthetic travelling wave). k_to_h0 is
not reachable: every multigrid solve's assembly writes the bf16 copy itself;
the transfers' oversized-group branches (more than kRG members, more than kRGS
list entries) are built by no mesh of the suite.
"""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

import amg_ref as R
import test_gpu_amg_setup as S
import vcycle_ref as V
from conftest import load_golden
from mofhip import DeviceMesh, synth
from mofhip.mesh import (amg_levels, amg_readback, amg_vcycle, amg_vcycle_tables, assembly_readback, force_index32,
                         vcycle_launches)

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF   # a quiet NaN no kernel produces
TWO_VALUED_CAP = 0.05

# case -> (mesh, batch, systems read back, MOF_AMG_SMOOTH, zh of the second run, instances that must have run;
#          _pk: the packed index words, which every symmetric-read mesh of these sizes takes)
CASES = {
    "G1_ico642": ("G1_ico642", 5, (0, 3, 4), None, 0,
                  ("res0_ns_pk", "restrict2", "subcycle", "prolong0_x1", "post0_x1_zh_pk")),
    "G1_ico642_smoothed": ("G1_ico642", 5, (0, 4), "1", None, ("restrict0_sa2", "prolong0_sa_x1", "subcycle")),
    "G2_cap641": ("G2_cap641", 5, (0, 4), None, 1,
                  ("bsweep_h", "bsweep_f", "restrict0_sa2", "prolong0_sa_x2", "post0_x2_zf_pk")),
    "hull3000": ("hull3000", 3, (0, 2), "0", 1, ("res0_ns", "restrict2", "prolong0_x2", "post0_x2_zf")),
    "hull_chain": ("hull_chain", 3, (0, 2), None, None, ("res3", "restrict0_sa3", "prolong3_sa", "post3", "subcycle")),
    "ico32": ("ico32", 3, (0, 2), None, None, ("res3", "restrict3", "prolong3", "post3", "subcycle")),
    "S1s": ("S1s", 3, (0, 2), None, 1, ("res0_ns_pk", "post0_x2_zf_pk", "bsweep_h", "bsweep_f")),
    "flat7": ("flat7", 3, (0, 2), None, None, ("subcycle",)),
    # the 32-bit index tables forced (mof_test_force_index32): the mirrored, unpacked instances on a regular mesh
    "G1_ico642_index32": ("G1_ico642", 5, (0, 3, 4), None, 0, ("res0_ns", "restrict2", "prolong0_x1", "post0_x1_zh")),
    # full system groups beside a group of one: 17 = one 16-system prolongation group + 1 = two 8-system
    # restriction groups + 1; 9 = one 8-system group + 1 for level 1's prolongation (kNS3) and restriction (kNSR)
    "G1_ico642_smoothed_b17": ("G1_ico642", 17, (0, 8, 16), "1", None,
                               ("restrict0_sa2", "prolong0_sa_x1", "subcycle")),
    "hull_chain_b9": ("hull_chain", 9, (0, 7, 8), None, None,
                      ("res3", "restrict0_sa3", "prolong3_sa", "post3", "subcycle")),
}
INDEX32 = ("G1_ico642_index32",)
# the instance the second run (forced zh) adds
OTHER_ZH = {"G1_ico642": "post0_x1_zf_pk", "G2_cap641": "post0_x2_zh_pk", "S1s": "post0_x2_zh_pk",
            "hull3000": "post0_x2_zh", "G1_ico642_index32": "post0_x1_zf"}


def x0dec(words):
    """the x0 format: one uint32 per vertex, two bf16 -> (N, 2) float64"""
    w = np.ascontiguousarray(words, dtype=np.uint32)
    return np.stack([(w << np.uint32(16)).view(np.float32), (w & np.uint32(0xFFFF0000)).view(np.float32)],
                    axis=-1).astype(np.float64)


def f2dec(words):
    return np.ascontiguousarray(words, dtype=np.uint32).view(np.float32).astype(np.float64)


def boundary_vertex(adj):
    """A vertex with an edge that lies in one triangle only (its two ends have
    one common neighbour), from the level-0 adjacency; None on a closed mesh."""
    adj = sp.lil_matrix(adj)
    adj.setdiag(0)
    adj = adj.tocsr()
    adj.eliminate_zeros()
    common = (adj @ adj).tocsr()
    for i in range(adj.shape[0]):
        for j in adj.indices[adj.indptr[i]:adj.indptr[i + 1]]:
            if j != i and common[i, j] == 1:
                return i
    return None


def inputs(B, N, rhs, adj, open_surface, smooth_rhs=True):
    rng = np.random.default_rng(20)
    r = np.zeros((B, N, 2), dtype=np.float32)
    kinds = {0: "normal", 1: "zero", 2: "rhs" if B == 3 and smooth_rhs else "normal", 3: "rhs", 4: "impulse"}
    kinds.update({b: "normal" for b in range(5, B)})
    v = boundary_vertex(adj) if open_surface else N // 3
    assert v is not None
    for b in range(B):
        k = kinds[b]
        scale = np.sqrt((rhs[b] ** 2).mean())
        if k == "normal":
            r[b] = rng.standard_normal((N, 2)) * scale
        elif k == "rhs":
            r[b] = rhs[b]
        elif k == "impulse":
            r[b, v] = (scale, -0.5 * scale)
    return r, kinds


def build_cycle(H, T, lev):
    """The vcycle_ref.Cycle of one system from its read-back operators."""
    lv = H["levels"]
    L = len(lv)
    l0 = lv[0]
    mir = l0["mirror"]
    # the row kernels' own reads: through the mirror table, or every block at its position
    level0 = l0 if l0["sym"] else dict(l0, mirror=np.where(mir >= 0, np.arange(len(mir)), -1).astype(mir.dtype))
    assert np.array_equal(l0["diag_pos"], l0["sell_off"][np.arange(l0["n"]) >> 6] + (np.arange(l0["n"]) & 63))
    blk0 = R.h0_dec(lev[0]["A0h"])
    A = [R.sell_to_csr(level0, blk0)]
    Dinv = [V.block_diag(np.linalg.inv(blk0[l0["diag_pos"]]))]
    for l in range(1, L):
        if lv[l]["has_Ah"]:
            codes, scale = R.a9_dec(lev[l]["Ah"], lev[l]["Ah22"])
            blk = (codes - 128).astype(np.float64) * scale.astype(np.float64)[:, None, None]
        else:
            blk = S.blocks33(lev[l])
        A.append(R.sell_to_csr(lv[l], blk))
        if l < L - 1:
            Dinv.append(V.block_diag(R.h9_dec(lev[l]["Dh"], lev[l]["Dh22"])))
    P = [R.prolongator(lv[l], lv[l + 1]["n"]) for l in range(L - 1)]
    ring = None
    if T["bsw_n"]:
        ring = (2 * T["bsw_rows"].astype(np.int64)[:, None] + np.arange(2)[None]).ravel()
    return V.Cycle(A, Dinv, P, lev[-1]["cinv"].astype(np.float64).T, H["omega"], H["omega1"], ring=ring,
                   sweeps=T["bsw_sweeps"])


@functools.lru_cache(maxsize=None)
def run(case):
    """One batch solved, the operators read back, then the hook's runs: all
    systems with and without the taps, a mapped subset, retired neighbours,
    and where the case has one the other z format."""
    name, B, systems, smooth, zh_other, _ = CASES[case]
    if name.startswith("G") and len(load_golden(name)["I"]) < B + 1:
        # a batch longer than the golden recording (G1_ico642: 16 frames): the golden mesh under the
        # synthetic meshes' travelling wave
        g = load_golden(name)
        p, n, t, a, lam = g["coordinates"], g["normals"], g["triangles"], g["areas"], float(g["lambda_"])
        I, tk = synth.travelling_wave(p, B + 1), np.arange(float(B + 1))
    else:
        (p, n, t, a), I, tk, lam = S.mesh_and_fields(name, B + 1)
    old = os.environ.get("MOF_AMG_SMOOTH")
    if smooth is not None:
        os.environ["MOF_AMG_SMOOTH"] = smooth  # read when the handle's hierarchy is built
    try:
        if case in INDEX32:
            with force_index32():
                m = DeviceMesh(p, n, t, a)
        else:
            m = DeviceMesh(p, n, t, a)
        Vs, st = m.solve_range(I, tk, 0, B, lam, precision="mixed", precond="amg", batch=B)
    finally:
        if smooth is not None:
            if old is None:
                del os.environ["MOF_AMG_SMOOTH"]
            else:
                os.environ["MOF_AMG_SMOOTH"] = old
    assert Vs.shape[0] == B and st["failed"] == st["recovered"] == 0, st
    H = amg_levels(m)
    lv = H["levels"]
    T = amg_vcycle_tables(m, len(lv), systems[0])
    sizes = [v["n"] for v in lv]
    N = sizes[0]
    out = {"H": H, "T": T, "ops": {}, "ring": {}}
    rhs = np.stack([assembly_readback(m, b)["rhs"] for b in range(B)])
    for s in systems:
        lev = [{"A0h": assembly_readback(m, s)["A0h"]}]
        for l in range(1, len(lv)):
            lev.append(amg_readback(m, l, s, lv[l]["n"], lv[l]["sell_nb"], lv[l]["has_Ah"],
                                    H["nc"] if l + 1 == len(lv) else 0))
        out["ops"][s] = lev
        if T["bsw_n"]:
            out["ring"][s] = amg_vcycle_tables(m, len(lv), s)["bsw_A"]
    stored = R.stored_positions(lv[0])
    adj = sp.coo_matrix((np.ones(int(stored.sum())), (lv[0]["sell_row"][stored], lv[0]["sell_col"][stored])),
                        shape=(N, N)).tocsr()
    # flat7's right-hand side (49 vertices in a plane) cancels in r - A x0 until 12 % of stage 3's
    # windows span two bf16 values: its system 2 takes a second normal vector
    r, kinds = inputs(B, N, rhs, adj, T["bsw_n"] > 0, smooth_rhs=case != "flat7")
    out.update(r=r, kinds=kinds)
    everyone = tuple(range(B))
    c0 = vcycle_launches()
    out["full"] = amg_vcycle(m, r, sizes, everyone, tap=True, sentinel=SENTINEL)
    c1 = vcycle_launches()
    out["ran"] = {k: c1[k] - c0[k] for k in c0}
    out["notap"] = amg_vcycle(m, r, sizes, everyone, sentinel=SENTINEL)
    # an odd number of the systems read back, in another order than their slots: every multi-system
    # group of the launch (2, 4, 8, 16 systems) is partial
    out["subset_map"] = tuple(reversed(systems)) if len(systems) % 2 else (systems[-1],)
    out["subset"] = amg_vcycle(m, r, sizes, everyone, smap=out["subset_map"], sentinel=SENTINEL)
    out["retired_mask"] = np.array([b not in systems for b in range(B)], dtype=np.uint8)
    out["retired"] = amg_vcycle(m, r, sizes, everyone, retired=out["retired_mask"], sentinel=SENTINEL)
    if zh_other is not None:
        c1 = vcycle_launches()
        out["other"] = amg_vcycle(m, r, sizes, everyone, zh=zh_other, tap=True, sentinel=SENTINEL)
        c2 = vcycle_launches()
        out["ran_other"] = {k: c2[k] - c1[k] for k in c1}
    m.close()
    return out


@functools.lru_cache(maxsize=None)
def cycle_of(case, s):
    d = run(case)
    return build_cycle(d["H"], d["T"], d["ops"][s])


def kernel_names(d, o, ran):
    """The instance behind each stage of this run."""
    lv, Sx = d["H"]["levels"], o["S"]
    post0 = [k for k in ran if k.startswith("post0_") and ran[k] > 0]
    assert len(post0) == 1, ran
    names = {"res0": "res0_ns_pk" if ran["res0_ns_pk"] else "res0_ns",
             "restrict0": "restrict0_sa2" if lv[0]["smoothed"] else "restrict2",
             "prolong0": ("prolong0_sa_x%d" if lv[0]["smoothed"] else "prolong0_x%d") % o["xm"],
             "post0": post0[0], "bsweep_pre": "bsweep_h", "bsweep_post": "bsweep_f" if o["xm"] == 2 else "bsweep_h"}
    for l in range(1, len(lv)):
        sub = l >= Sx
        names["res", l] = "subcycle" if sub else "res3"
        names["restrict", l] = "subcycle" if sub else ("restrict0_sa3" if lv[l]["smoothed"] else "restrict3")
        names["prolong", l] = "subcycle" if sub else ("prolong3_sa" if lv[l]["smoothed"] else "prolong3")
        names["post", l] = "subcycle" if sub else "post3"
    return names


def stage_checks(c, d, o, s, names, sweeps=None, P0_restrict=None, y1=None):
    """The twelve stages of system s of the hook run o against the cycle c:
    a list of (stage, level, kernel, all within the bound, share of two-valued
    bf16 windows, largest error / bound). sweeps / P0_restrict / y1: a
    reference wrong in that one thing (the negative controls)."""
    T, L = d["T"], c.L
    sy = o["sys"][s]
    taps, coarse = sy["taps"], sy["coarse"]
    r = d["r"][s].astype(np.float64).ravel()
    ring = c.ring
    off = np.ones(len(r), dtype=bool)
    if ring is not None:
        off[ring] = False
    recs = []

    def add(stage, l, kernel, res, exact=True):
        ok, two, ratio = res
        recs.append((stage, l, kernel, bool(np.all(ok)) and bool(exact), two, ratio))

    def vec3(a):
        return a[:, :3].astype(np.float64).ravel()

    def nodes3(a, l):  # a level's r: stored at the member positions
        return a[T["levels"][l]["apos"], :3].astype(np.float64).ravel()

    t0, t1 = x0dec(taps[0]).ravel(), x0dec(taps[1]).ravel()
    add(1, 0, "presmooth", V.check_bf16(t0, V.pre_smooth(c, 0, r), V.bound_pre_smooth(c, 0, r)))
    if ring is None:
        assert np.array_equal(taps[0], taps[1])
    else:
        e, beta = V.ring_sweeps(c, r, t0, sweeps), V.bound_ring_sweeps(c, r, t0, sweeps)
        same = np.array_equal(np.repeat(taps[0], 2)[off], np.repeat(taps[1], 2)[off])
        add(2, 0, names["bsweep_pre"], V.check_bf16(t1[ring], e[ring], beta[ring]), same)
    r1 = x0dec(sy["r1"])[T["levels"][0]["apos"]].ravel()
    add(3, 0, names["res0"], V.check_bf16(r1, V.residual(c, 0, r, t1), V.bound_residual(c, 0, r, t1)))
    cr = c if P0_restrict is None else c.copy(P=[P0_restrict] + c.P[1:])
    b = {1: vec3(coarse[1]["b"])}
    add(4, 0, names["restrict0"], V.check_f32(b[1], V.restrict(cr, 0, r1), V.bound_restrict(cr, 0, r1)))
    xpre, bpre = {}, {}
    for l in range(1, L - 1):
        xpre[l], bpre[l] = V.pre_smooth(c, l, b[l]), V.bound_pre_smooth(c, l, b[l])
        rl = nodes3(coarse[l]["r"], l)
        add(5, l, names["res", l], V.check_f32(rl, V.residual(c, l, b[l], xpre[l]),
                                               V.bound_residual(c, l, b[l], xpre[l], bpre[l])))
        b[l + 1] = vec3(coarse[l + 1]["b"])
        add(4, l, names["restrict", l], V.check_f32(b[l + 1], V.restrict(c, l, rl), V.bound_restrict(c, l, rl)))
    y = vec3(coarse[L - 1]["y"])
    add(6, L - 1, "subcycle", V.check_f32(y, V.coarsest(c, b[L - 1]), V.bound_coarsest(c, b[L - 1])))
    for l in range(L - 2, 0, -1):
        xl = vec3(coarse[l]["x"])
        add(7, l, names["prolong", l], V.check_f32(xl, V.prolong(c, l, xpre[l], y),
                                                   V.bound_prolong(c, l, xpre[l], y, bpre[l])))
        yl = vec3(coarse[l]["y"])
        add(8, l, names["post", l], V.check_f32(yl, V.post_smooth(c, l, b[l], xl),
                                                V.bound_post_smooth(c, l, b[l], xl)))
        y = yl
    if y1 is not None:
        y = y1
    bf = o["xm"] == 1  # the corrected iterate: the x0 format in place, or float2
    dec = (lambda t: x0dec(t).ravel()) if bf else (lambda t: f2dec(t).ravel())
    chk = V.check_bf16 if bf else V.check_f32
    t2, t3 = dec(taps[2]), dec(taps[3])
    add(9, 0, names["prolong0"], chk(t2, V.prolong(c, 0, t1, y), V.bound_prolong(c, 0, t1, y)))
    if ring is None:
        assert np.array_equal(taps[2], taps[3])
    else:
        e, beta = V.ring_sweeps(c, r, t2, sweeps), V.bound_ring_sweeps(c, r, t2, sweeps)
        w2, w3 = (np.repeat(taps[k], 2) if bf else taps[k].ravel() for k in (2, 3))
        add(10, 0, names["bsweep_post"], chk(t3[ring], e[ring], beta[ring]), np.array_equal(w2[off], w3[off]))
    z = o["z"][s].astype(np.float64).ravel()
    add(11, 0, names["post0"], (V.check_bf16 if o["zh"] else V.check_f32)(
        z, V.post_smooth(c, 0, r, t3), V.bound_post_smooth(c, 0, r, t3)))
    rz = float(r @ z)
    add(12, 0, names["post0"] + " r.z", V.check_f32(np.array([o["rz"][s]]), np.array([rz]),
                                                     np.array([2 * len(r) * 2.0 ** -53 * float(np.abs(r) @ np.abs(z))])))
    return recs


RATIOS = {}


def chain(case, which, ran_key):
    d = run(case)
    o, ran = d[which], d[ran_key]
    names = kernel_names(d, o, ran)
    zero = [b for b, k in d["kinds"].items() if k == "zero" and b < len(d["r"])]
    for b in zero:
        assert (o["z"][b] == 0).all() and o["rz"][b] == 0.0, (case, b)
    for s in CASES[case][2]:
        for stage, l, k, ok, two, ratio in stage_checks(cycle_of(case, s), d, o, s, names):
            RATIOS[k] = max(RATIOS.get(k, 0.0), ratio)
            print("%s (%s) system %d (%s) stage %2d level %d %-18s error / bound %.3f, two-valued windows %.3f"
                  % (case, which, s, d["kinds"][s], stage, l, k, ratio, two))
            assert ok, (case, s, stage, l, k, ratio)
            assert two <= TWO_VALUED_CAP, (case, s, stage, l, k, two)
    print("largest error / bound so far:", {k: round(v, 3) for k, v in sorted(RATIOS.items())})


@pytest.mark.parametrize("case", list(CASES))
def test_stage_chain(case):
    """Every stage of the cycle within its derived bound of the fp64 reference
    on the input its kernel read, for every system read back; the zero system's
    z exactly zero; the instances the case claims did run."""
    d = run(case)
    print(case, "levels", [v["n"] for v in d["H"]["levels"]], "S", d["full"]["S"], "xm", d["full"]["xm"], "zh",
          d["full"]["zh"], "launches", {k: v for k, v in d["ran"].items() if v})
    for k in CASES[case][5]:
        assert d["ran"][k] > 0, (k, d["ran"])
    if case.startswith("G1_ico642"):
        assert d["full"]["S"] == 1 and d["ran"]["res3"] == d["ran"]["post3"] == 0  # every coarse level fused
    if case == "S1s":
        assert d["H"]["levels"][0]["sym"]
    if case == "flat7":
        assert sum(int(v["dead"].sum()) for v in d["H"]["levels"]) > 0  # dead coarse dofs
    assert d["full"]["zh"] == d["T"]["zh"] and d["full"]["xm"] == d["T"]["xm"]
    chain(case, "full", "ran")


@pytest.mark.parametrize("case", list(OTHER_ZH))
def test_stage_chain_other_z_format(case):
    """The same with z's other format forced (k_post0_ns's remaining instances)."""
    d = run(case)
    assert d["other"]["zh"] != d["full"]["zh"]
    assert d["ran_other"][OTHER_ZH[case]] > 0, d["ran_other"]
    chain(case, "other", "ran_other")
    for s in CASES[case][2]:  # nothing before k_post0_ns depends on it
        assert same_state(d["full"], d["other"], s, z=False)


def same_state(a, b, s, z=True):
    """System s's z, r1 and every coarse vector bit for bit."""
    ok = not z or (a["zh"] == b["zh"] and np.array_equal(a["z_words"][s], b["z_words"][s]) and
                   a["rz"][s].tobytes() == b["rz"][s].tobytes())
    ok = ok and np.array_equal(a["sys"][s]["r1"], b["sys"][s]["r1"])
    for la, lb in zip(a["sys"][s]["coarse"][1:], b["sys"][s]["coarse"][1:]):
        for k in la:
            ok = ok and la[k].tobytes() == lb[k].tobytes()
    return ok


def untouched(o, s):
    """System s's z, r1 and coarse vectors still hold the sentinel."""
    ok = (o["z_words"][s] == SENTINEL).all() and (o["sys"][s]["r1"] == SENTINEL).all() and o["rz"][s] == 0.0
    for lev in o["sys"][s]["coarse"][1:]:
        for k in lev:
            ok = ok and (lev[k].view(np.uint32) == SENTINEL).all()
    return bool(ok)


@pytest.mark.parametrize("case", list(CASES))
def test_tap_changes_nothing(case):
    """z and every buffer the cycle leaves are bit-identical with and without
    the taps."""
    d = run(case)
    assert np.array_equal(d["full"]["z_words"], d["notap"]["z_words"])
    assert d["full"]["rz"].tobytes() == d["notap"]["rz"].tobytes()
    for s in range(len(d["r"])):
        assert same_state(d["full"], d["notap"], s), (case, s)
        assert not d["notap"]["sys"][s]["taps"]


@pytest.mark.parametrize("case", list(CASES))
def test_systems_sharing_a_launch(case):
    """A system's bits do not depend on which systems share its launches: all B,
    a mapped subset of odd count in another slot order (every 2-, 4-, 8- and
    16-system group partial), retired neighbours. Unmapped and retired systems
    keep every byte of their z and level buffers."""
    d = run(case)
    B = len(d["r"])
    assert len(d["subset_map"]) % 2 == 1
    for which, live in (("subset", d["subset_map"]), ("retired", [b for b in range(B) if not d["retired_mask"][b]])):
        assert 0 < len(live) < B
        for s in range(B):
            if s in live:
                assert same_state(d["full"], d[which], s), (case, which, s)
            else:
                assert untouched(d[which], s), (case, which, s)


def test_packed_index_words_change_no_bit():
    """The cycle with the packed index words and with the 32-bit tables: the
    same bits in z and in every buffer it leaves."""
    a, b = run("G1_ico642"), run("G1_ico642_index32")
    assert a["ran"]["res0_ns_pk"] and b["ran"]["res0_ns"] and not b["ran"]["res0_ns_pk"]
    assert np.array_equal(a["r"], b["r"])
    for which in ("full", "other"):
        assert np.array_equal(a[which]["z_words"], b[which]["z_words"])
        for s in range(len(a["r"])):
            assert same_state(a[which], b[which], s), (which, s)


@pytest.mark.parametrize("case", list(CASES))
def test_stored_operators_symmetric(case):
    """What the cycle's symmetry rests on, on every mesh: the operators the
    sweeps read (level 0's bf16 copy as the row kernels read it -- through the
    mirror table, or block by block on a plain-read mesh --, the int8 copies),
    the stored D^-1 and the coarsest inverse are symmetric to the bit."""
    d = run(case)
    lv = d["H"]["levels"]
    for s in CASES[case][2]:
        c = cycle_of(case, s)
        for l, A in enumerate(c.A[:-1]):
            assert abs(A - A.T).max() == 0.0, (case, s, "A", l, abs(A - A.T).max())
        blk0 = R.h0_dec(d["ops"][s][0]["A0h"])[lv[0]["diag_pos"]]  # the smoother's D on level 0
        assert np.array_equal(blk0[:, 0, 1], blk0[:, 1, 0]), (case, s)
        for l in range(1, len(lv) - 1):
            D = R.h9_bits(d["ops"][s][l]["Dh"], d["ops"][s][l]["Dh22"])
            assert np.array_equal(D, D.transpose(0, 2, 1)), (case, s, "D^-1", l)
        assert np.array_equal(c.cinvT, c.cinvT.T), (case, s, V.asymmetry(c.cinvT))


def failing(recs):
    return {(stage, l) for stage, l, _, ok, _, _ in recs if not ok}


def test_negative_controls():
    """A reference wrong in one thing is reported by the stage that thing
    belongs to (and the right reference by none)."""
    d = run("G1_ico642")
    o, s = d["full"], 0
    names = kernel_names(d, o, d["ran"])
    c = cycle_of("G1_ico642", s)
    assert c.L >= 3 and not failing(stage_checks(c, d, o, s, names))
    # w1 = 1.05 for 1.1: the coarse residual, prolongation and post-smoothing
    bad = failing(stage_checks(c.copy(w1=c.w1 * 1.05 / 1.1), d, o, s, names))
    assert {(5, 1), (7, 1), (8, 1)} <= bad and not {(1, 0), (3, 0), (4, 0), (9, 0), (11, 0)} & bad, bad
    print("w1 1.05 for 1.1: caught at", sorted(bad))
    # one member dropped from one aggregate's restriction
    P0 = c.P[0].tolil()
    col = 3 * (c.P[0].shape[1] // 6)
    rows = c.P[0].tocsc()[:, col].nonzero()[0]
    P0[rows[len(rows) // 2] // 2 * 2:rows[len(rows) // 2] // 2 * 2 + 2, :] = 0.0
    bad = failing(stage_checks(c, d, o, s, names, P0_restrict=P0.tocsr()))
    assert bad == {(4, 0)}, bad
    print("one member dropped from an aggregate's restriction: caught at", sorted(bad))
    # a coarse block read untransposed where its twin is meant
    lv1 = d["H"]["levels"][1]
    up = np.flatnonzero(lv1["twin"] >= 0)
    A1 = c.A[1].tolil()
    blocks = [(int(lv1["sell_row"][p]), int(lv1["sell_col"][p])) for p in up]
    asym = [(i, j) for i, j in blocks if not np.allclose(A1[3 * i:3 * i + 3, 3 * j:3 * j + 3].toarray(),
                                                         A1[3 * i:3 * i + 3, 3 * j:3 * j + 3].toarray().T)]
    i, j = asym[len(asym) // 2]
    A1[3 * j:3 * j + 3, 3 * i:3 * i + 3] = A1[3 * i:3 * i + 3, 3 * j:3 * j + 3].toarray()  # the twin: not transposed
    bad = failing(stage_checks(c.copy(A=[c.A[0], A1.tocsr()] + c.A[2:]), d, o, s, names))
    assert bad and bad <= {(5, 1), (8, 1)}, bad
    print("a coarse twin block read untransposed: caught at", sorted(bad))
    # y of the next system read back prolonged into this one
    other = CASES["G1_ico642"][2][1]
    y1 = o["sys"][other]["coarse"][1]["y"][:, :3].astype(np.float64).ravel()
    bad = failing(stage_checks(c, d, o, s, names, y1=y1))
    assert bad == {(9, 0)}, bad
    print("another system's y prolonged: caught at", sorted(bad))
    # one ring sweep instead of two
    d = run("G2_cap641")
    o = d["full"]
    names = kernel_names(d, o, d["ran"])
    c = cycle_of("G2_cap641", s)
    assert c.sweeps == 2 and not failing(stage_checks(c, d, o, s, names))
    bad = failing(stage_checks(c, d, o, s, names, sweeps=1))
    assert bad == {(2, 0), (10, 0)}, bad
    print("one ring sweep instead of two: caught at", sorted(bad))


@pytest.mark.parametrize("case", ["G2_cap641", "S1s"])
def test_ring_matrix(case):
    """k_bsw_extract: bsw_A holds, byte for byte, the level-0 sweep-copy blocks
    bsw_bsrc names -- transposed where its transpose bit is set -- and zero in
    the padding slots."""
    d = run(case)
    T = d["T"]
    bsrc = T["bsw_bsrc"]
    assert T["bsw_n"] > 0 and (bsrc >= 0).any() and (bsrc < 0).any() and T["bsw_sweeps"] == 2
    assert ((bsrc[bsrc >= 0] & R.MIR_T) != 0).any() == d["H"]["levels"][0]["sym"]
    for s in CASES[case][2]:
        h = np.ascontiguousarray(d["ops"][s][0]["A0h"]).view("<u2").reshape(-1, 4)
        want = np.zeros((len(bsrc), 4), dtype=np.uint16)
        on = bsrc >= 0
        blk = h[bsrc[on] & R.MIR_POS]
        tr = (bsrc[on] & R.MIR_T) != 0
        blk = np.where(tr[:, None], blk[:, [0, 2, 1, 3]], blk)
        want[on] = blk
        assert d["ring"][s].tobytes() == want.tobytes(), (case, s)


@pytest.mark.parametrize("case", ["G1_ico642", "G2_cap641"])
def test_whole_operator(case):
    """The cycle as a matrix, from the read-back operators (int8 sweep copies,
    bf16 D^-1, w1 = 1.1 included): symmetric to 1e-12 of its norm and positive
    definite, which the PCG needs. Printed and recorded: the spectrum of
    M_ref A0h (the contraction the iteration counts come from) and the
    distance of the kernel's z from M_ref r (the price of the bf16 iterates; no
    bar)."""
    d = run(case)
    for s in CASES[case][2]:
        c = cycle_of(case, s)
        M = V.M_ref(c)
        assert M.shape == (2 * d["H"]["levels"][0]["n"],) * 2
        asym = V.asymmetry(M)
        parts = {"A%d" % l: V.asymmetry(a.toarray()) for l, a in enumerate(c.A[:-1])}
        parts.update({"D%d^-1" % l: V.asymmetry(a.toarray()) for l, a in enumerate(c.Dinv)})
        parts["cinv"] = V.asymmetry(c.cinvT)
        print("%s system %d: asymmetry of the stored operators" % (case, s), {k: "%.1e" % v for k, v in parts.items()})
        ev = np.linalg.eigvalsh(0.5 * (M + M.T))
        A = c.A[0].toarray()
        Lc = np.linalg.cholesky(0.5 * (M + M.T))
        sp_MA = np.linalg.eigvalsh(Lc.T @ A @ Lc)
        r = d["r"][s].astype(np.float64).ravel()
        z = d["full"]["z"][s].astype(np.float64).ravel()
        want = M @ r
        dist = np.linalg.norm(z - want) / max(np.linalg.norm(want), 1e-300)
        print("%s system %d (%s): asymmetry %.2e, eig(M) in [%.3e, %.3e], eig(M A) in [%.4f, %.4f] "
              "(rho(I - M A) %.4f), |z - M r| / |M r| %.2e"
              % (case, s, d["kinds"][s], asym, ev.min(), ev.max(), sp_MA.min(), sp_MA.max(),
                 np.abs(1.0 - sp_MA).max(), dist))
        assert asym <= 1e-12, (case, s, asym)
        assert ev.min() > 0, (case, s, ev.min())
        assert not V.is_symmetric(V.M_ref(c, post=False))
