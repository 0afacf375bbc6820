"""The inner PCG (csrc/mof_pcg.hip: k_pcg_init, k_pcg_tol, k_pcg_spmv, k_red_pq,
k_red_rzrr, k_pcg_update, k_pcg_conv_early and the host loop pcg<V>() that
chains them) and the refinement step (k_outer_update, k_outer_check) against
the fp64 checker tests/pcg_ref.py, stage by stage.

Every case builds a handle and solves one batch of 5 systems with each
preconditioner it needs (so A32, the block-Jacobi D^-1, the multigrid and, on
icosphere(8), the fp64 operator are live). mof_test_pcg_inner then runs the
production pcg<V>() itself on right-hand sides of the test's own -- the
assembled f of the travelling wave; system 3's is a quarter of system 0's --
capped at K = 0, 1, 2, ... iterations up to the step after the slowest system
stops. With cap K the solve ends with the check launch of SpMV K, so it leaves
x_K, r_K, z_K, p_K, q_K and step K's scalars: runs are bit-reproducible
(asserted first), so the state after cap K is the input of the transition cap
K + 1 shows, and every stage is checked on the values it read
(pcg_ref.check_first, check_step; the bounds are derived in pcg_ref's
docstring, none is tuned). alpha and beta are reproduced exactly from the
device's own sums.

With the multigrid z_{K+1} must equal, byte for byte, mof_test_amg_vcycle
applied to the hook's r_{K+1} (tests/test_gpu_vcycle.py checks that cycle), a
system k_pcg_conv_early marked keeps the z of the step before, and the x0 that
k_pcg_init / k_pcg_update wrote is checked against w D0^-1 r (vcycle_ref's
pre-smoothing stage and bound) wherever the cycle left it alone: at every cap
on a mesh whose cycle corrects a float2 copy and runs no boundary sweeps
(random_sphere(1500): k_pcg_init's at cap 0, k_pcg_update's after), and on
every mesh for a system at the step k_pcg_conv_early stopped it (the cycle
skipped it). Elsewhere the cycle overwrites x0 in place.

The invariant that catches a lost or doubled deferred x update,
|(b - A x) - r| <= E_k per dof, with E_k accumulated from the per-step bounds
(pcg_ref.Drift), holds at every cap and at every system's last step; the final
state is then compared byte for byte across the ways pcg() can get there: all
systems / a compacted map ({1, 3} inactive: 3 of 5 <= 0.9 B; their buffers
keep a sentinel), the default chunks (a system stopping in the middle of a
chunk), the first chunk ending at the slowest system's step (the owed launch
issued alone; the launch counters show it), and the first chunk ending at the
fastest system's step with the tail compacted.

The eager fp64 solve is covered by the "f64" variant on icosphere(8)
(fused=False); tests/test_gpu_fused.py ties the fused kernel to it bit for bit,
so it is not repeated here.

Largest error / bound per stage seen on an MI355X (test_stage_chain prints
them, -s), fp32 / fp64 solve:
  r -= alpha q, x += alpha p, p = z + beta p   0.50 (fused: one rounding) / 1.00
  q = A z (FIRST) 0.25 / 0.33   q = A z + beta q 0.26 / 0.29   z = D^-1 r 0.64 / 0.66
  r.z, r.r, p.q <= 0.003 / 0.002   |(b - A x) - r| / E 0.19 / 0.24
  x0: inside its bf16 window (error / (bound + half a bf16 ulp) 1.00)
Steps to stop (rtol 1e-4 multigrid, 0.03 block Jacobi): icosphere(8) 5-6 and
3-5, icosphere(32) 9-12 and 13-18, the cap 5-6 and 5-8, random_sphere(1500)
8-10 and 7-12; the quarter copy (system 3) is the slowest everywhere. No fault
was found.
"""
import functools
import types

import numpy as np
import pytest

import amg_ref as R
import pcg_ref as P
import vcycle_ref as V
from conftest import load_golden
from mofhip import DeviceMesh, synth
from mofhip.mesh import (amg_levels, amg_vcycle, amg_vcycle_tables, assembly_readback, force_index32, outer_readback,
                         pcg_inner, pcg_launches)

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF   # a quiet NaN no kernel produces
B = 5
INACTIVE = (1, 3)
LAM = 0.01
K_SELF_RED_BLK = 32     # mof_pcg.hip kSelfRedBlk
# the hook's inner tolerance per preconditioner: the multigrid production's 1e-4; block Jacobi, which
# needs hundreds of steps for that, a tolerance it meets in about as many steps as the multigrid
# (0.1: 2 to 3 steps on icosphere(8), 8 to 13 on icosphere(32))
RTOL = {"amg": 1e-4, "jacobi": 0.03}
KMAX_CAP = 40           # a case whose slowest system takes more steps than this is too slow for the suite

# case -> (mesh, 32-bit tables forced, variants (preconditioner, precision), the SpMV instances each must run)
CASES = {
    "ico8": ("ico8", False, (("amg", "mixed"), ("jacobi", "mixed"), ("jacobi", "f64")),
             ("spmv_f32_zh_pk", "spmv_f32_pk", "spmv_f64")),
    "ico8_index32": ("ico8", True, (("amg", "mixed"), ("jacobi", "mixed")), ("spmv_f32_zh", "spmv_f32")),
    "ico32": ("ico32", False, (("amg", "mixed"), ("jacobi", "mixed")), ("spmv_f32_zh_pk", "spmv_f32_pk")),
    "cap": ("G2_cap641", False, (("amg", "mixed"), ("jacobi", "mixed")), ("spmv_f32_pk", "spmv_f32_pk")),
    "rand1500": ("rand1500", False, (("amg", "mixed"), ("jacobi", "mixed")), ("spmv_f32", "spmv_f32")),
}
VARIANTS = [(c, i) for c, v in CASES.items() for i in range(len(v[2]))]


def mesh_and_fields(name, T):
    if name.startswith("G"):
        g = load_golden(name)
        return (g["coordinates"], g["normals"], g["triangles"], g["areas"]), g["I"][:T], g["t_k"][:T], float(g["lambda_"])
    if name == "ico8":
        p, t = synth.icosphere(8)
    elif name == "ico32":
        p, t = synth.icosphere(32, jitter=0.005)
    else:
        p, t = synth.random_sphere(1500, 10.0, seed=3)
    return (p, synth.vertex_normals(p, t), t, synth.triangle_areas(p, t)), synth.travelling_wave(p, T), \
        np.arange(float(T)), LAM


def state(o, b):
    """System b's state (pcg_ref's format) from a hook run."""
    f = lambda a: a[b].astype(np.float64).ravel()  # noqa: E731
    return {"x": f(o["x"]), "r": f(o["r"]), "z": f(o["z"]), "p": f(o["p"]), "q": f(o["q"]),
            "scal": o["scal"][:, b, :].copy(), "conv": int(o["sys"]["CONV"][b]), "tol2": float(o["sys"]["TOL2"][b])}


def words(o, k, s):
    """System s's vector k of a hook run as stored (z: the pairs alone where it is bf16)."""
    return o["z_words"][s] if k == "z" else o["words"][k][s]


def same_bytes(a, b, s, keys="xrzpq"):
    return all(words(a, k, s).tobytes() == words(b, k, s).tobytes() for k in keys)


def spmv_delta(c0, c1):
    return {k: c1[k] - c0[k] for k in c0 if c1[k] != c0[k]}


@functools.lru_cache(maxsize=None)
def run(case):
    """The handle, its solves, every hook run of the case's variants; host data only."""
    name, index32, variants, _ = CASES[case]
    (p, n, t, a), I, tk, lam = mesh_and_fields(name, B + 1)
    if index32:
        with force_index32():
            m = DeviceMesh(p, n, t, a)
    else:
        m = DeviceMesh(p, n, t, a)
    out = {"variants": {}}
    # the multigrid solve first (its hierarchy gives the level-0 tables), then block Jacobi (the multigrid
    # assembly keeps no fp32 D^-1), each exactly one batch; neither touches the other's operators
    Vs, st = m.solve_range(I, tk, 0, B, lam, precision="mixed", precond="amg", batch=B)
    assert st["failed"] == st["recovered"] == 0, st
    H = amg_levels(m)
    T = amg_vcycle_tables(m, len(H["levels"]), 0)
    A0h = [assembly_readback(m, b)["A0h"] for b in range(B)]
    Vj, st = m.solve_range(I, tk, 0, B, lam, precision="mixed", precond="jacobi", batch=B)
    assert st["failed"] == st["recovered"] == 0, st
    assert np.abs(Vj - Vs).max() <= 1e-6 * np.abs(Vs).max()
    l0 = H["levels"][0]
    N = l0["n"]
    rb = [assembly_readback(m, b) for b in range(B)]
    rhs = np.stack([v["rhs"] for v in rb])
    rhs[3] = 0.25 * rhs[0]
    out.update(H=H, T=T, N=N, rhs=rhs, sizes=[v["n"] for v in H["levels"]], A0h=A0h)
    lev = None
    for precond, precision in variants:
        if precision == "f64":
            V64, st = m.solve_range(I, tk, 0, B, lam, precision="f64", batch=B, fused=False)
            assert st["failed"] == st["recovered"] == 0 and st["fused_launches"] == 0, st
            assert np.abs(V64 - Vs).max() <= 1e-6 * np.abs(Vs).max()
        kw = dict(precond=precond, precision=precision, sentinel=SENTINEL)
        rtol = RTOL[precond]
        c0 = pcg_launches()
        probe = pcg_inner(m, rhs, rtol, 400, a_system=0, **kw)
        c1 = pcg_launches()
        conv = [int(c) for c in probe["sys"]["CONV"]]
        assert min(conv) >= 1 and not probe["sys"]["FAILED"].any(), (case, precond, conv)
        kmax = max(conv) + 1
        assert kmax <= KMAX_CAP, (case, precond, conv)
        if lev is None:
            lev = P.level0(l0["sell_off"], l0["sell_col"], l0["mirror"], N, sym=probe["sym"])
            assert l0["sym"] == probe["sym"]
        v = {"probe": probe, "conv": conv, "kmax": kmax, "ran_probe": spmv_delta(c0, c1), "rtol": rtol,
             "dtype": np.float32 if precision == "mixed" else np.float64}
        if precision == "mixed":
            assert np.array_equal(probe["A"].reshape(-1, 4), rb[0]["A32"])  # the hook's copy is the assembly's
            v["blocks"] = [x["A32"] for x in rb]
        else:
            v["blocks"] = [pcg_inner(m, rhs, rtol, 0, a_system=b, **kw)["A"] for b in range(B)]
        v["caps"] = [pcg_inner(m, rhs, rtol, K, **kw) for K in range(kmax + 1)]
        c0 = pcg_launches()
        v["again"] = pcg_inner(m, rhs, rtol, 2, **kw)
        v["ran_cap2"] = spmv_delta(c0, pcg_launches())
        if precond == "amg":  # the production cycle on the r each cap left
            v["cycle"] = [amg_vcycle(m, o["r"], out["sizes"]) for o in v["caps"]]
        act = np.array([b not in INACTIVE for b in range(B)], dtype=np.uint8)
        c0 = pcg_launches()
        v["masked"] = [pcg_inner(m, rhs, rtol, K, active=act, **kw) for K in (0, 1, 2, 3, 400)]
        v["ran_masked"] = spmv_delta(c0, pcg_launches())
        # the chunk boundary: pcg()'s own hints, as the previous batch would have left them
        # (the probe's: the slowest system's step; with a bulk hint one past the fastest system's step the
        # first chunk ends there and, if the slowest is 2 steps further, the tail runs compacted)
        c0 = pcg_launches()
        v["hint_slowest"] = pcg_inner(m, rhs, rtol, 400, hint=(probe["hint"][0], 0), **kw)
        v["ran_hint_slowest"] = spmv_delta(c0, pcg_launches())
        c0 = pcg_launches()
        v["hint_split"] = pcg_inner(m, rhs, rtol, 400, hint=(probe["hint"][0], min(conv) + 1), **kw)
        v["ran_hint_split"] = spmv_delta(c0, pcg_launches())
        c0 = pcg_launches()
        v["cap0_again"] = pcg_inner(m, rhs, rtol, 0, **kw)
        v["ran_cap0"] = spmv_delta(c0, pcg_launches())
        # the tolerance of a later refinement step, from the handle's own scalars
        v["tol_outer"] = pcg_inner(m, rhs, rtol, 0, outer_rtol=1e-8, etol=1e-7, **kw)
        # failure flags: a zero rhs, a NaN in one system's rhs
        bad = rhs.copy()
        bad[2] = 0.0
        bad[4, N // 2, 1] = np.nan
        v["bad"] = pcg_inner(m, bad, rtol, 400, **kw)
        out["variants"][precond, precision] = v
    out["lev"] = lev
    m.close()
    return out


@functools.lru_cache(maxsize=None)
def op_of(case, vi, b, untransposed=False):
    d = run(case)
    v = d["variants"][CASES[case][2][vi]]
    lev = P.untranspose_one(d["lev"], v["blocks"][b]) if untransposed else d["lev"]
    return P.Op(lev, v["blocks"][b])


def smoother(d, b, omega=None):
    """What vcycle_ref's pre-smoothing stage takes: level 0's D^-1 from the bf16 diagonal blocks."""
    blk0 = R.h0_dec(d["A0h"][b])[d["H"]["levels"][0]["diag_pos"]]
    w = d["H"]["omega"] if omega is None else omega
    return types.SimpleNamespace(Dinv=[V.block_diag(np.linalg.inv(blk0))], omega=lambda l: w)


def x0dec(words):
    w = np.ascontiguousarray(words, dtype=np.uint32)
    return np.stack([(w << np.uint32(16)).view(np.float32), (w & np.uint32(0xFFFF0000)).view(np.float32)],
                    axis=-1).astype(np.float64).ravel()


def x0_kept(d):
    """The cycle leaves the x0 buffer alone: it corrects a float2 copy and runs no boundary sweeps."""
    return d["T"]["xm"] == 2 and d["T"]["bsw_n"] == 0


def check_x0(d, o, b, omega=None):
    c = smoother(d, b, omega)
    r = o["r"][b].astype(np.float64).ravel()
    ok, _, ratio = V.check_bf16(x0dec(o["x0_words"][b]), V.pre_smooth(c, 0, r), V.bound_pre_smooth(c, 0, r))
    return bool(ok.all()), ratio


RATIOS = {}


def note(key, ratio):
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)


def chain(case, vi, b, control=None, untransposed=False):
    """System b's stage checks from cap 0 to its last step, and the invariant
    at every cap: [(cap, stage, ok, ratio)]."""
    d = run(case)
    precond, precision = CASES[case][2][vi]
    v = d["variants"][precond, precision]
    dt = v["dtype"]
    op = op_of(case, vi, b, untransposed)
    rhs = d["rhs"][b].ravel()
    dinv = None if precond == "amg" else v["caps"][0]["dinv"][b]
    S = [state(o, b) for o in v["caps"]]
    conv = v["conv"][b]
    recs = []
    first, bq = P.check_first(op, rhs, S[0], dt, dinv)
    recs += [(0, k, ok, r) for k, ok, r in first]
    drift = P.Drift(op, rhs, P.unit(dt))
    drift.spmv(0.0, bq, np.zeros(op.n), np.zeros(op.n))
    for K in range(conv):
        step, info = P.check_step(op, S[K], S[K + 1], K, dt, dinv, control=control)
        recs += [(K + 1, k, ok, r) for k, ok, r in step]
        assert info["stopped"] == (K + 1 == conv), (case, b, K)
        drift.update(info["alpha"], info["br"])
        drift.spmv(info["beta"], info["bq"], info["bp"], info["bx"])
        x = S[K]["x"] if control == "drop_x" and K + 1 == conv else S[K + 1]["x"]
        ok, ratio = P.within(P.true_residual_gap(op, rhs, x, S[K + 1]["r"]), 0.0, drift.E)
        recs.append((K + 1, "|(b - A x) - r| <= E", ok, ratio))
    return recs


@pytest.mark.parametrize("case", list(CASES))
def test_runs_are_reproducible_and_instances_ran(case):
    """Two runs of the same cap leave the same bytes (what lets the state after
    cap K stand for the input of cap K + 1); cap 0 runs the FIRST instance alone,
    and each variant ran the SpMV instance the case claims -- and the k_red_*
    launches exactly above kSelfRedBlk row blocks."""
    d = run(case)
    for (precond, precision), want in zip(CASES[case][2], CASES[case][3]):
        v = d["variants"][precond, precision]
        a, b = v["caps"][2], v["again"]
        for s in range(B):
            assert same_bytes(a, b, s), (case, precond, s)
        assert a["scal"].tobytes() == b["scal"].tobytes()
        assert all(np.array_equal(a["sys"][k], b["sys"][k]) for k in a["sys"])
        ran = v["ran_cap2"]
        print(case, precond, precision, "nblk", a["nblk"], "selfred", a["selfred"], "zh", a["zh"], "sym", a["sym"],
              "packed", a["packed"], "conv", v["conv"], "cap 2 ran", ran, "probe ran", v["ran_probe"])
        first = want.replace("spmv_f32", "spmv_f32_first").replace("spmv_f64", "spmv_f64_first")
        # SpMV 0 (FIRST), SpMV 1, the check launch of SpMV 2; two updates
        assert {k: n for k, n in ran.items() if k.startswith("spmv")} == {want: 2, first: 1}, ran
        assert ran["update"] == 2, ran
        assert {k: n for k, n in v["ran_cap0"].items() if k.startswith("spmv")} == {first: 1}, v["ran_cap0"]
        assert "update" not in v["ran_cap0"]
        for s in range(B):
            assert same_bytes(v["caps"][0], v["cap0_again"], s), (case, precond, s)
        assert a["selfred"] == (a["nblk"] <= K_SELF_RED_BLK)
        assert ("red_pq" in ran) == ("red_rzrr" in ran) == (not a["selfred"]), ran
        assert ("conv_early" in ran) == (precond == "amg"), ran
        assert a["zh"] == (("_zh" in want)) and a["packed"] == ("_pk" in want)
    if case == "ico8":
        assert d["variants"]["amg", "mixed"]["caps"][0]["nblk"] == 3 and d["N"] == 642
    if case == "ico32":
        assert d["variants"]["amg", "mixed"]["caps"][0]["nblk"] == 41 and d["N"] == 10242
    if case == "ico8_index32":
        assert d["variants"]["amg", "mixed"]["caps"][0]["sym"]


def test_every_instance_is_claimed():
    """The cases' table names every k_pcg_spmv instance -- fp32 with and without
    bf16 z and packed index words, fp64 -- and the test above holds each case to
    its claim, the FIRST form and the other one (ten instances, none
    unreachable)."""
    claimed = {w for v in CASES.values() for w in v[3]}
    assert claimed == {"spmv_f32", "spmv_f32_pk", "spmv_f32_zh", "spmv_f32_zh_pk", "spmv_f64"}


@pytest.mark.parametrize("case,vi", VARIANTS)
def test_stage_chain(case, vi):
    """Every stage of every step of every system within its derived bound of
    the fp64 reference, on the input that stage read; the true-residual
    invariant at every cap up to each system's last step."""
    d = run(case)
    precond, precision = CASES[case][2][vi]
    v = d["variants"][precond, precision]
    print(case, precond, precision, "steps to stop", v["conv"])
    for b in range(B):
        for cap, stage, ok, ratio in chain(case, vi, b):
            note((precision, stage), ratio)
            assert ok, (case, precond, precision, b, cap, stage, ratio)
    print("largest error / bound so far:", {"%s %s" % k: round(r, 3) for k, r in sorted(RATIOS.items())})


@pytest.mark.parametrize("case", list(CASES))
def test_multigrid_z_and_x0(case):
    """z_{K+1} is the production cycle's output on r_{K+1}, byte for byte; a
    system k_pcg_conv_early stopped keeps its z; x0 is w D0^-1 r where the cycle
    left it alone."""
    d = run(case)
    v = d["variants"]["amg", "mixed"]
    kept = x0_kept(d)
    print(case, "xm", d["T"]["xm"], "ring rows", d["T"]["bsw_n"], "x0 kept by the cycle:", kept)
    seen_init = seen_update = seen_stop = 0
    for K, (o, cyc) in enumerate(zip(v["caps"], v["cycle"])):
        assert cyc["zh"] == o["zh"]
        for b in range(B):
            c = v["conv"][b]
            if K < c:  # running: the cycle ran on r_K
                assert o["z_words"][b].tobytes() == cyc["z_words"][b].tobytes(), (case, K, b)
            else:      # stopped at step c by k_pcg_conv_early: the z of step c - 1, never touched again
                assert o["z_words"][b].tobytes() == v["caps"][c - 1]["z_words"][b].tobytes(), (case, K, b)
                assert o["sys"]["CONV"][b] == c
            if kept and K <= c:
                ok, ratio = check_x0(d, o, b)
                note(("mixed", "x0 = w D^-1 r (k_pcg_init)" if K == 0 else "x0 = w D^-1 r (k_pcg_update)"), ratio)
                assert ok, (case, K, b, ratio)
                seen_init += K == 0
                seen_update += K > 0
            if K == c:  # written by update c - 1, then the cycle skipped the system
                ok, ratio = check_x0(d, o, b)
                note(("mixed", "x0 = w D^-1 r (k_pcg_update)"), ratio)
                assert ok, (case, K, b, ratio)
                seen_stop += 1
    assert seen_stop == B and (not kept or (seen_init == B and seen_update >= B))
    print("largest error / (bound + half a bf16 ulp) so far:",
          {k[1]: round(r, 3) for k, r in sorted(RATIOS.items()) if k[1].startswith("x0 = w")})
    if case == "rand1500":
        assert kept


@pytest.mark.parametrize("case,vi", VARIANTS)
def test_final_state_whichever_way(case, vi):
    """Every system's last x, r and flags are the same bytes at every cap past
    its last step, under the compacted map, and whichever launch applied the
    deferred x update: one inside a chunk, the owed launch issued alone after a
    chunk that ends at the slowest system's step, a compacted tail."""
    d = run(case)
    precond, precision = CASES[case][2][vi]
    v = d["variants"][precond, precision]
    conv, probe = v["conv"], v["probe"]
    for b in range(B):
        for K in range(conv[b], v["kmax"] + 1):  # a stopped system's x, r never change again
            assert same_bytes(v["caps"][K], probe, b, "xr"), (case, b, K)
            assert v["caps"][K]["sys"]["CONV"][b] == conv[b]
        for K in range(conv[b]):
            assert v["caps"][K]["sys"]["CONV"][b] == -1 and v["caps"][K]["sys"]["FAILED"][b] == 0
    # default chunks of 8: some system stops inside a chunk
    assert any(c % 8 != 0 for c in conv)
    for which in ("hint_slowest", "hint_split"):
        o = v[which]
        for b in range(B):
            assert same_bytes(o, probe, b, "xrpq"), (case, which, b)
        assert np.array_equal(o["sys"]["CONV"], probe["sys"]["CONV"])
        assert o["hint"][0] == probe["hint"][0]
    if case == "ico32":
        # here the split hint does compact the tail: the slowest system is 2 steps past the first chunk's
        # end, at which at most 0.9 B systems are still running or owed their x update
        first_chunk = min(conv) + 1
        assert probe["hint"][0] >= first_chunk + 2
        assert 0 < sum(c >= first_chunk for c in conv) <= 0.9 * B
        assert v["ran_hint_split"].get("compact", 0) >= 1, v["ran_hint_split"]
    # one chunk to the slowest system's step: never compacted; {1, 3} inactive: from the start of each solve
    assert "compact" not in v["ran_hint_slowest"], v["ran_hint_slowest"]
    assert v["ran_masked"]["compact"] >= 5, v["ran_masked"]
    cmax = max(conv)
    ran = v["ran_hint_slowest"]
    n_spmv = sum(n for k, n in ran.items() if k.startswith("spmv"))
    if precond == "amg":
        # the chunk ran cmax iterations, the last one marked the slowest system early, and the
        # launch that owes it x += alpha p went out alone
        assert probe["hint"][0] == cmax
        assert ran["update"] == cmax and ran["conv_early"] == cmax and n_spmv == cmax + 1, ran
    else:
        # no early mark: SpMV cmax sees the slowest system's |r|^2 inside the chunk of cmax + 1
        assert probe["hint"][0] == cmax + 1
        assert ran["update"] == cmax + 1 and n_spmv == cmax + 1, ran
    # {1, 3} inactive: the compacted map; their buffers keep the sentinel, the others their bits
    for o, K in zip(v["masked"], (0, 1, 2, 3, None)):
        ref = probe if K is None else v["caps"][K]
        for b in range(B):
            if b in INACTIVE:
                for k in "xrzpq":
                    assert (words(o, k, b).view(np.uint32) == SENTINEL).all(), (case, K, b, k)
                assert precond != "amg" or (o["x0_words"][b] == SENTINEL).all()
                assert o["sys"]["CONV"][b] == 0 and o["sys"]["ACTIVE"][b] == 0
            else:
                assert same_bytes(o, ref, b, "xrpq"), (case, K, b)
                assert o["z_words"][b].tobytes() == ref["z_words"][b].tobytes()
                assert o["scal"][:, b].tobytes() == ref["scal"][:, b].tobytes()
                assert o["sys"]["CONV"][b] == ref["sys"]["CONV"][b]


@pytest.mark.parametrize("case,vi", VARIANTS)
def test_stop_rule(case, vi):
    """SD_TOL2 = t^2 rr_0 with k_pcg_tol's t; SI_CONV is the first step whose own
    device |r|^2 is <= SD_TOL2; SD_BEST / SI_BEST_IT follow the running minimum;
    SD_RR0 is rr_0. With outer_rtol > 0 t follows from the handle's own scalars."""
    d = run(case)
    precond, precision = CASES[case][2][vi]
    v = d["variants"][precond, precision]
    for b in range(B):
        rr = [float(v["caps"][K]["scal"][K & 1, b, 1]) for K in range(v["conv"][b] + 1)]
        sys0 = v["caps"][0]["sys"]
        assert sys0["TOL2"][b] == P.tol2(v["rtol"], rr[0]) and sys0["RR0"][b] == rr[0]
        assert P.conv_step(rr, sys0["TOL2"][b]) == v["conv"][b]
        for K in range(v["conv"][b] + 1):
            s = v["caps"][K]["sys"]
            want = P.best(rr[:K + 1] if K < v["conv"][b] else rr[:v["conv"][b]])
            assert (s["BEST"][b], s["BEST_IT"][b]) == want, (case, b, K)
            assert s["TOL2"][b] == sys0["TOL2"][b]
        # a later refinement step's tolerance: t from SD_FF, SD_RR, SD_EST, SD_XMAX as the hook returns them
        s = v["tol_outer"]["sys"]
        t = P.inner_tol(v["rtol"], 1e-8, 1e-7, s["FF"][b], s["RR"][b], s["EST"][b], s["XMAX"][b])
        # the quotient and the root are correctly rounded on the device too; the products round alike
        assert abs(s["TOL2"][b] - P.tol2(t, rr[0])) <= 4 * P.U53 * s["TOL2"][b], (case, b, t)
        assert v["rtol"] <= t <= 0.5


@pytest.mark.parametrize("case,vi", [(c, i) for c, i in VARIANTS if c.startswith("ico8")])
def test_failure_flags(case, vi):
    """A zero right-hand side stops at step 0 with x = 0; a NaN in one system's
    right-hand side breaks that system down (FW_BREAKDOWN) and no other
    system's bytes change; a cap smaller than needed fails nothing."""
    d = run(case)
    precond, precision = CASES[case][2][vi]
    v = d["variants"][precond, precision]
    o, probe = v["bad"], v["probe"]
    s = o["sys"]
    assert s["CONV"][2] == 0 and s["FAILED"][2] == 0 and (o["x"][2] == 0).all() and (o["r"][2] == 0).all()
    assert s["FAILED"][4] == 1 and s["FAIL_WHY"][4] == 1 and s["ACTIVE"][4] == 0 and s["CONV"][4] < 0
    for b in (0, 1, 3):
        assert same_bytes(o, probe, b, "xrpq"), (case, b)
        assert s["CONV"][b] == probe["sys"]["CONV"][b] and s["FAILED"][b] == 0
    for K in range(min(v["conv"])):
        s = v["caps"][K]["sys"]
        assert (s["CONV"] < 0).all() and not s["FAILED"].any() and s["ACTIVE"].all()


def fails(case, vi, b, **kw):
    return {stage for _, stage, ok, _ in chain(case, vi, b, **kw) if not ok}


def test_negative_controls():
    """A reference wrong in one thing fails the check that thing belongs to
    (the device is never perturbed), and the right reference fails none."""
    case, b = "ico8", 0
    for vi in (0, 1):  # the multigrid (bf16 z, packed words), block Jacobi
        assert not fails(case, vi, b)
        bad = fails(case, vi, b, untransposed=True)
        assert bad and bad <= {"q = A z", "q = A z + beta q", "|(b - A x) - r| <= E"}, bad
        print("one lower block left untransposed: caught at", sorted(bad))
        bad = fails(case, vi, b, control="beta_slot")
        assert {"p = z + beta p", "q = A z + beta q"} <= bad, bad
        print("beta from the swapped slots: caught at", sorted(bad))
        bad = fails(case, vi, b, control="drop_x")
        assert bad == {"x += alpha p", "|(b - A x) - r| <= E"}, bad
        print("the deferred x update dropped: caught at", sorted(bad))
        bad = fails(case, vi, b, control="pq_row")
        assert bad == {"p.q"}, bad
        print("a row past the owned ones in p.q: caught at", sorted(bad))
    d = run(case)
    v = d["variants"]["amg", "mixed"]
    c = v["conv"][b]
    assert check_x0(d, v["caps"][c], b)[0] and not check_x0(d, v["caps"][c], b, omega=1.0)[0]
    print("w left out of x0: caught")


# ---- the refinement step ---------------------------------------------------------------------

RTOL_OUT, ETOL = 1e-8, 1e-7
INNER = 1e-4


@functools.lru_cache(maxsize=None)
def run_outer(name):
    (p, n, t, a), I, tk, lam = mesh_and_fields(name, B + 1)
    m = DeviceMesh(p, n, t, a)
    out = {"steps": []}
    for o in (1, 2, 3):
        c0 = pcg_launches()
        _, st = m.solve_range(I, tk, 0, B, lam, precision="mixed", precond="amg", batch=B, max_outer=o,
                              rtol=RTOL_OUT, inner_rtol=INNER, etol=ETOL, recovery=False)
        c1 = pcg_launches()
        rd = outer_readback(m, B)
        rd["ran"] = spmv_delta(c0, c1)
        rd["stats"] = st
        out["steps"].append(rd)
    out["rhs"] = np.stack([assembly_readback(m, b)["rhs"] for b in range(B)])
    m.close()
    return out


@pytest.mark.parametrize("name", ["ico32", "G2_cap641"])
def test_outer_step(name):
    """After refinement step o (max_outer = o): x64 is the fp64 sum of the inner
    x's exactly; SD_RR, SD_FF are the sums of r64^2 and f^2; SD_REL, SD_EST,
    SD_XMAX, SI_MET and the retirement follow from them as k_outer_check states;
    a retired system's x64 never changes again; the next inner solve's SD_TOL2
    follows from these scalars (k_pcg_tol)."""
    d = run_outer(name)
    rhs = d["rhs"]
    n = rhs[0].size
    prev, active = None, np.ones(B, dtype=bool)
    for o, rd in enumerate(d["steps"], start=1):
        s = rd["sys"]
        print(name, "max_outer", o, "ran", rd["ran"], "REL", s["REL"], "EST", s["EST"], "XMAX", s["XMAX"])
        assert rd["ran"]["outer_update"] == rd["ran"]["outer_check"] == rd["stats"]["outer_steps"] <= o
        for b in range(B):
            x64, xin = rd["x64"][b], rd["xin"][b].astype(np.float64)
            if not active[b]:
                assert np.array_equal(x64, prev["x64"][b]), (name, o, b)  # retired: no later step touches it
                assert s["RR"][b] == prev["sys"]["RR"][b]
                continue
            base = np.zeros_like(x64) if o == 1 else prev["x64"][b]
            assert np.array_equal(x64, base + xin), (name, o, b)
            r64 = rd["r64"][b].ravel()
            rr, ff = float(r64 @ r64), float(rhs[b].ravel() @ rhs[b].ravel())
            # fp64 sums of n rounded products in another order: (n + 1) 2^-53 of the sum
            assert abs(s["RR"][b] - rr) <= (n + 1) * P.U53 * rr and abs(s["FF"][b] - ff) <= (n + 1) * P.U53 * ff
            dmax, xmax = float(np.abs(xin).max()), float(np.abs(x64).max())
            assert s["XMAX"][b] == xmax
            rel, est, met, retired = P.outer_check(s["RR"][b], s["FF"][b], dmax, xmax,
                                                   0.0 if o == 1 else prev["sys"]["RR"][b], o == 1, RTOL_OUT, ETOL)
            assert abs(s["REL"][b] - rel) <= 4 * P.U53 * rel and abs(s["EST"][b] - est) <= 4 * P.U53 * est
            assert s["MET"][b] == met
            if o > 1:  # this step's inner tolerance, from the scalars the step before left
                q = prev["sys"]
                t = P.inner_tol(INNER, RTOL_OUT, ETOL, q["FF"][b], q["RR"][b], q["EST"][b], q["XMAX"][b])
                assert abs(s["TOL2"][b] - P.tol2(t, s["RR0"][b])) <= 4 * P.U53 * s["TOL2"][b], (name, o, b, t)
                r32 = prev["r64"][b].astype(np.float32).astype(np.float64).ravel()
                assert abs(s["RR0"][b] - float(r32 @ r32)) <= n * P.U53 * float(r32 @ r32)
            else:
                assert s["TOL2"][b] == P.tol2(INNER, s["RR0"][b])
            active[b] = not retired
        prev = rd
