"""Spatiotemporal modes on the GPU (mof_modes_gram, mof_modes_project,
mofhip.modes) against numpy and the reference's two S4 scripts (the golden
vectors of tests/golden/G11_modes.npz; bars: tests/modes_ref.py).

1. Exact data, bitwise: with V of seeded integers in [-8, 8] every product and
   partial sum is an integer below 2^53, so S and A are exact in any summation
   order and must equal numpy's bit for bit -- the fp64 matrix-core row map, a
   row / column swap, the sign of A, a lost tail column, a lost chunk or block
   pair all show. The same for the projection with dyadic P, Q.
2. Gram on real data: within 2 (2N) u (|V| |V|^T) of numpy, exactly
   (anti)symmetric; the chunk hook moves it by no more than that, the pass hook
   alone not at all.
3. Modes against the reference: the Weyl / Davis-Kahan bars of an eta |G|
   perturbation of the Gram matrix, eta = 4 K N u (derived in modes_ref.py).
4. The bars of 3 are loose by construction (check 1 is the sharp one): every
   test prints what it measured. Measured on an MI355X, worst over the inputs:
   DESIGN.md §5.5.

Shapes: K below, at and over one 16-row tile (5, 15, 16, 17), three ragged
tiles (40), two and three 64-row blocks (70, 130: the off-diagonal block pairs
and the pair index); N not a multiple of 4, 16 or 64, odd (641: the 8-byte
loads) and even, and 4099 (three of the library's own 2048-column chunks, the
last of 3 columns); 256-column chunks (642 columns: three with a ragged tail);
passes of 7 rows (which split K >= 15), of 2 rows and, for the Gram matrix, of
one chunk each; host and device pointers.
"""
import ctypes

import numpy as np
import pytest

from conftest import load_golden

import modes_ref as R
from mofhip import _lib as L
from mofhip.modes import (calculate_V_k_from_complex, modes_gram, modes_project, spatiotemporal_modes, velocity_modes,
                          velocity_modes_device)

pytestmark = pytest.mark.gpu

SHAPES = [(K, N) for K in (5, 15, 16, 17, 40) for N in (641, 642, 1000)] + [(70, 642), (130, 641), (17, 4099)]
INPUTS = ("G1_ico642", "G2_cap641", "G3_ico642_f32", "M1")


@pytest.fixture(scope="module")
def g11():
    return load_golden("G11_modes")


@pytest.fixture(scope="module")
def fields(g11):
    """name -> (V_k (K, 2N) f64, e or None); read once, never modified."""
    out = {"M1": (g11["M1_V"].astype(np.float64), None)}
    for name in INPUTS[:3]:
        g = load_golden(name)
        out[name] = (np.ascontiguousarray(g["V_k"]), g["e"])
    return out


@pytest.fixture
def hooks():
    """chunk / pass hooks, reset afterwards."""
    def set_(chunk=0, rows=0):
        assert L.lib().mof_test_modes_chunk(chunk) == L.MOF_OK
        assert L.lib().mof_test_modes_pass(rows) == L.MOF_OK
    yield set_
    set_(0, 0)


def int_fields(K, N):
    rng = np.random.default_rng(1000 * K + N)
    return rng.integers(-8, 9, size=(K, 2 * N)).astype(np.float64)


def exact_gram(V):
    Vi = V.astype(np.int64)
    N = Vi.shape[1] // 2
    V1, V2 = Vi[:, :N], Vi[:, N:]
    return (Vi @ Vi.T).astype(np.float64), (V2 @ V1.T - V1 @ V2.T).astype(np.float64)


def device_gram(V, kind):
    import torch
    K, N = V.shape[0], V.shape[1] // 2
    dV = torch.from_numpy(V).cuda()
    dS = torch.full((K, K), np.nan, dtype=torch.float64, device="cuda")
    dA = torch.full((K, K), np.nan, dtype=torch.float64, device="cuda")
    fl = (L.MOF_MODES_COMPLEX if kind == "complex" else 0) | L.MOF_IO_DEVICE
    torch.cuda.synchronize()
    L.check(L.lib().mof_modes_gram(0, ctypes.c_void_p(dV.data_ptr()), K, N, fl, None, ctypes.c_void_p(dS.data_ptr()),
                                   ctypes.c_void_p(dA.data_ptr()) if kind == "complex" else None))
    return dS.cpu().numpy(), dA.cpu().numpy()


# ---- 1. exact data -------------------------------------------------------
@pytest.mark.parametrize("K,N", SHAPES)
def test_gram_exact_integers(K, N, hooks):
    V = int_fields(K, N)
    S0, A0 = exact_gram(V)
    assert not np.array_equal(A0, np.zeros_like(A0)) and not np.array_equal(S0, S0[::-1, ::-1])
    # (chunk, pass): 256-column chunks in one pass, in passes of 7 rows' worth
    # of values and in passes of one chunk each (pass 1: every shape here);
    # N = 4099 spans three of the library's own 2048-column chunks
    for chunk, rows in ((0, 0), (256, 0), (256, 7), (256, 1), (0, 1)):
        hooks(chunk, rows)
        S, A = modes_gram(V, "complex")
        assert np.array_equal(S, S0), (chunk, rows, np.argwhere(S != S0)[:4])
        assert np.array_equal(A, A0), (chunk, rows, np.argwhere(A != A0)[:4])
        Sc, Ac = modes_gram(V, "concat")
        assert Ac is None and np.array_equal(Sc, S0)
    hooks(256, 0)
    S, A = device_gram(V, "complex")
    assert np.array_equal(S, S0) and np.array_equal(A, A0)
    S, _ = device_gram(V, "concat")
    assert np.array_equal(S, S0)


@pytest.mark.parametrize("K,N", SHAPES)
def test_project_exact_dyadic(K, N, hooks):
    import torch
    V = int_fields(K, N)
    rng = np.random.default_rng(7 * K + N)
    r = min(K, 6)  # two launches of four modes, the second ragged
    P8, Q8 = rng.integers(-16, 17, size=(2, K, r))
    W = (P8 + 1j * Q8) / 8.0
    V1, V2 = V[:, :N].astype(np.int64), V[:, N:].astype(np.int64)
    Y8 = np.concatenate([P8.T @ V1 + Q8.T @ V2, P8.T @ V2 - Q8.T @ V1], axis=1)
    Yc8 = P8.T @ V.astype(np.int64)
    for kind, ref8, Wk in (("complex", Y8, W), ("concat", Yc8, W.real)):
        sig0 = np.sqrt((ref8 * ref8).sum(axis=1).astype(np.float64) / 64.0)
        assert ((ref8 * ref8).sum(axis=1) < 2 ** 53).all()
        for rows in (0, 7, 2):  # 2: several passes at every K here
            hooks(0, rows)
            Y, sig = modes_project(V, Wk, kind)
            assert np.array_equal(Y, ref8 / 8.0), (kind, rows)
            assert np.array_equal(sig, sig0), (kind, rows, sig - sig0)
        # device pointers
        fl = (L.MOF_MODES_COMPLEX if kind == "complex" else 0) | L.MOF_IO_DEVICE
        dV = torch.from_numpy(V).cuda()
        dP = torch.from_numpy(np.ascontiguousarray(W.real)).cuda()
        dQ = torch.from_numpy(np.ascontiguousarray(W.imag)).cuda()
        dY = torch.full((r, 2 * N), np.nan, dtype=torch.float64, device="cuda")
        ds = torch.full((r,), np.nan, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        L.check(L.lib().mof_modes_project(0, p(dV), K, N, p(dP), p(dQ) if kind == "complex" else None, r, fl, None,
                                          p(dY), p(ds)))
        assert np.array_equal(dY.cpu().numpy(), ref8 / 8.0) and np.array_equal(ds.cpu().numpy(), sig0)


# ---- 2. Gram on real data ------------------------------------------------
@pytest.mark.parametrize("name", INPUTS)
def test_gram_real_data(name, fields, hooks):
    V, _ = fields[name]
    N = V.shape[1] // 2
    V1, V2 = V[:, :N], V[:, N:]
    S0, A0 = V @ V.T, V2 @ V1.T - V1 @ V2.T
    bound = R.gram_bound(V)
    S, A = modes_gram(V, "complex")
    assert np.array_equal(S, S.T) and np.array_equal(A, -A.T) and not A.diagonal().any()
    eS, eA = np.abs(S - S0) / bound, np.abs(A - A0) / bound
    print("%s: |S - numpy| / bound %.3g, |A - numpy| / bound %.3g" % (name, eS.max(), eA.max()))
    assert eS.max() <= 1 and eA.max() <= 1
    hooks(0, 7)
    Sp, Ap = modes_gram(V, "complex")
    assert np.array_equal(Sp, S) and np.array_equal(Ap, A), "the pass size moved the Gram matrix"
    Sd, Ad = device_gram(V, "complex")
    assert np.array_equal(Sd, S) and np.array_equal(Ad, A), "device pointers moved the Gram matrix"
    for chunk, rows in ((256, 0), (256, 7)):
        hooks(chunk, rows)
        Sc, Ac = modes_gram(V, "complex")
        mS, mA = np.abs(Sc - S) / bound, np.abs(Ac - A) / bound
        print("%s: chunk %d pass %d moves S by %.3g, A by %.3g of the bound" % (name, chunk, rows, mS.max(), mA.max()))
        assert mS.max() <= 1 and mA.max() <= 1
        assert np.array_equal(Sc, Sc.T) and np.array_equal(Ac, -Ac.T)
    hooks(256, 0)
    S1, A1 = modes_gram(V, "complex")
    hooks(256, 1)  # one chunk per pass: three or four passes on every input
    S2, A2 = modes_gram(V, "complex")
    assert np.array_equal(S1, S2) and np.array_equal(A1, A2)
    Sk, _ = modes_gram(V, "concat")
    assert np.array_equal(Sk, S2)


# ---- 3. modes against the reference --------------------------------------
@pytest.mark.parametrize("kind", ("complex", "concat"))
@pytest.mark.parametrize("name", INPUTS)
def test_modes_against_reference(name, kind, fields, g11):
    import torch
    V, e = fields[name]
    K, N = V.shape[0], V.shape[1] // 2
    r = min(4, K)
    pre = "%s_%s_" % (name, kind)
    U0, Sg0, VT0 = g11[pre + "U"], g11[pre + "Sigma"], g11[pre + "VT"]
    res = spatiotemporal_modes(V, e, r, kind) if e is not None else velocity_modes(V, r, kind)
    assert res["U"].shape == (K, r) and res["Sigma"].shape == (K,) and res["Y"].shape == (r, 2 * N)
    assert res["VT"].shape == ((r, N) if kind == "complex" else (r, 2 * N))
    eta, g2 = R.eta(K, N), R.gap2(Sg0)[:r]
    # Sigma, every j (Weyl)
    bars = eta * Sg0[0] ** 2 / Sg0
    dS = np.abs(res["Sigma"] - Sg0)
    # sigma_r and the rank-one terms (Davis-Kahan)
    bar_v = 4 * eta * Sg0[0] / g2
    d_sr = np.abs(res["sigma_r"] - Sg0[:r])
    r1 = R.rank_one_errors(kind, res["U"], res["Y"], U0, Sg0, VT0)
    print("%s: Sigma err / bar %.3g (abs %.3g); sigma_r rel err %.3g (bar %.3g); rank-one err / sigma_1 %.3g (bar %.3g)"
          % (pre, (dS / bars).max(), dS.max(), (d_sr / Sg0[:r]).max(), (bar_v / Sg0[:r]).max(), (r1 / Sg0[0]).max(),
             (bar_v / Sg0[0]).max()))
    assert (dS <= bars).all()
    assert (d_sr <= bar_v).all()
    assert (r1 <= bar_v).all()
    if kind == "concat":
        bar_u = 4 * eta / g2
        direct = np.abs(U0.mean(axis=0)) >= 100 * bar_u
        assert (~direct).sum() <= 1
        assert direct.all(), "the stored inputs keep all four modes direct"
        for j in range(r):
            dU, dV = np.abs(res["U"][:, j] - U0[:, j]).max(), np.abs(res["VT"][j] - VT0[j]).max()
            if not direct[j]:
                dU = min(dU, np.abs(res["U"][:, j] + U0[:, j]).max())
                dV = min(dV, np.abs(res["VT"][j] + VT0[j]).max())
            print("%s mode %d: |U - ref| %.3g, |VT - ref| %.3g (bar %.3g)" % (pre, j, dU, dV, bar_u[j]))
            assert dU <= bar_u[j] and dV <= bar_u[j]
    # the sign rule holds on what is returned, and U, VT, Y moved together
    assert (np.mean(np.real(res["U"]), axis=0) >= 0).all()
    VTp = res["Y"] / res["sigma_r"][:, None]
    assert np.array_equal(res["VT"], R.complex_Y(VTp) if kind == "complex" else VTp)
    # the percentages (no stored input has one at a rounding boundary: asserted by the maker)
    assert np.array_equal(res["percentages"][:r], g11[pre + "pct"][:r])
    assert np.array_equal(res["percentages_squared"][:r], g11[pre + "pct2"][:r])
    # the mode vectors: mof_velocity_vectors of Y, bit-identical to numpy
    if e is not None:
        want = np.array([calculate_V_k_from_complex(R.complex_Y(res["Y"][j:j + 1])[0], e) for j in range(r)])
        assert np.array_equal(res["mode_vectors"], want)
    # fields still in HBM: the same numbers
    dV = torch.from_numpy(V).cuda()
    de = torch.from_numpy(np.ascontiguousarray(e)).cuda() if e is not None else None
    tm = {}
    dev = velocity_modes_device(dV.data_ptr(), K, N, r, kind, e_ptr=de.data_ptr() if e is not None else None,
                                timings=tm)
    for key in res:
        assert np.array_equal(dev[key], res[key]), key
    assert set(tm) == {"ms_gram", "ms_eigh", "ms_project"}


def test_nan_frame_is_named(fields):
    V = fields["G2_cap641"][0].copy()
    V[3, 17] = np.nan
    V[1, 700] = np.inf
    with pytest.raises(ValueError, match=r"frame\(s\) 1, 3"):
        velocity_modes(V, 2, "complex")
