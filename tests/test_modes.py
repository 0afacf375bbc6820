"""Spatiotemporal modes without a GPU: the numpy restatement of the three
passes (tests/modes_ref.py) pinned to the reference's golden vectors
(tests/golden/G11_modes.npz) within the bars the GPU tests use, the three
restated helpers of the scripts bit-identical to the reference's outputs, the
NaN-frame error, the argument errors and the export table."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden

import modes_ref as R
from mofhip import _lib as L
from mofhip import modes as M

INPUTS = ("G1_ico642", "G2_cap641", "G3_ico642_f32", "M1")


@pytest.fixture(scope="module")
def g11():
    return load_golden("G11_modes")


@pytest.fixture(scope="module")
def fields(g11):
    out = {"M1": (g11["M1_V"].astype(np.float64), None)}
    for name in INPUTS[:3]:
        g = load_golden(name)
        out[name] = (g["V_k"], g["e"])
    return out


@pytest.mark.parametrize("kind", ("complex", "concat"))
@pytest.mark.parametrize("name", INPUTS)
def test_restatement_against_reference(name, kind, fields, g11):
    V, _ = fields[name]
    K, N = V.shape[0], V.shape[1] // 2
    r = min(4, K)
    pre = "%s_%s_" % (name, kind)
    U0, Sg0, VT0 = g11[pre + "U"], g11[pre + "Sigma"], g11[pre + "VT"]
    eta, g2 = R.eta(K, N), R.gap2(Sg0)[:r]
    assert (g2 >= 1e-4).all()
    bars = eta * Sg0[0] ** 2 / Sg0
    assert R.percent_boundary_clear(Sg0, bars, r).all()
    bar_v = 4 * eta * Sg0[0] / g2
    for chunk in (R.CHUNK, 256):
        m = R.modes(V, r, kind, chunk)
        dS = np.abs(m["Sigma"] - Sg0)
        d_sr = np.abs(m["sigma_r"] - Sg0[:r])
        r1 = R.rank_one_errors(kind, m["U"], m["Y"], U0, Sg0, VT0)
        print("%s chunk %d: Sigma err / bar %.3g, sigma_r rel %.3g, rank-one / sigma_1 %.3g"
              % (pre, chunk, (dS / bars).max(), (d_sr / Sg0[:r]).max(), (r1 / Sg0[0]).max()))
        assert (dS <= bars).all() and (d_sr <= bar_v).all() and (r1 <= bar_v).all()
        if kind == "concat":
            bar_u = 4 * eta / g2
            assert (np.abs(U0.mean(axis=0)) >= 100 * bar_u).all()  # every stored mode compares directly
            assert (np.abs(m["U"] - U0).max(axis=0) <= bar_u).all()
            assert (np.abs(m["VT"] - VT0).max(axis=1) <= bar_u).all()
        pct, pct2 = M.calculate_percentages(m["Sigma"])
        assert np.array_equal(pct[:r], g11[pre + "pct"][:r]) and np.array_equal(pct2[:r], g11[pre + "pct2"][:r])


def test_m1_exercises_the_antisymmetric_half(fields):
    S, A = R.gram(fields["M1"][0], "complex")
    assert np.linalg.norm(A) >= 0.1 * np.linalg.norm(S)
    assert np.array_equal(S, S.T) and np.array_equal(A, -A.T)


def test_gram_restatement_within_bound(fields):
    for name in INPUTS:
        V = fields[name][0]
        N = V.shape[1] // 2
        S, A = R.gram(V, "complex", 256)
        bound = R.gram_bound(V)
        assert (np.abs(S - V @ V.T) <= bound).all()
        assert (np.abs(A - (V[:, N:] @ V[:, :N].T - V[:, :N] @ V[:, N:].T)) <= bound).all()


def test_helpers_bit_identical(fields, g11):
    V, e = fields["G2_cap641"]
    X = M.process_V_k_to_complex(V)
    assert X.dtype == g11["G2_cap641_X"].dtype and np.array_equal(X, g11["G2_cap641_X"])
    assert np.array_equal(np.signbit(X.real), np.signbit(g11["G2_cap641_X"].real))
    neg = M.process_V_k_to_complex(np.array([[-0.0, 1.0, np.inf, -0.0]]))
    assert np.signbit(neg.real[0, 0]) and neg[0, 1] == complex(1.0, -0.0) and np.signbit(neg.imag[0, 1])
    for kind in ("complex", "concat"):
        pre = "G2_cap641_%s_" % kind
        Sg, VT = g11[pre + "Sigma"], g11[pre + "VT"]
        pct, pct2 = M.calculate_percentages(Sg)
        assert np.array_equal(pct, g11[pre + "pct"]) and np.array_equal(pct2, g11[pre + "pct2"])
        N = V.shape[1] // 2
        for t in range(4):
            vt = VT[t] if kind == "complex" else VT[t, :N] + VT[t, N:] * 1j
            got = M.calculate_V_k_from_complex(Sg[t] * vt, e)
            assert np.array_equal(got, g11[pre + "vectors"][t])


def test_nan_frame_raises_before_eigh():
    S = np.eye(6)
    S[2, 2] = np.nan
    S[5, 5] = np.inf
    with pytest.raises(ValueError, match=r"frame\(s\) 2, 5"):
        M.gram_eig(S, np.zeros((6, 6)))


def test_gram_eig_orders_and_clamps():
    rng = np.random.default_rng(3)
    B = rng.standard_normal((6, 3)) + 1j * rng.standard_normal((6, 3))
    G = B @ B.conj().T  # rank 3: three eigenvalues are rounding noise of either sign
    Sigma, W = M.gram_eig(G.real, G.imag)
    assert (np.diff(Sigma) <= 0).all() and (Sigma >= 0).all() and not np.isnan(Sigma).any()
    assert np.allclose(Sigma[:3], np.linalg.svd(B, compute_uv=False))
    assert np.allclose(W.conj().T @ W, np.eye(6))


def test_zero_norm_mode_gets_a_zero_row():
    """V_k of rank below nmodes: sigma_r == 0 gives a zero VT row, not NaN."""
    Y = np.array([[3.0, 0.0, 4.0, 0.0], [0.0, 0.0, 0.0, 0.0]])
    U = np.array([[1.0, 0.0], [0.0, 1.0]])
    for kind in ("complex", "concat"):
        with np.errstate(all="raise"):
            res = M._finish(kind, 2, np.array([5.0, 0.0]), U, Y.copy(), np.array([5.0, 0.0]))
        assert np.array_equal(res["VT"][1], np.zeros_like(res["VT"][1]))
        assert np.array_equal(R.complex_Y(Y[:1] / 5.0)[0] if kind == "complex" else Y[0] / 5.0, res["VT"][0])


def test_python_argument_errors():
    V = np.zeros((3, 8))
    with pytest.raises(ValueError):
        M.velocity_modes(V, 2, kind="real")
    with pytest.raises(ValueError):
        M.velocity_modes(V, 4)  # nmodes > K
    with pytest.raises(ValueError):
        M.velocity_modes(V, 0)
    with pytest.raises(ValueError):
        M.velocity_modes(np.zeros((3, 7)))
    with pytest.raises(ValueError):
        M.modes_project(V, np.zeros((2, 1)))
    with pytest.raises(ValueError):
        M.velocity_modes_device(0, 3, 4)


def test_c_argument_errors():
    """MOF_E_ARG before any device work."""
    lib = L.lib()
    buf = np.zeros(64)
    p = ctypes.c_void_p(buf.ctypes.data)
    for K, N in ((0, 4), (4, 0), (-1, 4), (8193, 4)):
        assert lib.mof_modes_gram(0, p, K, N, L.MOF_MODES_COMPLEX, None, p, p) == L.MOF_E_ARG
        assert lib.mof_modes_project(0, p, K, N, p, p, 1, L.MOF_MODES_COMPLEX, None, p, p) == L.MOF_E_ARG
    assert lib.mof_modes_gram(0, p, 2, 2 ** 29 + 1, 0, None, p, None) == L.MOF_E_ARG  # 2N past int32
    assert lib.mof_modes_project(0, p, 2, 2 ** 29 + 1, p, p, 1, 0, None, p, p) == L.MOF_E_ARG
    assert lib.mof_modes_project(0, p, 2, 4, p, p, 3, 0, None, p, p) == L.MOF_E_ARG  # r > K
    assert b"1 .. K" in lib.mof_last_error()
    assert lib.mof_modes_project(0, p, 2, 4, p, p, 0, 0, None, p, p) == L.MOF_E_ARG
    assert lib.mof_modes_gram(0, None, 2, 4, 0, None, p, None) == L.MOF_E_ARG
    assert lib.mof_modes_gram(0, p, 2, 4, L.MOF_MODES_COMPLEX, None, p, None) == L.MOF_E_ARG  # A missing
    assert lib.mof_modes_project(0, p, 2, 4, p, None, 1, L.MOF_MODES_COMPLEX, None, p, None) == L.MOF_E_ARG
    with pytest.raises(L.MofError):
        L.check(lib.mof_modes_gram(0, p, 0, 4, 0, None, p, None))


def test_exports_and_flag():
    lib = L.lib()
    for name in ("mof_modes_gram", "mof_modes_project", "mof_test_modes_chunk", "mof_test_modes_pass"):
        assert name in L.EXPORTS and hasattr(lib, name)
    flags = [L.MOF_IO_DEVICE, L.MOF_NO_BLOCK_JACOBI, L.MOF_TIME_SPMV, L.MOF_PRECOND_AMG, L.MOF_NO_RECOVERY,
             L.MOF_COORDS_F32, L.MOF_DD_STAGED, L.MOF_SOLVE_FUSED, L.MOF_SOLVE_EAGER, L.MOF_WAVE_PHASE,
             L.MOF_WIND_ALL_LEVELS, L.MOF_MODES_COMPLEX]
    assert len(set(flags)) == len(flags) and L.MOF_MODES_COMPLEX == 2048
    assert L.MOF_ABI_VERSION == 4 and lib.mof_abi_version() == 4
    assert lib.mof_test_modes_chunk(0) == L.MOF_OK and lib.mof_test_modes_pass(0) == L.MOF_OK
    import mofhip
    for name in ("velocity_modes", "velocity_modes_device", "spatiotemporal_modes", "process_V_k_to_complex",
                 "calculate_V_k_from_complex", "calculate_percentages"):
        assert hasattr(mofhip, name)
