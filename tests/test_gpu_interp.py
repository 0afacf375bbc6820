"""The electrode interpolation on the GPU (mof_rbf_eval, mofhip.interp) against
its numpy restatement and the reference's two S2 scripts (the golden vectors
of tests/golden/G12_rbf.npz). u = 2^-53, phi (N, E) = interp.rbf_phi -- scipy's
cdist and multiquadric bit for bit (tests/test_interp.py) --, S[t, i] =
sum_e |phi[i, e]| |W[t, e]|.

1. One-hot, bitwise: W[t, :] zero but W[t, e_t] = +-2^k, so the exact sum is
   one exactly representable product and every other term an exact zero:
   out[t, :] must equal W[t, e_t] phi[:, e_t] bit for bit. A wrong electrode or
   vertex map, the operand layout, a lost K-chunk, the padding to four
   electrodes and the tile and pass tails all show.
2. General (seeded normal) weights against a np.longdouble sum of the same
   phi: |out - sum| <= (E + 1) u S, gamma_E of E fused multiply-adds in any
   order; the pass hook changes no bit; two calls give the same bits.
3. The reference's nodes and epsilon: both planes within 2 (E + 1) u S of the
   reference's fields (both sides carry gamma_E); the angle within
   (bar_re + bar_im) / |z| + 8 u pi of the reference's, as a wrapped
   difference (the second term: ocml's documented atan2 accuracy with margin).
4. End to end, interpolation(...) from the raw inputs: |gpu - ref| <=
   |numpy chain - ref| + 2 (E + 1) u S, the chain being rbf_weights + @ in
   numpy -- the triangle inequality: the GPU and the chain evaluate the same
   weights, so they differ by two evaluations' rounding. For the phase input
   the same in the angle: the evaluation's bar over |z| plus atan2's 8 u pi.
5. Into the solver: rbf_eval_device's output pointer handed to the
   device-pointer solve gives the V of the same I passed from the host, bit
   for bit.
6. Bad arguments: MOF_E_ARG and nothing written.

Shapes: E below, at and over one chunk of four (1, 3, 4, 5), at the limits of
the kernel's three variants (62, 64 | 65, 128 | 129, 130, 256); T below, at
and over one 16-frame tile (1, 15, 16, 17), three ragged tiles (40), 300
(frame tiles spread over grid.y) and 4100 (two of the library's own passes);
N = 1, 15 (below one vertex tile), 641 (odd, ragged in every variant's block)
and 3249; passes of 7 frames; host and device pointers.
"""
import ctypes

import numpy as np
import pytest

from conftest import load_golden

from mofhip import _lib as L
from mofhip import interp
from mofhip.mesh import DeviceMesh

pytestmark = pytest.mark.gpu

U = 2.0 ** -53

# (E, T, N): the issue's sizes, each at least once, and the library's own thresholds
ONE_HOT = [(1, 1, 1), (1, 40, 15), (3, 15, 15), (3, 17, 1), (4, 16, 641), (5, 17, 641), (62, 1, 641),
           (62, 40, 3249), (64, 16, 15), (64, 17, 641), (65, 17, 641), (65, 40, 3249), (130, 40, 641),
           (130, 15, 3249), (128, 17, 641), (129, 16, 641), (256, 17, 641), (62, 300, 641), (5, 4100, 15)]
GENERAL = [(5, 15, 15), (62, 40, 3249), (65, 16, 641), (130, 17, 641), (256, 40, 641), (62, 300, 641)]


@pytest.fixture(scope="module")
def g12():
    return load_golden("G12_rbf")


@pytest.fixture
def pass_hook():
    def set_(frames=0):
        assert L.lib().mof_test_rbf_pass(frames) == L.MOF_OK
    yield set_
    set_(0)


_geometry = {}


def geometry(E, N):
    """(points (N, 3), electrodes (E, 3), epsilon, phi (N, E)); computed once
    per shape, never modified."""
    if (E, N) not in _geometry:
        rng = np.random.default_rng(1000 * E + N)
        xi = 30.0 * rng.standard_normal((E, 3))
        pts = 30.0 * rng.standard_normal((N, 3))
        if N > 2:
            pts[1] = xi[E // 2]  # a vertex on an electrode: r = 0, phi = 1
        eps = float(interp.rbf_epsilon(xi)) if E > 1 else 12.5
        phi = interp.rbf_phi(pts, xi, eps)
        for a in (xi, pts, phi):
            a.setflags(write=False)
        _geometry[(E, N)] = (pts, xi, eps, phi)
    return _geometry[(E, N)]


def device_eval(pts, xi, eps, W, angle=False):
    """rbf_eval through device pointers; the outputs start as NaN."""
    import torch
    T, N = W.shape[0], len(pts)
    cplx = np.iscomplexobj(W)
    up = lambda a: torch.from_numpy(np.array(a, dtype=np.float64)).cuda()  # noqa: E731 (a copy: the shared geometry is read-only)
    dp, dx, dwr = up(pts), up(xi), up(W.real)
    dwi = up(W.imag) if cplx else None
    do = torch.full((T, N), np.nan, dtype=torch.float64, device="cuda")
    doi = torch.full((T, N), np.nan, dtype=torch.float64, device="cuda") if cplx and not angle else None
    torch.cuda.synchronize()
    interp.rbf_eval_device(dp.data_ptr(), N, dx.data_ptr(), len(xi), eps, dwr.data_ptr(), T, do.data_ptr(),
                           W_im_ptr=dwi.data_ptr() if cplx else None,
                           out_im_ptr=doi.data_ptr() if doi is not None else None, angle=angle)
    out = do.cpu().numpy()
    return out + 1j * doi.cpu().numpy() if doi is not None else out


# ---- 1. one-hot, bitwise -------------------------------------------------
@pytest.mark.parametrize("E,T,N", ONE_HOT)
def test_one_hot_bitwise(E, T, N, pass_hook):
    pts, xi, eps, phi = geometry(E, N)
    stride = max(1, E // T)
    e_t = (E - 1 - stride * np.arange(T)) % E
    rng = np.random.default_rng(E + 7 * T + N)
    val = np.ldexp(rng.choice([-1.0, 1.0], T), rng.integers(-20, 21, T))
    W = np.zeros((T, E))
    W[np.arange(T), e_t] = val
    want = val[:, None] * phi[:, e_t].T
    assert np.isfinite(want).all() and (want != 0).all()
    for frames in (0, 7):
        pass_hook(frames)
        out = interp.rbf_eval(pts, xi, W, eps)
        bad = np.argwhere(out != want)
        print("E %d T %d N %d pass %d: %d entries differ" % (E, T, N, frames, len(bad)))
        assert not len(bad), (frames, bad[:4])
    pass_hook(0)
    assert np.array_equal(device_eval(pts, xi, eps, W), want)
    # the imaginary plane the same way: the one-hot weights at another electrode and sign
    Wi = np.zeros((T, E))
    Wi[np.arange(T), e_t[::-1]] = -val
    z = interp.rbf_eval(pts, xi, W + 1j * Wi, eps)
    assert np.array_equal(z.real, want) and np.array_equal(z.imag, -val[:, None] * phi[:, e_t[::-1]].T)


# ---- 2. general weights --------------------------------------------------
@pytest.mark.parametrize("E,T,N", GENERAL)
def test_general_weights(E, T, N, pass_hook):
    pts, xi, eps, phi = geometry(E, N)
    rng = np.random.default_rng(3 * E + T + N)
    W = rng.standard_normal((T, E)) + 1j * rng.standard_normal((T, E))
    pl = phi.astype(np.longdouble)
    S_re, S_im = np.abs(W.real) @ phi.T, np.abs(W.imag) @ phi.T
    ex_re = W.real.astype(np.longdouble) @ pl.T
    ex_im = W.imag.astype(np.longdouble) @ pl.T
    out = interp.rbf_eval(pts, xi, W.real.copy(), eps)
    z = interp.rbf_eval(pts, xi, W, eps)
    e0 = (np.abs(out - ex_re) / ((E + 1) * U * S_re)).astype(np.float64).max()
    e1 = (np.abs(z.imag - ex_im) / ((E + 1) * U * S_im)).astype(np.float64).max()
    print("E %d T %d N %d: |out - longdouble| %.3g, imaginary plane %.3g of (E + 1) u S" % (E, T, N, e0, e1))
    assert e0 <= 1 and e1 <= 1
    assert np.array_equal(z.real, out), "the real plane depends on the imaginary one"
    ang = interp.rbf_eval(pts, xi, W, eps, angle=True)
    pass_hook(7)
    assert np.array_equal(interp.rbf_eval(pts, xi, W, eps), z), "the pass size moved the result"
    assert np.array_equal(interp.rbf_eval(pts, xi, W, eps, angle=True), ang), "the pass size moved the angle"
    pass_hook(0)
    assert np.array_equal(interp.rbf_eval(pts, xi, W, eps), z), "two calls differ"
    assert np.array_equal(device_eval(pts, xi, eps, W), z), "device pointers moved the result"
    assert np.array_equal(device_eval(pts, xi, eps, W, angle=True), ang)
    # the angle is atan2 of the two planes the call returns otherwise
    d = np.abs(np.angle(np.exp(1j * (ang - np.angle(z)))))
    print("angle against np.angle of the planes: %.3g u pi" % (d.max() / (U * np.pi)))
    assert d.max() <= 8 * U * np.pi


# ---- 3. the reference's nodes --------------------------------------------
def planes_bar(nodes, phi, E):
    return (2 * (E + 1) * U * (np.abs(nodes.real) @ phi.T),
            2 * (E + 1) * U * (np.abs(nodes.imag) @ phi.T))


def wrapped(a, b):
    return np.abs(np.angle(np.exp(1j * (a - b))))


def test_reference_nodes(g12):
    pts, xi, eps = g12["points"], g12["electrodes"], float(g12["epsilon"])
    E = len(xi)
    phi = interp.rbf_phi(pts, xi, eps)
    out = interp.rbf_eval(pts, xi, g12["real_nodes"], eps)
    bar, _ = planes_bar(g12["real_nodes"], phi, E)
    e = np.abs(out - g12["real_field"]) / bar
    print("real: |gpu - reference| %.3g of 2 (E + 1) u S = %.3g u S" % (e.max(), e.max() * 2 * (E + 1)))
    assert e.max() <= 1
    nodes, ref = g12["phase_nodes"], g12["phase_field"]
    z = interp.rbf_eval(pts, xi, nodes, eps)
    bre, bim = planes_bar(nodes, phi, E)
    er, ei = np.abs(z.real - ref.real) / bre, np.abs(z.imag - ref.imag) / bim
    print("phase: planes %.3g, %.3g of 2 (E + 1) u S = %.3g, %.3g u S"
          % (er.max(), ei.max(), er.max() * 2 * (E + 1), ei.max() * 2 * (E + 1)))
    assert er.max() <= 1 and ei.max() <= 1
    ang = interp.rbf_eval(pts, xi, nodes, eps, angle=True)
    abar = (bre + bim) / np.abs(ref) + 8 * U * np.pi
    d = wrapped(ang, g12["phase_angle"])
    print("phase: |angle - reference| %.3g rad, %.3g of the bar (min |z| %.4g)" % (d.max(), (d / abar).max(),
                                                                                  np.abs(ref).min()))
    assert (d <= abar).all()


# ---- 4. end to end -------------------------------------------------------
def test_interpolation_end_to_end(g12):
    from scipy.signal import hilbert
    pts, xi = g12["points"], g12["electrodes"]
    E = len(xi)
    phi = interp.rbf_phi(pts, xi, interp.rbf_epsilon(xi))
    a, b = int(g12["real_start"]), int(g12["real_stop"])
    out = interp.interpolation(pts, g12["real_data"], xi, a, b)
    W = interp.rbf_weights(xi, g12["real_data"][a:b])
    chain = (phi @ W.T).T
    ref = g12["real_field"]
    bar = np.abs(chain - ref) + planes_bar(W, phi, E)[0]
    e = np.abs(out - ref)
    print("real: |gpu - ref| %.3g of max|ref| (numpy chain %.3g), %.3g of the bar"
          % (e.max() / np.abs(ref).max(), np.abs(chain - ref).max() / np.abs(ref).max(), (e / bar).max()))
    assert (e <= bar).all()
    # the phase script: exp(1j * angle(hilbert(potentials))), sliced, to the angle
    ph = np.exp(1j * np.angle(hilbert(g12["phase_pot"])))
    a, b = int(g12["phase_start"]), int(g12["phase_stop"])
    ang = interp.interpolation(pts, ph, xi, a, b)
    assert ang.dtype == np.float64 and ang.shape == (b - a, len(pts))
    W = interp.rbf_weights(xi, ph[a:b])
    chain = (phi @ W.T).T
    bre, bim = planes_bar(W, phi, E)
    ref = g12["phase_angle"]
    bar = wrapped(np.angle(chain), ref) + (bre + bim) / np.abs(chain) + 8 * U * np.pi
    d = wrapped(ang, ref)
    print("phase: |gpu angle - ref| %.3g rad (numpy chain %.3g), %.3g of the bar"
          % (d.max(), wrapped(np.angle(chain), ref).max(), (d / bar).max()))
    assert (d <= bar).all()


# ---- 5. into the solver --------------------------------------------------
def test_into_the_solver():
    import torch
    g = load_golden("G2_cap641")
    coords = np.ascontiguousarray(g["coordinates"], dtype=np.float64)
    N, E, T = len(coords), 5, 4
    rng = np.random.default_rng(5)
    xi = np.ascontiguousarray(coords[rng.choice(N, E, replace=False)])
    W = interp.rbf_weights(xi, rng.standard_normal((T, E)))
    eps = float(interp.rbf_epsilon(xi))
    tk, lam = g["t_k"][:T], float(g["lambda_"])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    dp, dx, dw = up(coords), up(xi), up(W)
    dI = torch.full((T, N), np.nan, dtype=torch.float64, device="cuda")
    dV = torch.full((T - 1, 2 * N), np.nan, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    interp.rbf_eval_device(dp.data_ptr(), N, dx.data_ptr(), E, eps, dw.data_ptr(), T, dI.data_ptr())
    mesh = DeviceMesh(coords, g["normals"], g["triangles"], g["areas"], device=0)
    try:
        st = mesh.solve_range_device(dI.data_ptr(), dI.data_ptr(), T, tk, 0, T - 1, lam, dV.data_ptr())
        I = dI.cpu().numpy()
        assert np.array_equal(I, interp.rbf_eval(coords, xi, W, eps))
        V, st_h = mesh.solve_range(I, tk, 0, T - 1, lam)
    finally:
        mesh.close()
    Vd = dV.cpu().numpy()
    print("solve of the interpolated I: %d systems, %d iterations, max|V| %.3g" % (st["systems"], st["iterations"],
                                                                                  np.abs(V).max()))
    assert st["failed"] == 0 and st_h["failed"] == 0 and np.isfinite(V).all() and np.abs(V).max() > 0
    assert np.array_equal(Vd, V)


# ---- 6. bad arguments ----------------------------------------------------
def test_bad_arguments():
    N, E, T = 7, 3, 2
    rng = np.random.default_rng(6)
    pts, xi, Wr, Wi = rng.standard_normal((N, 3)), rng.standard_normal((E, 3)), rng.standard_normal((T, E)), \
        rng.standard_normal((T, E))
    big = rng.standard_normal((257, 3))
    Wbig = rng.standard_normal((T, 257))
    out, out_im = np.full((T, N), 7.0), np.full((T, N), 7.0)
    p = L.ptr
    A = L.MOF_RBF_ANGLE
    good = dict(points=p(pts), N=N, el=p(xi), E=E, eps=1.5, wr=p(Wr), wi=p(Wi), T=T, flags=0, out=p(out),
                out_im=p(out_im))
    cases = {"N = 0": dict(N=0), "E = 0": dict(E=0), "T = 0": dict(T=0), "N < 0": dict(N=-1),
             "epsilon nan": dict(eps=float("nan")), "epsilon inf": dict(eps=float("inf")), "epsilon 0": dict(eps=0.0),
             "epsilon < 0": dict(eps=-1.5), "points NULL": dict(points=None), "electrodes NULL": dict(el=None),
             "W_re NULL": dict(wr=None), "out NULL": dict(out=None),
             "out_im NULL with W_im": dict(out_im=None), "angle without W_im": dict(wi=None, flags=A),
             "E over the cap": dict(el=p(big), E=257, wr=p(Wbig), wi=None)}
    for name, change in cases.items():
        a = dict(good, **change)
        rc = L.lib().mof_rbf_eval(0, a["points"], a["N"], a["el"], a["E"], a["eps"], a["wr"], a["wi"], a["T"],
                                  a["flags"], None, a["out"], a["out_im"])
        print("%s: %d (%s)" % (name, rc, L.lib().mof_last_error().decode()))
        assert rc == L.MOF_E_ARG, name
        assert (out == 7.0).all() and (out_im == 7.0).all(), name
    # the cap itself and the documented NULLs are accepted
    assert interp.MAX_ELECTRODES == 256
    rc = L.lib().mof_rbf_eval(0, p(pts), N, p(xi), E, 1.5, p(Wr), p(Wi), T, A, None, p(out), None)
    assert rc == L.MOF_OK and not (out == 7.0).any() and (out_im == 7.0).all()
