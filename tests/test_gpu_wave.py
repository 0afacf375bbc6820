"""Wave speed on the GPU (mof_wave_speed) against the reference's
S5_compute_wave_v.py: the golden vectors of tests/golden/G8_wave.npz and the
numpy checker tests/wave_ref.py (pinned to them bit for bit by test_wave.py).

Bars. dXdt restates numpy's operations one by one: bit-identical. The spatial
half runs as one sparse operator, a reordering of the reference's sums:
|grad_ab - ref| and |grad_norm - ref| <= 1e-13 max|grad_M| (about 30 eps x (3 x
valence + the projection's operations) ~ 3e-15 at worst, margin ~30; the same
reordering in numpy measured 1.6e-16). speed is the IEEE quotient of the
returned dXdt and grad_norm, and within 1e-12 relative of the reference's at
every vertex (the inputs keep every vertex gradient above 1e-3 max|grad_M|).
"""
import numpy as np
import pytest

from conftest import load_golden

import wave_ref
from mofhip import DeviceMesh, MofError
from mofhip import _lib as L
from mofhip.wave import wave_speed, wave_speed_device, wave_velocity_amplitude, wave_velocity_phase

pytestmark = pytest.mark.gpu

MESHES = ["G1_ico642", "G2_cap641", "G3_ico642_f32"]
ALL = ("speed", "grad_norm", "dXdt", "grad_ab")
BAR = 1e-13


@pytest.fixture(scope="module")
def g8():
    g = load_golden("G8_wave")
    return {k: v.astype(np.float64) if k.endswith("_phases") else v for k, v in g.items()}


@pytest.fixture(scope="module")
def meshes():
    made = {}

    def get(name, reorder=True):
        if (name, reorder) not in made:
            g = load_golden(name)
            made[name, reorder] = (g, DeviceMesh(g["coordinates"], g["normals"], g["triangles"], g["areas"],
                                                 reorder=reorder))
        return made[name, reorder]

    yield get
    for _, m in made.values():
        m.close()


@pytest.fixture(scope="module")
def refs(g8):
    """wave_ref on (mesh, mode), computed once and never modified."""
    made = {}

    def get(name, mode):
        if (name, mode) not in made:
            g = load_golden(name)
            X = g8[name + "_phases"]
            X = X if mode == "phase" else np.cos(X)
            r = wave_ref.wave_speed(g["coordinates"], g["triangles"], g["areas"], g["e"], X, float(g8["dt"]),
                                    phase=mode == "phase")
            r["X"] = X
            for v in r.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            made[name, mode] = r
        return made[name, mode]

    return get


def numpy_dxdt(X, dt, mode):
    if mode == "phase":
        return wave_ref.temporal_gradient_phase(X, dt)
    return np.gradient(X, axis=0, edge_order=2) / dt


def check_against(out, r, X, dt, mode, golden_speed=None):
    speed, gn, d, ab = out
    assert np.array_equal(d, numpy_dxdt(X, dt, mode))
    bar = BAR * r["max_grad_M"]
    e_ab, e_gn = np.abs(ab - r["grad_ab"]).max(), np.abs(gn - r["grad_norm"]).max()
    print("max|grad_M| %.3g  |grad_ab - ref| %.3g  |grad_norm - ref| %.3g  bar %.3g"
          % (r["max_grad_M"], e_ab, e_gn, bar))
    assert e_ab <= bar and e_gn <= bar
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(speed, d / gn, equal_nan=True)
    if golden_speed is not None:
        diff, mag = np.abs(speed - golden_speed), np.abs(golden_speed)
        print("speed: max relative difference %.3g, min g / max|grad_M| %.3g"
              % ((diff[mag > 0] / mag[mag > 0]).max(), r["grad_norm"].min() / r["max_grad_M"]))
        assert np.isfinite(speed).all() and (diff <= 1e-12 * mag).all()  # a zero speed is a zero dXdt: exact


@pytest.mark.parametrize("name", MESHES)
@pytest.mark.parametrize("mode", ["phase", "amp"])
def test_parity_with_reference(g8, meshes, refs, name, mode):
    _, m = meshes(name)
    r = refs(name, mode)
    dt = float(g8["dt"])
    out = wave_speed(m, r["X"], dt, phase=mode == "phase", outputs=ALL)
    if mode == "phase":  # the golden (alpha, beta) themselves
        assert np.abs(out[3] - g8[name + "_ab_phase"]).max() <= BAR * r["max_grad_M"]
    check_against(out, r, r["X"], dt, mode, g8["%s_speed_%s" % (name, mode)])
    # the functions with the reference's names
    f = wave_velocity_phase if mode == "phase" else wave_velocity_amplitude
    assert np.array_equal(f(m, r["X"], dt, len(r["X"]), None), out[0], equal_nan=True)


@pytest.mark.parametrize("mode", ["phase", "amp"])
def test_pass_boundaries(g8, meshes, refs, mode):
    """T = 5 split into passes of 1, 2, 3 and 5 frames and the library's own
    choice: the first and last frames of a pass that are not those of the
    sequence take the centred difference from the neighbouring pass's rows."""
    _, m = meshes("G2_cap641")
    X, dt = refs("G2_cap641", mode)["X"], float(g8["dt"])
    base = wave_speed(m, X, dt, phase=mode == "phase", outputs=ALL, frames_per_pass=0)
    assert np.array_equal(base[2], numpy_dxdt(X, dt, mode))
    for fpp in (1, 2, 3, 5):
        out = wave_speed(m, X, dt, phase=mode == "phase", outputs=ALL, frames_per_pass=fpp)
        for a, b, k in zip(out, base, ALL):
            assert np.array_equal(a, b, equal_nan=True), (fpp, k)


def test_minimum_lengths(g8, meshes, refs):
    g, m = meshes("G1_ico642")
    dt = float(g8["dt"])
    for mode, T in (("phase", 2), ("amp", 3)):
        X = refs("G1_ico642", mode)["X"][:T]
        r = wave_ref.wave_speed(g["coordinates"], g["triangles"], g["areas"], g["e"], X, dt, phase=mode == "phase")
        for fpp in (0, 1):
            out = wave_speed(m, X, dt, phase=mode == "phase", outputs=ALL, frames_per_pass=fpp)
            check_against(out, r, X, dt, mode)
        with pytest.raises(MofError) as ei:
            wave_speed(m, X[:T - 1], dt, phase=mode == "phase")
        assert ei.value.code == L.MOF_E_ARG


def test_argument_errors(g8, meshes, refs):
    _, m = meshes("G1_ico642")
    X = refs("G1_ico642", "phase")["X"]
    out = np.empty_like(X)
    fn, h = L.lib().mof_wave_speed, m.handle()
    P = L.MOF_WAVE_PHASE
    assert fn(h, L.ptr(X), 5, 0.1, P, 0, None, None, None, None, None) == L.MOF_E_ARG  # no output
    assert b"output" in L.lib().mof_last_error()
    assert fn(None, L.ptr(X), 5, 0.1, P, 0, None, L.ptr(out), None, None, None) == L.MOF_E_ARG
    assert fn(h, None, 5, 0.1, P, 0, None, L.ptr(out), None, None, None) == L.MOF_E_ARG
    assert fn(h, L.ptr(X), 5, 0.0, P, 0, None, L.ptr(out), None, None, None) == L.MOF_E_ARG
    assert fn(h, L.ptr(X), 5, 0.1, P, -1, None, L.ptr(out), None, None, None) == L.MOF_E_ARG
    assert fn(h, L.ptr(X), 5, 0.1, P, 0, None, L.ptr(out), None, None, None) == L.MOF_OK


def test_vertex_order(g8, meshes, refs):
    """A handle that keeps the caller's vertex order (no RCM): the same dXdt
    bits, the gradient within the bar."""
    _, m = meshes("G1_ico642", reorder=False)
    dt = float(g8["dt"])
    for mode in ("phase", "amp"):
        r = refs("G1_ico642", mode)
        out = wave_speed(m, r["X"], dt, phase=mode == "phase", outputs=ALL)
        check_against(out, r, r["X"], dt, mode, g8["G1_ico642_speed_" + mode])


@pytest.mark.parametrize("mode", ["phase", "amp"])
def test_zero_gradient(g8, meshes, refs, mode):
    _, m = meshes("G1_ico642")
    dt = float(g8["dt"])
    X = refs("G1_ico642", mode)["X"][:3].copy()
    X[1] = 0.0
    speed, gn, d, ab = wave_speed(m, X, dt, phase=mode == "phase", outputs=ALL)
    assert np.array_equal(d, numpy_dxdt(X, dt, mode))
    assert not gn[1].any() and not ab[1].any()
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(speed[1], d[1] / np.zeros_like(d[1]), equal_nan=True)
    assert np.isinf(speed[1]).any()


def test_output_selection(g8, meshes, refs):
    _, m = meshes("G3_ico642_f32")
    X, dt = refs("G3_ico642_f32", "phase")["X"], float(g8["dt"])
    full = wave_speed(m, X, dt, outputs=ALL, frames_per_pass=2)
    for k, name in enumerate(ALL):
        assert np.array_equal(wave_speed(m, X, dt, outputs=(name,), frames_per_pass=2), full[k], equal_nan=True), name
    assert np.array_equal(wave_speed(m, X, dt), full[0], equal_nan=True)  # default: the speed


@pytest.mark.parametrize("mode", ["phase", "amp"])
def test_device_pointers(g8, meshes, refs, mode):
    import torch
    _, m = meshes("G2_cap641")
    X, dt = refs("G2_cap641", mode)["X"], float(g8["dt"])
    host = wave_speed(m, X, dt, phase=mode == "phase", outputs=ALL, frames_per_pass=2)
    dev = torch.device("cuda", 0)
    Xd = torch.from_numpy(X.copy()).to(dev)  # the shared reference input is read-only
    T, N = X.shape
    outs = [torch.full((T, N, 2) if k == "grad_ab" else (T, N), -7.0, dtype=torch.float64, device=dev) for k in ALL]
    torch.cuda.synchronize()
    wave_speed_device(m, Xd.data_ptr(), T, dt, phase=mode == "phase", frames_per_pass=2,
                      speed_ptr=outs[0].data_ptr(), grad_norm_ptr=outs[1].data_ptr(),
                      dXdt_ptr=outs[2].data_ptr(), grad_ab_ptr=outs[3].data_ptr())
    for o, h, k in zip(outs, host, ALL):
        assert np.array_equal(o.cpu().numpy(), h, equal_nan=True), k


def test_solver_unaffected(g8, meshes, refs):
    g, m = meshes("G1_ico642")
    I, tk, lam = g["I"][:4], g["t_k"][:4], float(g["lambda_"])
    V0, _ = m.solve_range(I, tk, 0, 3, lam, precision="mixed", precond="amg")
    wave_speed(m, refs("G1_ico642", "phase")["X"], float(g8["dt"]), outputs=ALL)
    V1, _ = m.solve_range(I, tk, 0, 3, lam, precision="mixed", precond="amg")
    assert np.array_equal(V0, V1)


@pytest.mark.slow
def test_160k_sample():
    """C3 (163,842 vertices, many row blocks and a ragged last slice), T = 4 in
    passes of 3: grad_norm on every 97th vertex against wave_ref run on the
    triangles around the sample, dXdt everywhere."""
    from mofhip import synth
    p, t, n, a = synth.mesh_for_config("C3")
    m = DeviceMesh(p, n, t, a)
    e, _, _ = m.geometry()
    T, dt = 4, 1.0 / 512
    theta = p @ np.array([0.31, -0.23, 0.17]) + 0.9
    X = np.mod(theta[None, :] - 0.7 * np.arange(T)[:, None] + np.pi, 2 * np.pi) - np.pi
    sample = list(range(0, len(p), 97))
    r = wave_ref.wave_speed(p, t, a, e, X, dt, vertices=sample)
    speed, gn, d, ab = wave_speed(m, X, dt, outputs=ALL, frames_per_pass=3)
    m.close()
    assert np.array_equal(d, wave_ref.temporal_gradient_phase(X, dt))
    bar = BAR * r["max_grad_M"]
    e_gn, e_ab = np.abs(gn[:, sample] - r["grad_norm"]).max(), np.abs(ab[:, sample] - r["grad_ab"]).max()
    print("max|grad_M| %.3g  |grad_norm - ref| %.3g  |grad_ab - ref| %.3g  bar %.3g"
          % (r["max_grad_M"], e_gn, e_ab, bar))
    assert e_gn <= bar and e_ab <= bar
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(speed, d / gn, equal_nan=True)
