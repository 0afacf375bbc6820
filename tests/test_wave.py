"""Wave speed (S5_compute_wave_v.py), the parts that need no GPU: the numpy
checker tests/wave_ref.py reproduces every array captured from the reference
(tests/golden/G8_wave.npz) bit for bit, and the library and package carry the
new entry point."""
import numpy as np
import pytest

from conftest import load_golden

import wave_ref

MESHES = ["G1_ico642", "G2_cap641", "G3_ico642_f32"]


@pytest.fixture(scope="module")
def g8():
    g = load_golden("G8_wave")
    return {k: v.astype(np.float64) if k.endswith("_phases") else v for k, v in g.items()}


@pytest.mark.parametrize("name", MESHES)
@pytest.mark.parametrize("mode", ["phase", "amp"])
def test_wave_ref_reproduces_the_reference(g8, name, mode):
    g = load_golden(name)
    X = g8[name + "_phases"]
    if mode == "amp":
        X = np.cos(X)
    r = wave_ref.wave_speed(g["coordinates"], g["triangles"], g["areas"], g["e"], X, float(g8["dt"]),
                            phase=mode == "phase")
    if mode == "phase":  # the amplitudes' (alpha, beta) are pinned through their speed
        assert np.array_equal(r["grad_ab"], g8[name + "_ab_phase"])
    assert np.array_equal(r["speed"], g8["%s_speed_%s" % (name, mode)])
    assert np.isfinite(r["speed"]).all()
    key = "%s_grad_point_%s" % (name, mode)
    if key in g8:
        assert np.array_equal(r["grad_point"], g8[key])


def test_amplitude_gradient_is_numpy_gradient(g8):
    X = np.cos(g8["G1_ico642_phases"])
    dt = float(g8["dt"])
    assert np.array_equal(wave_ref.temporal_gradient_amplitude(X, dt), np.gradient(X, axis=0, edge_order=2) / dt)
    assert np.array_equal(wave_ref.temporal_gradient_amplitude(X[:3], dt),
                          np.gradient(X[:3], axis=0, edge_order=2) / dt)


def test_vertex_subset_matches_full_run(g8):
    g = load_golden("G2_cap641")
    X = g8["G2_cap641_phases"]
    sub = list(range(0, len(g["coordinates"]), 97))
    full = wave_ref.wave_speed(g["coordinates"], g["triangles"], g["areas"], g["e"], X, float(g8["dt"]))
    part = wave_ref.wave_speed(g["coordinates"], g["triangles"], g["areas"], g["e"], X, float(g8["dt"]),
                               vertices=sub)
    for k in ("dXdt", "grad_ab", "grad_norm", "speed"):
        assert np.array_equal(part[k], full[k][:, sub]), k


def test_entry_point_is_exported():
    from mofhip import _lib as L
    assert "mof_wave_speed" in L.EXPORTS
    assert hasattr(L.lib(), "mof_wave_speed")


def test_package_exports_wave():
    import mofhip
    import mofhip.wave as W
    for name in ("wave_speed", "wave_velocity_phase", "wave_velocity_amplitude",
                 "compute_temporal_gradient_phase"):
        assert callable(getattr(W, name))
        assert getattr(mofhip, name) is getattr(W, name)


def test_host_temporal_gradient_phase(g8):
    from mofhip.wave import compute_temporal_gradient_phase
    X = g8["G1_ico642_phases"]
    dt = float(g8["dt"])
    assert np.array_equal(compute_temporal_gradient_phase(X, dt), wave_ref.temporal_gradient_phase(X, dt))
    assert np.array_equal(compute_temporal_gradient_phase(X[:2], dt), wave_ref.temporal_gradient_phase(X[:2], dt))
