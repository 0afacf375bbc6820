"""Capture the electrode-interpolation golden vectors from the reference itself
(container-only tool, like make_golden_modes.py).

Loads the reference's ``S2_interpolate.py`` and ``S2_interpolate_phases.py`` by
path (bytecode writing disabled; ``mne``, ``pyvista`` and ``matplotlib``, used
only for file input and plotting, replaced by stubs where missing -- the
``pv.read`` stub returns an object whose ``.points`` are the stored vertices)
and calls their ``interpolation`` with the scripts' ``Rbf`` name replaced by a
recording subclass of scipy's: the scripts return nothing and only save, so
the subclass keeps each frame's ``nodes``, ``epsilon`` and the call's result.
The phase script's input is formed as its ``__main__`` forms it:
``np.exp(1j * compute_phase_from_potentials(potentials))``, the script's own
``hilbert`` call over the last axis.

Inputs (seeded, stored):
  points       the S1s patch ``synth.electrode_surface(8, 10.0)``, 3,249
               vertices, as float32 (what pyvista hands the scripts)
  electrodes   the jittered 8 x 8 grid the patch is drawn from
               (``default_rng(0)``, on the radius-70 sphere) without rows 27
               and 28, the stimulated pair: E = 62
  real_data    (8, 62): ``1e-4 sin(0.05 x + 0.03 y - 0.3 t)``, t = 0 .. 7;
               the call takes samples 1 .. 6 (real_start, real_stop)
  phase_pot    (64, 62): ``sin(0.05 x + 0.03 y - 0.3 t)``; the call takes
               samples 0 .. 7 of the unit phasors (phase_start, phase_stop)

Asserted here: cond_2(A) <= 1e6; min |z| >= 0.01 over the complex fields (the
angle is well conditioned); the no-contraction numpy phi of mofhip.interp
equals the reference's ``_function(cdist(...))`` bit for bit; epsilon and A of
mofhip.interp equal the reference's bit for bit. Printed: what the pure-numpy
chain (``rbf_weights`` + ``@``) measures against the reference.

Stored in ``G12_rbf.npz`` (only data): the inputs above, and per case
  real_nodes (6, 62), real_field (6, 3249), epsilon
  phase_nodes (8, 62) complex, phase_field (8, 3249) complex, phase_angle

Run:  python tests/golden/make_golden_rbf.py <path of the reference>
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "manifold-based-optical-flow-method_amd"))

SCRIPTS = {"real": "S2_interpolate.py", "phase": "S2_interpolate_phases.py"}
U = 2.0 ** -53


def load_reference(ref, points):
    sys.dont_write_bytecode = True
    for name in ("pyvista", "mne", "matplotlib"):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    if not hasattr(sys.modules["matplotlib"], "pyplot"):
        try:
            import matplotlib.pyplot  # noqa: F401
        except ImportError:
            sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"] = types.ModuleType("matplotlib.pyplot")
    from scipy.interpolate import Rbf

    class RecordingRbf(Rbf):
        calls = []

        def __call__(self, *args):
            out = Rbf.__call__(self, *args)
            RecordingRbf.calls.append((self, out))
            return out

    surface = types.SimpleNamespace(points=points)
    mods = {}
    for kind, fname in SCRIPTS.items():
        spec = importlib.util.spec_from_file_location("s2_" + kind, os.path.join(ref, fname))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.Rbf = RecordingRbf
        mod.pv = types.SimpleNamespace(read=lambda path: surface)
        mods[kind] = mod
    return mods, RecordingRbf


def electrode_grid(n_side=8, spacing=10.0, jitter=0.15, radius=70.0, seed=0):
    """The grid synth.electrode_surface starts from, statement by statement."""
    rng = np.random.default_rng(seed)
    g = (np.arange(n_side) - 0.5 * (n_side - 1)) * spacing
    x, y = np.meshgrid(g, g, indexing="ij")
    xy = np.stack([x.ravel(), y.ravel()], axis=1)
    xy += jitter * spacing * rng.uniform(-1.0, 1.0, size=xy.shape)
    z = np.sqrt(np.maximum(radius ** 2 - (xy ** 2).sum(axis=1), 0.0)) - radius
    return np.column_stack([xy, z])


def run(mod, rec, data, coordinates, start, stop):
    """The script's interpolation on one input: (nodes, epsilon, fields, phi)
    of its frames, from the recorder."""
    del rec.calls[:]
    mod.interpolation("surface.ply", data, coordinates, start, stop, None, False)
    assert len(rec.calls) == stop - start
    nodes = np.array([r.nodes for r, _ in rec.calls])
    eps = {float(r.epsilon) for r, _ in rec.calls}
    assert len(eps) == 1
    return nodes, eps.pop(), np.array([o for _, o in rec.calls]), rec.calls[0][0]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    from mofhip import synth
    from mofhip.interp import rbf_epsilon, rbf_matrix, rbf_phi, rbf_weights
    points = synth.electrode_surface(8, 10.0)[0].astype(np.float32)
    assert points.shape == (3249, 3)
    electrodes = np.delete(electrode_grid(), (27, 28), axis=0)
    E = len(electrodes)
    assert E == 62
    x, y = electrodes[:, 0], electrodes[:, 1]
    real_data = 1e-4 * np.sin(0.05 * x + 0.03 * y - 0.3 * np.arange(8)[:, None])
    phase_pot = np.sin(0.05 * x + 0.03 * y - 0.3 * np.arange(64)[:, None])
    mods, rec = load_reference(sys.argv[1], points)
    out = {"points": points, "electrodes": electrodes, "real_data": real_data, "phase_pot": phase_pot,
           "real_start": np.array(1), "real_stop": np.array(7), "phase_start": np.array(0),
           "phase_stop": np.array(8)}

    phasors = np.exp(1j * mods["phase"].compute_phase_from_potentials(phase_pot))
    for kind, data, (a, b) in (("real", real_data, (1, 7)), ("phase", phasors, (0, 8))):
        nodes, eps, field, rbf = run(mods[kind], rec, data, electrodes, a, b)
        A = rbf.A
        cond = np.linalg.cond(A, 2)
        assert cond <= 1e6, cond
        # the restatement against the reference, bit for bit
        assert eps == rbf_epsilon(electrodes) and np.array_equal(A, rbf_matrix(electrodes))
        p64 = points.astype(np.float64)
        phi_ref = rbf._function(rbf._call_norm(p64.T, rbf.xi))
        phi = rbf_phi(p64, electrodes, eps)
        assert np.array_equal(phi, phi_ref), "numpy phi differs from the reference's"
        # the pure-numpy chain against the reference
        W = rbf_weights(electrodes, data[a:b])
        S = np.abs(phi) @ np.abs(nodes).T
        chain = phi @ W.T
        d = np.abs(chain.T - field)
        print("%s: cond2(A) %.3g, epsilon %.17g; numpy chain vs reference: %.3g of max|ref|, %.3g u S; weights "
              "within %.3g relative; numpy phi @ reference's nodes vs reference: %.3g u S"
              % (kind, cond, eps, d.max() / np.abs(field).max(), (d / (U * S.T)).max(),
                 np.abs(W - nodes).max() / np.abs(nodes).max(),
                 (np.abs((phi @ nodes.T).T - field) / (U * S.T)).max()))
        out["epsilon"] = np.array(eps)
        out[kind + "_nodes"] = nodes
        out[kind + "_field"] = field
        if kind == "phase":
            assert np.iscomplexobj(field) and np.abs(field).min() >= 0.01, np.abs(field).min()
            print("phase: min |z| %.4g" % np.abs(field).min())
            out["phase_angle"] = np.angle(field)
    path = os.path.join(HERE, "G12_rbf.npz")
    np.savez_compressed(path, **out)
    print("G12_rbf", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
