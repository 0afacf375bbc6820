"""Capture the wave-speed golden vectors from the reference itself
(container-only tool, like make_golden.py).

Imports ``S5_compute_wave_v.py`` from ``/root/reference`` (read-only; bytecode
writing disabled; pyvista, absent here and only used by the script's plotting
and ``__main__``, replaced by an empty module) and runs its functions on the
meshes of G1, G2 and G3 with a small stand-in for the pyvista surface:
``points``, ``faces``, ``compute_cell_sizes()['Area']`` and
``point_cell_ids(i)`` (ascending triangle ids).

Input per mesh: T = 5 frames of a wrapped travelling phase,
``phases[t] = wrap(k . x + 0.9 - 0.7 t)`` with dt = 1/512; the amplitude input is
``np.cos(phases)``. Stored in ``G8_wave.npz`` per mesh (keys prefixed with the
fixture's name; the mesh arrays stay in the fixture they come from):
  phases                      (T, N), stored as float32 (exact)
  speed_phase, speed_amp      wave_velocity_phase / wave_velocity_amplitude
  ab_phase                    (alpha, beta) of the phases from compute_grad_M_I,
                              project_vector_to_plane, express_vector_on_basis
                              (the amplitudes' are pinned through speed_amp:
                              with them the file would outgrow the fixtures
                              beside it)
  grad_point_phase            compute_grad_M_I's result (G1 only)
Only data is stored: inputs and the reference's outputs.

Run:  python tests/golden/make_golden_wave.py
"""
from __future__ import annotations

import contextlib
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
MESHES = ("G1_ico642", "G2_cap641", "G3_ico642_f32")
T, DT = 5, 1.0 / 512


def load_reference():
    sys.dont_write_bytecode = True
    sys.modules.setdefault("pyvista", types.ModuleType("pyvista"))
    sys.path.insert(0, REF)
    import importlib
    mod = importlib.import_module("S5_compute_wave_v")
    sys.path.remove(REF)
    return mod


class Surface:
    """What the reference takes from its pyvista surface."""

    def __init__(self, points, triangles, areas):
        self.points = points
        tri = np.asarray(triangles, dtype=np.int64)
        self.faces = np.hstack([np.full((len(tri), 1), 3, dtype=np.int64), tri]).reshape(-1)
        self._areas = areas
        self._ids = [[] for _ in range(len(points))]
        for q, t in enumerate(tri.tolist()):
            for v in t:
                self._ids[v].append(q)

    def compute_cell_sizes(self, length=False, volume=False):
        return {"Area": self._areas}

    def point_cell_ids(self, index):
        return self._ids[index]


def wrapped_phase(points):
    p = np.asarray(points, dtype=np.float64)
    k = np.array([0.31, -0.23, 0.17])
    theta = p @ k + 0.9
    t = np.arange(T, dtype=np.float64)[:, None]
    x = np.mod(theta[None, :] - 0.7 * t + np.pi, 2 * np.pi) - np.pi
    # float32-representable values: the fixture compresses better. This k and
    # offset keep every vertex gradient above 1e-3 of the largest
    # per-triangle gradient in both modes on the three meshes (the zeros of
    # the gradient fall between vertices), so the speed is compared everywhere
    return x.astype(np.float32).astype(np.float64)


def tangent_ab(ref, surface, X, e):
    tri = surface.faces.reshape(-1, 4)[:, 1:]
    gp = ref.compute_grad_M_I(surface.points, tri, X, surface, surface._areas)
    ab = np.zeros((len(X), len(surface.points), 2))
    for t in range(len(X)):
        for i in range(len(surface.points)):
            vt = ref.project_vector_to_plane(gp[t][i], e[i][0], e[i][1])
            ab[t, i, 0], ab[t, i, 1] = ref.express_vector_on_basis(vt, e[i][0], e[i][1])
    return gp, ab


def main():
    ref = load_reference()
    out = {"dt": np.float64(DT)}
    for name in MESHES:
        with np.load(os.path.join(HERE, name + ".npz"), allow_pickle=False) as z:
            coords, tri, areas, e = z["coordinates"], z["triangles"], z["areas"], z["e"]
        surf = Surface(coords, tri, areas)
        phases = wrapped_phase(coords)
        amps = np.cos(phases)
        with contextlib.redirect_stdout(io.StringIO()):
            vp = ref.wave_velocity_phase(surf, phases, DT, T, e)
            va = ref.wave_velocity_amplitude(surf, amps, DT, T, e)
            gp, abp = tangent_ab(ref, surf, phases, e)
            _, aba = tangent_ab(ref, surf, amps, e)  # printed below, not stored
        out[name + "_phases"] = phases.astype(np.float32)  # exact: float32-representable values
        out[name + "_speed_phase"], out[name + "_speed_amp"] = vp, va
        out[name + "_ab_phase"] = abp
        if name == "G1_ico642":
            out[name + "_grad_point_phase"] = gp
        for tag, ab, v in (("phase", abp, vp), ("amp", aba, va)):
            g = np.sqrt((ab ** 2).sum(axis=2))
            print(name, tag, "min g / max g %.3g" % (g.min() / g.max()), "finite", bool(np.isfinite(v).all()),
                  "wrapped differences", int((np.abs(np.diff(phases, axis=0)) > np.pi).sum()))
    path = os.path.join(HERE, "G8_wave.npz")
    np.savez_compressed(path, **out)
    print("G8_wave", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
