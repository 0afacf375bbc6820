"""Wave speed on the mesh: the reference's ``S5_compute_wave_v.py`` on the GPU.

The reference estimates the propagation speed of a phase (or amplitude) field
X (T, N) as ``(dX/dt) / |grad_M X|`` per vertex and frame, in nested Python
loops over triangles x frames and vertices x frames (S5:14-171).
``mof_wave_speed`` does the same in one fused pass per chunk of frames on a
:class:`~mofhip.mesh.DeviceMesh` handle, which already holds ``e``, ``grad_w``,
the areas and the vertex adjacency in HBM.

The functions named like the reference's take a ``DeviceMesh`` where the
reference takes its pyvista ``surface`` and return what it returns (the
signed speed; S5's ``/ 1000`` and ``abs`` stay with the caller). The
reference's progress prints of array shapes are not restated, and
``compute_phase_from_potentials`` (scipy ``hilbert``) stays with scipy.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib as L
from .mesh import DeviceMesh

OUTPUTS = ("speed", "grad_norm", "dXdt", "grad_ab")


def wave_speed(mesh: DeviceMesh, X, dt, phase=True, device=None, frames_per_pass=0, outputs=("speed",)):
    """The requested arrays of ``outputs`` (names from :data:`OUTPUTS`), in
    that order as a tuple -- a single array for a single name. X (T, N) in the
    caller's vertex order: phases (``phase=True``: wrapped differences,
    S5:60-77) or amplitudes (``np.gradient(edge_order=2)``, S5:24).
    ``speed``, ``grad_norm``, ``dXdt`` are (T, N), ``grad_ab`` (T, N, 2).
    ``frames_per_pass``: frames per device pass (0: the library's choice; the
    results do not depend on it)."""
    names = (outputs,) if isinstance(outputs, str) else tuple(outputs)
    for n in names:
        if n not in OUTPUTS:
            raise ValueError("unknown output %r (one of %s)" % (n, ", ".join(OUTPUTS)))
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[1] != mesh.N:
        raise ValueError("X must be (T, N)")
    T = X.shape[0]
    arr = {n: np.empty((T, mesh.N, 2) if n == "grad_ab" else (T, mesh.N)) for n in names}
    h = mesh.handle(device)
    with mesh.lock(device):
        L.check(L.lib().mof_wave_speed(
            h, L.ptr(X), T, float(dt), L.MOF_WAVE_PHASE if phase else 0, int(frames_per_pass), None,
            *[L.ptr(arr[n]) if n in arr else None for n in OUTPUTS]))
    res = tuple(arr[n] for n in names)
    return res[0] if isinstance(outputs, str) or len(res) == 1 else res


def wave_speed_device(mesh: DeviceMesh, X_ptr: int, T: int, dt, phase=True, device=None, frames_per_pass=0,
                      stream=None, speed_ptr=None, grad_norm_ptr=None, dXdt_ptr=None, grad_ab_ptr=None):
    """Device-pointer form: X and the outputs are already in HBM on the
    handle's device (``stream``: a hipStream_t or None); returns when done."""
    h = mesh.handle(device)
    with mesh.lock(device):
        L.check(L.lib().mof_wave_speed(
            h, ctypes.c_void_p(X_ptr), int(T), float(dt), (L.MOF_WAVE_PHASE if phase else 0) | L.MOF_IO_DEVICE,
            int(frames_per_pass), stream, *[ctypes.c_void_p(p) if p else None
                                            for p in (speed_ptr, grad_norm_ptr, dXdt_ptr, grad_ab_ptr)]))


def _check_steps(X, time_steps):
    if int(time_steps) != len(X):
        raise ValueError("time_steps must be the number of frames")


def wave_velocity_phase(mesh: DeviceMesh, phases, dt, time_steps, e=None):
    """``wave_velocity_phase(surface, phases, dt, time_steps, e)`` (S5:79-123).
    ``e`` is accepted for the signature; the handle's own bases are used."""
    _check_steps(phases, time_steps)
    return wave_speed(mesh, phases, dt, phase=True)


def wave_velocity_amplitude(mesh: DeviceMesh, potentials, dt, time_steps, e=None):
    """``wave_velocity_amplitude(surface, potentials, dt, time_steps, e)``
    (S5:14-58)."""
    _check_steps(potentials, time_steps)
    return wave_speed(mesh, potentials, dt, phase=False)


def angle_subtract(f1, f2, angleFlag=True):
    """Difference of angles in [-pi, pi) (S5:225-233)."""
    return np.mod(f1 - f2 + np.pi, 2 * np.pi) - np.pi if angleFlag else f1 - f2


def compute_temporal_gradient_phase(data, dt):
    """Host numpy: one-sided wrapped differences at the two ends, centred
    ones between (S5:60-77)."""
    data = np.asarray(data)
    t = data.shape[0]
    gradients = np.zeros_like(data)
    gradients[0] = angle_subtract(data[1], data[0]) / dt
    for i in range(1, t - 1):
        gradients[i] = angle_subtract(data[i + 1], data[i - 1]) / (2 * dt)
    gradients[t - 1] = angle_subtract(data[t - 1], data[t - 2]) / dt
    return gradients
