"""Potentials on the mesh from the electrodes: the reference's
``S2_interpolate.py`` and ``S2_interpolate_phases.py``.

Both scripts build ``scipy.interpolate.Rbf(x, y, z, d)`` with all defaults
(multiquadric, euclidean norm, ``smooth = 0``) for every frame and evaluate it
at the surface's vertices. The ``E x E`` matrix of an ``Rbf`` depends on the
electrodes alone, so the frames share it:

1. :func:`rbf_weights`: ``A = sqrt((r / epsilon)^2 + 1)`` on the electrodes'
   pairwise distances and **one** ``numpy.linalg.solve(A, data.T)`` for all
   frames on the host, ``O(E^3 + E^2 T)`` (the library links no LAPACK: the
   same division of labour as ``eigh`` in :mod:`mofhip.modes`);
2. ``mof_rbf_eval``: ``out[t, i] = sum_e W[t, e] phi(i, e)`` on the fp64 matrix
   cores, ``phi`` generated on the fly -- scipy's ``cdist`` and multiquadric
   bit for bit -- and never stored; for the phase script's complex data both
   planes, or directly ``np.angle`` of the interpolant.

:func:`interpolation` is named and called like the scripts' function, with the
vertices where they read ``pv.read(surface_path).points``; it returns the
array the scripts only save. MNE / TSV reading, the channel selection and
``hilbert`` stay with the caller (scipy). Other ``Rbf`` functions, norms and
``smooth != 0`` are not restated.

Accuracy: the evaluation is within ``(E + 1) u sum_e |W phi|`` of the exact
sum, ``u = 2^-53``; the weights carry the solve's ``cond(A)`` (about 2e4 on a
62-electrode grid), as the reference's do.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib as L

MAX_ELECTRODES = 256  # include/mof.h: mof_rbf_eval's cap on E


def _coordinates(coordinates):
    xi = np.asarray(coordinates, dtype=np.float64)
    if xi.ndim != 2 or xi.shape[1] != 3 or xi.shape[0] < 1:
        raise ValueError("need coordinates (E, 3) with E >= 1")
    return xi


def rbf_epsilon(coordinates):
    """``Rbf(...).epsilon`` for electrodes (E, 3): "the average distance
    between nodes" of the bounding box with its zero extents left out."""
    xi = _coordinates(coordinates).T
    ximax = np.amax(xi, axis=1)
    ximin = np.amin(xi, axis=1)
    edges = ximax - ximin
    edges = edges[np.nonzero(edges)]
    if edges.size == 0:
        raise ValueError("the electrodes' bounding box has no extent: epsilon is undefined")
    return np.power(np.prod(edges) / xi.shape[-1], 1.0 / edges.size)


def rbf_phi(points, coordinates, epsilon):
    """``phi (N, E)``: the multiquadric of the distances from points (N, 3) to
    electrodes (E, 3), statement by statement what ``mof_rbf_eval`` computes
    and bit-identical to ``Rbf._function(cdist(points, electrodes))``."""
    p = np.asarray(points, dtype=np.float64)
    xi = _coordinates(coordinates)
    dx = p[:, None, 0] - xi[None, :, 0]
    dy = p[:, None, 1] - xi[None, :, 1]
    dz = p[:, None, 2] - xi[None, :, 2]
    r = np.sqrt((dx * dx + dy * dy) + dz * dz)
    q = (1.0 / epsilon) * r
    return np.sqrt(q * q + 1)


def rbf_matrix(coordinates, epsilon=None):
    """``Rbf(...).A`` (E, E) for ``smooth = 0``."""
    xi = _coordinates(coordinates)
    return rbf_phi(xi, xi, rbf_epsilon(xi) if epsilon is None else epsilon)


def rbf_weights(coordinates, data, epsilon=None):
    """``Rbf(...).nodes`` of every frame: data (T, E), real or complex, to the
    weights (T, E) by one ``numpy.linalg.solve`` of the shared matrix."""
    xi = _coordinates(coordinates)
    d = np.asarray(data)
    if d.ndim != 2 or d.shape[1] != xi.shape[0]:
        raise ValueError("need data (T, E) with one column per electrode")
    if not np.iscomplexobj(d):
        d = d.astype(np.float64, copy=False)
    return np.ascontiguousarray(np.linalg.solve(rbf_matrix(xi, epsilon), d.T).T)


def _flags(angle, complex_):
    if angle and not complex_:
        raise ValueError("angle=True needs complex weights")
    return L.MOF_RBF_ANGLE if angle else 0


def rbf_eval(points, coordinates, weights, epsilon=None, angle=False, device: int = 0):
    """The interpolant of every frame at points (N, 3): (T, N) float64, or
    complex for complex weights -- or, with ``angle=True``, its ``np.angle``
    as float64 straight from the device."""
    p = np.ascontiguousarray(points, dtype=np.float64)
    xi = np.ascontiguousarray(_coordinates(coordinates))
    if p.ndim != 2 or p.shape[1] != 3 or p.shape[0] < 1:
        raise ValueError("need points (N, 3) with N >= 1")
    W = np.asarray(weights)
    if W.ndim != 2 or W.shape[1] != xi.shape[0] or W.shape[0] < 1:
        raise ValueError("need weights (T, E) with T >= 1")
    cplx = np.iscomplexobj(W)
    fl = _flags(angle, cplx)
    eps = float(rbf_epsilon(xi) if epsilon is None else epsilon)
    T, E, N = W.shape[0], xi.shape[0], p.shape[0]
    Wr = np.ascontiguousarray(W.real, dtype=np.float64)
    Wi = np.ascontiguousarray(W.imag, dtype=np.float64) if cplx else None
    out = np.empty((T, N))
    out_im = np.empty((T, N)) if cplx and not angle else None
    L.check(L.lib().mof_rbf_eval(int(device), L.ptr(p), N, L.ptr(xi), E, eps, L.ptr(Wr),
                                 L.ptr(Wi) if cplx else None, T, fl, None, L.ptr(out),
                                 L.ptr(out_im) if out_im is not None else None))
    if out_im is None:
        return out
    res = np.empty((T, N), dtype=complex)
    res.real = out
    res.imag = out_im
    return res


def rbf_eval_device(points_ptr: int, N: int, coordinates_ptr: int, E: int, epsilon, W_re_ptr: int, T: int,
                    out_ptr: int, W_im_ptr=None, out_im_ptr=None, angle=False, device: int = 0, stream=None):
    """Device-pointer form: points (N, 3), electrodes (E, 3), the weights'
    planes (T, E) and the outputs (T, N), all float64 already in HBM on
    ``device`` (``stream``: a hipStream_t or None); returns when done."""
    p = lambda a: ctypes.c_void_p(a) if a else None  # noqa: E731
    L.check(L.lib().mof_rbf_eval(int(device), p(points_ptr), int(N), p(coordinates_ptr), int(E), float(epsilon),
                                 p(W_re_ptr), p(W_im_ptr), int(T), _flags(angle, bool(W_im_ptr)) | L.MOF_IO_DEVICE,
                                 stream, p(out_ptr), p(out_im_ptr)))


def interpolation(points, ieeg_data_array, coordinates, start_sample, end_sample, save_path=None, ifsave=False,
                  device: int = 0):
    """``interpolation(surface_path, ieeg_data_array, coordinates, start_sample,
    end_sample, save_path, ifsave)`` of the two S2 scripts, with ``points``
    (N, 3) where they read ``pv.read(surface_path).points`` (float32 points
    are widened exactly, as ``Rbf`` does). Returns the (T, N) array the
    scripts save: the interpolated potentials for real data, ``np.angle`` of
    the interpolant for complex data (the phase script's ``exp(1j * phases)``).
    With ``ifsave`` it is written to ``save_path`` in the bytes of
    ``pd.DataFrame(values).to_csv(save_path)``, which ``load_potentials``
    reads back."""
    data = np.asarray(ieeg_data_array)[start_sample:end_sample]
    if data.ndim != 2 or data.shape[0] < 1:
        raise ValueError("need ieeg_data_array (time, electrodes) and a non-empty sample range")
    W = rbf_weights(coordinates, data)
    values = rbf_eval(points, coordinates, W, angle=np.iscomplexobj(W), device=device)
    if ifsave:
        from .csvio import write_csv
        write_csv(save_path, values)
    return values
