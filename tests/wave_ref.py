"""CPU checker of the wave-speed path: S5_compute_wave_v.py restated in numpy.

Every step keeps the reference's operations and their order -- the same numpy
calls on the same operands, with the time axis vectorised where the reference
applies one elementwise operation per frame -- so the results equal the
reference's bit for bit (tests/test_wave.py pins that against
tests/golden/G8_wave.npz, captured from the reference itself). The triangles
of a vertex are taken in ascending index.

Line numbers: S5_compute_wave_v.py of the reference.
"""
from __future__ import annotations

import numpy as np


def gradient_w(p_i, p_j, p_k):
    """compute_gradient_w (S5:125-134); float32 points stay float32."""
    vector_jk = p_k - p_j
    vector_ji = p_i - p_j
    perpendicular_vector = np.dot(vector_ji, vector_jk) * vector_jk / np.dot(vector_jk, vector_jk)
    vector_ih = p_j - p_i + perpendicular_vector
    return vector_ih / np.dot(vector_ih, vector_ih)


def triangle_gradients(coordinates, triangles, X, only=None):
    """grad_w (M,3,3) and grad_M (T,M,3) (S5:143-159). only: the triangle ids
    to fill (the others stay zero)."""
    T, M = len(X), len(triangles)
    grad_w = np.zeros((M, 3, 3))
    grad_M = np.zeros((T, M, 3))
    for q in (range(M) if only is None else only):
        A, B, C = triangles[q]
        grad_w[q][0] = gradient_w(coordinates[A], coordinates[B], coordinates[C])
        grad_w[q][1] = gradient_w(coordinates[B], coordinates[A], coordinates[C])
        grad_w[q][2] = gradient_w(coordinates[C], coordinates[A], coordinates[B])
        g = grad_w[q]
        grad_M[:, q] = (X[:, A, None] * g[0] + X[:, B, None] * g[1] + X[:, C, None] * g[2])
    return grad_w, grad_M


def incident_triangles(triangles, N):
    """point_cell_ids of every vertex, ascending."""
    ids = [[] for _ in range(N)]
    for q, tri in enumerate(np.asarray(triangles).tolist()):
        for v in tri:
            ids[v].append(q)
    return ids


def vertex_gradients(grad_M, areas, ids, vertices):
    """grad_point (T, len(vertices), 3): area-weighted mean (S5:161-169)."""
    out = np.zeros((grad_M.shape[0], len(vertices), 3))
    for n, i in enumerate(vertices):
        all_areas = 0
        for q in ids[i]:
            out[:, n] += grad_M[:, q] * areas[q]
            all_areas += areas[q]
        with np.errstate(invalid="ignore", divide="ignore"):
            out[:, n] /= all_areas
    return out


def tangent_components(grad_point, e, vertices):
    """(alpha, beta) (T, len(vertices), 2): project_vector_to_plane then
    express_vector_on_basis (S5:173-191)."""
    T = grad_point.shape[0]
    out = np.zeros((T, len(vertices), 2))
    for n, i in enumerate(vertices):
        e1, e2 = e[i][0], e[i][1]
        nrm = np.cross(e1, e2)
        for t in range(T):
            V = grad_point[t, n]
            Vt = V - np.dot(V, nrm) * nrm / np.dot(nrm, nrm)
            out[t, n, 0] = np.dot(Vt, e1) / np.dot(e1, e1)
            out[t, n, 1] = np.dot(Vt, e2) / np.dot(e2, e2)
    return out


def angle_subtract(f1, f2):
    return np.mod(f1 - f2 + np.pi, 2 * np.pi) - np.pi  # S5:230


def temporal_gradient_phase(data, dt):
    """compute_temporal_gradient_phase (S5:60-77)."""
    t = data.shape[0]
    g = np.zeros_like(data)
    g[0] = angle_subtract(data[1], data[0]) / dt
    for i in range(1, t - 1):
        g[i] = angle_subtract(data[i + 1], data[i - 1]) / (2 * dt)
    g[t - 1] = angle_subtract(data[t - 1], data[t - 2]) / dt
    return g


def temporal_gradient_amplitude(data, dt):
    """np.gradient(data, axis=0, edge_order=2) / dt (S5:24), spelled out."""
    g = np.zeros_like(data)
    g[0] = (-1.5 * data[0] + 2.0 * data[1]) - 0.5 * data[2]
    g[-1] = (0.5 * data[-3] - 2.0 * data[-2]) + 1.5 * data[-1]
    g[1:-1] = (data[2:] - data[:-2]) / 2.0
    return g / dt


def wave_speed(coordinates, triangles, areas, e, X, dt, phase=True, vertices=None):
    """Every quantity of wave_velocity_phase / wave_velocity_amplitude
    (S5:14-123) for the listed vertices (default: all): dict with dXdt,
    grad_point, grad_ab, grad_norm, speed and max_grad_M (the largest
    per-triangle gradient entry, the scale of the parity bars)."""
    X = np.asarray(X, dtype=np.float64)
    N = len(coordinates)
    ids = incident_triangles(triangles, N)
    if vertices is None:
        vertices, only = list(range(N)), None
    else:
        vertices = [int(v) for v in vertices]
        only = sorted({q for i in vertices for q in ids[i]})
    d = (temporal_gradient_phase(X, dt) if phase else temporal_gradient_amplitude(X, dt))[:, vertices]
    _, grad_M = triangle_gradients(coordinates, triangles, X, only)
    gp = vertex_gradients(grad_M, areas, ids, vertices)
    ab = tangent_components(gp, e, vertices)
    # S5:52 squares numpy scalars, which goes through the C library's pow (an
    # array's ** 2 is a multiplication, and differs from it in the last bit
    # now and then): element by element, as the reference does
    gn = np.zeros(ab.shape[:2])
    for t in range(ab.shape[0]):
        for n in range(ab.shape[1]):
            gn[t, n] = np.sqrt(ab[t, n, 0] ** 2 + ab[t, n, 1] ** 2)
    with np.errstate(invalid="ignore", divide="ignore"):
        speed = d / gn  # S5:56
    return {"dXdt": d, "grad_point": gp, "grad_ab": ab, "grad_norm": gn, "speed": speed,
            "max_grad_M": float(np.abs(grad_M).max())}
