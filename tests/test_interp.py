"""The host half of the electrode interpolation (mofhip.interp: the
reference's two S2 scripts) against scipy's Rbf and the golden vectors captured
from the scripts (tests/golden/G12_rbf.npz). No GPU: the device evaluation is
replaced by its numpy restatement where `interpolation` is exercised.

1. rbf_epsilon, rbf_matrix and rbf_phi equal ``Rbf(...).epsilon``, ``.A`` and
   ``Rbf._function(cdist(...))`` bit for bit -- on the golden's 62 electrodes,
   on float32-valued ones, on a planar grid (a zero extent of the bounding
   box, which epsilon leaves out) and on E = 2.
2. rbf_weights against the scripts' ``nodes``: both are backward-stable solves
   of the same matrix, so each is within 4 E u cond_2(A) |nodes| of the exact
   weights: the bar is 8 E u cond_2(A) max|nodes|.
3. interpolation: the slice ``[start_sample:end_sample]``, real data to the
   field, complex data to its angle, and the saved file.
"""
import numpy as np
import pytest
from scipy.interpolate import Rbf

from conftest import load_golden

from mofhip import interp

U = 2.0 ** -53


@pytest.fixture(scope="module")
def g12():
    return load_golden("G12_rbf")


def electrode_sets(g12):
    rng = np.random.default_rng(12)
    grid = np.stack(np.meshgrid(np.arange(4.0), np.arange(5.0), indexing="ij"), axis=-1).reshape(-1, 2)
    return {"golden": g12["electrodes"],
            "f32": (40 * rng.standard_normal((69, 3))).astype(np.float32),
            "planar": np.column_stack([7.5 * grid + rng.uniform(-1, 1, grid.shape), np.full(len(grid), 3.25)]),
            "pair": rng.standard_normal((2, 3))}


@pytest.mark.parametrize("name", ("golden", "f32", "planar", "pair"))
def test_epsilon_matrix_phi_bitwise(name, g12):
    xi = electrode_sets(g12)[name]
    rbf = Rbf(xi[:, 0], xi[:, 1], xi[:, 2], np.zeros(len(xi)))
    eps = interp.rbf_epsilon(xi)
    assert eps == rbf.epsilon
    assert np.array_equal(interp.rbf_matrix(xi), rbf.A)
    assert np.array_equal(interp.rbf_matrix(xi, 3.5), Rbf(xi[:, 0], xi[:, 1], xi[:, 2], np.zeros(len(xi)), epsilon=3.5).A)
    pts = g12["points"][::13].astype(np.float64)
    want = rbf._function(rbf._call_norm(pts.T, rbf.xi))
    assert np.array_equal(interp.rbf_phi(pts, xi, eps), want)
    # a one-hot nodes vector through scipy's own __call__: exactly w * phi[:, k]
    k = len(xi) // 2
    rbf.nodes = np.zeros(len(xi))
    rbf.nodes[k] = -0.125
    assert np.array_equal(rbf(pts[:, 0], pts[:, 1], pts[:, 2]), -0.125 * want[:, k])


def test_epsilon_of_one_electrode_is_refused():
    with pytest.raises(ValueError):
        interp.rbf_epsilon(np.array([[1.0, 2.0, 3.0]]))


@pytest.mark.parametrize("kind", ("real", "phase"))
def test_weights_against_reference_nodes(kind, g12):
    xi = g12["electrodes"]
    E = len(xi)
    if kind == "real":
        data = g12["real_data"][int(g12["real_start"]):int(g12["real_stop"])]
    else:
        from scipy.signal import hilbert
        data = np.exp(1j * np.angle(hilbert(g12["phase_pot"])))[int(g12["phase_start"]):int(g12["phase_stop"])]
    nodes = g12[kind + "_nodes"]
    W = interp.rbf_weights(xi, data)
    assert W.shape == nodes.shape and W.flags.c_contiguous
    assert np.iscomplexobj(W) == (kind == "phase")
    cond = np.linalg.cond(interp.rbf_matrix(xi), 2)
    bar = 8 * E * U * cond * np.abs(nodes).max()
    err = np.abs(W - nodes).max()
    print("%s: |weights - nodes| %.3g = %.3g of the bar (cond2 %.3g, %.3g relative to max|nodes|)"
          % (kind, err, err / bar, cond, err / np.abs(nodes).max()))
    assert err <= bar


def numpy_eval(points, coordinates, weights, epsilon=None, angle=False, device=0):
    phi = interp.rbf_phi(points, coordinates, interp.rbf_epsilon(coordinates) if epsilon is None else epsilon)
    out = (phi @ np.asarray(weights).T).T
    return np.angle(out) if angle else out


def test_interpolation_semantics(g12, monkeypatch, tmp_path):
    seen = []

    def spy(points, coordinates, weights, epsilon=None, angle=False, device=0):
        seen.append((np.asarray(weights).shape, bool(angle), np.asarray(points).dtype))
        return numpy_eval(points, coordinates, weights, epsilon, angle)

    monkeypatch.setattr(interp, "rbf_eval", spy)
    xi, pts = g12["electrodes"], g12["points"][:200]
    a, b = int(g12["real_start"]), int(g12["real_stop"])
    out = interp.interpolation(pts, g12["real_data"], xi, a, b)
    assert seen[-1] == ((b - a, len(xi)), False, np.float32) and out.shape == (b - a, 200) and out.dtype == np.float64
    # the slice is the scripts': frames [a, b) of the input, nothing else
    again = interp.interpolation(pts, g12["real_data"][a:b], xi, 0, b - a)
    assert np.array_equal(out, again)
    # against the scripts' field: the weights' bar (check 2) through sum |phi|, plus two evaluations' rounding
    ref = g12["real_field"][:, :200]
    phi = np.abs(interp.rbf_phi(pts, xi, interp.rbf_epsilon(xi)))
    cond = np.linalg.cond(interp.rbf_matrix(xi), 2)
    E = len(xi)

    def bar(nodes):
        return (8 * E * U * cond * np.abs(nodes).max() * phi.sum(axis=1)[None, :]
                + 2 * (E + 1) * U * (np.abs(nodes) @ phi.T))

    err = np.abs(out - ref) / bar(g12["real_nodes"])
    print("real: |field - reference| %.3g of the bar" % err.max())
    assert err.max() <= 1
    # complex data: the angle of the interpolant, as the phase script saves it
    from scipy.signal import hilbert
    ph = np.exp(1j * np.angle(hilbert(g12["phase_pot"])))
    ang = interp.interpolation(pts, ph, xi, 0, 8)
    assert seen[-1] == ((8, len(xi)), True, np.float32) and ang.dtype == np.float64
    d = np.abs(np.angle(np.exp(1j * (ang - g12["phase_angle"][:, :200]))))
    zbar = 2 * bar(g12["phase_nodes"]) / np.abs(g12["phase_field"][:, :200]) + 8 * U * np.pi  # both planes
    print("phase: |angle - reference| %.3g of the bar" % (d / zbar).max())
    assert (d <= zbar).all()
    with pytest.raises(ValueError):
        interp.interpolation(pts, g12["real_data"], xi, 5, 5)
    # ifsave: the bytes of pd.DataFrame(values).to_csv(path)
    import pandas as pd
    path = tmp_path / "interpolation_data.csv"
    saved = interp.interpolation(pts, g12["real_data"], xi, a, b, str(path), True)
    want = tmp_path / "pandas.csv"
    pd.DataFrame(saved).to_csv(want)
    assert path.read_bytes() == want.read_bytes()
    assert np.array_equal(pd.read_csv(path, header="infer", index_col=0).values.shape, saved.shape)


def test_eval_argument_checks():
    xi = np.zeros((3, 3))
    with pytest.raises(ValueError):
        interp.rbf_eval(np.zeros((4, 3)), xi, np.zeros((2, 3)), 1.0, angle=True)  # the angle of real weights
    with pytest.raises(ValueError):
        interp.rbf_eval(np.zeros((4, 3)), xi, np.zeros((2, 4)), 1.0)
    with pytest.raises(ValueError):
        interp.rbf_eval(np.zeros((4, 2)), xi, np.zeros((2, 3)), 1.0)
    with pytest.raises(ValueError):
        interp.rbf_weights(xi, np.zeros((2, 4)))
