"""Capture the spatiotemporal-mode golden vectors from the reference itself
(container-only tool, like make_golden_winding.py).

Loads the reference's two ``S4_spatiotemporal_decomposition_*`` scripts by
path (their file names hold a space; bytecode writing disabled; ``pyvista``,
``mne``, ``matplotlib``, ``yaml`` and ``utils.draw_optical_flow_field``, used
only for plotting and file input, replaced by empty modules where missing) and
runs, for every input, their ``process_V_k_to_complex``, the decomposition
statements of their ``__main__`` -- read from the script and executed here
with ``full_matrices=False``, chosen by data flow: every one-line assignment
that calls only numpy and ``calculate_percentages`` and whose inputs exist,
starting from ``V_k_coord``, which is the svd, the percentages, the cut to
four modes and the sign flip -- and their ``extract_modes`` with the plot call
replaced by a recorder, which yields ``calculate_V_k_from_complex(sigma * vt, e)``.

Inputs: the ``V_k`` of G1 (K = 15, N = 642), G2 (K = 5, N = 641) and G3, and
one synthetic ``M1``: K = 40, N = 1000, X = sum_j 0.8^j a_j b_j^H with complex
orthonormal a_j, b_j (QR of ``default_rng(0)`` normals), rounded to float32 so
that the stored input is exact and small. The goldens' complex and concat
spectra coincide to the digits printed (their A is negligible): M1 is the
input that exercises the antisymmetric half.

Asserted here, from the reference's own numbers (tests/modes_ref.py holds the
formulas): |A|_F >= 0.1 |S|_F on M1; gap2_j >= 1e-4 for the first four modes
of every input and kind; every real (concat) mode among them passes the
sign-rule condition |mean U_j| >= 100 * 4 eta / gap2_j; no percentage of the
first four lies within the Sigma bar of a rounding boundary; and
tests/modes_ref.py reproduces every stored quantity within its bars.

Stored in ``G11_modes.npz`` (keys ``<input>_<kind>_...``; only data):
  M1_V (40, 2000) float32          the synthetic input (the others: G1-G3's V_k)
  G2_cap641_X                      process_V_k_to_complex of G2's V_k
  U (K, 4), Sigma (K,), VT (4, N) complex / (4, 2N)   after the sign flip
  pct, pct2 (K,)                   calculate_percentages(Sigma)
  G2_cap641_<kind>_vectors (4, N, 3)   extract_modes' velocity vectors
  ref_seconds                      the svd's seconds

Run:  python tests/golden/make_golden_modes.py <path of the reference>
"""
from __future__ import annotations

import ast
import importlib.util
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import modes_ref as R  # noqa: E402

SCRIPTS = {"complex": "S4_spatiotemporal_decomposition_ComplexMatrices .py",
           "concat": "S4_spatiotemporal_decomposition_ConcatMatrices .py"}
# what a statement of __main__ may call and still be run here: numpy, len and
# the script's own percentages -- file input and plotting call something else
CALLS_OK = ("np", "len", "calculate_percentages")


def load_reference(ref):
    sys.dont_write_bytecode = True
    for name in ("pyvista", "mne", "yaml", "matplotlib"):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    if not hasattr(sys.modules["matplotlib"], "pyplot"):
        try:
            import matplotlib.pyplot  # noqa: F401
        except ImportError:
            sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"] = types.ModuleType("matplotlib.pyplot")
    saved = {k: sys.modules.get(k) for k in ("utils", "utils.draw_optical_flow_field")}
    utils = types.ModuleType("utils")
    utils.draw_optical_flow_field = types.ModuleType("utils.draw_optical_flow_field")
    sys.modules["utils"], sys.modules["utils.draw_optical_flow_field"] = utils, utils.draw_optical_flow_field
    mods = {}
    for kind, fname in SCRIPTS.items():
        path = os.path.join(ref, fname)
        spec = importlib.util.spec_from_file_location("s4_" + kind, path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        with open(path, encoding="utf-8") as f:
            lines = f.read().splitlines()
        start = next(i for i, l in enumerate(lines) if "__main__" in l and l.startswith("if"))
        mod._main = main_assignments(lines[start + 1:])
        mods[kind] = mod
    for k, v in saved.items():
        if v is None:
            del sys.modules[k]
        else:
            sys.modules[k] = v
    return mods


def call_root(node):
    """The leftmost name of a call's function: np of np.linalg.svd(...)."""
    f = node.func
    while isinstance(f, ast.Attribute):
        f = f.value
    return f.id if isinstance(f, ast.Name) else None


def main_assignments(lines):
    """The one-line assignments of __main__ that call nothing outside
    CALLS_OK, parsed; the svd asked for thin factors. Which of them run is
    decided when they do: those whose inputs exist (run_reference)."""
    out, thin = [], 0
    for line in lines:
        try:
            tree = ast.parse(line.strip())
        except SyntaxError:  # a piece of a statement that spans lines
            continue
        if len(tree.body) != 1 or not isinstance(tree.body[0], ast.Assign):
            continue
        calls = [n for n in ast.walk(tree) if isinstance(n, ast.Call)]
        if any(call_root(c) not in CALLS_OK for c in calls):
            continue
        for c in calls:
            if isinstance(c.func, ast.Attribute) and c.func.attr == "svd":
                for kw in c.keywords:
                    if kw.arg == "full_matrices":
                        kw.value = ast.Constant(False)
                        thin += 1
        out.append(ast.fix_missing_locations(tree))
    assert thin == 1
    return out


def run_reference(mod, kind, V_k, e):
    """The script on one input: full Sigma, and U, VT, the percentages and the
    mode vectors of its first four modes. Starting from V_k_coord, every
    assignment of __main__ whose inputs exist by then is executed, in the
    script's order: the svd, the percentages, the cut and the sign flip run;
    what hangs on files or figures finds its inputs missing and is passed
    over."""
    rec, pcts = [], []
    mod.plot_surface_with_velocity_arrows = lambda path, velocity, *a, **k: rec.append(np.array(velocity))
    mod.surface_path = None

    def percentages(Sigma):
        pcts.append(mod.calculate_percentages(Sigma))
        return pcts[-1]

    ns = {"np": np, "len": len, "nmodeplot": 4, "calculate_percentages": percentages,
          "V_k_coord": mod.process_V_k_to_complex(V_k)}
    sigma_full, secs = None, None
    for tree in mod._main:
        loads = {n.id for n in ast.walk(tree) if isinstance(n, ast.Name) and isinstance(n.ctx, ast.Load)}
        if not loads <= set(ns):
            continue
        is_svd = any(isinstance(n, ast.Attribute) and n.attr == "svd" for n in ast.walk(tree))
        t0 = time.perf_counter()
        exec(compile(tree, "<__main__ of the script>", "exec"), ns)
        if is_svd:
            secs = time.perf_counter() - t0
            sigma_full = ns["Sigma"].copy()
    assert len(pcts) == 1 and sigma_full is not None
    U, Sigma, VT = ns["U"], ns["Sigma"], ns["VT"]
    assert np.array_equal(Sigma, sigma_full[:4]) and U.shape[1] == len(Sigma)  # min(4, K) modes: G3 has K = 3
    assert (np.mean(np.real(U), axis=0) >= 0).all()  # the sign flip ran
    if e is not None:
        if kind == "complex":
            mod.extract_modes(Sigma, VT, e, len(Sigma))
        else:
            # the script hands extract_modes the halves of VT as one complex array, which it has built by then
            N = VT.shape[1] // 2
            final = [v for v in ns.values() if isinstance(v, np.ndarray) and np.iscomplexobj(v)
                     and v.shape == (len(Sigma), N) and np.array_equal(v.real, VT[:, :N])
                     and np.array_equal(v.imag, VT[:, N:])]
            assert final
            mod.extract_modes(Sigma, final[0], e, len(Sigma), pcts[0][1])
    return {"X": ns["V_k_coord"], "U": U, "Sigma": sigma_full, "VT": VT, "pct": pcts[0][0], "pct2": pcts[0][1],
            "vectors": np.array(rec) if rec else None, "secs": secs}


def m1_fields():
    rng = np.random.default_rng(0)
    K, N = 40, 1000
    a, _ = np.linalg.qr(rng.standard_normal((K, K)) + 1j * rng.standard_normal((K, K)))
    b, _ = np.linalg.qr(rng.standard_normal((N, K)) + 1j * rng.standard_normal((N, K)))
    X = (a * 0.8 ** np.arange(K)) @ b.conj().T
    return np.concatenate([X.real, X.imag], axis=1).astype(np.float32)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    mods = load_reference(sys.argv[1])
    out = {"M1_V": m1_fields()}
    inputs = []
    for name in ("G1_ico642", "G2_cap641", "G3_ico642_f32"):
        with np.load(os.path.join(HERE, name + ".npz"), allow_pickle=False) as z:
            inputs.append((name, z["V_k"], z["e"]))
    inputs.append(("M1", out["M1_V"].astype(np.float64), None))
    for name, V, e in inputs:
        K, N = V.shape[0], V.shape[1] // 2
        eta = R.eta(K, N)
        for kind, mod in mods.items():
            ref = run_reference(mod, kind, V, e)
            pre = "%s_%s_" % (name, kind)
            assert np.array_equal(ref["X"], R.complex_Y(V))
            if name == "G2_cap641":
                out["G2_cap641_X"] = ref["X"]
                out[pre + "vectors"] = ref["vectors"]
            Sg = ref["Sigma"]
            g2 = R.gap2(Sg)
            assert (g2[:4] >= 1e-4).all(), (pre, g2[:4])
            bars = eta * Sg[0] ** 2 / Sg
            r = min(4, K)
            clear = R.percent_boundary_clear(Sg, bars, r)
            assert clear.all(), (pre, clear)
            if kind == "concat":
                cond = np.abs(ref["U"].mean(axis=0)) / (100 * 4 * eta / g2[:4])
                assert (cond >= 1).all(), (pre, cond)
                print(pre, "sign rule: |mean U_j| over 100 bars:", cond)
            S, A = R.gram(V, kind)
            if name == "M1" and kind == "complex":
                print("M1 |A|_F / |S|_F = %.3g" % (np.linalg.norm(A) / np.linalg.norm(S)))
                assert np.linalg.norm(A) >= 0.1 * np.linalg.norm(S)
            # the restatement against the reference, within the bars
            m = R.modes(V, r, kind)
            dS = np.abs(m["Sigma"] - Sg)
            assert (dS <= bars).all(), (pre, (dS / bars).max())
            bar_v = 4 * eta * Sg[0] / g2[:4]
            d_sr = np.abs(m["sigma_r"] - Sg[:4])
            r1 = R.rank_one_errors(kind, m["U"], m["Y"], ref["U"], Sg, ref["VT"])
            assert (d_sr <= bar_v).all() and (r1 <= bar_v).all(), (pre, d_sr / bar_v, r1 / bar_v)
            print(pre, "K %d N %d sigma %s gap2 %s" % (K, N, Sg[:5], g2[:5]))
            print(pre, "restatement: Sigma err / bar %.3g, sigma_r rel %.3g, rank-one / sigma_1 %.3g (bar %.3g)"
                  % ((dS / bars).max(), (d_sr / Sg[:4]).max(), (r1 / Sg[0]).max(), (bar_v / Sg[0]).max()))
            out[pre + "U"] = ref["U"]
            out[pre + "Sigma"] = Sg
            out[pre + "VT"] = ref["VT"]
            out[pre + "pct"] = ref["pct"]
            out[pre + "pct2"] = ref["pct2"]
            out[pre + "ref_seconds"] = np.array(ref["secs"])
    path = os.path.join(HERE, "G11_modes.npz")
    np.savez_compressed(path, **out)
    print("G11_modes", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
