"""bench.py's plain / --full split and --dump-outputs.

A plain run (the driver's ``--gpus 1 --steps K --warmup W``) runs none of the
extras; ``--full`` restores their defaults. ``--dump-outputs DIR`` writes the
V of the last timed step: all of it when small, else rows drawn by a fixed
seed. On the GPU the dumped V of the C1 job (642 vertices, 15 timesteps) is
checked against the oracle's A_k, f_k and spsolve at the project's bar."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parse(monkeypatch, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_has_no_extras(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "3", "--warmup", "1", "--legs", "F3", "--host-batches", "2")
    assert a.steps == 3 and a.warmup == 1 and not a.full and a.dump_outputs is None
    assert a.no_cpu_baseline and a.parity_samples == 0 and a.legs == "none" and a.host_batches == 0


def test_full_keeps_the_extras_and_their_options(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert a.full and not a.no_cpu_baseline and a.parity_samples == 2 and a.legs == "auto" and a.host_batches == 4
    a = _parse(monkeypatch, "--full", "--no-cpu-baseline", "--legs", "F3", "--host-batches", "0")
    assert a.no_cpu_baseline and a.legs == "F3" and a.host_batches == 0 and a.parity_samples == 2


def test_dump_outputs_whole_and_seeded_sample(tmp_path, monkeypatch):
    import bench
    V = np.arange(40 * 6, dtype=np.float64).reshape(40, 6)
    info = bench.dump_outputs(str(tmp_path / "a"), 0, 1, V, 100, None)
    assert info["rows"] == "all" and info["V.npy"] == [40, 6]
    got = np.load(tmp_path / "a" / "V.npy")
    assert got.dtype == np.float64 and np.array_equal(got, V)
    assert np.array_equal(np.load(tmp_path / "a" / "V_timesteps.npy"), 100.0 + np.arange(40))
    # a budget of 10 rows: the same 10 distinct rows every time, in order
    monkeypatch.setattr(bench, "DUMP_BYTES", 10 * 6 * 8)
    picks = []
    for d in ("b", "c"):
        info = bench.dump_outputs(str(tmp_path / d), 0, 1, V, 100, None)
        assert info["rows"] == "seeded sample" and info["V.npy"] == [10, 6] and info["rows_of_last_step"] == 40
        ts = np.load(tmp_path / d / "V_timesteps.npy")
        assert np.array_equal(np.load(tmp_path / d / "V.npy"), V[(ts - 100).astype(int)])
        picks.append(ts)
    assert np.array_equal(picks[0], picks[1]) and np.all(np.diff(picks[0]) > 0)
    # two ranks share the budget and write their own files
    info = bench.dump_outputs(str(tmp_path / "d"), 1, 2, V, 0, None)
    assert info["V_rank1.npy"] == [5, 6] and os.path.exists(tmp_path / "d" / "V_timesteps_rank1.npy")


@pytest.mark.gpu
def test_plain_bench_dumps_the_last_step(tmp_path):
    import oracle
    from mofhip import synth
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--config", "C1",
                          "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path)],
                         capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["config"]["timesteps_timed"] == 2 * 15 and line["ms_per_step"] > 0
    assert line["unit"] == "timesteps/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    # one step = the 15-timestep job; ms_per_step is rounded to 1 us of a ~0.5 ms step
    assert abs(line["value"] - 15e3 / line["ms_per_step"]) <= 1e-2 * line["value"]
    assert line["parity"] is None and line["host_io"] is None and line["legs"] is None
    assert line["cpu_baseline"] is None and "defect" not in line
    assert line["dump_outputs"]["V.npy"] == [15, 2 * 642] and line["dump_outputs"]["rows"] == "all"
    V = np.load(tmp_path / "V.npy")
    assert V.dtype == np.float64 and V.shape == (15, 2 * 642) and np.isfinite(V).all()
    assert np.array_equal(np.load(tmp_path / "V_timesteps.npy"), np.arange(15.0))
    p, t, n, a = synth.mesh_for_config("C1")
    I = synth.config_wave("C1", p, 16)
    a2, gw, e, iw = oracle.geometry(p, n, t, a)
    tk = list(range(16))
    for k in (0, 7, 14):
        Vo = oracle.worker(k, a2, gw, e, iw, t, tk, a, 0.01, I[k], I[k + 1])
        err = float(np.abs(V[k] - Vo).max())
        assert err < 1e-6 * max(1.0, float(np.abs(Vo).max())), (k, err)
