"""The size function that decides, per mesh, whether the fp64 residual runs
with a row slice's geometry staged in LDS (k_residual_lds) or as the row
kernel (csrc/mof_pattern.cpp staged_bytes, kStagedRes), on the CPU through the
host-only mof_residual_probe: a 64-row slice of w a2 slots and t incidence
slots stages 64 (36 w + 192 t + 48) bytes, and the mesh takes the staged
kernel when its widest slice fits the kernel's fixed 160 KiB. That the
decision a handle takes is the probe's, whatever the batch, needs a handle:
tests/test_gpu_residual_lds.py counts the launches of each kernel."""
import numpy as np

from mofhip import synth
from mofhip.mesh import residual_probe

CAP = 160 * 1024


def slice_bytes(w_a2, w_inc):
    return 64 * (36 * w_a2 + 192 * w_inc + 48)


def fan(valence):
    """A closed fan: a hub of the given valence and its rim (one slice)."""
    tri = [(0, 1 + k, 1 + (k + 1) % valence) for k in range(valence)]
    return np.array(tri, dtype=np.int32), valence + 1


def test_regular_slice_of_seven_slots_and_six_incidences():
    assert slice_bytes(7, 6) == 92928
    p, t = synth.icosphere(8)  # valence 5 and 6 only: 7 a2 slots, 6 incidence slots
    pr = residual_probe(t, len(p))
    assert pr == {"staged_bytes": 92928, "staged_used": True}
    # the widest slice is the same in either vertex order
    assert residual_probe(t, len(p), reorder=False) == pr


def test_widest_slice_against_the_cap():
    # hub of valence v: v + 1 a2 slots, v incidence slots
    t, n = fan(10)
    assert slice_bytes(11, 10) == 151296 <= CAP
    assert residual_probe(t, n) == {"staged_bytes": 151296, "staged_used": True}
    t, n = fan(11)
    assert slice_bytes(12, 11) == 165888 > CAP
    assert residual_probe(t, n) == {"staged_bytes": 165888, "staged_used": False}


def test_one_wide_slice_refuses_the_mesh():
    """An icosphere (every slice fits) and a valence-12 hub beside it: the
    widest slice decides, so the whole mesh keeps the row kernel."""
    p, t = synth.icosphere(4)
    assert residual_probe(t, len(p))["staged_used"]
    f, nf = fan(12)
    t2 = np.concatenate([np.asarray(t, dtype=np.int32), f + len(p)])
    pr = residual_probe(t2, len(p) + nf)
    assert pr["staged_bytes"] >= slice_bytes(13, 12) > CAP
    assert not pr["staged_used"]
