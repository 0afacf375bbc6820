"""The size function that decides, per mesh, whether the mixed-precision row
assembly runs with a row slice's geometry staged in LDS (k_assemble_lds) or as
the row kernel (csrc/mof_pattern.cpp staged_bytes, kStagedAsm), on the CPU through the
host-only mof_assembly_probe: a 64-row slice of t incidence slots and w a2
slots stages 64 (112 t + 48 w + 48) bytes, and the mesh takes the staged
kernel when no row is wider than the kernel's 8 register slots and its widest
slice fits the kernel's fixed 160 KiB. That a handle's launches follow the
probe, whatever the batch, needs a handle: tests/test_gpu_assembly_lds.py
counts the launches of each kernel."""
import itertools

import numpy as np

from mofhip import synth
from mofhip.mesh import assembly_probe

CAP = 160 * 1024


def slice_bytes(w_inc, w_a2):
    # per row: 7 planes of 16 B per incidence (tinc | 4 x two hat gradients | g8, A_T | w12, tslot),
    # 3 per a2 slot (flags + e_j as floats, 2 planes | the fp32 lambda a2 block), 3 for e_i
    return 64 * 16 * (7 * w_inc + 3 * w_a2 + 3)


def fan(valence):
    """A closed fan: a hub of the given valence and its rim (one slice)."""
    tri = [(0, 1 + k, 1 + (k + 1) % valence) for k in range(valence)]
    return np.array(tri, dtype=np.int32), valence + 1


def widest(tri, n):
    """(incidence slots, a2 slots) of the widest row, restated with numpy: a
    one-slice mesh's slice is as wide as its widest row in either."""
    tri = np.asarray(tri)
    inc = np.bincount(tri.ravel(), minlength=n).max()
    nb = [set() for _ in range(n)]
    for a, b, c in tri.tolist():
        for u in (a, b, c):
            nb[u].update((a, b, c))
    return int(inc), max(len(s) for s in nb)


def test_regular_slice_of_seven_slots_and_six_incidences():
    assert slice_bytes(6, 7) == 64 * (6 * 112 + 7 * 48 + 48) == 67584
    p, t = synth.icosphere(8)  # valence 5 and 6 only: 6 incidence slots, 7 a2 slots
    pr = assembly_probe(t, len(p))
    assert pr == {"staged_bytes": 67584, "staged_used": True}
    # the widest slice is the same in either vertex order
    assert assembly_probe(t, len(p), reorder=False) == pr


def test_row_width_against_the_register_slots():
    # hub of valence v: v incidence slots, v + 1 a2 slots
    t, n = fan(7)
    assert widest(t, n) == (7, 8)
    assert assembly_probe(t, n) == {"staged_bytes": slice_bytes(7, 8), "staged_used": True}
    t, n = fan(8)  # max_w = 9: the bytes would fit, the row does not
    assert widest(t, n) == (8, 9) and slice_bytes(8, 9) <= CAP
    assert assembly_probe(t, n) == {"staged_bytes": slice_bytes(8, 9), "staged_used": False}


def test_slice_past_the_cap_by_bytes():
    """Every triangle over 8 vertices: rows of 8 blocks (they fit the register
    slots) with 21 incidences each, 178,176 B -- refused by the bytes alone.
    With every triangle over 7 vertices (15 incidences, 7 blocks) it fits."""
    t = np.array(list(itertools.combinations(range(8), 3)), dtype=np.int32)
    assert widest(t, 8) == (21, 8) and slice_bytes(21, 8) == 178176 > CAP
    assert assembly_probe(t, 8) == {"staged_bytes": 178176, "staged_used": False}
    t = np.array(list(itertools.combinations(range(7), 3)), dtype=np.int32)
    assert widest(t, 7) == (15, 7) and slice_bytes(15, 7) <= CAP
    assert assembly_probe(t, 7) == {"staged_bytes": slice_bytes(15, 7), "staged_used": True}


def test_one_wide_slice_refuses_the_mesh():
    """An icosphere (every slice fits) and a valence-8 hub beside it: the
    widest row decides, so the whole mesh keeps the row kernel."""
    p, t = synth.icosphere(4)
    assert assembly_probe(t, len(p))["staged_used"]
    f, nf = fan(8)
    t2 = np.concatenate([np.asarray(t, dtype=np.int32), f + len(p)])
    pr = assembly_probe(t2, len(p) + nf)
    assert pr["staged_bytes"] >= slice_bytes(6, 7)
    assert not pr["staged_used"]
