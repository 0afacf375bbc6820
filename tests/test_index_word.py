"""The packed index words of the level-0 row products (csrc/mof_pattern.cpp
sell_index_pack) on the CPU, through the host-only mof_index_probe: decoding a
word gives exactly the column, position, transpose flag and padding flag of
the two 32-bit tables it replaces; a mesh whose deltas do not fit 16 bits
keeps the two tables."""
import numpy as np
import pytest

from mofhip import synth
from mofhip.mesh import index_probe

MIR_T = 1 << 30
PAD = -32768


def decode(pr):
    """(column, position, transposed, padding) of every SELL position from the
    packed words alone (plus sell_off for the position's row), as the kernels
    decode them."""
    off, w = pr["sell_off"], pr["packed"]
    pos = np.arange(len(w), dtype=np.int64)
    sl = np.searchsorted(off, pos, side="right") - 1
    lane = (pos - off[sl]) % 64
    row = sl * 64 + lane
    dcol = (w & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int64)
    dpos = (w >> 16).astype(np.uint16).view(np.int16).astype(np.int64)
    pad = dpos == PAD
    diag = off[sl].astype(np.int64) + lane  # slot 0 of the row: what padding reads
    return row + dcol, np.where(pad, diag, pos + dpos), (dpos != 0) & ~pad, pad, row


def check_tables(pr, N):
    assert pr["sym_used"] and pr["packed_used"]
    col, rd, tr, pad, row = decode(pr)
    mir = pr["mir"].astype(np.int64)
    assert np.array_equal(pad, mir < 0)
    live = ~pad
    assert np.array_equal(col[live], pr["col"][live])
    assert np.array_equal(rd[live], (mir & (MIR_T - 1))[live])
    assert np.array_equal(tr[live], ((mir & MIR_T) != 0)[live])
    # padding: the row's own column (masked) where the row exists
    ex = pad & (row < N)
    assert np.array_equal(col[ex], row[ex]) and np.array_equal(pr["col"][ex], row[ex])
    # symmetric reads really transpose something, and every read stays in the table
    assert tr.any() and rd.min() >= 0 and rd.max() < len(mir)
    return int(np.diff(pr["sell_off"]).max() // 64)


@pytest.mark.parametrize("mesh", ["ico642", "cap641"])
def test_packed_words_decode_to_the_tables(mesh):
    p, t = synth.icosphere(8) if mesh == "ico642" else synth.spherical_cap(16)
    assert len(p) == (642 if mesh == "ico642" else 641)
    check_tables(index_probe(t, len(p)), len(p))


def test_packed_words_wide_rows_forced_symmetric():
    """An irregular hull (plain reads by itself) with symmetric reads forced:
    rows wider than the 8 slots of one load chunk."""
    p, t = synth.random_sphere(1500, 10.0, seed=0)
    assert not index_probe(t, len(p))["sym_used"]
    assert check_tables(index_probe(t, len(p), sym=1), len(p)) > 8


def test_plain_reads_take_no_packed_words():
    p, t = synth.icosphere(8)
    pr = index_probe(t, len(p), sym=0)
    assert not pr["sym_used"] and not pr["packed_used"] and not pr["packed"].any()


def test_delta_overflow_keeps_the_32_bit_tables():
    """A randomly relabelled 16,002-vertex icosphere kept in the caller's
    order: columns up to ~16,000 rows and twins ~110,000 positions away."""
    p, t, _ = synth.permute_vertices(*synth.icosphere(40), seed=0)
    pr = index_probe(t, len(p), sym=1, reorder=False)
    pos = np.arange(len(pr["mir"]))
    live = pr["mir"] >= 0
    far = np.abs((pr["mir"] & (MIR_T - 1)) - pos)[live].max()
    assert far > 32767  # it really overflows
    assert pr["sym_used"] and not pr["packed_used"] and not pr["packed"].any()
    # the same mesh in the library's own (RCM) order fits
    check_tables(index_probe(t, len(p), sym=1), len(p))


def test_c3_takes_the_packed_path():
    p, t, _, _ = synth.mesh_for_config("C3")
    assert len(p) == 163842
    assert check_tables(index_probe(t, len(p)), len(p)) <= 8
