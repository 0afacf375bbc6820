"""The fp64 checker of the multigrid setup (tests/amg_ref.py) checked itself,
on the CPU: the storage formats against hand-packed words and their encoders,
and the term-by-term evaluation of Galerkin gather lists against P^T A P on a
small random block matrix with a random aggregation, laid out as the library
lays its levels out (SELL-64, diagonal first, upper blocks with terms and
lower twins without; level 0 read through a mirror table)."""
import numpy as np
import pytest

import amg_ref as R


# ---- formats ---------------------------------------------------------------------

def test_bf16_rounds_to_nearest_even():
    x = np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0xBF808000, 0x00000000, 0x80000000],
                 dtype=np.uint32).view(np.float32)
    assert list(R.bf16_bits(x)) == [0x3F80, 0x3F82, 0x3F80, 0x3F81, 0xBF80, 0x0000, 0x8000]
    rng = np.random.default_rng(0)
    y = (rng.standard_normal(4096) * 10.0 ** rng.integers(-6, 6, 4096)).astype(np.float32)
    back = R.bf16_value(R.bf16_bits(y)).astype(np.float64)
    assert (np.abs(back - y) <= 0.5 * R.bf16_ulp(y)).all()
    assert np.array_equal(R.bf16_bits(back.astype(np.float32)), R.bf16_bits(y))


def _blocks(rng, n, bs):
    """Random blocks, one of zeros and one whose largest entry is negative."""
    b = (rng.standard_normal((n, bs, bs)) * 10.0 ** rng.integers(-3, 3, (n, 1, 1))).astype(np.float32)
    b[1] = 0.0
    b[2] = -np.abs(b[2])
    b[2, 0, 0] = -2.0 * np.abs(b[2]).max()
    return b


def test_h0_layout_and_round_trip():
    w = R.h0_enc(np.array([[[1.0, -2.0], [0.5, 3.0]]], dtype=np.float32))
    assert w.dtype == np.uint64 and int(w[0]) == (0x3F80 | 0xC000 << 16) | (0x3F00 | 0x4040 << 16) << 32
    assert np.array_equal(R.h0_dec(w), [[[1.0, -2.0], [0.5, 3.0]]])
    rng = np.random.default_rng(1)
    b = _blocks(rng, 64, 2)
    d = R.h0_dec(R.h0_enc(b))
    assert (np.abs(d - b) <= 0.5 * R.bf16_ulp(b)).all() and (d[1] == 0).all() and d[2, 0, 0] < 0
    assert np.array_equal(R.h0_enc(d.astype(np.float32)), R.h0_enc(b))  # decoded values are fixed points
    # the same bytes seen as word pairs
    assert np.array_equal(R.h0_dec(R.h0_enc(b).view(np.uint32).reshape(-1, 2)), d)


def test_h9_layout_and_round_trip():
    one = np.arange(1.0, 10.0, dtype=np.float32).reshape(1, 3, 3)
    Dh, Dh22 = R.h9_enc(one)
    bits = [int(v) for v in R.bf16_bits(one.ravel())]
    assert Dh.shape == (1, 4) and [int(v) for v in Dh[0]] == [bits[2 * k] | bits[2 * k + 1] << 16 for k in range(4)]
    assert int(Dh22[0]) == bits[8]
    assert np.array_equal(R.h9_dec(Dh, Dh22), one)
    rng = np.random.default_rng(2)
    b = _blocks(rng, 64, 3)
    Dh, Dh22 = R.h9_enc(b)
    d = R.h9_dec(Dh, Dh22)
    assert (np.abs(d - b) <= 0.5 * R.bf16_ulp(b)).all() and (d[1] == 0).all() and d[2, 0, 0] < 0
    again = R.h9_enc(d.astype(np.float32))
    assert np.array_equal(again[0], Dh) and np.array_equal(again[1], Dh22)


def test_a9_layout_and_round_trip():
    k = np.array([[-127, 1, 2], [3, -4, 5], [6, 7, -8]])
    Ah, Ah22 = R.a9_enc((0.5 * k).astype(np.float32)[None])  # max |a| / 127 = 0.5 exactly
    assert [int(v) for v in Ah[0]] == [1 | 129 << 8 | 130 << 16 | 131 << 24, 124 | 133 << 8 | 134 << 16 | 135 << 24]
    assert [int(v) for v in Ah22[0]] == [120, 0x3F00]
    codes, scale = R.a9_dec(Ah, Ah22)
    assert np.array_equal(codes[0] - 128, k) and scale[0] == 0.5
    rng = np.random.default_rng(3)
    b = _blocks(rng, 64, 3)
    Ah, Ah22 = R.a9_enc(b)
    codes, scale = R.a9_dec(Ah, Ah22)
    assert scale[1] == 0 and (codes[1] == 128).all()  # the block of zeros
    assert codes[2, 0, 0] == 1 and (codes[2] <= 128).all()  # its largest entry is negative: -127
    assert codes.min() >= 1 and codes.max() <= 255
    m = np.abs(b).reshape(-1, 9).max(axis=1)
    assert np.array_equal(R.bf16_bits(scale), R.bf16_bits(m / np.float32(127.0)))
    # bf16(m / 127) >= m / 127.5, so no entry is clamped by more than the rounding: half a step
    val = (codes - 128) * scale.astype(np.float64)[:, None, None]
    assert (np.abs(val - b) <= 0.5 * scale[:, None, None] * (1 + 1e-6)).all()
    again = R.a9_enc(val.astype(np.float32))
    assert np.array_equal(again[0], Ah)
    # a transposed block: the same scale, the transposed codes
    ct, st = R.a9_dec(*R.a9_enc(b.transpose(0, 2, 1)))
    assert np.array_equal(st, scale) and np.array_equal(ct, codes.transpose(0, 2, 1))


# ---- a small hierarchy laid out as the library's -----------------------------------

def sell_layout(adj, n):
    """SELL-64 tables of an adjacency (lists of sorted columns, self included):
    slot 0 the diagonal, then the other columns ascending; padding names the
    row itself."""
    ns = (n + 63) // 64
    off = np.zeros(ns + 1, dtype=np.int32)
    for s in range(ns):
        off[s + 1] = off[s] + 64 * max(len(adj[i]) for i in range(64 * s, min(n, 64 * s + 64)))
    nb = int(off[-1])
    col, row = np.zeros(nb, dtype=np.int32), np.zeros(nb, dtype=np.int32)
    diag = np.zeros(n, dtype=np.int32)
    where = {}
    for s in range(ns):
        w = (off[s + 1] - off[s]) // 64
        for l in range(64):
            i = 64 * s + l
            cols = [i] + [j for j in adj[i] if j != i] if i < n else []
            for t in range(w):
                pos = int(off[s]) + 64 * t + l
                row[pos] = i
                col[pos] = cols[t] if t < len(cols) else min(i, n - 1) if i >= n else i
                if t < len(cols):
                    where[(i, cols[t])] = pos
            if i < n:
                diag[i] = int(off[s]) + l
    return {"n": n, "sell_nb": nb, "sell_off": off, "sell_col": col, "sell_row": row, "diag_pos": diag}, where


def build_pair(bs, seed):
    """A fine level (bs = 2: read through a mirror table, its lower blocks
    never written) with a random block-SPD matrix, a random aggregation with
    one dead coarse dof, and the coarse level with hand-built gather lists."""
    rng = np.random.default_rng(seed)
    n, nc = 150, 37
    adj = [{i} for i in range(n)]
    for i, j in rng.integers(0, n, (4 * n, 2)):
        adj[i].add(int(j))
        adj[j].add(int(i))
    adj = [sorted(a) for a in adj]
    F, fpos = sell_layout(adj, n)
    F["bs"] = bs
    # block-SPD: a symmetric random part plus a dominant diagonal
    dense = np.zeros((bs * n, bs * n))
    for (i, j) in fpos:
        if j >= i:
            b = rng.standard_normal((bs, bs))
            dense[bs * i:bs * i + bs, bs * j:bs * j + bs] = b
            dense[bs * j:bs * j + bs, bs * i:bs * i + bs] = b.T
    dense = 0.5 * (dense + dense.T) + 4.0 * max(len(a) for a in adj) * np.eye(bs * n)
    blocks = np.full((F["sell_nb"], bs, bs), np.nan)
    mirror = np.full(F["sell_nb"], -1, dtype=np.int32)
    for (i, j), pos in fpos.items():
        if bs == 2 and j < i:  # symmetric reads: the transposed upper twin, this block stays unwritten
            mirror[pos] = fpos[(j, i)] | R.MIR_T
        else:
            mirror[pos] = pos
            blocks[pos] = dense[bs * i:bs * i + bs, bs * j:bs * j + bs]
    blocks[mirror < 0] = 0.0  # padding
    F["mirror"] = mirror if bs == 2 else np.zeros(0, dtype=np.int32)
    agg = np.concatenate([np.arange(nc), rng.integers(0, nc, n - nc)]).astype(np.int32)
    rng.shuffle(agg)
    Q = rng.standard_normal((n, bs, 3)).astype(np.float32)
    dead = np.zeros((nc, 3), dtype=np.uint8)
    dead[5, 2] = 1
    Q[agg == 5, :, 2] = 0.0
    F.update(agg=agg, pptr=np.arange(n + 1, dtype=np.int32), pcol=agg.copy(), Q=Q, smoothed=False)
    cadj = [set() for _ in range(nc)]
    for (i, j) in fpos:
        cadj[agg[i]].add(int(agg[j]))
    C, cpos = sell_layout([sorted(a) for a in cadj], nc)
    C.update(bs=3, dead=dead, mirror=np.zeros(0, dtype=np.int32))
    terms = {}
    for (i, j), pos in sorted(fpos.items()):
        if agg[j] >= agg[i]:
            terms.setdefault(cpos[(int(agg[i]), int(agg[j]))], []).append((int(mirror[pos]) if bs == 2 else pos, i, j))
    gptr, gent = [0], []
    twin = np.full(C["sell_nb"], -1, dtype=np.int32)
    for pos in range(C["sell_nb"]):
        gent += terms.get(pos, [])
        gptr.append(len(gent))
    for (I, J), pos in cpos.items():
        if J > I:
            twin[pos] = cpos[(J, I)]
    C["twin"] = twin
    F.update(gptr=np.array(gptr, dtype=np.int32), gent=np.array(gent, dtype=np.int32).reshape(-1, 3))
    return F, C, blocks, dense


@pytest.mark.parametrize("bs", [2, 3])
def test_gather_lists_equal_the_triple_product(bs):
    F, C, blocks, dense = build_pair(bs, seed=10 + bs)
    A = R.sell_to_csr(F, blocks)
    assert np.array_equal(A.toarray(), dense)  # the mirror table's transposes, no unwritten block read
    P = R.prolongator(F, C["n"])
    ref = R.galerkin_ref(P, A, C["dead"])
    full = P.toarray().T @ dense @ P.toarray() + np.diag(C["dead"].ravel().astype(np.float64))
    assert np.abs(ref.toarray() - full).max() <= 1e-13 * np.abs(full).max()
    Cl, S, K = R.galerkin_lists(F, blocks)
    upper = np.flatnonzero(np.diff(F["gptr"]) > 0)
    stored = R.stored_positions(C)
    I, J = C["sell_row"][upper], C["sell_col"][upper]
    assert stored[upper].all() and (J >= I).all() and len(upper) + (C["twin"] >= 0).sum() == stored.sum()
    want = R.csr_blocks(ref, I, J)
    dg = upper == C["diag_pos"][I]
    got = Cl[upper] + dg[:, None, None] * np.eye(3)[None] * C["dead"][I][:, :, None]
    assert (K[upper] == np.diff(F["gptr"])[upper] * bs * bs).all()
    assert (np.abs(got - want) <= 1e-13 * (S[upper] + 1.0 * dg[:, None, None])).all()
    assert got[C["diag_pos"][5] == upper][0][2, 2] == 1.0  # the dead dof: a unit diagonal, nothing else
    # the bound bites: without one mid-list term the same comparison fails, at that position only
    p, g = R.mid_list_term(F, blocks)
    Cd, _, _ = R.galerkin_lists(F, blocks, drop=g)
    bad = np.abs(Cd[upper] - Cl[upper]) > 1e-13 * S[upper]
    assert bad.any() and list(np.flatnonzero(bad.any(axis=(1, 2)))) == [int(np.flatnonzero(upper == p)[0])]


def test_sweep_inverse():
    rng = np.random.default_rng(7)
    B = rng.standard_normal((33, 33))
    M = B @ B.T + 33 * np.eye(33)
    X = np.linalg.inv(M)
    assert np.abs(R.sweep_inverse(M) - X).max() <= 1e-13 * np.abs(X).max()
    # row k stands in for column k: an asymmetry of the input is not inverted, it is an error
    E = np.triu(rng.standard_normal((33, 33)), 1) * 1e-6
    off = np.abs(R.sweep_inverse(M + E) - np.linalg.inv(M + E)).max()
    assert 1e-10 * np.abs(X).max() < off < 1e-4 * np.abs(X).max()


def test_csr_blocks_outside_the_pattern_are_zero():
    F, C, blocks, _ = build_pair(3, seed=4)
    A = R.sell_to_csr(F, blocks)
    i = 0
    j = next(k for k in range(F["n"]) if A[3 * i, 3 * k] == 0 and A[3 * i + 1, 3 * k + 2] == 0)
    b = R.csr_blocks(A, [i, i], [i, j])
    assert np.array_equal(b[0], A[0:3, 0:3].toarray()) and (b[1] == 0).all()
