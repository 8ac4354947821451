"""The embedding-geometry kernels on the device (csrc/geometry.hip) against the float64 model of tests/geometry_model.py, and what
is built on them: ops.uniformity_sum / row_gram, EliMRec.geometry_device / embedding_geometry / alignment,
evaluator.GeometryReport, --geometry_report, torch.ops.elimrec.uniformity_sum / row_gram.

Tolerances are derived, not measured.
Uniformity: |log(S / pairs) - model| <= 2 t (d + 4) 2^-23 + 4 * 2^-23: the worst-case fp32 error of a cosine of unit rows times
the slope 2 t of the exponent, plus 2 ulp each for expf and for the fp32 rounding of its argument; every term's relative error is
within that, so the mean's is; the float64 sum adds nothing visible.
Gram: the products of the fp32 unit rows are exact in float64, so only the order of n additions differs from the model's:
|dG_ab| <= n 2^-52 sum |x^_a x^_b|, likewise for m.
Alignment: twice the cosine's error, (d + 4) 2^-22.

The cell grid of uniformity_sum (tiles of TILE = 64 query positions x chunks of CHUNK = 2048 candidate positions, only the live
cells launched, decoded from blockIdx.x through 32 (g nc - g (g - 1) / 2)) is trivial up to two chunks. The smallest list at which
its arithmetic shows, with today's constants:
  g (g - 1) / 2 is not 0              n = 2 CHUNK + 1 = 4097   (a tile in chunk-row g = 2)
  more than one live chunk at g >= 1  n = 2 CHUNK + 1 = 4097   (nc = 3: chunk-row 1 meets the chunks 1 and 2)
  a reduce thread adds a second cell  n = 3 CHUNK + 1 = 6145   (289 cells; 192 at n = 3 CHUNK)
All three hold from n = 6145 on, but there chunk-row g = 3 is a single tile of a single position, which holds no pair, so nothing
it computes can be seen. The multi-chunk tests use n = 3 CHUNK + TILE + 1 = 6209: nc = 4, 98 tiles, 290 live cells, and chunk-row 3
holds a full tile (a pair to see) and a second tile (within / live is not 0 there). At that n the per-cell probes run the general
form (d = 4) and the register forms d = 64 (SR = 64) and d = 128 (SR = 32); the dense lists run d = 32 (SR = 64), d = 68 (general,
SR = 16) and d = 128. d = 256 stays at one chunk.
Not reachable: the last cell (tile 97, chunk 3) is launched and has its float64 in the workspace, but its tile is the one position
n - 1 with nothing behind it -- it can only be required to add 0 (gm.live_cells lists it, brute force over the pairs does not:
tests/test_geometry_cpu.py). pairs is n_valid (n_valid - 1) / 2 and not a count of the terms added, so a term taken with q <= p
cannot show in the counts; it shows as 2 S with one pair in the list.
Gram: the (bi <= bj) decode of blockIdx.y runs nb = 1, 2, 4 in test_gram_sizes and nb = 3 (d = 132: a last block of 4 columns;
d = 192: full blocks) over 2 and 3 segments in test_gram_three_column_blocks."""
import functools
import time

import numpy as np
import pytest
import torch

import geometry_model as gm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _consts():
    from elimrec_amd import ops
    return ops.GEOMETRY_TILE, ops.GEOMETRY_CHUNK, ops.GEOMETRY_SEGMENT


def _rows(n_rows, d, seed, zero=()):
    rng = np.random.default_rng(seed)
    T = rng.standard_normal((n_rows, d)).astype(np.float32) * rng.uniform(0.5, 3.0, (n_rows, 1)).astype(np.float32)
    T[list(zero)] = 0.0
    return T


def _tol(t, d):
    return 2.0 * t * (d + 4) * 2.0 ** -23 + 4 * 2.0 ** -23


def _uni(T, sq, rows, t=2.0, table=None, norms=None):
    from elimrec_amd import ops
    S, pairs, n_valid = ops.uniformity_sum(_t(T) if table is None else table, _t(sq) if norms is None else norms,
                                           _t(np.asarray(rows, dtype=np.int32)), t)
    return S, pairs, n_valid, ops.uniformity_value(S, pairs)


def _check_uni(T, sq, rows, t=2.0, **kw):
    S, pairs, n_valid, uni = _uni(T, sq, rows, t, **kw)
    wS, wpairs, wn, wuni = gm.uniformity_model(T, sq, rows, t)
    print("uniformity n=%d d=%d t=%g: got %.12g want %.12g diff %.3g tol %.3g" % (len(rows), T.shape[1], t, uni, wuni, abs(uni - wuni),
                                                                                _tol(t, T.shape[1])))
    assert (pairs, n_valid) == (wpairs, wn)
    if wn < 2:
        assert S == 0.0 and np.isnan(uni)
    else:
        assert abs(uni - wuni) <= _tol(t, T.shape[1])
    return S, pairs, n_valid, uni


# --------------------------------------------------------------------------- uniformity
@pytest.mark.parametrize("d", [4, 32, 64, 68, 128, 256])
def test_uniformity_sizes(d):
    TILE, CHUNK, _ = _consts()
    sizes = [0, 1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1] + ([CHUNK + 1] if d == 4 else [])
    T = _rows(max(sizes), d, 100 + d)
    sq = gm.sqnorms(T)
    for n in sizes:
        _check_uni(T, sq, np.arange(n), 2.0)
    _check_uni(T, sq, np.arange(2 * TILE + 1), 0.5)


@pytest.mark.parametrize("d", [4, 64, 68])
def test_uniformity_of_a_column_slice_with_strided_norms(d):
    TILE, _, _ = _consts()
    n = 2 * TILE + 1
    T = _rows(n, d, 7 + d, zero=(5,))
    sq = gm.sqnorms(T)
    wide = np.full((n + 2, d + 12), np.nan, dtype=np.float32)
    wide[1:1 + n, 8:8 + d] = T
    norms = np.full((n, 3), np.nan, dtype=np.float32)
    norms[:, 1] = sq
    table, nview = _t(wide)[1:1 + n, 8:8 + d], _t(norms)[:, 1]
    assert nview.stride(0) == 3 and table.stride(0) == d + 12
    for t in (0.5, 2.0):
        _check_uni(T, sq, np.arange(n), t, table=table, norms=nview)
    odd = np.full((n, d + 3), np.nan, dtype=np.float32)                       # a row stride that is no multiple of 4: no vector load
    odd[:, :d] = T
    _check_uni(T, sq, np.arange(n), 2.0, table=_t(odd)[:, :d])


@pytest.mark.parametrize("d", [4, 64, 68])
def test_uniformity_lists(d):
    TILE, _, _ = _consts()
    n_rows = 90
    T = _rows(n_rows, d, 31 + d, zero=(0, 17, 89))
    sq = gm.sqnorms(T)
    rng = np.random.default_rng(5)
    rows = rng.integers(0, n_rows, size=2 * TILE + 9)                        # repeated ids, rows without a norm
    rows[[3, 64, 100]] = -1
    rows[[0, 65, 136]] = [n_rows, n_rows + 1000, 2 ** 31 - 1]                # past the table
    rows[10] = -7
    S, pairs, n_valid, _ = _check_uni(T, sq, rows)
    assert n_valid < rows.size - 6
    _check_uni(T, sq, [0, 17, 89, -1, n_rows])                               # nothing valid
    _check_uni(T, sq, [0, 4, 17])                                            # one valid row: no pair
    _check_uni(T, sq, np.full(TILE + 3, -1))


def test_uniformity_fixed_cases():
    for d in (4, 64, 68):
        x = _rows(1, d, d)[0]
        T = np.stack([x, -x, 2 * x, np.zeros(d, dtype=np.float32)])
        sq = gm.sqnorms(T)
        for t in (0.5, 2.0):
            S, pairs, n, uni = _uni(T, sq, [0, 1], t)                        # antipodal
            assert (pairs, n) == (1, 2) and abs(uni + 4 * t) <= _tol(t, d)
            S, pairs, n, uni = _uni(T, sq, [0] * 70 + [2] * 70, t)          # all rows equal (up to scale)
            assert (pairs, n) == (140 * 139 // 2, 140) and abs(uni) <= _tol(t, d)
            S, pairs, n, uni = _uni(T, sq, [0, 0], t)                        # a repeated id contributes a pair
            assert (pairs, n) == (1, 2) and abs(uni) <= _tol(t, d)
            S, pairs, n, uni = _uni(T, sq, [0, 3, 1, 0], t)                  # (x, -x), (x, x), (-x, x)
            assert (pairs, n) == (3, 3) and abs(uni - np.log((2 * np.exp(-4.0 * t) + 1) / 3)) <= _tol(t, d)


@pytest.mark.parametrize("d", [64, 68])
def test_uniformity_invariance(d):
    TILE, CHUNK, _ = _consts()
    n = CHUNK + TILE + 5 if d == 64 else 2 * TILE + 1
    T = _rows(n + 40, d, 900 + d)
    sq = gm.sqnorms(T)
    rows = np.random.default_rng(1).permutation(n + 40)[:n]
    a, b = _uni(T, sq, rows), _uni(T, sq, rows)
    assert np.float64(a[0]).tobytes() == np.float64(b[0]).tobytes() and a[1:3] == b[1:3]      # two calls: the same bits
    r = _uni(T, sq, rows[::-1].copy())
    assert r[1:3] == a[1:3] and abs(r[0] - a[0]) <= a[1] * 2.0 ** -52 * a[0]
    assert abs(a[3] - gm.uniformity_model(T, sq, rows, 2.0)[3]) <= _tol(2.0, d)
    # a sub-list does not depend on what else is in the table: the same rows inside another table, at other ids
    sub = rows[:TILE + 7]
    small = T[sub]
    c = _uni(T, sq, sub)
    e = _uni(small, gm.sqnorms(small), np.arange(sub.size))
    assert np.float64(c[0]).tobytes() == np.float64(e[0]).tobytes() and c[1:3] == e[1:3]


# --------------------------------------------------------------------------- uniformity: the cell grid beyond two chunks
@functools.lru_cache(maxsize=None)
def _cell_probes(n, TILE, CHUNK):
    """[(tile, chunk, [(p, q), ...])] over gm.live_cells(n): position pairs p < q with p in the tile and q in the chunk, at the first
    and last position of each (all the corners that have p < q); in the diagonal cell also q = p + 1 inside the tile, q = the
    first position of the next tile against the tile's first and its last position, while that tile lies in the same chunk."""
    out = []
    for i, c in gm.live_cells(n, TILE, CHUNK):
        p_lo, p_hi = i * TILE, min((i + 1) * TILE, n) - 1
        q_lo, q_hi = c * CHUNK, min((c + 1) * CHUNK, n) - 1
        probes = [(p, q) for p in (p_lo, p_hi) for q in (q_lo, q_hi) if p < q]
        if c == i * TILE // CHUNK:
            probes += [(p, q) for p, q in ((p_lo, p_lo + 1), (p_lo, p_hi + 1), (p_hi, p_hi + 1)) if p < q <= q_hi]
        assert all(p // TILE == i and q // CHUNK == c and p < q < n for p, q in probes)
        out.append((i, c, sorted(set(probes))))
    return out


def _one_pair_list(n, d):
    """A resident list of n entries, all -1, its NaN-filled workspace and the call that puts two ids in and takes them out."""
    from elimrec_amd import ops
    rows = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    ws = torch.empty(ops.uniformity_workspace(n, d), dtype=torch.uint8, device=DEV)

    def run(table, norms, entries, t):
        for p, r in entries:
            rows[p] = r
        ws.fill_(255)                                                        # NaN in every cell: one left unwritten reaches S
        got = ops.uniformity_sum(table, norms, rows, t, workspace=ws)
        for p, _ in entries:
            rows[p] = -1
        return got
    return run


@pytest.mark.parametrize("d", [4, 64, 128])
def test_uniformity_one_pair_in_every_cell(d):
    """n = 3 CHUNK + TILE + 1 (6209: nc = 4, 290 live cells), the list all -1 but two entries p < q placed in one live cell, for every
    live cell and every probe of _cell_probes: S is that one term. n is the smallest list at which g (g - 1) / 2 is not 0, a
    chunk-row g >= 1 has more than one live chunk, a reduce thread adds a second cell AND chunk-row g = 3 holds a pair and a second
    tile (the first three hold from 3 CHUNK + 1 = 6145 on: the module's docstring). A cell that is dropped gives S = 0 (NaN where it
    was never written), one run twice 2 S, a term taken with q <= p 2 S as well. The last cell (tile 97, chunk 3) holds no pair."""
    TILE, CHUNK, _ = _consts()
    n, t = 3 * CHUNK + TILE + 1, 2.0
    T = _rows(64, d, 1200 + d)
    sq = gm.sqnorms(T)
    X = gm.unit_rows(T, sq, np.arange(64)).astype(np.float64)
    table, norms, run = _t(T), _t(sq), _one_pair_list(n, d)
    probes = _cell_probes(n, TILE, CHUNK)
    assert len(probes) == 290 and [(i, c) for i, c, pq in probes if not pq] == [((n - 1) // TILE, (n - 1) // CHUNK)]
    corners = {(p - i * TILE, q - c * CHUNK) for i, c, pq in probes for p, q in pq}
    assert corners >= {(0, 0), (0, CHUNK - 1), (TILE - 1, 0), (TILE - 1, CHUNK - 1)}
    k, worst, start = 0, 0.0, time.perf_counter()
    for i, c, pq in probes:
        for p, q in pq:
            a, b = k % 64, (7 * k + 3) % 64                                  # two different rows of the table (6 k + 3 is odd)
            k += 1
            S, pairs, n_valid = run(table, norms, ((p, a), (q, b)), t)
            want = 2.0 * t * (float(X[a] @ X[b]) - 1.0)
            assert (pairs, n_valid) == (1, 2), (i, c, p, q, pairs, n_valid)
            assert S > 0 and abs(np.log(S) - want) <= _tol(t, d), (i, c, p, q, S, np.exp(want))
            worst = max(worst, abs(np.log(S) - want))
    print("one pair per cell d=%d: %d launches over %d cells in %.2f s, worst |log S - want| %.3g, tol %.3g"
          % (d, k, len(probes), time.perf_counter() - start, worst, _tol(t, d)))


def test_uniformity_entries_that_are_no_pair_and_equal_ids_that_are():
    """The same n at d = 4. One valid entry (p == q) belongs to no cell's strict triangle: pairs = 0, S = 0 exactly -- every one of
    the 290 cells, the pairless last one too, writes its 0 over the NaN -- and a NaN value. Two entries with the SAME id at different
    positions are a pair: S = 1 within the tolerance, in every cell."""
    from elimrec_amd import ops
    TILE, CHUNK, _ = _consts()
    n, t, d = 3 * CHUNK + TILE + 1, 2.0, 4
    T = _rows(64, d, 1300)
    sq = gm.sqnorms(T)
    table, norms, run = _t(T), _t(sq), _one_pair_list(n, d)
    for p in sorted({i * TILE for i in range((n + TILE - 1) // TILE)} | {c * CHUNK - 1 for c in range(1, 4)} | {n - 2, n - 1}):
        S, pairs, n_valid = run(table, norms, ((p, p % 64),), t)
        assert (S, pairs, n_valid) == (0.0, 0, 1) and np.isnan(ops.uniformity_value(S, pairs)), (p, S, pairs, n_valid)
    for k, (i, c, pq) in enumerate(_cell_probes(n, TILE, CHUNK)):
        if pq:
            p, q = pq[k % len(pq)]
            S, pairs, n_valid = run(table, norms, ((p, k % 64), (q, k % 64)), t)
            assert (pairs, n_valid) == (1, 2) and S > 0 and abs(np.log(S)) <= _tol(t, d), (i, c, p, q, S)


def _dense_list(n, d, TILE, seed):
    """(T, rows): every entry valid, the row at POSITION p one of 7 fixed random unit directions, u[p // TILE % 7], plus 0.05-scaled
    Gaussian noise, times a scale in [0.5, 3]; the positions' rows lie in the table in a random order, so rows is a permutation."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((7, d))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    x = (u[np.arange(n) // TILE % 7] + 0.05 * rng.standard_normal((n, d))) * rng.uniform(0.5, 3.0, (n, 1))
    rows = rng.permutation(n)
    T = np.empty((n, d), dtype=np.float32)
    T[rows] = x.astype(np.float32)
    return T, rows


@pytest.mark.parametrize("d,t", [(32, 2.0), (32, 8.0), (32, 0.5), (68, 2.0), (128, 2.0)])
def test_uniformity_dense_list_whose_cells_differ(d, t):
    """n = 3 CHUNK + TILE + 1, every entry valid, against the float64 model (an n^2 product). With i.i.d. rows every cell has
    nearly the same sum and a cell computed twice in place of another would move S by less than the tolerance; here a tile's rows
    share one of 7 directions, so the cells differ. That is asserted on the model's cell sums, over all pairs of cells A, B:
      |A - B| > 100 tol max(A, B) for at least 90 %: the two are far outside each other's rounding error;
      |A - B| > 2 tol S for at least 80 %: B in place of A moves log S by more than 2 tol, which the kernel's own error (<= tol)
      cannot bring back inside tol. (A mean cell is S / 290 = 3.4e-3 S and tol is 5e-6 .. 7e-5, so a few per cent between two cells
      are enough; cells of the same direction and chunk differ by their noise alone and make up the rest.)"""
    TILE, CHUNK, _ = _consts()
    n = 3 * CHUNK + TILE + 1
    T, rows = _dense_list(n, d, TILE, 500 + d)
    sq = gm.sqnorms(T)
    wS, wpairs, wn, wuni, cells = gm.uniformity_model(T, sq, rows, t, cells=(TILE, CHUNK))
    cells, tol = np.asarray(cells), _tol(t, d)
    assert cells.size == 290 and wn == n
    upper = np.triu_indices(cells.size, 1)
    diff = np.abs(cells[:, None] - cells[None, :])[upper]
    apart, seen = (diff > 100 * tol * np.maximum(cells[:, None], cells[None, :])[upper]).mean(), (diff > 2 * tol * wS).mean()
    print("dense d=%d t=%g: cell pairs apart by > 100 tol of the larger: %.3f, by > 2 tol S: %.3f" % (d, t, apart, seen))
    assert apart >= 0.9 and seen >= 0.8
    table, norms = _t(T), _t(sq)
    a, b = _uni(T, sq, rows, t, table=table, norms=norms), _uni(T, sq, rows, t, table=table, norms=norms)
    print("dense d=%d t=%g: got %.12g want %.12g diff %.3g tol %.3g" % (d, t, a[3], wuni, abs(a[3] - wuni), tol))
    assert a[1:3] == (wpairs, wn) and abs(a[3] - wuni) <= tol
    assert np.float64(a[0]).tobytes() == np.float64(b[0]).tobytes() and a[1:3] == b[1:3]      # two calls: the same bits
    r = _uni(T, sq, rows[::-1].copy(), t, table=table, norms=norms)
    assert r[1:3] == a[1:3] and abs(r[0] - a[0]) <= a[1] * 2.0 ** -52 * a[0]


def test_temperature_limits_on_the_device():
    """t = 8 (GEOMETRY_MAX_T) is taken; the library itself refuses a t past it, 0 and NaN before it writes anything."""
    from elimrec_amd import _lib, ops
    TILE, _, _ = _consts()
    n = TILE + 1
    T = _rows(n, 4, 8)
    sq = gm.sqnorms(T)
    assert ops.GEOMETRY_MAX_T == 8.0
    _check_uni(T, sq, np.arange(n), 8.0)
    table, norms, rows = _t(T), _t(sq), _t(np.arange(n, dtype=np.int32))
    S = torch.full((1,), -7.0, dtype=torch.float64, device=DEV)
    counts = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    ws = torch.empty(ops.uniformity_workspace(n, 4), dtype=torch.uint8, device=DEV)
    lib = _lib.load()
    for bad in (8.0000001, float(np.nextafter(8.0, 9.0)), 0.0, -2.0, float("nan"), float("inf")):
        rc = lib.elimrec_uniformity_sum(table.data_ptr(), table.stride(0), n, 4, norms.data_ptr(), 1, rows.data_ptr(), n, bad,
                                        S.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream())
        assert rc != 0 and b"0 < t <= 8" in lib.elimrec_last_error(), (bad, rc)
        with pytest.raises(ValueError, match="0 < t <= 8"):
            ops.uniformity_sum(table, norms, rows, bad)
        torch.cuda.synchronize()
        assert S.item() == -7.0 and counts.tolist() == [-7, -7]


# --------------------------------------------------------------------------- Gram
def _check_gram(T, sq, rows, table=None, norms=None):
    from elimrec_amd import ops
    d = T.shape[1]
    G, m, n_valid = ops.row_gram(_t(T) if table is None else table, _t(sq) if norms is None else norms, _t(np.asarray(rows, dtype=np.int32)))
    assert G.dtype == m.dtype == torch.float64 and tuple(G.shape) == (d, d) and tuple(m.shape) == (d,)
    G, m = G.cpu().numpy(), m.cpu().numpy()
    wG, wm, wn, A, a = gm.gram_model(T, sq, rows)
    assert n_valid == wn
    assert np.array_equal(G, G.T)                                            # exactly symmetric
    n = max(len(rows), 1)
    assert (np.abs(G - wG) <= n * 2.0 ** -52 * A).all() and (np.abs(m - wm) <= n * 2.0 ** -52 * a).all()
    if wn:
        assert abs(np.trace(G) / wn - 1.0) <= (d + 4) * 2.0 ** -23
    return G, m, n_valid


@pytest.mark.parametrize("d", [4, 64, 68, 256])
def test_gram_sizes(d):
    _, _, SEG = _consts()
    sizes = [1, SEG - 1] if d == 256 else [1, SEG - 1, SEG, SEG + 1, 2 * SEG + 3]
    T = _rows(max(sizes), d, 300 + d, zero=(3,) if max(sizes) > 3 else ())
    sq = gm.sqnorms(T)
    for n in sizes:
        _check_gram(T, sq, np.arange(n))
    G, m, n_valid = _check_gram(T, sq, [])
    assert n_valid == 0 and not G.any() and not m.any()


@pytest.mark.parametrize("d", [4, 68])
def test_gram_lists_and_forms(d):
    _, _, SEG = _consts()
    n_rows = 90
    T = _rows(n_rows, d, 77 + d, zero=(0, 17))
    sq = gm.sqnorms(T)
    rows = np.random.default_rng(9).integers(0, n_rows, size=SEG + 41)
    rows[[3, 64, 500]] = -1
    rows[[0, 65, 520]] = [n_rows, n_rows + 1000, 2 ** 31 - 1]
    G, m, n_valid = _check_gram(T, sq, rows)
    assert 0 < n_valid < rows.size - 6
    _check_gram(T, sq, [0, 17, -1, n_rows])                                  # nothing valid
    wide = np.full((n_rows + 2, d + 12), np.nan, dtype=np.float32)
    wide[1:1 + n_rows, 8:8 + d] = T
    norms = np.full((n_rows, 3), np.nan, dtype=np.float32)
    norms[:, 1] = sq
    G2, m2, _ = _check_gram(T, sq, rows, table=_t(wide)[1:1 + n_rows, 8:8 + d], norms=_t(norms)[:, 1])
    assert G2.tobytes() == G.tobytes() and m2.tobytes() == m.tobytes()       # the bits do not depend on the table's form


@pytest.mark.parametrize("d", [132, 192])
def test_gram_three_column_blocks(d):
    """nb = 3 column blocks (d = 132: the last one 4 columns wide; d = 192: all full), 2 and 3 segments, a list with invalid
    entries and rows without a norm: the six tiles (bi <= bj) of blockIdx.y. An element whose row and column lie in different blocks
    is named on its own: only a tile decoded to the right (bi, bj), and mirrored, puts the model's value there."""
    _, _, SEG = _consts()
    n_rows = 90
    T = _rows(n_rows, d, 400 + d, zero=(0, 17))
    sq = gm.sqnorms(T)
    rng = np.random.default_rng(11)
    block = np.arange(d) // 64
    assert block.max() == 2
    for n in (SEG + 1, 2 * SEG + 3):
        rows = rng.integers(0, n_rows, size=n)
        rows[[3, 64, 500]] = -1
        rows[[0, 65, SEG]] = [n_rows, n_rows + 1000, 2 ** 31 - 1]
        G, m, n_valid = _check_gram(T, sq, rows)
        assert 0 < n_valid < n - 6
        wG, _, _, A, _ = gm.gram_model(T, sq, rows)
        for bi in range(3):
            for bj in range(3):
                if bi != bj:
                    sel = np.ix_(block == bi, block == bj)
                    assert (np.abs(G[sel] - wG[sel]) <= n * 2.0 ** -52 * A[sel]).all(), "column blocks (%d, %d) at n = %d" % (bi, bj, n)
                    # and the model's block is far from 0: a tile that was never written, or written elsewhere, would not pass
                    assert np.abs(wG[sel]).max() > 1e6 * n * 2.0 ** -52 * A[sel].max()


def test_torch_ops_return_what_the_ops_return():
    from elimrec_amd import ops, torch_ops
    t_ops = torch_ops.load()
    TILE, _, _ = _consts()
    T = _rows(2 * TILE + 1, 64, 4, zero=(2,))
    sq = gm.sqnorms(T)
    rows = _t(np.r_[np.arange(2 * TILE + 1), -1, 5].astype(np.int32))
    S, pairs, n_valid = ops.uniformity_sum(_t(T), _t(sq), rows, 0.5)
    s2, counts = t_ops.uniformity_sum(_t(T), _t(sq), rows, 0.5)
    assert s2.cpu().numpy().tobytes() == np.float64(S).tobytes() and counts.cpu().tolist() == [pairs, n_valid]
    G, m, n = ops.row_gram(_t(T), _t(sq), rows)
    g2, m2, c2 = t_ops.row_gram(_t(T), _t(sq), rows)
    assert torch.equal(G, g2) and torch.equal(m, m2) and c2.cpu().tolist() == [n]
    with pytest.raises(RuntimeError, match="0 < t <= 8"):
        t_ops.uniformity_sum(_t(T), _t(sq), rows, 0.0)


# --------------------------------------------------------------------------- the model and the report
def _forward(name, extra=()):
    from helpers import build_model_from_fixture, load_golden
    g = load_golden(name)
    model, _ = build_model_from_fixture(g, DEV, extra_argv=extra)
    model.bpr_loss(_t(g["step1/users"]), _t(g["step1/pos"]), _t(g["step1/neg"]))
    return model


def _host_tables(model):
    """(Y, sqn) of the cached tables copied to the host, the pending forward made real first."""
    sqn = model._block_sqnorms(model._cached_tables("the test needs"))
    return model._ws["Y"].cpu().numpy(), sqn.cpu().numpy()


def _space_tables(model, Y, sqn, side, h):
    lo, n = model._side_rows(side)
    d = model.latent_dim
    return Y[lo:lo + n, h * d:(h + 1) * d], sqn[lo:lo + n, h]


def _check_row(got, want, t, d):
    """One row of GEOMETRY_COLUMNS against the model's: n exact, uniformity within its bound, the spectrum columns -- float64
    eigenvalues of Gram matrices that agree to n 2^-52 -- to 1e-9."""
    assert got[0] == want[0]
    for k in range(1, 6):
        if np.isnan(want[k]):
            assert np.isnan(got[k]), (k, got, want)
        else:
            assert abs(got[k] - want[k]) <= (_tol(t, d) if k == 1 else 1e-9 * max(1.0, abs(want[k]))), (k, got, want)


@pytest.mark.parametrize("name", ["ml3", "kwai"])
def test_embedding_geometry_and_alignment(name):
    from helpers import build_model_from_fixture, load_golden
    from elimrec_amd.evaluator import GEOMETRY_COLUMNS, CandidateScoringError
    from elimrec_amd.model import Geometry
    fresh, _ = build_model_from_fixture(load_golden(name), DEV)
    with pytest.raises(RuntimeError):
        fresh.embedding_geometry()
    model = _forward(name)
    Y, sqn = _host_tables(model)
    d, spaces = model.latent_dim, ("fused",) + tuple(model._mods)
    assert len(spaces) == (2 if name == "kwai" else 4)
    for side in ("item", "user"):
        for t in (2.0, 0.5):
            got = model.embedding_geometry(side=side, t=t)
            assert isinstance(got, Geometry) and got.columns == GEOMETRY_COLUMNS and got.labels == spaces
            assert got.values.device.type == "cpu" and tuple(got.values.shape) == (len(spaces), 6) and got.values.dtype == torch.float64
            for h in range(len(spaces)):
                T, sq = _space_tables(model, Y, sqn, side, h)
                _check_row(got.values[h].numpy(), gm.geometry_row_model(T, sq, np.arange(T.shape[0]), t), t, d)
    T, sq = _space_tables(model, Y, sqn, "item", 1)
    sub = [5, 2, 2, 9, 0]
    one = model.embedding_geometry(space=spaces[1], rows=sub)
    assert one.labels == (spaces[1],) and tuple(one.values.shape) == (1, 6)
    _check_row(one.values[0].numpy(), gm.geometry_row_model(T, sq, sub, 2.0), 2.0, d)
    raw = model.geometry_device("item", spaces[1], _t(np.asarray(sub + [-1, 10 ** 6], dtype=np.int32)))
    assert all(x.is_cuda for x in raw) and int(raw[2].item()) == 5 and int(raw[1].item()) == 10
    # alignment: per space against the model, and bit for bit 2 - 2 x the score pick_hard_negatives returns
    U_, I = model.num_users, model.num_items
    rng = np.random.default_rng(3)
    users, items = rng.integers(0, U_, 50), rng.integers(0, I, 50)
    got = model.alignment(users, items)
    assert got.device.type == "cpu" and got.dtype == torch.float32 and tuple(got.shape) == (50, len(spaces))
    for h, s in enumerate(spaces):
        TU, squ = _space_tables(model, Y, sqn, "user", h)
        TI, sqi = _space_tables(model, Y, sqn, "item", h)
        want = gm.alignment_model(TU, squ, TI, sqi, users, items)
        assert np.abs(got[:, h].numpy().astype(np.float64) - want).max() <= (d + 4) * 2.0 ** -22
        score = model.hard_negatives_device(_t(users.astype(np.int64)), _t(items.astype(np.int32).reshape(-1, 1)), s)[2].cpu().numpy()
        assert got[:, h].numpy().tobytes() == (np.float32(2) - np.float32(2) * score).astype(np.float32).tobytes()
        assert model.alignment(users, items, space=s).numpy().tobytes() == got[:, h].contiguous().numpy().tobytes()
    model._eval_shard = object()
    try:
        with pytest.raises(CandidateScoringError):
            model.embedding_geometry()
    finally:
        model._eval_shard = None


@pytest.mark.parametrize("name,views", [("ml3", (None, None)), ("ml3", ([1, 3, 5], [1, 4])), ("kwai", ([2, 4], [2]))])
def test_geometry_report(name, views, monkeypatch):
    from elimrec_amd import ops
    from elimrec_amd.evaluator import GEOMETRY_COLUMNS, GeometryReport, GeometryTables
    model = _forward(name)
    train, test = model.dataset.get_user_train_dict(), model.dataset.get_user_test_dict()
    report = GeometryReport(model.dataset, train, test, group_view=views[0], item_group_view=views[1], t=0.5)
    calls = []
    real = ops.uniformity_sum_device
    monkeypatch.setattr(ops, "uniformity_sum_device", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    final, buf = report.evaluate(model)
    Y, sqn = _host_tables(model)
    d, spaces = model.latent_dim, ("fused",) + tuple(model._mods)
    n_sets = len(report.row_sets)
    assert isinstance(final, GeometryTables) and final.columns == GEOMETRY_COLUMNS and len(calls) == len(spaces) * n_sets
    assert final.values.shape == (len(spaces) * n_sets, 6) and (n_sets > 2) == (views[0] is not None)
    single = 0
    for h, s in enumerate(spaces):
        for k, (label, side, ids) in enumerate(report.row_sets):
            T, sq = _space_tables(model, Y, sqn, side, h)
            assert ids is None or ids.size > 0                                # an empty group is omitted
            want = gm.geometry_row_model(T, sq, np.arange(T.shape[0]) if ids is None else ids, 0.5)
            _check_row(final.values[h * n_sets + k], want, 0.5, d)
            assert final.labels[h * n_sets + k].startswith("%s %s" % (s, label.rstrip(":")))
            single += want[0] == 1 and np.isnan(final.values[h * n_sets + k][1])
    # alignment: the float64 mean of the pairs' fp32 values, rounded once; the pairs' values within (d + 4) 2^-22 of the model's
    assert final.align.shape == (2 * len(spaces), len(report.align_columns)) and final.align.dtype == np.float32
    for w, which in enumerate(("align_train", "align_test")):
        users, items, cols, positions = report._pairs[which]
        pair_rows = model.alignment(users, items).numpy()
        for h in range(len(spaces)):
            TU, squ = _space_tables(model, Y, sqn, "user", h)
            TI, sqi = _space_tables(model, Y, sqn, "item", h)
            want = gm.alignment_model(TU, squ, TI, sqi, users, items)
            row = final.align[2 * h + w]
            for c in range(len(report.align_columns)):
                if c in cols:
                    p = positions[cols.index(c)]
                    assert row[c] == np.float32(pair_rows[p, h].astype(np.float64).mean())
                    assert abs(float(row[c]) - want[p].mean()) <= (d + 4) * 2.0 ** -22 + 2.0 ** -23
                else:
                    assert np.isnan(row[c])                                  # a group without a pair
            assert final.align_labels[2 * h + w].startswith("%s %s" % (spaces[h], which))
        bare = [(sqn[users, h] == 0) | (sqn[model.num_users + items, h] == 0) for h in range(len(spaces))]
        assert [report.num_no_norm[(which, s)] for s in spaces] == [int(b.sum()) for b in bare]
    lines = buf.split("\n")
    assert lines[0].startswith("columns:") and all(c in lines[0] for c in GEOMETRY_COLUMNS)
    assert sum(ln.startswith("columns:") for ln in lines) == 2 and len(lines) == 2 + len(final.labels) + len(final.align_labels)
    # a second evaluate on the same table version launches nothing
    n_calls = len(calls)
    again, buf2 = report.evaluate(model)
    assert len(calls) == n_calls and buf2 == buf and again is final
    if views[0] is not None and name == "ml3":
        assert single >= 0


def test_a_group_with_a_single_row_has_no_uniformity():
    """A GeometryReport whose item view isolates single items: NaN uniformity and spectrum, n = 1, centre = 1."""
    from elimrec_amd.evaluator import GeometryReport
    model = _forward("ml3")
    train, test = model.dataset.get_user_train_dict(), model.dataset.get_user_test_dict()
    counts = np.bincount(np.asarray([i for v in train.values() for i in v], dtype=np.int64), minlength=model.num_items)
    alone = [int(c) for c in np.unique(counts) if c > 0 and (counts == c).sum() == 1]
    assert alone, "the fixture has an item whose training count no other item shares"
    c = alone[0]
    view = [c - 1, c] if c > 1 else [c]
    report = GeometryReport(model.dataset, train, test, item_group_view=view)
    final, _ = report.evaluate(model)
    label = "item (%d,%d]" % (c - 1 if c > 1 else 0, c)
    hits = [k for k, x in enumerate(final.labels) if label in x]
    assert len(hits) == 1 + len(model._mods)
    for k in hits:
        n, uni, erank, top1, rank99, centre = final.values[k]
        assert n == 1 and np.isnan(uni) and np.isnan(erank) and np.isnan(top1) and np.isnan(rank99) and abs(centre - 1) <= 2.0 ** -22


def test_driver_switch(tmp_path):
    from test_lists_gpu import _driver
    view = ["--group_view=[10,30]", "--item_group_view=[1,4]", "--neighbour_report=3"]
    off, ev0, te0 = _driver(tmp_path / "a", view)
    assert not any("[geometry]" in ln for ln in off)
    zero, ev2, te2 = _driver(tmp_path / "c", view + ["--geometry_report=0"])
    assert zero == off and ev0.tobytes() == ev2.tobytes() and te0.tobytes() == te2.tobytes()
    on, ev1, te1 = _driver(tmp_path / "b", view + ["--geometry_report=1", "--geometry_t=0.5"])
    added = [k for k, ln in enumerate(on) if ln.startswith("  [geometry]")]
    assert len(added) == 1 and added[0] == len(on) - 1                       # once, after both effects' lines and [neighbours]
    assert [ln for k, ln in enumerate(on) if k not in added] == off          # every other line is as it was
    block = on[added[0]]
    assert "t = 0.5" in block.split("\n")[0] and all(c in block for c in ("uniformity", "erank", "top1", "rank99", "centre"))
    assert all(x in block for x in ("fused user:", "fused item:", "fused align_train:", "fused align_test:", "item cold"))
    assert ev0.tobytes() == ev1.tobytes() and te0.tobytes() == te1.tobytes()
