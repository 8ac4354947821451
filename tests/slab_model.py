"""Float64 model of the slab-major hops (csrc/slab.hip: sell_tier_kernel, tile_ballot_kernel, sell_hop_kernel + sell_fixup_kernel;
csrc/sweep.hip: sweep_rows_kernel), the graphs their tests share and numpy walks of the host plans. Nothing here calls a project
kernel; the plans it walks are built with device="cpu" (numpy only).

The arithmetic is propagate_model.hop -- (A x over the rows of src_mask + add on the rows of add_mask) * scale as a float64 value
and the |A||x| (+ |add|) |scale| magnitude -- and the criterion is fp64_tools.assert_close with K = the row's own length + 3
(propagate_model.hop_K): cutting a row into lane groups, quarters or segments reorders the same additions, which the bound covers.

The wave-tile hop sorts rows into four tiers by length, with G = 64 / LPR lane groups per wave (tiers()):
    unsplit  <= T          a lane group per row
    wave     (T, T1]       T1 = (64 if G <= 8 else 32) G: a wave per row, neighbours dealt round-robin to the G groups
    workgroup (T1, T2]     T2 = 256 G: four waves on contiguous quarters
    segmented > T2         T-long segments, partial rows, tickets, the last arriver combines (stream_combine)
tier_ladder(T, G) holds a row on and next to every such boundary.
"""
import functools

import numpy as np
import scipy.sparse as sp

from propagate_model import _from_lengths, bitmap_words, bits_of, hop, hop_K, row_lengths     # noqa: F401 (the tests' one import)

UNSPLIT, WAVE, WORKGROUP, SEGMENTED = 0, 1, 2, 3
TIER_NAMES = ("unsplit", "wave", "workgroup", "segmented")


def tiers(T, G):
    """(T1, T2) of a tiered plan with threshold T and G lane groups per wave."""
    return (64 if G <= 8 else 32) * G, 256 * G


def tier_of(lengths, T, G):
    """Tier of every row length."""
    T1, T2 = tiers(T, G)
    n = np.asarray(lengths, dtype=np.int64)
    return (n > T).astype(np.int64) + (n > T1) + (n > T2)


def n_segments(lengths, T, G):
    """Segments the tiered plan cuts the rows above T2 into."""
    n = np.asarray(lengths, dtype=np.int64)
    return int(np.where(n > tiers(T, G)[1], (n + T - 1) // T, 0).sum())


def plan_counts(lengths, T, G):
    """What a tiered SellPlan must report for these row lengths: dict(n_w1, n_w4, n_seg, n_long, n_fin)."""
    t = tier_of(lengths, T, G)
    return dict(n_w1=int((t == WAVE).sum()), n_w4=int((t == WORKGROUP).sum()), n_seg=n_segments(lengths, T, G),
                n_long=int((t > UNSPLIT).sum()), n_fin=int((t == UNSPLIT).sum()))


# ----------------------------------------------------------------------------------------------------------- tier ladder
def big_row(T, G):
    """The longest row: >= 9 G segments (a lane group of stream_combine adds >= 9 partials: the 8-wide loop + a remainder)."""
    T2 = tiers(T, G)[1]
    return 9 * G * T if 9 * G * T > T2 else T2 + 3 * T + 5


def ladder_named_lengths(T, G):
    """The row lengths the ladder holds by construction, in row order (row 0 is the empty one).
    Workgroup rows: the plan cuts a row of n entries into quarters of q' = G ceil(ceil(n / 4) / G), so the fourth wave keeps
    n - 3 q' >= n / 4 - 3 G entries: above T1 >= 32 G it never has a single neighbour (that needs n <= 12 G + 1). Its SHORTEST
    share in the tier is the row of T1 + 1 entries (13 G + 1 of 64 G + 1 at G <= 8, 5 G + 1 of 32 G + 1 above), which is here;
    4q, 4q - 1 and 3q + 1 with q a multiple of G are full quarters, a last quarter one short, and a length on no boundary."""
    T1, T2 = tiers(T, G)
    q = (T1 // 3 // G + 1) * G                                     # the least multiple of G with T1 < 3q + 1 (and 4q <= T2)
    unsplit = [0, 1, 2, T - 1, T] + [n for n in (G - 1, G, G + 1) if 0 <= n <= T]
    wave = [T + 1, T + 2] + [n for n in (63, 64, 65, 127, 128, 129) if T < n <= T1]
    wave += [n for n in sorted({G // 2, G - 1, G, G + 1}) if T + 2 < n <= T1]      # below G: lane groups without a neighbour
    wave += [T1 - 1, T1]
    wgrp = [T1 + 1, 4 * q, 4 * q - 1, 3 * q + 1, T2 - 1, T2]
    seg = [T2 + 1, T2 + T, big_row(T, G)]
    assert all(T < n <= T1 for n in wave) and all(T1 < n <= T2 for n in wgrp) and (T2 + 1) % T == 1
    return unsplit + wave + wgrp + seg


def _ladder_lengths(T, G):
    T1, T2 = tiers(T, G)
    lens = ladder_named_lengths(T, G)
    n_named = len(lens)
    t = tier_of(lens, T, G)
    if int((t == WAVE).sum()) % 4 == 0:
        lens.append(T + 3 if T + 3 <= T1 else T + 1)
    if int((t == WORKGROUP).sum()) % 4 == 0:
        lens.append(T1 + 2)
    k = 0
    while n_segments(lens, T, G) % (4 * G) == 0:                   # (a row of T2 + 2 + k entries: 256 G / T + 1 segments more)
        lens.append(T2 + 2 + k)
        k += 1
    n = big_row(T, G) + 37                                         # the longest row + a margin
    fill = [1, 0, 2, 1, 3, 1, 0, 1, 5, 1, 0, 2, 7, 1, 0, 4]                # light: the size of the ladder is that of its long rows
    while (n - 1 - len(lens) + int((tier_of(lens, T, G) == UNSPLIT).sum()) + 1) % (4 * G) == 0:
        n += 1
    lens += [min(fill[i % len(fill)], T) for i in range(n - 1 - len(lens))]
    lens.append(0)                                                 # the last row is empty
    return lens, n_named


@functools.lru_cache(maxsize=None)
def tier_ladder(T, G, seed=0):
    """(m, named): a square CSR matrix (float32 weights in +-[0.1, 1.1], sorted distinct columns) with a row on and next to
    every tier boundary of a tiered plan (threshold T, G lane groups), and {row: length} of the rows that are there by
    construction. Row 0 and the last row are empty; the filler rows make the numbers of wave rows, workgroup rows, segments and
    unsplit rows no multiple of 4, 4, 4 G and 4 G (the tile padding runs)."""
    lens, n_named = _ladder_lengths(T, G)
    m = _from_lengths(lens, len(lens), seed + 64 * T + G)
    return m, {r: int(lens[r]) for r in range(n_named)}


@functools.lru_cache(maxsize=None)
def tier_ladder_flat(T, G, seed=0):
    """The ladder with no row above T (n_long == 0): the longer rows keep length mod (T + 1) entries."""
    lens, _ = _ladder_lengths(T, G)
    return _from_lengths([n if n <= T else n % (T + 1) for n in lens], len(lens), seed + 64 * T + G + 1)


@functools.lru_cache(maxsize=None)
def tier_ladder_long(T, G, seed=0):
    """Only the ladder's rows above T (n_tfin == 0): a few dozen rows over as many sources as the square ladder has."""
    lens, _ = _ladder_lengths(T, G)
    return _from_lengths([n for n in lens if n > T], len(lens), seed + 64 * T + G + 2)


def one_row_per_tier(lengths, T, G, which=0, empty=True):
    """A row of every tier (the which-th of each) and, with `empty`, the which-th empty row."""
    lengths = np.asarray(lengths)
    t = tier_of(lengths, T, G)
    rows = [int(np.nonzero((t == k) & (lengths > 0))[0][which]) for k in range(4) if int(((t == k) & (lengths > 0)).sum()) > which]
    if empty:
        rows.append(int(np.nonzero(lengths == 0)[0][which]))
    return rows


# ----------------------------------------------------------------------------------------------------------- sweep ladder
SWEEP_NAMED = (0, 1, 7, 8, 9, 15, 16, 17, 63, 65)


@functools.lru_cache(maxsize=None)
def sweep_ladder(U, I, seed=0):
    """The symmetric-pattern bipartite graph [[0, R], [Q, 0]] (Q has R^T's pattern and weights of its own). User rows:
    0, 1, 7, 8, 9, 15, 16, 17, 63, 65 entries, one row of all I items, then fillers -- among them rows of 20, 28 and 40 CONSECUTIVE
    items from item 0 on, which lie in one source window whatever the window (3, 4 and 5 step records of eight entries)."""
    assert U % 32 != 0 and U >= 29 and I >= 130
    rs = np.random.RandomState(seed + U)
    lens = list(SWEEP_NAMED) + [I]
    fill = [20, 28, 40, 3, 24, 12, 33, 2, 5, 0, 26, 18]
    lens += [fill[i % len(fill)] for i in range(U - len(lens))]
    R = _from_lengths(lens, I, seed + U).tolil()
    for r in range(len(SWEEP_NAMED) + 1, U):
        if lens[r] in (20, 28, 40):
            R.rows[r], R.data[r] = list(range(lens[r])), list(R.data[r])
    R = R.tocsr().astype(np.float32)
    Q = R.T.tocsr().astype(np.float32)
    Q.data = ((0.1 + rs.rand(Q.nnz)) * np.where(rs.rand(Q.nnz) < 0.5, -1.0, 1.0)).astype(np.float32)
    m = sp.bmat([[None, R], [Q, None]], format="csr").astype(np.float32)
    m.sort_indices()
    assert np.array_equal(np.diff(m.indptr[:U + 1]), lens)
    return m


def wave_stretches(geometry):
    """Step counts of every (row block, wave) of a SweepPlan.geometry()."""
    return np.diff(np.asarray(geometry["slot_ptr"].cpu().numpy(), dtype=np.int64))


# ----------------------------------------------------------------------------------------------------------- layout
def slab_layout(X, ns, w):
    """Row-major [n x ns*w] -> the flat slab-major [ns][n][w] of SlabTable.from_rows."""
    X = np.asarray(X)
    n = X.shape[0]
    assert X.shape[1] == ns * w
    return np.ascontiguousarray(X.reshape(n, ns, w).transpose(1, 0, 2)).reshape(-1)


def slab_dense(flat, n, ns, w):
    """The inverse: flat [ns][n][w] -> row-major [n x ns*w] (SlabTable.dense)."""
    return np.ascontiguousarray(np.asarray(flat).reshape(ns, n, w).transpose(1, 0, 2)).reshape(n, ns * w)


# ----------------------------------------------------------------------------------------------------------- plan walks
def _h(plan, key, dtype=np.int64):
    return plan.t[key].cpu().numpy().astype(dtype)


def tile_bases(plan):
    """(t1_base, tseg_base, tfin_base, n_tiles) of a tiered plan: first tile of the wave rows, segment tiles, unsplit-row tiles."""
    d = plan.desc
    t1 = int(d.n_t4)
    return t1, t1 + int(d.n_t1), t1 + int(d.n_t1) + int(d.n_tseg), t1 + int(d.n_t1) + int(d.n_tseg) + int(d.n_tfin)


def _triples(rows, cols, vals):
    o = np.lexsort((cols, rows))
    return rows[o], cols[o], vals[o]


def csr_triples(m):
    m = sp.csr_matrix(m)
    return _triples(np.repeat(np.arange(m.shape[0], dtype=np.int64), np.diff(m.indptr)), m.indices.astype(np.int64), m.data.astype(np.float32))


def _slot_rows(plan, slots_long, dst):
    """Row of a segment slot: through the split-row number the plan stores beside it; the slot must lie in that row's range."""
    long_rows, seg_ptr = _h(plan, "long_rows"), _h(plan, "long_seg_ptr")
    assert np.all((seg_ptr[slots_long] <= dst) & (dst < seg_ptr[slots_long + 1])), "a segment slot outside its row's range"
    return long_rows[slots_long]


def walk_tiles(plan):
    """Every (row, col, val) a tiered plan's wave tiles hold, sorted by (row, col): tile t, lane group g, step j is entry
    tile_off[t] + j G + g for j < tile_len[t, g]; tile_dst[t, g] is the row (wave / workgroup / unsplit tiles) or the segment
    slot, whose row is long_rows[tile_long[.]] (segment tiles). Also checks the padding: no destination -> no length."""
    G = plan.tile_groups
    t1, tseg, tfin, n_tiles = tile_bases(plan)
    off, glen, dst = _h(plan, "tile_off"), _h(plan, "tile_len"), _h(plan, "tile_dst")
    tcol, tval = _h(plan, "tile_col"), plan.t["tile_val"].cpu().numpy()
    assert len(off) == n_tiles + 1 and len(glen) == n_tiles * G == len(dst)
    assert np.all(glen[dst < 0] == 0), "a padding slot with a length"
    steps = np.diff(off) // G
    assert np.all(np.diff(off) % G == 0) and np.all(glen.reshape(-1, G).max(1) == steps if n_tiles else True)
    slot = np.arange(n_tiles * G)
    tile = slot // G
    row = dst.copy()
    is_seg = (tile >= tseg) & (tile < tfin) & (dst >= 0)
    if is_seg.any():
        row[is_seg] = _slot_rows(plan, _h(plan, "tile_long")[slot[is_seg] - tseg * G], dst[is_seg])
    it = np.repeat(slot, glen)
    j = np.arange(len(it)) - np.repeat(np.cumsum(glen) - glen, glen)
    pos = off[it // G] + j * G + it % G
    assert len(np.unique(pos)) == len(pos), "two entries in one index slot"
    return _triples(row[it], tcol[pos], tval[pos])


def walk_sell(plan):
    """The same for the two-launch SELL-64 arrays: item i, step j is entry (blk_off[i / 64] + j) 64 + i % 64; the items below
    n_seg_items are segments (item_dst = slot, item_long = split-row number)."""
    dst, ilen, blk = _h(plan, "item_dst"), _h(plan, "item_len"), _h(plan, "blk_off")
    col, val = _h(plan, "col"), plan.t["val"].cpu().numpy()
    assert len(dst) == plan.n_items and plan.n_items % 64 == 0 and plan.n_seg_items % 64 == 0
    assert np.all(ilen[dst < 0] == 0), "a padding item with a length"
    item = np.arange(plan.n_items)
    row = dst.copy()
    is_seg = (item < plan.n_seg_items) & (dst >= 0)
    if is_seg.any():
        row[is_seg] = _slot_rows(plan, _h(plan, "item_long")[item[is_seg]], dst[is_seg])
    it = np.repeat(item, ilen)
    j = np.arange(len(it)) - np.repeat(np.cumsum(ilen) - ilen, ilen)
    pos = (blk[it // 64] + j) * 64 + it % 64
    assert len(np.unique(pos)) == len(pos), "two entries in one index slot"
    return _triples(row[it], col[pos], val[pos])


# ----------------------------------------------------------------------------------------------------------- ballot bitmaps
def tile_lines(plan, ti):
    """The sources of every 64-entry index line of tile ti (a list of arrays; padding slots left out)."""
    G = plan.tile_groups
    off, glen, tcol = _h(plan, "tile_off"), _h(plan, "tile_len"), _h(plan, "tile_col")
    lo, hi = int(off[ti]), int(off[ti + 1])
    p = np.arange(hi - lo)
    real = (p // G) < glen[ti * G + p % G]
    return [tcol[lo + p[(p // 64 == k) & real]] for k in range((hi - lo + 63) // 64)]


def longest_wave_tile(plan):
    """(tile, row) of the longest wave row: the wave rows are laid out by decreasing length."""
    assert plan.n_w1 > 0
    ti = tile_bases(plan)[0]
    return ti, int(_h(plan, "tile_dst")[ti * plan.tile_groups])


def source_patterns(plan, m):
    """Named source-row bitmaps (bool [n_src]) for the masked hop of a host-built tiered plan of m: none / all active; only the
    sources in index line 0, in the last line, in one middle line of the longest wave row's tile; every 64th source; every source
    but the longest wave row's own."""
    n = m.shape[1]
    ti, row = longest_wave_tile(plan)
    lines = tile_lines(plan, ti)
    own = sp.csr_matrix(m).indices[m.indptr[row]:m.indptr[row + 1]]
    return {"none": np.zeros(n, dtype=bool), "all": np.ones(n, dtype=bool),
            "line 0 only": bits_of(lines[0], n), "last line only": bits_of(lines[-1], n),
            "middle line only": bits_of(lines[len(lines) // 2], n),
            "every 64th": np.arange(n) % 64 == 0, "not the row's own": ~bits_of(own, n)}
