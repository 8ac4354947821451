"""The graphs, the case matrix and the exact numpy restatements the graph set-up tests share (tests/test_plan_build_gpu.py,
tests/test_adj_build_gpu.py on the device; tests/test_graph_build_cpu.py checks the cases themselves and the host forms). Nothing
here calls a project kernel. The tier ladders are slab_model's; everything compares bit for bit."""
import functools

import numpy as np
import torch

import slab_model as sm

# ----------------------------------------------------------------------------------------------------------- plan cases
PLAN_T = (32, 4)                       # 4: wave rows shorter than G
PLAN_G = (1, 2, 4, 8, 16, 32, 64)      # lane groups per wave: d = 256 .. 4 geometries
PLAN_KINDS = ("ladder", "flat", "long")
PLAN_CASES = [(T, G, kind) for T in PLAN_T for G in PLAN_G for kind in PLAN_KINDS]
SPLIT_LADDERS = ((4, 8), (32, 64))     # these also run side_split None / 0 / 1 / n
SPLITS = ("none", "0", "1", "n")
ROWS_FROM_LADDERS = ((4, 8), (32, 16))
ROWS_FROM_KINDS = ("one", "between long rows", "last named", "n - 1")
# one geometry (d, w, gs) of test_slab_hop_gpu.GEOMS per G: 64 / ((d / w / gs) (w / 4)) = G
HOP_GEOMS = {1: (256, 32, 1), 2: (128, 32, 1), 4: (64, 32, 1), 8: (32, 32, 1), 16: (16, 16, 1), 32: (8, 8, 1), 64: (4, 4, 1)}


def ladder_matrix(kind, T, G):
    return {"ladder": lambda: sm.tier_ladder(T, G)[0], "flat": lambda: sm.tier_ladder_flat(T, G), "long": lambda: sm.tier_ladder_long(T, G)}[kind]()


def default_split(m):
    """n // 3 for the square ladders, None for `long` (a few dozen rows over many sources)."""
    return m.shape[0] // 3 if m.shape[0] == m.shape[1] else None


def split_value(m, name):
    return {"none": None, "0": 0, "1": 1, "n": m.shape[0]}[name]


def rows_from_value(T, G, name):
    """rows_from of the (T, G) ladder: 1; strictly between two of the named rows above T; the last named row; n - 1 (only the empty
    last row is left)."""
    m, named = sm.tier_ladder(T, G)
    long_named = sorted(r for r, n in named.items() if n > T)
    mid = long_named[len(long_named) // 2]          # named long rows on both sides of it: some leave the plan, some stay
    assert long_named[0] < mid < long_named[-1]
    return {"one": 1, "between long rows": mid, "last named": max(named), "n - 1": m.shape[0] - 1}[name]


def equal_rows_graph(n, T, seed=5):
    """n rows of exactly T entries each: the sort has nothing but the row number (and the side) to go by."""
    return sm._from_lengths([T] * n, max(n, T + 3), seed)


def one_segmented_row(T, G, seed=6):
    """One row of T2 + 1 entries: a single segmented row and nothing else."""
    T2 = sm.tiers(T, G)[1]
    return sm._from_lengths([T2 + 1], T2 + 9, seed)


def plans_equal(host, devp):
    """The device-built plan is the host-built one: counts, every array with dtype and shape, every non-pointer descriptor field."""
    assert (host.n_rows, host.n_src, host.nnz, host.n_seg, host.n_long, host.n_w1, host.n_w4, host.n_tiles, host.tile_groups,
            host.sell_entries, host.sell_seg_entries) == (devp.n_rows, devp.n_src, devp.nnz, devp.n_seg, devp.n_long, devp.n_w1, devp.n_w4,
                                                          devp.n_tiles, devp.tile_groups, devp.sell_entries, devp.sell_seg_entries)
    for k in ("long_rows", "long_seg_ptr", "long_index", "tile_off", "tile_len", "tile_dst", "tile_long", "tile_col", "tile_val", "rowptr",
              "csr_col", "csr_val"):
        a, b = host.t[k], devp.t[k]
        if a.device != b.device:
            a, b = a.cpu(), b.cpu()
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), k
    for f, _ in host.desc._fields_:
        if not f.startswith("d_"):
            assert getattr(host.desc, f) == getattr(devp.desc, f), f


def triples_from(m, rows_from):
    """csr_triples(m) of the rows >= rows_from."""
    r, c, v = sm.csr_triples(m)
    keep = r >= rows_from
    return r[keep], c[keep], v[keep]


def visited_positions(plan):
    """The positions of tile_col / tile_val that hold an entry (walk_tiles' index arithmetic): tile t, group g, step j ->
    tile_off[t] + j G + g for j < tile_len[t, g]."""
    G = plan.tile_groups
    off, glen = sm._h(plan, "tile_off"), sm._h(plan, "tile_len")
    it = np.repeat(np.arange(len(glen)), glen)
    j = np.arange(len(it)) - np.repeat(np.cumsum(glen) - glen, glen)
    return off[it // G] + j * G + it % G


def check_plan_against_matrix(plan, m, T, G, rows_from=0):
    """What a tiered plan of m must be, whoever built it: its tiles hold exactly m's entries of the rows >= rows_from; its counts
    are those of the row lengths; tile_col / tile_val are zero wherever no entry went, the 128 trailing entries included (whole
    64-entry lines are loaded past a tile's end); long_index is -1 below rows_from."""
    lens = sm.row_lengths(m).copy()
    for got, want in zip(sm.walk_tiles(plan), triples_from(m, rows_from)):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    lens_in = lens[rows_from:]
    c = sm.plan_counts(lens_in, T, G)
    assert (plan.n_w1, plan.n_w4, plan.n_seg, plan.n_long) == (c["n_w1"], c["n_w4"], c["n_seg"], c["n_long"])
    tcol, tval = sm._h(plan, "tile_col"), plan.t["tile_val"].cpu().numpy()
    assert len(tcol) == len(tval) == plan.sell_entries + 128 == int(sm._h(plan, "tile_off")[-1]) + 128
    free = np.ones(len(tcol), dtype=bool)
    free[visited_positions(plan)] = False
    assert int((~free).sum()) == int(lens_in.sum())
    assert not tcol[free].any() and not tval.view(np.uint32)[free].any(), "padding that is not zero"
    li = sm._h(plan, "long_index")
    assert np.all(li[:rows_from] == -1) and np.array_equal(li[rows_from:] >= 0, lens_in > T)
    return c


# ----------------------------------------------------------------------------------------------------------- the row key
def row_order(lengths, T, G, side_split, rows_from):
    """elimrec_plan_rows' stage-1 outputs from the row lengths alone. order: rows sorted by (class, side, 2^32 - 1 - length), stable --
    workgroup rows, wave rows, segmented rows (by row number), short rows (the side at or above side_split first), the rows below
    rows_from (by row number). counts: rows per class 0..4, rows above T, segments."""
    n = np.asarray(lengths, dtype=np.int64)
    r = np.arange(len(n), dtype=np.int64)
    T1, T2 = sm.tiers(T, G)
    cls = np.where(n <= T, 3, np.where(n <= T1, 1, np.where(n <= T2, 0, 2)))
    cls = np.where(r < rows_from, 4, cls)
    side = ((cls == 3) & (r < (-1 if side_split is None else side_split))).astype(np.int64)
    sec = np.where((cls == 2) | (cls == 4), 0, 2 ** 32 - 1 - n)
    order = np.lexsort((r, sec, side, cls))
    live = cls != 4
    counts = [int((cls == k).sum()) for k in range(5)] + [int((live & (n > T)).sum()), int(np.where(cls == 2, (n + T - 1) // T, 0).sum())]
    return order.astype(np.int32), np.asarray(counts, dtype=np.int64)


def plan_row_order(plan, n_rows, rows_from):
    """The same concatenation read off a finished plan (either builder): the rows of its workgroup tiles, wave tiles, the segmented
    rows by row number, the short rows in tile order, the rows below rows_from."""
    G = plan.tile_groups
    t1, tseg, tfin, n_tiles = sm.tile_bases(plan)
    dst = sm._h(plan, "tile_dst").reshape(-1, G)
    w4 = dst[0:t1:4, 0]
    w1 = dst[t1:t1 + plan.n_w1, 0]
    long_rows, seg_ptr = sm._h(plan, "long_rows")[:plan.n_long], sm._h(plan, "long_seg_ptr")
    split = long_rows[np.diff(seg_ptr) > 0] if plan.n_long else np.zeros(0, np.int64)
    short = dst[tfin:].reshape(-1)
    short = short[short >= 0]
    return np.concatenate([w4, w1, split, short, np.arange(rows_from)]).astype(np.int32)


# ----------------------------------------------------------------------------------------------------------- adjacency cases
ADJ_TYPES = ("pre", "plain", "gcmc", "norm", "mean")
LADDER_ADJ = (32, 8)


@functools.lru_cache(maxsize=None)
def bipartite_ladder():
    """(users, items, U, I, lens): the interactions of R = the (32, 8) ladder's row lengths over big_row + 37 items -- the user
    degrees sit on every tier boundary of a (T, G) = (32, 8) plan of the adjacency."""
    T, G = LADDER_ADJ
    lens, _ = sm._ladder_lengths(T, G)
    R = sm._from_lengths(lens, sm.big_row(T, G) + 37, 977).tocoo()
    return R.row.astype(np.int64), R.col.astype(np.int64), R.shape[0], R.shape[1], np.asarray(lens, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def adj_cases():
    """name -> (users, items, U, I): unique pairs, in no particular order."""
    i64 = lambda a: np.asarray(a, dtype=np.int64)
    rng = np.random.RandomState(11)
    cases = {"no interactions 1 x 1": (i64([]), i64([]), 1, 1), "no interactions 3 x 5": (i64([]), i64([]), 3, 5),
             "one interaction": (i64([1]), i64([2]), 3, 4),
             "one user, all 300 items": (np.zeros(300, np.int64), rng.permutation(300).astype(np.int64), 1, 300),
             "one item, all 300 users": (rng.permutation(300).astype(np.int64), np.zeros(300, np.int64), 300, 1),
             "complete 3 x 5": (np.repeat(np.arange(3), 5).astype(np.int64), np.tile(np.arange(5), 3).astype(np.int64), 3, 5)}
    # first and last user, first and last item isolated: empty leading / trailing rows of both blocks, the row search at 0 and N
    pairs = np.unique(np.stack([rng.randint(1, 8, 40), rng.randint(1, 11, 40)], 1), axis=0)
    pairs = pairs[rng.permutation(len(pairs))]
    cases["isolated ends 9 x 12"] = (pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64), 9, 12)
    # N = 70 000, every interacting node's id above 65 536 (users from 65 600 on, item nodes are U + i)
    U, I = 66000, 4000
    pairs = np.unique(np.stack([rng.randint(65600, U, 2100), rng.randint(0, I, 2100)], 1), axis=0)
    pairs = pairs[rng.permutation(len(pairs))]
    cases["ids above 65 536"] = (pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64), U, I)
    u, i, U, I, _ = bipartite_ladder()
    p = rng.permutation(len(u))
    cases["bipartite ladder"] = (u[p], i[p], U, I)
    return cases


def duplicate_lists():
    """name -> (users, items, U, I): valid lists but for ONE pair that appears twice."""
    rng = np.random.RandomState(12)
    U, I = 50, 70
    pairs = np.unique(np.stack([rng.randint(0, U, 900), rng.randint(0, I, 900)], 1), axis=0)
    pairs = pairs[rng.permutation(len(pairs))]
    first = np.concatenate([pairs[:1], pairs])
    last = np.concatenate([pairs, pairs[-1:]])
    far = np.concatenate([pairs[:700], pairs[3:4], pairs[700:]])
    return {k: (v[:, 0].astype(np.int64), v[:, 1].astype(np.int64), U, I) for k, v in (("first two", first), ("last two", last), ("far apart", far))}
