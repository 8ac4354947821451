"""The graph set-up tests' cases and host forms, without a GPU: the case matrix of tests/test_plan_build_gpu.py and
tests/test_adj_build_gpu.py holds what it must; the host plan (slab.SellPlan(..., device="cpu"), the definition csrc/plan.hip
reproduces) passes the same builder-independent checks the device plan is put to; the numpy restatement of plan.hip's row key gives
the host plan's row order; and the cases tell a broken key, quarter length, padding branch or degree apart. All exact."""
import numpy as np
import pytest
import scipy.sparse as sp

import graph_build_cases as gc
import slab_model as sm

_HOST = {}


def _host(m, T, G, split, rows_from=0):
    from elimrec_amd import slab
    key = (id(m), T, G, split, rows_from)
    if key not in _HOST:
        _HOST[key] = (m, slab.SellPlan(m, "cpu", threshold=T, side_split=split, tiered=True, ipw=G, rows_from=rows_from))
    return _HOST[key][1]


def test_cases_cover_the_issue():
    import test_slab_hop_gpu as hop_tests
    assert {c[0] for c in gc.PLAN_CASES} == {32, 4} and {c[1] for c in gc.PLAN_CASES} == {1, 2, 4, 8, 16, 32, 64}
    assert {c[2] for c in gc.PLAN_CASES} == {"ladder", "flat", "long"} and len(set(gc.PLAN_CASES)) == 2 * 7 * 3
    for T in gc.PLAN_T:
        for G in gc.PLAN_G:
            m, named = sm.tier_ladder(T, G)
            lens = sm.row_lengths(m)
            c = sm.plan_counts(lens, T, G)
            assert c["n_w1"] % 4 and c["n_w4"] % 4 and c["n_seg"] % (4 * G) and c["n_fin"] % (4 * G), (T, G, c)
            T1, T2 = sm.tiers(T, G)
            assert {0, T, T + 1, T1, T1 + 1, T2, T2 + 1} <= set(named.values()) and lens[0] == 0 and lens[-1] == 0
            flat, lng = sm.row_lengths(sm.tier_ladder_flat(T, G)), sm.row_lengths(sm.tier_ladder_long(T, G))
            assert flat.max() <= T and lng.min() > T and sm.plan_counts(flat, T, G)["n_long"] == 0 and sm.plan_counts(lng, T, G)["n_fin"] == 0
    m, _ = sm.tier_ladder(32, 64)
    assert m.shape == (18469, 18469) and m.nnz == 132211
    assert set(gc.SPLIT_LADDERS) == {(4, 8), (32, 64)} and set(gc.ROWS_FROM_LADDERS) == {(4, 8), (32, 16)}
    for T, G in gc.ROWS_FROM_LADDERS:
        m, named = sm.tier_ladder(T, G)
        lens = sm.row_lengths(m)
        v = {k: gc.rows_from_value(T, G, k) for k in gc.ROWS_FROM_KINDS}
        assert v["one"] == 1 and v["last named"] == max(named) and v["n - 1"] == m.shape[0] - 1 and lens[-1] == 0
        b = v["between long rows"]
        assert (lens[:b] > T).any() and (lens[b:] > T).any()
    assert set(gc.HOP_GEOMS) == set(gc.PLAN_G)
    for G, (d, w, gs) in gc.HOP_GEOMS.items():
        assert (d, w, gs) in hop_tests.GEOMS and 64 // ((d // w // gs) * (w // 4)) == G


@pytest.mark.parametrize("T,G,kind", gc.PLAN_CASES)
def test_host_plan_holds_its_matrix_and_the_row_key_orders_it(T, G, kind):
    """The host plan against its matrix by the checks the device plan gets (walk_tiles = csr_triples, counts, zero padding), and
    row_order -- plan.hip's (class, side, 2^32 - 1 - length) key restated in numpy -- against the row order read off the plan."""
    m = gc.ladder_matrix(kind, T, G)
    split = gc.default_split(m)
    plan = _host(m, T, G, split)
    c = gc.check_plan_against_matrix(plan, m, T, G)
    order, counts = gc.row_order(sm.row_lengths(m), T, G, split, 0)
    assert np.array_equal(order, gc.plan_row_order(plan, m.shape[0], 0))
    assert counts.tolist() == [c["n_w4"], c["n_w1"], int((sm.tier_of(sm.row_lengths(m), T, G) == sm.SEGMENTED).sum()), c["n_fin"], 0,
                               c["n_long"], c["n_seg"]]
    assert plan.desc.tile_kmax >= 1


@pytest.mark.parametrize("T,G", gc.SPLIT_LADDERS)
def test_side_split_at_the_ends_is_one_side(T, G):
    """side_split = 0: every short row is at or above it -- the order of side_split = None; side_split = n: every short row is
    below it -- the side bit is constant again and the order is the pure descending-length one. 1 and n // 3 are real splits."""
    m, _ = sm.tier_ladder(T, G)
    n, lens = m.shape[0], sm.row_lengths(m)
    orders = {}
    for name in gc.SPLITS:
        split = gc.split_value(m, name)
        plan = _host(m, T, G, split)
        gc.check_plan_against_matrix(plan, m, T, G)
        orders[name] = gc.plan_row_order(plan, n, 0)
        assert np.array_equal(orders[name], gc.row_order(lens, T, G, split, 0)[0])
    assert np.array_equal(orders["0"], orders["none"]) and np.array_equal(orders["n"], orders["none"])
    assert not np.array_equal(orders["1"], orders["none"])
    short = orders["none"][-int((lens <= T).sum()):]
    assert np.array_equal(short, np.nonzero(lens <= T)[0][np.argsort(-lens[lens <= T], kind="stable")])


@pytest.mark.parametrize("T,G", gc.ROWS_FROM_LADDERS)
@pytest.mark.parametrize("which", gc.ROWS_FROM_KINDS)
def test_host_plan_of_the_rows_from_a_row_on(T, G, which):
    m, _ = sm.tier_ladder(T, G)
    rf = gc.rows_from_value(T, G, which)
    plan = _host(m, T, G, gc.default_split(m), rf)
    gc.check_plan_against_matrix(plan, m, T, G, rows_from=rf)
    order, counts = gc.row_order(sm.row_lengths(m), T, G, gc.default_split(m), rf)
    assert np.array_equal(order, gc.plan_row_order(plan, m.shape[0], rf)) and counts[4] == rf
    if which == "n - 1":
        assert plan.n_long == 0 and plan.sell_entries == 0 and plan.desc.n_tfin == 4 and plan.desc.tile_kmax == 1


def test_degenerate_graphs_on_the_host():
    """Tiles of empty rows only: tile_kmax is 1, not 0 -- it is the ballot launch's grid.y and the stride of the masked hop's bit
    words, and elimrec_slab_hop refuses a tiered plan without it. A plan of no rows at all is refused."""
    from elimrec_amd import slab
    m = sp.csr_matrix((40, 40), dtype=np.float32)
    plan = slab.SellPlan(m, "cpu", threshold=4, side_split=13, tiered=True, ipw=8)
    assert (plan.desc.n_tfin, plan.desc.tile_kmax, plan.sell_entries, plan.n_tiles) == (8, 1, 0, 8)
    gc.check_plan_against_matrix(plan, m, 4, 8)
    one = sp.csr_matrix((np.ones(1, np.float32), ([0], [0])), shape=(1, 1))
    gc.check_plan_against_matrix(slab.SellPlan(one, "cpu", threshold=32, tiered=True, ipw=64), one, 32, 64)
    for T, G in ((32, 8), (4, 2)):
        seg = gc.one_segmented_row(T, G)
        plan = slab.SellPlan(seg, "cpu", threshold=T, side_split=0, tiered=True, ipw=G)
        c = gc.check_plan_against_matrix(plan, seg, T, G)
        assert (c["n_w1"], c["n_w4"], c["n_fin"], c["n_long"]) == (0, 0, 0, 1)
        d = plan.desc
        assert (d.n_t4, d.n_t1, d.n_tfin) == (0, 0, 0) and d.n_tseg * G == -(-c["n_seg"] // (4 * G)) * 4 * G > c["n_seg"]
    n, T = 45, 32
    eq = gc.equal_rows_graph(n, T)
    plan = slab.SellPlan(eq, "cpu", threshold=T, side_split=20, tiered=True, ipw=8)
    gc.check_plan_against_matrix(plan, eq, T, 8)
    assert gc.plan_row_order(plan, n, 0).tolist() == list(range(20, n)) + list(range(20))
    m, _ = sm.tier_ladder(4, 8)
    for bad in (m.shape[0], m.shape[0] + 1, -1):
        with pytest.raises(ValueError, match="rows_from"):
            slab.SellPlan(m, "cpu", threshold=4, tiered=True, ipw=8, rows_from=bad)


@pytest.mark.parametrize("T,G,kind", gc.PLAN_CASES)
def test_plan_workspace_holds_the_tiles_stage(T, G, kind):
    """elimrec_plan_workspace (a host function) covers what elimrec_plan_tiles carves out of it -- the segments' first positions
    (int64), six int32 arrays per segment, an int64 per tile, each rounded up to 256 bytes -- with the sort / scan scratch and the
    spare kilobyte still behind it. The `long` ladders have some twenty rows and up to 12 295 segments: sized by the rows alone (as
    it once was) the workspace ended inside the segment arrays."""
    from elimrec_amd import _lib
    lib = _lib.load()
    lens = sm.row_lengths(gc.ladder_matrix(kind, T, G))
    c = sm.plan_counts(lens, T, G)
    n_tiles = int(lib.elimrec_plan_tile_count(c["n_w4"], c["n_w1"], c["n_seg"], c["n_fin"], G))
    assert n_tiles == 4 * c["n_w4"] + -(-c["n_w1"] // 4) * 4 + (-(-c["n_seg"] // (4 * G)) + -(-c["n_fin"] // (4 * G))) * 4
    up = lambda b: -(-b // 256) * 256
    ns, n = max(c["n_seg"], 1), len(lens)
    tiles_stage = up(8 * ns) + 6 * up(4 * ns) + up(8 * max(n_tiles, 1))
    rows_stage = 2 * up(8 * n) + 5 * up(4 * n)
    ws = int(lib.elimrec_plan_workspace(n, c["n_seg"], n_tiles))
    assert ws >= max(tiles_stage, rows_stage) + 1024 and int(lib.elimrec_plan_workspace(n, 1, 1)) >= rows_stage + 1024
    if kind == "long":
        assert tiles_stage > rows_stage


def test_the_cases_tell_broken_builders_apart():
    """Restated on the host: what each of these mistakes in csrc/plan.hip / csrc/adj.hip would build differs from the definition on a
    case the device tests compare bit for bit."""
    # the side bit of the row key: without it the (4, 8) ladder's short rows come in another order
    m, _ = sm.tier_ladder(4, 8)
    lens, n = sm.row_lengths(m), m.shape[0]
    assert not np.array_equal(gc.row_order(lens, 4, 8, n // 3, 0)[0], gc.row_order(lens, 4, 8, None, 0)[0])
    for T in gc.PLAN_T:
        for G in gc.PLAN_G:
            lens = sm.row_lengths(sm.tier_ladder(T, G)[0])
            t = sm.tier_of(lens, T, G)
            # quarters padded to a multiple of G: some workgroup row's plain quarter is none (at G = 1 every length is)
            assert G == 1 or (((lens[t == sm.WORKGROUP] + 3) // 4) % G != 0).any()
            # padding slots behind the last segment and the last short row
            c = sm.plan_counts(lens, T, G)
            assert c["n_seg"] % (4 * G) and c["n_fin"] % (4 * G)
    # degrees without the diagonal: d + 1 and d + 2 index different table entries wherever a row has a neighbour
    from elimrec_amd.adjacency import _pow_table
    from elimrec_amd.model import create_adj_mat
    tab = _pow_table("norm", 5)
    assert len(tab) == 7 and len(set(tab[1:].tolist())) == 6
    u, i, U, I = gc.adj_cases()["complete 3 x 5"]
    a = create_adj_mat(u, i, U, I, "norm")
    assert np.array_equal(a.data[:6].view(np.uint32), np.full(6, tab[5 + 1]).view(np.uint32))


def test_adjacency_cases_are_what_they_claim():
    from elimrec_amd.model import create_adj_mat
    cases = gc.adj_cases()
    assert len(cases) == 9
    for name, (u, i, U, I) in cases.items():
        assert len(u) == len(i) and (len(u) == 0 or (u.min() >= 0 and u.max() < U and i.min() >= 0 and i.max() < I)), name
        assert len(np.unique(u * I + i)) == len(u), name
    deg = lambda name: np.diff(create_adj_mat(*cases[name], "plain").indptr)
    assert deg("one user, all 300 items").tolist() == [300] + [1] * 300 and deg("one item, all 300 users").tolist() == [1] * 300 + [300]
    assert deg("complete 3 x 5").tolist() == [5] * 3 + [3] * 5 and deg("one interaction").sum() == 2
    d = deg("isolated ends 9 x 12")
    assert d[0] == d[8] == d[9] == d[20] == 0 and d[1:8].min() > 0
    u, i, U, I = cases["ids above 65 536"]
    d = deg("ids above 65 536")
    assert U + I == 70000 and 1900 <= len(u) <= 2100 and np.nonzero(d)[0].min() > 65536
    # the bipartite ladder: the adjacency's user rows have the ladder's lengths (+ the diagonal for norm / mean)
    u, i, U, I, lens = gc.bipartite_ladder()
    T, G = gc.LADDER_ADJ
    assert U == len(lens) and I == sm.big_row(T, G) + 37 and sm._ladder_lengths(T, G)[0] == lens.tolist()
    for adj_type, extra in (("plain", 0), ("pre", 0), ("gcmc", 0), ("norm", 1), ("mean", 1)):
        a = create_adj_mat(*cases["bipartite ladder"], adj_type)
        assert np.array_equal(np.diff(a.indptr)[:U], lens + extra), adj_type
    c = sm.plan_counts(lens, T, G)
    assert min(c.values()) > 0
    for name, (u, i, U, I) in gc.duplicate_lists().items():
        code = u * I + i
        uniq, cnt = np.unique(code, return_counts=True)
        assert sorted(cnt.tolist())[-2:] == [1, 2], name
        where = np.nonzero(code == uniq[cnt == 2][0])[0].tolist()
        assert where == {"first two": [0, 1], "last two": [len(u) - 2, len(u) - 1], "far apart": [3, 700]}[name]
