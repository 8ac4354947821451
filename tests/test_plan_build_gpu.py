"""The device-side wave-tile plan (csrc/plan.hip: elimrec_plan_rows / _tiles / _scatter through slab.SellPlan.on_device) on the tier
ladders of tests/slab_model.py, and the layout conversion every slab test uses as plumbing (elimrec_slab_from_rows / _to_rows).

The host form slab.SellPlan(m, tiered=True) is the definition: the device plan must be it bit for bit -- counts, every array with
dtype and shape, every non-pointer descriptor field -- at every lane-group count G = 1 .. 64, thresholds 32 and 4 (wave rows shorter
than G), graphs with a row on and next to every tier boundary, with no long rows, with long rows only, for plans of the rows from a
row on, and on degenerate graphs. Independently of the host builder the device plan is walked against its matrix
(graph_build_cases.check_plan_against_matrix). One test calls the three entry points with guard words round every output buffer.
Every comparison is exact. Needs a GPU: `-m gpu`."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import graph_build_cases as gc
import slab_model as sm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
GUARD = 64
_HOST, _CSR = {}, {}


def _slab():
    from elimrec_amd import slab
    return slab


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).to(DEV)


def _csr(m):
    """The matrix's CSR on the device as on_device takes it, uploaded once per session."""
    if id(m) not in _CSR:
        _CSR[id(m)] = (m, _t(m.indptr, np.int64), _t(m.indices, np.int32), _t(m.data, np.float32))
    return _CSR[id(m)][1:]


def _host(m, T, G, split, rows_from=0):
    """The host-built plan on the device, built once per session."""
    key = (id(m), T, G, split, rows_from)
    if key not in _HOST:
        _HOST[key] = (m, _slab().SellPlan(m, DEV, threshold=T, side_split=split, tiered=True, ipw=G, rows_from=rows_from))
    return _HOST[key][1]


def _device(m, T, G, split, rows_from=0, share=None):
    rp, col, val = _csr(m)
    return _slab().SellPlan.on_device(rp, col, val, m.shape[1], threshold=T, side_split=split, ipw=G, rows_from=rows_from, share=share)


def _same_tiles(a, b):
    for k in ("tile_off", "tile_len", "tile_dst", "tile_long", "tile_col", "tile_val", "long_rows", "long_seg_ptr", "long_index"):
        assert torch.equal(a.t[k], b.t[k]), k


# ----------------------------------------------------------------------------------------------------------- the ladders
@pytest.mark.parametrize("T,G,kind", gc.PLAN_CASES)
def test_device_plan_is_the_host_plan_on_the_tier_ladders(T, G, kind):
    m = gc.ladder_matrix(kind, T, G)
    split = gc.default_split(m)
    devp = _device(m, T, G, split)
    gc.plans_equal(_host(m, T, G, split), devp)
    gc.check_plan_against_matrix(devp, m, T, G)


@pytest.mark.parametrize("T,G", gc.SPLIT_LADDERS)
def test_side_split_none_zero_one_and_n(T, G):
    """side_split = 0 and = n put every short row on one side: the key's side bit is constant and the plan is that of side_split =
    None, whose short rows go by descending length alone."""
    m, _ = sm.tier_ladder(T, G)
    plans = {}
    for name in gc.SPLITS:
        split = gc.split_value(m, name)
        plans[name] = _device(m, T, G, split)
        gc.plans_equal(_host(m, T, G, split), plans[name])
        gc.check_plan_against_matrix(plans[name], m, T, G)
    _same_tiles(plans["0"], plans["none"])
    _same_tiles(plans["n"], plans["none"])
    assert not torch.equal(plans["1"].t["tile_dst"], plans["none"].t["tile_dst"])
    lens = sm.row_lengths(m)
    short = gc.plan_row_order(plans["n"], m.shape[0], 0)[-int((lens <= T).sum()):]
    assert np.array_equal(short, np.nonzero(lens <= T)[0][np.argsort(-lens[lens <= T], kind="stable")])


@pytest.mark.parametrize("T,G", gc.ROWS_FROM_LADDERS)
@pytest.mark.parametrize("which", gc.ROWS_FROM_KINDS)
def test_plan_of_the_rows_from_a_row_on(T, G, which):
    """rows_from (the window sweep's item-row plan): the rows below take no part -- no tile, long_index -1 --, also where that cuts
    between the long rows or leaves the empty last row alone; with share= the CSR tensors are the full plan's own."""
    m, _ = sm.tier_ladder(T, G)
    split = gc.default_split(m)
    rf = gc.rows_from_value(T, G, which)
    share = _device(m, T, G, split) if which == "between long rows" else None
    devp = _device(m, T, G, split, rows_from=rf, share=share)
    gc.plans_equal(_host(m, T, G, split, rf), devp)
    gc.check_plan_against_matrix(devp, m, T, G, rows_from=rf)
    assert bool((devp.t["long_index"][:rf] == -1).all())
    if share is not None:
        assert devp.shared == ("rowptr", "csr_col", "csr_val") and all(devp.t[k] is share.t[k] for k in devp.shared)
        assert all(getattr(devp.desc, "d_" + k) == share.t[k].data_ptr() for k in devp.shared)
    else:
        assert devp.shared == ()


# ----------------------------------------------------------------------------------------------------------- degenerate graphs
def _both(m, T, G, split):
    slab = _slab()
    host = slab.SellPlan(m, DEV, threshold=T, side_split=split, tiered=True, ipw=G)
    devp = slab.SellPlan.on_device(_t(m.indptr, np.int64), _t(m.indices, np.int32), _t(m.data, np.float32), m.shape[1], threshold=T,
                                   side_split=split, ipw=G)
    gc.plans_equal(host, devp)
    c = gc.check_plan_against_matrix(devp, m, T, G)
    return host, devp, c


def test_a_graph_of_empty_rows():
    """csr_matrix((40, 40)) at T = 4, G = 8: eight tiles of empty rows. Both builders give tile_kmax = 1 (the host form used to give
    0): tile_kmax is the y extent of tile_ballot_kernel's grid and the row stride of the masked hop's bit words, and
    elimrec_slab_hop / elimrec_slab_source_bits refuse a tiered plan whose tile_kmax is not > 0 -- so 1 is the value the kernels
    need, and a masked hop on either plan runs and writes zeros."""
    slab = _slab()
    m = sp.csr_matrix((40, 40), dtype=np.float32)
    host, devp, _ = _both(m, 4, 8, 13)
    assert (devp.desc.n_tfin, devp.desc.tile_kmax, devp.sell_entries, devp.n_tiles) == (8, 1, 0, 8)
    X = slab.SlabTable(40, 1, 32, DEV).from_rows(torch.randn(40, 32, device=DEV))
    bits = torch.from_numpy(sm.bitmap_words(np.ones(40, dtype=bool))).to(DEV)
    for plan in (host, devp):
        for mask in (None, bits):
            y = X.like()
            y.data.fill_(NAN)
            slab.hop(plan, X, y, gs=1, src_mask=mask)
            assert torch.equal(y.data, torch.zeros_like(y.data))


def test_one_entry_one_segmented_row_and_rows_of_equal_length():
    one = sp.csr_matrix((np.full(1, 0.5, np.float32), ([0], [0])), shape=(1, 1))
    _, devp, c = _both(one, 32, 64, None)
    assert c["n_fin"] == 1 and devp.n_tiles == 4 and devp.sell_entries == 64
    # one row of T2 + 1 entries: nothing but segments, and padding tiles only in the segment stretch
    for T, G in ((32, 8), (4, 2)):
        _, devp, c = _both(gc.one_segmented_row(T, G), T, G, 0)
        d = devp.desc
        assert (c["n_w1"], c["n_w4"], c["n_fin"], c["n_long"]) == (0, 0, 0, 1) and (d.n_t4, d.n_t1, d.n_tfin) == (0, 0, 0)
        assert d.n_tseg * G == -(-c["n_seg"] // (4 * G)) * 4 * G > c["n_seg"]
        assert bool((devp.t["tile_dst"][c["n_seg"]:] == -1).all()) and bool((devp.t["tile_long"][c["n_seg"]:] == 0).all())
    # n rows of exactly T entries: nothing to sort by but the side and the row number -- the sort must be stable
    n, T = 45, 32
    _, devp, _ = _both(gc.equal_rows_graph(n, T), T, 8, 20)
    assert gc.plan_row_order(devp, n, 0).tolist() == list(range(20, n)) + list(range(20))


def test_a_plan_of_no_rows_is_refused_by_both_builders():
    """rows_from = n leaves no row: the host form would return tile arrays of no element (null pointers in the descriptor, which the
    hop refuses), the device form arrays of one. SweepPlan never asks for it -- its rows_from is the user count of a bipartite
    graph -- so both refuse it with the same error."""
    slab = _slab()
    m, _ = sm.tier_ladder(4, 8)
    n = m.shape[0]
    rp, col, val = _csr(m)
    for bad in (n, n + 1, -1):
        with pytest.raises(ValueError, match="rows_from must be in"):
            slab.SellPlan(m, DEV, threshold=4, tiered=True, ipw=8, rows_from=bad)
        with pytest.raises(ValueError, match="rows_from must be in"):
            slab.SellPlan.on_device(rp, col, val, n, threshold=4, ipw=8, rows_from=bad)


# ----------------------------------------------------------------------------------------------------------- guard words
class _Guarded(object):
    """Named buffers, each the interior of a larger tensor with GUARD sentinel elements on either side (-7, NaN for floats)."""

    def __init__(self):
        self.full, self.view, self.fill = {}, {}, {}

    def add(self, name, n, dtype, interior=None):
        fill = NAN if dtype == torch.float32 else -7
        full = torch.full((int(n) + 2 * GUARD,), fill, dtype=dtype, device=DEV)
        self.full[name], self.view[name], self.fill[name] = full, full[GUARD:GUARD + int(n)], fill
        if interior is not None:
            self.view[name].fill_(interior)
        return self.view[name]

    def ptr(self, name):
        return self.view[name].data_ptr()

    @staticmethod
    def _is_fill(t, fill):
        return bool(torch.isnan(t).all()) if fill != fill else bool((t == fill).all())

    def guards_intact(self):
        for name, full in self.full.items():
            assert self._is_fill(full[:GUARD], self.fill[name]) and self._is_fill(full[-GUARD:], self.fill[name]), name

    def untouched(self, names=None):
        for name in names or self.full:
            assert self._is_fill(self.full[name], self.fill[name]), name


def _shape_args(T, G):
    T1, T2 = sm.tiers(T, G)
    return T, T1, T2, T, G


def _stage1_buffers(n):
    b = _Guarded()
    b.add("order", n, torch.int32), b.add("long_rows", n + 1, torch.int32), b.add("long_index", n, torch.int32)
    b.add("long_seg_ptr", n + 1, torch.int32), b.add("counts", 8, torch.int64)
    return b


def _plan_rows(lib, b, rp, n, shape, split, rows_from, ws, ws_bytes):
    from elimrec_amd.ops import _stream
    return lib.elimrec_plan_rows(rp.data_ptr(), n, *shape, split, rows_from, b.ptr("order"), b.ptr("long_rows"), b.ptr("long_index"),
                                 b.ptr("long_seg_ptr"), b.ptr("counts"), ws.data_ptr(), ws_bytes, _stream())


def _stage2_buffers(b, n_tiles, n_tseg, G):
    b.add("tile_off", n_tiles + 1, torch.int64), b.add("tile_len", n_tiles * G, torch.int32), b.add("tile_dst", n_tiles * G, torch.int32)
    b.add("tile_long", max(n_tseg * G, 1), torch.int32), b.add("gb", n_tiles * G, torch.int64), b.add("gs", n_tiles * G, torch.int32)
    b.add("totals", 4, torch.int64)


def _plan_tiles(lib, b, rp, n, shape, split, rows_from, counts, ws, ws_bytes):
    from elimrec_amd.ops import _stream
    n_w4, n_w1, n_split, n_short, _, n_long, n_seg = counts
    return lib.elimrec_plan_tiles(rp.data_ptr(), n, *shape, split, rows_from, b.ptr("order"), b.ptr("long_rows"), b.ptr("long_seg_ptr"),
                                  n_w4, n_w1, n_split, n_short, n_long, n_seg, b.ptr("tile_off"), b.ptr("tile_len"), b.ptr("tile_dst"),
                                  b.ptr("tile_long"), b.ptr("gb"), b.ptr("gs"), b.ptr("totals"), ws.data_ptr(), ws_bytes, _stream())


def test_entry_points_write_inside_their_buffers_and_stage_one_is_the_row_key():
    """The three entry points called as on_device calls them, on the (4, 8) ladder with side_split = n // 3, every output buffer
    between guard words: the guards survive, the interiors are the host plan's arrays (what lies beyond the used part of a buffer
    stays as it was), and the stage-1 outputs on_device drops are right -- `order` is the rows sorted by the key (class, side,
    2^32 - 1 - length), stable, and counts[0:7] the rows per class, the long rows and the segments, both restated in numpy from
    the row lengths."""
    from elimrec_amd import _lib
    from elimrec_amd.ops import _stream
    lib = _lib.load()
    T, G = 4, 8
    m, _ = sm.tier_ladder(T, G)
    n, split = m.shape[0], m.shape[0] // 3
    host = _host(m, T, G, split)
    rp, col, val = _csr(m)
    shape = _shape_args(T, G)
    b = _stage1_buffers(n)
    ws = torch.empty(int(lib.elimrec_plan_workspace(n, 1, 1)), dtype=torch.uint8, device=DEV)
    _lib.check(_plan_rows(lib, b, rp, n, shape, split, 0, ws, ws.numel()), "plan_rows")
    torch.cuda.synchronize()
    b.guards_intact()
    want_order, want_counts = gc.row_order(sm.row_lengths(m), T, G, split, 0)
    counts = b.view["counts"].cpu().numpy()
    assert np.array_equal(counts[:7], want_counts) and counts[7] == -7
    assert np.array_equal(b.view["order"].cpu().numpy(), want_order)
    n_w4, n_w1, n_split, n_short, n_none, n_long, n_seg = (int(x) for x in counts[:7])
    assert (n_w1, n_w4, n_long, n_seg, n_none) == (host.n_w1, host.n_w4, host.n_long, host.n_seg, 0) and min(n_w4, n_w1, n_split, n_short) > 0
    assert torch.equal(b.view["long_index"], host.t["long_index"])
    assert torch.equal(b.view["long_rows"][:n_long], host.t["long_rows"]) and bool((b.view["long_rows"][n_long:] == -7).all())
    assert torch.equal(b.view["long_seg_ptr"][:n_long + 1], host.t["long_seg_ptr"]) and bool((b.view["long_seg_ptr"][n_long + 1:] == -7).all())
    # stage 2
    n_tiles = int(lib.elimrec_plan_tile_count(n_w4, n_w1, n_seg, n_short, G))
    n_tseg = -(-n_seg // (4 * G)) * 4
    assert n_tiles == host.n_tiles and n_tseg == host.desc.n_tseg
    _stage2_buffers(b, n_tiles, n_tseg, G)
    ws2 = torch.empty(int(lib.elimrec_plan_workspace(n, n_seg, n_tiles)), dtype=torch.uint8, device=DEV)
    _lib.check(_plan_tiles(lib, b, rp, n, shape, split, 0, counts[:7].tolist(), ws2, ws2.numel()), "plan_tiles")
    torch.cuda.synchronize()
    b.guards_intact()
    for k in ("tile_off", "tile_len", "tile_dst", "tile_long"):
        assert b.view[k].dtype == host.t[k].dtype and torch.equal(b.view[k], host.t[k]), k
    totals = b.view["totals"].cpu().numpy()
    assert totals.tolist() == [host.sell_entries, host.sell_seg_entries, host.desc.tile_kmax, -7]
    tile = np.arange(n_tiles * G) // G
    assert np.array_equal(b.view["gs"].cpu().numpy(), np.where(tile < 4 * n_w4 + n_w1, G, 1))
    dst, gb = host.t["tile_dst"].cpu().numpy().astype(np.int64), b.view["gb"].cpu().numpy()
    fin = tile >= host.n_tiles - host.desc.n_tfin
    assert np.array_equal(gb[fin], np.where(dst[fin] >= 0, m.indptr[np.maximum(dst[fin], 0)], 0))
    # stage 3: the caller zero-fills tile_col / tile_val [total + 128]
    total = int(totals[0])
    b.add("tile_col", total + 128, torch.int32, interior=0), b.add("tile_val", total + 128, torch.float32, interior=0.0)
    _lib.check(lib.elimrec_plan_scatter(n_tiles, G, b.ptr("tile_off"), b.ptr("gb"), b.ptr("tile_len"), b.ptr("gs"), col.data_ptr(), val.data_ptr(),
                                        b.ptr("tile_col"), b.ptr("tile_val"), _stream()), "plan_scatter")
    torch.cuda.synchronize()
    b.guards_intact()
    assert torch.equal(b.view["tile_col"], host.t["tile_col"])
    assert torch.equal(b.view["tile_val"].view(torch.int32), host.t["tile_val"].view(torch.int32))


def test_entry_points_refuse_bad_calls_and_write_nothing():
    """A workspace one byte short (rows stage, tiles stage), G = 65, T1 < T and n_rows = 0: the library's error, through _lib.check
    a RuntimeError, and not one output element written. Every buffer has the size a launch would need: only the stated size or
    shape is wrong."""
    from elimrec_amd import _lib
    lib = _lib.load()
    T, G = 4, 8
    m, _ = sm.tier_ladder(T, G)
    n, split = m.shape[0], m.shape[0] // 3
    rp, _, _ = _csr(m)
    T_, T1, T2, TS, G_ = _shape_args(T, G)
    ws = torch.empty(int(lib.elimrec_plan_workspace(n, 1, 1)), dtype=torch.uint8, device=DEV)
    for what, n_rows, shape, ws_bytes, rc_want in (("workspace", n, (T, T1, T2, TS, G), ws.numel() - 1, 10003),
                                                   ("G = 65", n, (T, T1, T2, TS, 65), ws.numel(), 10001),
                                                   ("T1 < T", n, (T, T - 1, T2, TS, G), ws.numel(), 10001),
                                                   ("n_rows = 0", 0, (T, T1, T2, TS, G), ws.numel(), 10001)):
        b = _stage1_buffers(n)
        rc = _plan_rows(lib, b, rp, n_rows, shape, split, 0, ws, ws_bytes)
        assert rc == rc_want, what
        with pytest.raises(RuntimeError, match="plan_rows"):
            _lib.check(rc, "plan_rows")
        torch.cuda.synchronize()
        b.untouched()
    # the tiles stage, after a good rows stage
    b = _stage1_buffers(n)
    _lib.check(_plan_rows(lib, b, rp, n, (T, T1, T2, TS, G), split, 0, ws, ws.numel()), "plan_rows")
    counts = b.view["counts"].cpu().numpy()[:7].tolist()
    n_w4, n_w1, _, n_short, _, _, n_seg = counts
    n_tiles = int(lib.elimrec_plan_tile_count(n_w4, n_w1, n_seg, n_short, G))
    _stage2_buffers(b, n_tiles, -(-n_seg // (4 * G)) * 4, G)
    need = int(lib.elimrec_plan_workspace(n, n_seg, n_tiles))
    ws2 = torch.empty(need, dtype=torch.uint8, device=DEV)
    rc = _plan_tiles(lib, b, rp, n, (T, T1, T2, TS, G), split, 0, counts, ws2, need - 1)
    assert rc == 10003
    with pytest.raises(RuntimeError, match="plan_tiles"):
        _lib.check(rc, "plan_tiles")
    torch.cuda.synchronize()
    b.untouched(("tile_off", "tile_len", "tile_dst", "tile_long", "gb", "gs", "totals"))
    b.guards_intact()


# ----------------------------------------------------------------------------------------------------------- a hop per G
@pytest.mark.parametrize("G", gc.PLAN_G)
def test_hop_on_the_device_plan_is_the_hop_on_the_host_plan(G):
    """slab.hop on the device-built plan of the (32, G) ladder, at a table geometry with 64 / LPR = G, equals the hop on the
    host-built plan bit for bit (which tests/test_slab_hop_gpu.py holds to float64). Random input, outputs pre-filled with NaN."""
    slab = _slab()
    d, w, gs = gc.HOP_GEOMS[G]
    m, _ = sm.tier_ladder(32, G)
    n, split = m.shape[0], gc.default_split(m)
    host, devp = _host(m, 32, G, split), _device(m, 32, G, split)
    X = torch.randn(n, d, generator=torch.Generator().manual_seed(G)).to(DEV)
    xs = slab.SlabTable(n, d // w, w, DEV).from_rows(X)
    ya, yb = xs.like(), xs.like()
    ya.data.fill_(NAN), yb.data.fill_(NAN)
    slab.hop(host, xs, ya, gs=gs)
    slab.hop(devp, xs, yb, gs=gs)
    assert not bool(torch.isnan(ya.data).any()) and torch.equal(ya.data, yb.data)


# ----------------------------------------------------------------------------------------------------------- layout conversion
@pytest.mark.parametrize("ns,w", [(1, 4), (2, 32), (8, 8), (3, 32), (1, 64)])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_layout_conversion_is_the_layout_model(n, ns, w):
    """elimrec_slab_from_rows on a column window of a wider, NaN-filled row-major tensor is slab_model.slab_layout of the window bit
    for bit; elimrec_slab_to_rows writes exactly the window of a sentinel-filled wider tensor. A window that does not start on a
    multiple of 4 columns, or a leading dimension that is no multiple of 4, is refused and nothing is written."""
    slab = _slab()
    cols = ns * w
    SENT = -7.25
    for col0 in (0, 4, 12):
        ld = col0 + cols + 8
        W = np.random.RandomState(n + 7 * ns + w + col0).randn(n, cols).astype(np.float32)
        wide = torch.full((n, ld), NAN, device=DEV)
        wide[:, col0:col0 + cols] = torch.from_numpy(W).to(DEV)
        assert wide.stride(0) > cols
        t = slab.SlabTable(n, ns, w, DEV)
        t.data.fill_(NAN)
        t.from_rows(wide, col0=col0)
        assert np.array_equal(t.data.cpu().numpy().view(np.uint32), sm.slab_layout(W, ns, w).view(np.uint32))
        out = torch.full((n, ld), SENT, device=DEV)
        t.to_rows(out, col0=col0)
        got = out.cpu().numpy()
        assert np.array_equal(got[:, col0:col0 + cols].view(np.uint32), W.view(np.uint32))
        assert np.array_equal(got[:, col0:col0 + cols], sm.slab_dense(sm.slab_layout(W, ns, w), n, ns, w))
        assert np.all(got[:, :col0] == SENT) and np.all(got[:, col0 + cols:] == SENT)
    # refused: col0 = 2; ld % 4 != 0 (buffers large enough for either launch)
    wide = torch.full((n, cols + 10), NAN, device=DEV)
    out = torch.full((n, cols + 10), SENT, device=DEV)
    t = slab.SlabTable(n, ns, w, DEV)
    t.data.fill_(SENT)
    with pytest.raises(RuntimeError, match="slab_from_rows"):
        t.from_rows(wide, col0=2)
    with pytest.raises(RuntimeError, match="slab_to_rows"):
        t.to_rows(out, col0=2)
    assert wide.stride(0) % 4 != 0
    with pytest.raises(RuntimeError, match="slab_from_rows"):
        t.from_rows(wide, col0=0)
    with pytest.raises(RuntimeError, match="slab_to_rows"):
        t.to_rows(out, col0=0)
    torch.cuda.synchronize()
    assert bool((t.data == SENT).all()) and bool((out == SENT).all())
