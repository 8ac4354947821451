"""The layer means at listed rows (csrc/rows_args.h: rows_piece under slab_rows_kernel<LR>) and the wide form (csrc/wide.hip)
against the float64 model of tests/rows_model.py, element by element, on the rows ladder: every length on and next to the 16-wide
groups of the inline hop on both sides of the user / item boundary, and rows of all three upper tiers of the tiered wave-tile plan
the engine runs with (their hop L comes out of the compact table slab.hop(seg_only=True) writes). Calls go through
elimrec_amd.slab; plans, tables and references are built once per session.

Every output starts as NaN. The bound is fp64_tools.assert_close with K = the row's own length + L + 2 (L + 2 where X^L is a
given table) and no absolute floor beyond TINY; what must be the same arithmetic compares bit for bit. The hop that writes the
long-row table takes the geometry's slab groups gs, raised where the hop could not run it or the ladder could not be built:
(256, 32) and (512, 32) go in groups of 32 lanes per row (G = 2), since one lane group per wave leaves a T = 64 plan without a
wave tier (T1 = 64 G) and the hop refuses more than 64 lanes per row. The rows kernel itself takes no gs.
"""
import types

import numpy as np
import pytest
import torch

import rows_model as rm
import slab_model as sm
from fp64_tools import NAN, TINY, all_nan, assert_close, same_bits, tau

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORST = {}          # family -> worst err / tol seen in this session (printed by the last test)

# (d, w, gs); the rows kernel runs LR = min(64, d / 4 rounded up to a power of two) lanes per listed row
GEOMS = [(4, 4, 1), (8, 8, 1), (16, 16, 1), (64, 8, 1), (64, 16, 1), (64, 32, 2), (64, 64, 1), (256, 32, 1), (512, 32, 1)]
LRS = [1, 2, 4, 16, 16, 16, 16, 64, 64]
LMAX = 8
CASES = ([(g, 64, 3) for g in GEOMS] + [(g, 64, L) for g in ((64, 32, 2), (4, 4, 1)) for L in (1, 2, 4, 8)] +
         [((64, 32, 2), 32, 3), ((8, 8, 1), 32, 8), ((256, 32, 1), 32, 1)])
FORM_GEOMS = [(64, 32, 2), (4, 4, 1), (512, 32, 1)]
PAD = -(1 << 30)


def _slab():
    from elimrec_amd import slab
    return slab


def _hop_gs(d, w, gs):
    ns = d // w
    while (ns // gs) * (w // 4) > 32:
        gs *= 2
    return gs


def _close(family, got, ref, scale, K, what):
    g = got.detach().double().cpu()
    tol = tau(K) * scale + TINY
    if isinstance(tol, torch.Tensor) and tol.shape != g.shape:
        tol = tol.expand_as(g)
    fin = torch.isfinite(g) & torch.isfinite(ref)
    if bool(fin.any()):
        WORST[family] = max(WORST.get(family, 0.0), float(((g - ref).abs()[fin] / tol[fin]).max()))
    assert_close(got, ref, scale, K, what)


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def _table(X, ns, w):
    return _slab().SlabTable(X.shape[0], ns, w, DEV).from_rows(X.to(DEV).contiguous())


def _ids(rows):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(rows, dtype=np.int32))).to(DEV)


# ----------------------------------------------------------------------------------------------------------- shared cases
_GEO, _LAYER = {}, {}


def _geo(d, w, gs, T, tiered=True):
    """The ladder of this geometry's lane groups, its plan, LMAX random layer tables (host and device) and the listed rows."""
    key = (d, w, gs, T, tiered)
    if key in _GEO:
        return _GEO[key]
    slab = _slab()
    ns, hgs = d // w, _hop_gs(d, w, gs)
    G = 64 // ((ns // hgs) * (w // 4))
    m, U, named = rm.rows_ladder(T, G)
    N = m.shape[0]
    plan = slab.SellPlan(m, DEV, threshold=T, side_split=U, tiered=tiered, ipw=G)
    lens = sm.row_lengths(m)
    if tiered:
        c = sm.plan_counts(lens, T, G)
        assert (plan.n_w1, plan.n_w4, plan.n_seg, plan.n_long) == (c["n_w1"], c["n_w4"], c["n_seg"], c["n_long"]) and min(c.values()) > 0
    else:
        assert not plan.tiered and plan.n_long == int((lens > T).sum()) > 0
    g = torch.Generator().manual_seed(1000 * d + w + T)
    X = [torch.randn(N, d, generator=g) for _ in range(LMAX)]
    rows = rm.listed_rows(m, U, named, 300, seed=d + T)
    what = "(d %d, w %d, gs %d) T %d%s" % (d, w, gs, T, "" if tiered else " two-launch")
    _GEO[key] = types.SimpleNamespace(key=key, d=d, w=w, ns=ns, hgs=hgs, G=G, T=T, m=m, U=U, named=named, N=N, plan=plan, lens=lens, X=X,
                                      xs=[_table(x, ns, w) for x in X], rows=rows, ids=_ids(rows).view(1, -1), what=what)
    return _GEO[key]


def _layer(c, L):
    """Per (case, L): the compact long-row table and the whole table of hop L (launched once, left unchanged), the float64
    reference at the listed rows, and the inline evaluation's outputs there."""
    key = (c.key, L)
    if key in _LAYER:
        return _LAYER[key]
    slab = _slab()
    long_tab = _nan(c.ns * c.plan.n_long * c.w)
    slab.hop(c.plan, c.xs[L - 1], long_tab, gs=c.hgs, seg_only=True)
    full = c.xs[0].like()
    full.data.fill_(NAN)
    slab.hop(c.plan, c.xs[L - 1], full, gs=c.hgs)
    R = len(c.rows)
    out, nar = _nan(R, c.d), _nan(R, c.d)
    cnt = torch.tensor([R], dtype=torch.int32, device=DEV)
    _rows(c, L, None, long_tab, c.ids, cnt, R, 1, out, nar)
    _LAYER[key] = types.SimpleNamespace(long_tab=long_tab, full=full, ref=rm.rows_ref(c.m, c.X[:L], None, c.rows, c.U), out=out, nar=nar,
                                        cnt=cnt, what="%s L %d" % (c.what, L))
    return _LAYER[key]


def _rows(c, L, last, long_tab, ids, counts, R, n_lists, out0, narrow, by_node=False, layers=None):
    layers = [t.data for t in c.xs[:L]] if layers is None else layers
    _slab().rows(c.plan, c.ns, c.w, L, c.U, layers + [last], long_tab, ids, counts, R, n_lists, out0, narrow, by_node)


def _check(family, out, nar, ref, what, sel=None):
    o, so, n, sn, K = ref if sel is None else tuple(t[sel] for t in ref)
    _close(family, out, o, so, K, what + ": out0")
    _close(family, nar, n, sn, K, what + ": narrow")


def test_geometry_table():
    assert [min(64, 1 << max(0, (d // 4 - 1).bit_length())) for d, _, _ in GEOMS] == LRS
    assert {g for g, T, L in CASES if T == 64 and L == 3} == set(GEOMS)
    for g in ((64, 32, 2), (4, 4, 1)):
        assert {L for gg, T, L in CASES if gg == g and T == 64} == {1, 2, 3, 4, 8}
    assert [_hop_gs(*g) for g in GEOMS] == [1, 1, 1, 1, 1, 2, 1, 2, 4]


# ============================================================================= slab.rows on the tiered plan
@pytest.mark.parametrize("geom,T,L", CASES)
def test_tiered_plan_inline_last_hop(geom, T, L):
    """Hop L inline over the CSR (rows up to T) and out of the seg_only table (all three upper tiers), against float64."""
    c = _geo(*geom, T)
    y = _layer(c, L)
    _check("rows inline", y.out, y.nar, y.ref, y.what)
    li = c.plan.t["long_index"].cpu().numpy()
    for (side, n), r in c.named.items():        # reached by construction, not by chance
        assert c.lens[r] == n and r in c.rows and li[r] == (-1 if n <= T else int((c.lens[:r] > T).sum()))
    R = len(c.rows)
    out, nar = _nan(R, c.d), _nan(R, c.d)
    _rows(c, L, None, y.long_tab, c.ids, y.cnt, R, 1, out, nar)
    assert same_bits(out, y.out) and same_bits(nar, y.nar), y.what + ": second launch differs"


@pytest.mark.parametrize("geom,T,L", CASES)
def test_inline_equals_the_table(geom, T, L):
    """layers[L] = the table slab.hop wrote on the same plan: the bits of the inline evaluation (lazily
    materialised tables are bit-identical to per-step ones), and the float64 bound of X^L taken as an input (K = L + 2)."""
    c = _geo(*geom, T)
    y = _layer(c, L)
    R = len(c.rows)
    out, nar = _nan(R, c.d), _nan(R, c.d)
    _rows(c, L, y.full.data, None, c.ids, None, R, 1, out, nar)
    _check("rows from tables", out, nar, rm.rows_ref(c.m, c.X[:L], y.full.dense().cpu(), c.rows, c.U), y.what + " (X^L given)")
    for name, a, b in (("out0", out, y.out), ("narrow", nar, y.nar)):
        if not same_bits(a, b):
            bad = (a.view(torch.int32) != b.view(torch.int32)).any(1).nonzero().flatten().cpu().numpy()
            raise AssertionError("%s: %s of %d rows differs between the inline hop and the table, lengths %s" % (
                y.what, name, len(bad), sorted(set(c.lens[c.rows[bad]].tolist()))[:12]))


@pytest.mark.parametrize("geom,T,L", CASES)
def test_only_what_is_wanted_is_read(geom, T, L):
    """The long table written under the bitmap of the listed rows only (NaN elsewhere), every layer table but X^(L-1) NaN in every
    row that is not listed: the same bits as before."""
    slab = _slab()
    c = _geo(*geom, T)
    y = _layer(c, L)
    listed = sm.bits_of(c.rows, c.N)
    mask = torch.zeros((c.N + 31) // 32 + 2, dtype=torch.int32, device=DEV)
    slab.rows_bitmap(_ids(np.sort(c.rows)).view(1, -1), c.N, mask)          # (the bitmap kernel takes sorted key lists)
    assert np.array_equal(mask.cpu().numpy()[:(c.N + 31) // 32], sm.bitmap_words(listed, pad=0))
    long_tab = _nan(c.ns * c.plan.n_long * c.w)
    slab.hop(c.plan, c.xs[L - 1], long_tab, gs=c.hgs, seg_only=True, add_mask=mask)
    lt = long_tab.view(c.ns, c.plan.n_long, c.w)
    is_l = torch.from_numpy(listed[c.lens > T]).to(DEV)
    assert all_nan(lt[:, ~is_l]) and not bool(torch.isnan(lt[:, is_l]).any()), y.what + ": the wanted rows of the long table"
    keep = torch.from_numpy(listed)[:, None]
    layers = [_table(torch.where(keep, x, torch.full_like(x, NAN)), c.ns, c.w).data for x in c.X[:L - 1]] + [c.xs[L - 1].data]
    R = len(c.rows)
    out, nar = _nan(R, c.d), _nan(R, c.d)
    _rows(c, L, None, long_tab, c.ids, y.cnt, R, 1, out, nar, layers=layers)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(nar).all()), y.what + ": a row nobody listed was read"
    _check("rows inline", out, nar, y.ref, y.what + " (wanted rows only)")
    assert same_bits(out, y.out) and same_bits(nar, y.nar)


# ============================================================================= list forms
_ALL = {}


def _all_rows(c, L):
    """rows = None over all N rows: outputs and float64 reference, once per geometry."""
    if c.key not in _ALL:
        y = _layer(c, L)
        out, nar = _nan(c.N, c.d), _nan(c.N, c.d)
        _rows(c, L, None, y.long_tab, None, None, c.N, 1, out, nar)
        _ALL[c.key] = (out, nar, rm.rows_ref(c.m, c.X[:L], None, np.arange(c.N), c.U))
    return _ALL[c.key]


@pytest.mark.parametrize("geom", FORM_GEOMS)
def test_list_forms(geom):
    """rows = None; 1, 2 and 8 lists with device counts (a count of 0 among them; the slots behind a count hold VALID ids, so only
    the count keeps them unwritten); 2 lists without counts and negative ids as padding, in the middle of a list too. Outputs are
    column views of one wider buffer (ld > d, the multi-rank send layout); R = 77 and N are no multiples of 256 / LR."""
    T, L = 64, 3
    c = _geo(*geom, T)
    y = _layer(c, L)
    out_all, nar_all, ref_all = _all_rows(c, L)
    assert c.N % 4 != 0
    _check("rows list forms", out_all, nar_all, ref_all, y.what + " rows = None")
    pos = torch.from_numpy(c.rows)
    assert same_bits(out_all[pos.to(DEV)], y.out) and same_bits(nar_all[pos.to(DEV)], y.nar), y.what + ": rows = None differs from the list"
    R, d = 77, c.d
    rs = np.random.RandomState(d)
    named = np.asarray(sorted(c.named.values()))
    for n_lists, counts in ((1, [77]), (2, [50, 77]), (8, [77, 0, 1, 33, 76, 5, 64, 17]), (2, None)):
        ids = np.stack([np.concatenate([rs.permutation(named), rs.randint(0, c.N, R)])[:R] for _ in range(n_lists)])
        if counts is None:
            live = rs.rand(n_lists, R) < 0.7
            live[0, :3], live[1, -1] = (False, True, False), True
            ids = np.where(live, ids, np.where(rs.rand(n_lists, R) < 0.5, PAD, -1))
        else:
            live = np.arange(R)[None, :] < np.asarray(counts)[:, None]
        packed = _nan(n_lists * R, 2 * d + 8)
        cnt = None if counts is None else torch.tensor(counts, dtype=torch.int32, device=DEV)
        _rows(c, L, None, y.long_tab, _ids(ids), cnt, R, n_lists, packed[:, :d], packed[:, d + 4:2 * d + 4])
        what = "%s, %d lists, %s" % (y.what, n_lists, "negative padding" if counts is None else "counts %s" % counts)
        lv = torch.from_numpy(live.reshape(-1)).to(DEV)
        node = torch.from_numpy(np.where(live, ids, 0).reshape(-1)).to(DEV)
        assert all_nan(packed[~lv]) and all_nan(packed[:, d:d + 4]) and all_nan(packed[:, 2 * d + 4:]), what + ": a slot that is not listed was written"
        assert same_bits(packed[lv, :d], out_all[node[lv]]) and same_bits(packed[lv, d + 4:2 * d + 4], nar_all[node[lv]]), what


@pytest.mark.parametrize("geom", FORM_GEOMS)
def test_narrow_by_node(geom):
    """narrow_by_node = 1 (the non-fused head's buffer): narrow lands in row `node` of an N-row buffer with its own leading
    dimension, out0 stays compact; every row of a node that is not listed keeps its NaN."""
    T, L = 64, 3
    c = _geo(*geom, T)
    y = _layer(c, L)
    R, d = len(c.rows), c.d
    out, by_node = _nan(R, d + 4), _nan(c.N, d + 8)
    _rows(c, L, None, y.long_tab, c.ids, None, R, 1, out[:, :d], by_node[:, :d], by_node=True)
    pos = torch.from_numpy(c.rows).to(DEV)
    assert same_bits(out[:, :d], y.out) and all_nan(out[:, d:]), y.what + ": out0 is not the compact one"
    assert same_bits(by_node[pos, :d], y.nar), y.what + ": narrow by node"
    _check("rows list forms", out[:, :d], by_node[pos, :d], y.ref, y.what + " by node")
    other = torch.ones(c.N, dtype=torch.bool, device=DEV)
    other[pos] = False
    assert all_nan(by_node[other]) and all_nan(by_node[:, d:]), y.what + ": a row of a node nobody listed was written"


def test_two_launch_plan():
    """The plan of the two-launch SELL form (tiered = False, threshold 32): split rows from its seg_only table."""
    L = 3
    c = _geo(64, 32, 2, 32, tiered=False)
    y = _layer(c, L)
    _check("rows two-launch", y.out, y.nar, y.ref, y.what)
    R = len(c.rows)
    out, nar = _nan(R, c.d), _nan(R, c.d)
    _rows(c, L, y.full.data, None, c.ids, None, R, 1, out, nar)
    assert same_bits(out, y.out) and same_bits(nar, y.nar), y.what + ": the inline hop differs from the table"


def test_refusals_write_nothing():
    slab = _slab()
    L = 3
    c = _geo(64, 32, 2, 64)
    y = _layer(c, L)
    R, d = len(c.rows), c.d
    X = [t.data for t in c.xs]
    out, nar, odd = _nan(R, d), _nan(R, d), _nan(R, d + 2)
    call = lambda **k: slab.rows(*[k.get(a, v) for a, v in (("plan", c.plan), ("ns", c.ns), ("w", c.w), ("L", L), ("U", c.U),
                                                            ("layers", X[:L] + [None]), ("long_tab", y.long_tab), ("ids", c.ids),
                                                            ("counts", None), ("R", R), ("n_lists", 1), ("out0", out), ("narrow", nar),
                                                            ("by_node", False))])
    for what, kw in (("L = 0", dict(L=0, layers=X[:1])), ("L = 9", dict(L=9, layers=X[:8] + X[:1] + [None])),
                     ("w = 12", dict(w=12, ns=5)), ("a missing middle layer", dict(layers=[X[0], None, X[2], None])),
                     ("no long table", dict(long_tab=None)), ("two lists without row ids", dict(ids=None, n_lists=2, R=R // 2)),
                     ("ld_out0 not a multiple of 4", dict(out0=odd[:, :d])), ("ld_narrow not a multiple of 4", dict(narrow=odd[:, :d]))):
        with pytest.raises(RuntimeError):
            call(**kw)
        torch.cuda.synchronize()
        assert all_nan(out) and all_nan(nar) and all_nan(odd), what + ": refused, but something was written"
    call()
    assert same_bits(out, y.out) and same_bits(nar, y.nar)


# ============================================================================= the wide form
WIDE_N = 301


@pytest.mark.parametrize("ns,w", [(1, 4), (2, 32), (8, 8)])
def test_wide_from_master_and_grad_are_exact(ns, w):
    slab = _slab()
    N, d = WIDE_N, ns * w
    assert (N * w // 4) % 256 != 0
    g = torch.Generator().manual_seed(d)
    E, GW = torch.randn(N, d, generator=g), torch.randn(N, 2 * d, generator=g)
    master, gw = _table(E, ns, w), _table(GW, 2 * ns, w)
    for U in (0, N, 117):
        wide = slab.SlabTable(N, 2 * ns, w, DEV)
        wide.data.fill_(NAN)
        slab.wide_from_master(master, U, wide)
        assert same_bits(wide.dense().cpu(), torch.from_numpy(rm.wide_ref.from_master(E.numpy(), U))), (ns, w, U)
        for scale in (1.0, 1.0 / 3.0):
            grad = slab.SlabTable(N, ns, w, DEV)
            grad.data.fill_(NAN)
            slab.wide_grad(gw, U, scale, grad)
            assert same_bits(grad.dense().cpu(), torch.from_numpy(rm.wide_ref.grad(GW.numpy(), U, scale))), (ns, w, U, scale)


@pytest.mark.parametrize("L", [1, 3, 8])
@pytest.mark.parametrize("ns,w", [(1, 4), (2, 32), (8, 8)])
def test_wide_rows(ns, w, L):
    slab = _slab()
    N, d = WIDE_N, ns * w
    g = torch.Generator().manual_seed(d + L)
    Xs = [torch.randn(N, 2 * d, generator=g) for _ in range(L + 1)]
    layers = [_table(x, 2 * ns, w).data for x in Xs]
    what = "wide rows (%d x %d) L %d" % (ns, w, L)
    packed = _nan(N, 2 * d + 8)                                           # strided outputs: two column views of one buffer
    slab.wide_rows(layers, N, ns, w, None, N, packed[:, :d], packed[:, d + 4:2 * d + 4])
    o, so, n, sn, K = rm.wide_ref.rows([x.numpy() for x in Xs], np.arange(N))
    _close("wide rows", packed[:, :d], o, so, K, what + " rows = None: out0")
    _close("wide rows", packed[:, d + 4:2 * d + 4], n, sn, K, what + " rows = None: narrow")
    assert all_nan(packed[:, d:d + 4]) and all_nan(packed[:, 2 * d + 4:])
    rs = np.random.RandomState(L)
    R = 77
    ids = rs.randint(0, N, R)
    ids[[0, 4, R - 1]] = (N - 1, 0, PAD)
    ids[rs.rand(R) < 0.2] = -1
    ids[1] = N - 2
    lists = _nan(R, 2 * d + 8)
    slab.wide_rows(layers, N, ns, w, _ids(ids), R, lists[:, :d], lists[:, d + 4:2 * d + 4])
    live = torch.from_numpy(ids >= 0).to(DEV)
    node = torch.from_numpy(np.maximum(ids, 0)).to(DEV)
    assert all_nan(lists[~live]) and all_nan(lists[:, d:d + 4]) and all_nan(lists[:, 2 * d + 4:]), what + ": a padded slot was written"
    assert same_bits(lists[live], packed[node[live]]), what + ": the list differs from rows = None"
    packed2 = _nan(N, 2 * d + 8)
    slab.wide_rows(layers, N, ns, w, None, N, packed2[:, :d], packed2[:, d + 4:2 * d + 4])
    assert same_bits(packed2, packed), what + ": second launch differs"


def test_zz_report_the_worst_ratios():
    """Prints the worst err / tol per kernel family of this session (pytest -s shows it; the figures of the commit message)."""
    print("\nworst err / tol: " + ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))
    assert all(v <= 1.0 for v in WORST.values())
