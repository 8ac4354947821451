"""The slab-major hops (csrc/slab.hip: sell_tier_kernel + tile_ballot_kernel, sell_hop_kernel + sell_fixup_kernel; csrc/sweep.hip:
sweep_rows_kernel) against the float64 model of tests/slab_model.py, element by element, on graphs built to hit every branch: the
tier ladders hold a row on and next to every boundary of the four row tiers for every lane-group count G = 64 / LPR, the sweep
ladders rows on and next to the eight-entry step records. Calls go through elimrec_amd.slab (ops.block_spmm only as the row-major
kernel the unsplit rows must equal bit for bit).

Every output starts as NaN; every input region the contract leaves unread holds NaN (source rows outside src_mask, add rows
outside add_mask, the swept side's own rows for a direct sweep). The bound is fp64_tools.assert_close with K = the row's own
length + 3 and scale = (|A||x| + |add|) |scale|, no absolute floor beyond TINY: a dropped or doubled neighbour of a short row, or
a gathered inactive row, cannot pass. What must be the same arithmetic compares bit for bit. No (geometry, T) pair is skipped:
every ladder can be built.
"""
import types

import numpy as np
import pytest
import torch

import slab_model as sm
from fp64_tools import NAN, TINY, all_nan, assert_close, same_bits, tau

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORST = {}          # family -> worst err / tol seen in this session (printed by the last test)

# (d, w, gs): LPR = (d / w / gs) * (w / 4) lanes per row piece
GEOMS = [(4, 4, 1), (8, 8, 1), (16, 16, 1), (32, 32, 1), (64, 32, 2), (32, 16, 1), (32, 8, 1), (96, 32, 3), (64, 32, 1), (64, 64, 1),
         (128, 32, 1), (256, 32, 2), (256, 32, 1)]
LPRS = [1, 2, 4, 8, 8, 8, 8, 8, 16, 16, 32, 32, 64]
THRESHOLDS = [32, 4]          # 4: wave rows shorter than G


def _slab():
    from elimrec_amd import slab
    return slab


def _lpr(d, w, gs):
    return (d // w // gs) * (w // 4)


def _rand(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _close(family, got, ref, scale, K, what):
    g = got.detach().double().cpu()
    tol = tau(K) * scale + TINY
    if isinstance(tol, torch.Tensor) and tol.shape != g.shape:
        tol = tol.expand_as(g)
    fin = torch.isfinite(g) & torch.isfinite(ref)
    if bool(fin.any()):
        WORST[family] = max(WORST.get(family, 0.0), float(((g - ref).abs()[fin] / tol[fin]).max()))
    assert_close(got, ref, scale, K, what)


def _table(X, ns, w):
    """Slab table of a host tensor [n x ns*w] (NaN rows and all)."""
    return _slab().SlabTable(X.shape[0], ns, w, DEV).from_rows(X.to(DEV).contiguous())


def _nan_table(n, ns, w):
    t = _slab().SlabTable(n, ns, w, DEV)
    t.data.fill_(NAN)
    return t


def _bits(mask):
    return torch.from_numpy(sm.bitmap_words(mask)).to(DEV)


def _keep(X, mask):
    """X with NaN in the rows outside mask."""
    return torch.where(torch.from_numpy(np.asarray(mask, dtype=bool))[:, None], X, torch.full_like(X, NAN))


def _row_mask(lens, T, G, seed, p=0.5):
    """A random row mask with one row of every tier and one empty row set, another of each clear."""
    mask = np.random.RandomState(seed).rand(len(lens)) < p
    mask[sm.one_row_per_tier(lens, T, G, which=0)] = True
    mask[sm.one_row_per_tier(lens, T, G, which=1)] = False
    return mask


# ----------------------------------------------------------------------------------------------------------- shared cases
_PLANS, _CASES = {}, {}


def _plan(kind, T, G, tiered=True):
    """(matrix, device plan) of a ladder, built once per session."""
    key = (kind, T, G, tiered)
    if key not in _PLANS:
        m = {"ladder": lambda: sm.tier_ladder(T, G)[0], "flat": lambda: sm.tier_ladder_flat(T, G), "long": lambda: sm.tier_ladder_long(T, G)}[kind]()
        split = m.shape[0] // 3 if m.shape[0] == m.shape[1] else None
        _PLANS[key] = (m, _slab().SellPlan(m, DEV, threshold=T, side_split=split, tiered=tiered, ipw=G))
    return _PLANS[key]


def _patterns(kind, T, G):
    key = ("patterns", kind, T, G)
    if key not in _PLANS:
        m, _ = _plan(kind, T, G)
        split = m.shape[0] // 3 if m.shape[0] == m.shape[1] else None
        _PLANS[key] = sm.source_patterns(_slab().SellPlan(m, "cpu", threshold=T, side_split=split, tiered=True, ipw=G), m)
    return _PLANS[key]


def _case(d, w, gs, T, tiered=True):
    """The ladder of this geometry's G, its plan, one input table, the float64 reference of the plain hop and the plain hop's
    output (launched once, left unchanged)."""
    key = (d, w, gs, T, tiered)
    if key in _CASES:
        return _CASES[key]
    slab = _slab()
    G = 64 // _lpr(d, w, gs)
    m, plan = _plan("ladder", T, G, tiered)
    n, ns = m.shape[0], d // w
    lens = sm.row_lengths(m)
    if tiered:
        c = sm.plan_counts(lens, T, G)
        assert (plan.n_w1, plan.n_w4, plan.n_seg, plan.n_long) == (c["n_w1"], c["n_w4"], c["n_seg"], c["n_long"]) and min(c.values()) > 0
    else:
        assert not plan.tiered and plan.n_long == int((lens > T).sum()) > 0
    X = _rand(1000 * d + w + gs, n, d)
    xs = _table(X, ns, w)
    y0 = _nan_table(n, ns, w)
    slab.hop(plan, xs, y0, gs=gs)
    (r, rs), _ = sm.hop(m, X)
    what = "(d %d, w %d, gs %d) LPR %d T %d%s" % (d, w, gs, _lpr(d, w, gs), T, "" if tiered else " two-launch")
    _CASES[key] = types.SimpleNamespace(T=T, G=G, m=m, plan=plan, n=n, ns=ns, d=d, w=w, gs=gs, lens=lens, X=X, xs=xs, K=sm.hop_K(m), ref=r,
                                        scale=rs, y0=y0, out0=y0.dense(), what=what)
    return _CASES[key]


def test_geometry_table_and_layout_model():
    slab = _slab()
    assert [_lpr(*g) for g in GEOMS] == LPRS
    for n, ns, w in ((5, 1, 4), (37, 3, 16), (70, 8, 32)):
        X = _rand(n, n, ns * w)
        t = _table(X, ns, w)
        assert same_bits(t.data.cpu(), torch.from_numpy(sm.slab_layout(X.numpy(), ns, w)))
        assert same_bits(t.dense().cpu(), X) and np.array_equal(sm.slab_dense(t.data.cpu().numpy(), n, ns, w), X.numpy())
    assert slab.choose_slabs(256) == (8, 32)


# ============================================================================= the wave-tile hop on the tier ladder
@pytest.mark.parametrize("T", THRESHOLDS)
@pytest.mark.parametrize("d,w,gs", GEOMS)
def test_tier_hop_plain_and_epilogue(d, w, gs, T):
    from elimrec_amd import ops
    slab = _slab()
    c = _case(d, w, gs, T)
    _close("tier hop", c.out0, c.ref, c.scale, c.K, c.what + " plain")                    # (a NaN left = a row not written: fails)
    assert not bool(c.out0[torch.from_numpy(c.lens == 0).to(DEV)].any()), c.what + ": an empty row is not zero"
    y = _nan_table(c.n, c.ns, w)
    slab.hop(c.plan, c.xs, y, gs=gs)
    assert same_bits(y.data, c.y0.data), c.what + ": second launch differs"
    if d <= 256:            # rows of <= T entries: the row-major kernel's fma chain
        rm = torch.full((c.n, d), NAN, device=DEV)
        ops.block_spmm(ops.Csr.from_scipy(c.m, DEV, C=d, threshold=T), c.X.to(DEV), Xout=rm)
        short = torch.from_numpy(c.lens <= T).to(DEV)
        assert same_bits(c.out0[short], rm[short]), c.what + ": unsplit rows differ from ops.block_spmm"
    add = _rand(d + 7, c.n, d)
    _, (ref, scale) = sm.hop(c.m, c.X, add1=add, scale=0.25)
    slab.hop(c.plan, c.xs, y, gs=gs, add=_table(add, c.ns, w), scale=0.25)
    _close("tier epilogue", y.dense(), ref, scale, c.K, c.what + " add, scale 0.25")
    mask = _row_mask(c.lens, T, c.G, seed=d + T)
    _, (ref, scale) = sm.hop(c.m, c.X, add1=add, add1_mask=mask, scale=1.0 / 3.0)
    y.data.fill_(NAN)
    slab.hop(c.plan, c.xs, y, gs=gs, add=_table(_keep(add, mask), c.ns, w), add_mask=_bits(mask), scale=1.0 / 3.0)
    _close("tier epilogue", y.dense(), ref, scale, c.K, c.what + " add under add_mask, scale 1/3")


@pytest.mark.parametrize("T", THRESHOLDS)
@pytest.mark.parametrize("d,w,gs", GEOMS)
def test_tier_hop_masked_source(d, w, gs, T):
    slab = _slab()
    c = _case(d, w, gs, T)
    S = _rand(d + 11, c.n, d)
    y, y2 = _nan_table(c.n, c.ns, w), _nan_table(c.n, c.ns, w)
    for name, mask in _patterns("ladder", T, c.G).items():
        what = "%s masked, %s" % (c.what, name)
        Sn = _keep(S, mask)
        src, bm = _table(Sn, c.ns, w), _bits(mask)
        _, (ref, scale) = sm.hop(c.m, Sn, add1=Sn, add1_mask=mask, scale=0.5, src_mask=mask)
        # the ballot words of the plan's scratch hold the COMPLEMENT's bits whenever a form below starts: neither the words
        # source_bits writes nor those of the one-call form can be left over from the other
        wrong = _bits(~mask)
        slab.source_bits(c.plan, c.ns, w, gs, wrong)
        y2.data.fill_(NAN)
        slab.source_bits(c.plan, c.ns, w, gs, bm)
        slab.hop(c.plan, src, y2, gs=gs, src_mask=bm, add=src, add_mask=bm, scale=0.5, bits_ready=True)
        _close("tier masked", y2.dense(), ref, scale, c.K, what + " (bits_ready)")
        slab.source_bits(c.plan, c.ns, w, gs, wrong)
        y.data.fill_(NAN)
        slab.hop(c.plan, src, y, gs=gs, src_mask=bm, add=src, add_mask=bm, scale=0.5)      # as the adjoint's first hop calls it
        got = y.dense()
        _close("tier masked", got, ref, scale, c.K, what)
        if name == "none":
            assert not bool(got.any()), what + ": not exactly zero"
        assert same_bits(y2.data, y.data), what + ": bits_ready differs from the one-call form"
    y.data.fill_(NAN)
    slab.hop(c.plan, c.xs, y, gs=gs, src_mask=_bits(np.ones(c.n, dtype=bool)))
    assert same_bits(y.data, c.y0.data), c.what + ": every source active differs from the plain hop"


@pytest.mark.parametrize("T", THRESHOLDS)
@pytest.mark.parametrize("d,w,gs", GEOMS)
def test_tier_hop_seg_only(d, w, gs, T):
    slab = _slab()
    c = _case(d, w, gs, T)
    n_long = c.plan.n_long
    rows = c.plan.t["long_rows"][:n_long].long()
    assert np.array_equal(rows.cpu().numpy(), np.nonzero(c.lens > T)[0])
    dense = lambda tab: tab.view(c.ns, n_long, w).permute(1, 0, 2).reshape(n_long, d)
    tab = torch.full((c.ns * n_long * w,), NAN, device=DEV)
    slab.hop(c.plan, c.xs, tab, gs=gs, seg_only=True)
    assert same_bits(dense(tab).contiguous(), c.out0[rows].contiguous()), c.what + ": seg_only differs from the plain hop's rows"
    # only the wanted rows: one of every long tier, the others must stay untouched
    wanted = np.zeros(c.n, dtype=bool)
    wanted[sm.one_row_per_tier(c.lens, T, c.G, which=1, empty=False)[1:]] = True
    is_w = torch.from_numpy(wanted[c.lens > T]).to(DEV)
    assert int(is_w.sum()) == 3 and sorted(sm.tier_of(c.lens[wanted], T, c.G)) == [1, 2, 3]
    tab2 = torch.full((c.ns * n_long * w,), NAN, device=DEV)
    slab.hop(c.plan, c.xs, tab2, gs=gs, seg_only=True, add_mask=_bits(wanted))
    assert same_bits(dense(tab2)[is_w].contiguous(), c.out0[rows][is_w].contiguous()), c.what + ": wanted rows differ"
    assert all_nan(dense(tab2)[~is_w]), c.what + ": a row nobody wanted was written"
    y = _nan_table(c.n, c.ns, w)                   # tickets and partial rows are left at rest
    slab.hop(c.plan, c.xs, y, gs=gs)
    assert same_bits(y.data, c.y0.data), c.what + ": the hop after seg_only differs"


@pytest.mark.parametrize("T", THRESHOLDS)
def test_a_columns_arithmetic_depends_on_the_lane_groups_only(T):
    """LPR 8 five ways over one plan and one X: slab width and slabs per group only move a column to another lane."""
    slab = _slab()
    m, plan = _plan("ladder", T, 8)
    n = m.shape[0]
    X96 = _rand(96 + T, n, 96)
    outs = {}
    for d, w, gs in ((32, 32, 1), (32, 16, 1), (32, 8, 1), (64, 32, 2), (96, 32, 3)):
        assert _lpr(d, w, gs) == 8
        y = _nan_table(n, d // w, w)
        slab.hop(plan, _table(X96[:, :d].contiguous(), d // w, w), y, gs=gs)
        outs[(d, w, gs)] = y.dense()
    first = outs[(32, 32, 1)]
    assert not any(bool(torch.isnan(out).any()) for out in outs.values()), "a slab was not written"
    for g, out in outs.items():
        assert same_bits(out[:, :32].contiguous(), first), "%s T %d: the first 32 columns differ from (32, 32, 1)" % (g, T)
    assert same_bits(outs[(96, 32, 3)][:, :64].contiguous(), outs[(64, 32, 2)])


@pytest.mark.parametrize("T", THRESHOLDS)
@pytest.mark.parametrize("d,w,gs", [(32, 32, 1), (8, 8, 1)])
def test_tier_hop_on_degenerate_plans(d, w, gs, T):
    """No row above T (n_long == 0) and no row up to T (n_tfin == 0)."""
    slab = _slab()
    G, ns = 64 // _lpr(d, w, gs), d // w
    for kind in ("flat", "long"):
        m, plan = _plan(kind, T, G)
        nr, n = m.shape
        assert (plan.n_long == 0) if kind == "flat" else (int(plan.desc.n_tfin) == 0 and plan.n_long == nr)
        what = "(d %d, w %d) T %d %s ladder" % (d, w, T, kind)
        X, K = _rand(d + T, n, d), sm.hop_K(m)
        (r, rs), _ = sm.hop(m, X)
        y = _nan_table(nr, ns, w)
        slab.hop(plan, _table(X, ns, w), y, gs=gs)
        _close("degenerate plans", y.dense(), r, rs, K, what + " plain")
        pats = _patterns(kind, T, G) if kind == "long" else {"every 64th": np.arange(n) % 64 == 0, "none": np.zeros(n, dtype=bool)}
        for name, mask in pats.items():
            Sn = _keep(X, mask)
            src, bm = _table(Sn, ns, w), _bits(mask)
            y.data.fill_(NAN)
            slab.source_bits(plan, ns, w, gs, _bits(~mask))         # (the scratch holds the complement's bits: see the ladder test)
            if kind == "flat":
                _, (ref, scale) = sm.hop(m, Sn, add1=Sn, add1_mask=mask, scale=0.5, src_mask=mask)
                slab.hop(plan, src, y, gs=gs, src_mask=bm, add=src, add_mask=bm, scale=0.5)
            else:           # fewer rows than sources: no addend of the source's shape
                _, (ref, scale) = sm.hop(m, Sn, scale=0.5, src_mask=mask)
                slab.hop(plan, src, y, gs=gs, src_mask=bm, scale=0.5)
            _close("degenerate plans", y.dense(), ref, scale, K, "%s masked, %s" % (what, name))
            y2 = _nan_table(nr, ns, w)
            slab.source_bits(plan, ns, w, gs, _bits(~mask))
            slab.source_bits(plan, ns, w, gs, bm)
            kw = dict(add=src, add_mask=bm) if kind == "flat" else {}
            slab.hop(plan, src, y2, gs=gs, src_mask=bm, scale=0.5, bits_ready=True, **kw)
            assert same_bits(y2.data, y.data), "%s masked, %s: bits_ready differs from the one-call form" % (what, name)


# ============================================================================= the two-launch SELL form
@pytest.mark.parametrize("T", THRESHOLDS)
@pytest.mark.parametrize("d,w,gs", [(64, 32, 2), (8, 8, 1), (128, 32, 1), (4, 4, 1)])
def test_two_launch_form(d, w, gs, T):
    slab = _slab()
    c = _case(d, w, gs, T, tiered=False)
    _close("two-launch", c.out0, c.ref, c.scale, c.K, c.what + " plain")
    y = _nan_table(c.n, c.ns, w)
    slab.hop(c.plan, c.xs, y, gs=gs)
    assert same_bits(y.data, c.y0.data), c.what + ": second launch differs"
    S = _rand(d + 13, c.n, d)
    for name, mask in (("a row of every tier", _row_mask(c.lens, T, c.G, seed=d, p=0.15)), ("every 64th", np.arange(c.n) % 64 == 0),
                       ("none", np.zeros(c.n, dtype=bool))):
        Sn = _keep(S, mask)
        src, bm = _table(Sn, c.ns, w), _bits(mask)
        _, (ref, scale) = sm.hop(c.m, Sn, add1=Sn, add1_mask=mask, scale=0.5, src_mask=mask)
        y.data.fill_(NAN)
        slab.hop(c.plan, src, y, gs=gs, src_mask=bm, add=src, add_mask=bm, scale=0.5)
        _close("two-launch", y.dense(), ref, scale, c.K, "%s masked, %s" % (c.what, name))
    add, mask = _rand(d + 7, c.n, d), _row_mask(c.lens, T, c.G, seed=d + T)
    _, (ref, scale) = sm.hop(c.m, c.X, add1=add, add1_mask=mask, scale=1.0 / 3.0)
    y.data.fill_(NAN)
    slab.hop(c.plan, c.xs, y, gs=gs, add=_table(_keep(add, mask), c.ns, w), add_mask=_bits(mask), scale=1.0 / 3.0)
    _close("two-launch", y.dense(), ref, scale, c.K, c.what + " add under add_mask, scale 1/3")
    n_long = c.plan.n_long
    rows = c.plan.t["long_rows"][:n_long].long()
    tab = torch.full((c.ns * n_long * w,), NAN, device=DEV)
    slab.hop(c.plan, c.xs, tab, gs=gs, seg_only=True)
    lt = tab.view(c.ns, n_long, w).permute(1, 0, 2).reshape(n_long, d).contiguous()
    assert same_bits(lt, c.out0[rows].contiguous()), c.what + ": seg_only differs from the plain hop's rows"


@pytest.mark.parametrize("d,w,gs", [(64, 32, 2), (256, 32, 1)])
def test_two_launch_form_without_split_rows(d, w, gs):
    """No row above T (n_long == 0): the SELL launch alone, no fix-up launch; LPR 8 and LPR 64 (one row piece per wave)."""
    slab = _slab()
    T, G, ns = 32, 64 // _lpr(d, w, gs), d // w
    m, plan = _plan("flat", T, G, tiered=False)
    n = m.shape[0]
    assert not plan.tiered and plan.n_long == 0
    what = "(d %d, w %d, gs %d) LPR %d T %d two-launch, flat ladder" % (d, w, gs, _lpr(d, w, gs), T)
    X, K = _rand(d + T, n, d), sm.hop_K(m)
    (r, rs), _ = sm.hop(m, X)
    y = _nan_table(n, ns, w)
    slab.hop(plan, _table(X, ns, w), y, gs=gs)
    _close("two-launch", y.dense(), r, rs, K, what + " plain")
    for name, mask in (("every 64th", np.arange(n) % 64 == 0), ("none", np.zeros(n, dtype=bool))):
        Sn = _keep(X, mask)
        src, bm = _table(Sn, ns, w), _bits(mask)
        _, (ref, scale) = sm.hop(m, Sn, add1=Sn, add1_mask=mask, scale=0.5, src_mask=mask)
        y.data.fill_(NAN)
        slab.hop(plan, src, y, gs=gs, src_mask=bm, add=src, add_mask=bm, scale=0.5)
        _close("two-launch", y.dense(), ref, scale, K, "%s masked, %s" % (what, name))


# ============================================================================= the window sweep
SWEEP_GEOMS = [(32, 32), (64, 32), (256, 32), (512, 32), (16, 16), (64, 16)]
SWEEP_LADDERS = [(29, 700), (37, 700), (523, 1100)]  # fewer swept rows than row blocks (29: at every geometry; 37: below 8 slabs); several
                                                     # rows per block and wave
SWEEP_WINDOWS = [64, 333]
SWEEP_T = 32


def _sweep_plan(m, U, d, w):
    slab = _slab()
    ns = d // w
    gs = slab.choose_groups(ns)
    ipw = 64 // ((ns // gs) * (w // 4))
    plan = slab.SellPlan(m, DEV, threshold=SWEEP_T, side_split=U, tiered=True, ipw=ipw)
    return plan, slab.SweepPlan(plan, m, U, DEV, threshold=SWEEP_T, ipw=ipw), ns, gs


@pytest.mark.parametrize("window", SWEEP_WINDOWS)
@pytest.mark.parametrize("U,I", SWEEP_LADDERS)
@pytest.mark.parametrize("d,w", SWEEP_GEOMS)
def test_window_sweep(d, w, U, I, window, monkeypatch):
    slab = _slab()
    monkeypatch.setenv("ELIMREC_SWEEP_WINDOW", str(window))
    m = sm.sweep_ladder(U, I)
    n = U + I
    plan, sweep, ns, gs = _sweep_plan(m, U, d, w)
    what = "sweep (d %d, w %d) U %d I %d window %d" % (d, w, U, I, window)
    user = np.arange(n) < U
    X = _rand(d + U, n, d)
    xs = _table(X, ns, w)
    tile = _nan_table(n, ns, w)
    slab.hop(plan, xs, tile, gs=gs)                                  # the tile hop over all rows, before the plan has a swept side
    K = sm.hop_K(m)[:U]
    (r, rs), _ = sm.hop(m, X)
    # ---- direct: the swept side's own rows of the source are never read, the other side's rows of the output never written
    xn = _table(_keep(X, ~user), ns, w)
    y = _nan_table(n, ns, w)
    sweep.hop(xn, y)
    got = y.dense()
    _close("window sweep", got[:U], r[:U], rs[:U], K, what + " direct")
    assert all_nan(got[U:]), what + ": rows of the other side were written"
    y2 = _nan_table(n, ns, w)
    sweep.hop(xn, y2)
    assert same_bits(y2.data, y.data), what + ": second launch differs"
    add = _rand(d + 7, n, d)
    _, (ref, scale) = sm.hop(m, X, add1=add, scale=0.25)
    y2.data.fill_(NAN)
    sweep.hop(xn, y2, add=_table(_keep(add, user), ns, w), scale=0.25)
    _close("window sweep", y2.dense()[:U], ref[:U], scale[:U], K, what + " add, scale 0.25")
    mask = np.random.RandomState(U + d).rand(n) < 0.5
    mask[:12] = np.arange(12) % 2 == 0
    _, (ref, scale) = sm.hop(m, X, add1=add, add1_mask=mask, scale=1.0 / 3.0)
    y2.data.fill_(NAN)
    sweep.hop(xn, y2, add=_table(_keep(add, mask & user), ns, w), add_mask=_bits(mask), scale=1.0 / 3.0)
    _close("window sweep", y2.dense()[:U], ref[:U], scale[:U], K, what + " add under add_mask, scale 1/3")
    assert all_nan(y2.dense()[U:])
    # ---- through slab.hop: the tile hop over the item rows + the sweep over the user rows
    plan.sweep = sweep
    assert slab._swept(plan, xs)
    y3 = _nan_table(n, ns, w)
    slab.hop(plan, xs, y3, gs=gs)
    got3 = y3.dense()
    assert same_bits(got3[U:].contiguous(), tile.dense()[U:].contiguous()), what + ": item rows differ from the tile hop's"
    assert same_bits(got3[:U].contiguous(), got[:U].contiguous()), what + ": user rows differ from the direct sweep's"
    _close("window sweep", tile.dense()[:U], r[:U], rs[:U], K, what + " (the tile hop on the same rows)")


def test_sweep_cases_reach_every_remainder_of_the_record_pipeline(monkeypatch):
    """Wave stretches of 0, 1, 2, 3, 4 and >= 5 steps (PF = 4 records in flight: the partial last round with nothing, one, two and
    three steps, and the full round) all occur among the cases above; the U = 29 ladder has fewer rows than row blocks at every
    geometry (nb = parts * passes * 32 >= 32), the U = 37 ladder wherever a slab has more than one row part (below 8 slabs)."""
    seen = set()
    for U, I in SWEEP_LADDERS:
        m = sm.sweep_ladder(U, I)
        for d, w in SWEEP_GEOMS:
            for window in SWEEP_WINDOWS:
                monkeypatch.setenv("ELIMREC_SWEEP_WINDOW", str(window))
                _, sweep, ns, _ = _sweep_plan(m, U, d, w)
                g = sweep.geometry(ns, w)
                assert g["n_win"] == -(-I // window)
                if U == 29 or (U == 37 and ns < 8):          # (8 slabs and more: one row part, 32 blocks)
                    assert U < g["parts"] * g["passes"] * g["bpx"]
                seen |= set(np.minimum(sm.wave_stretches(g), 5).tolist())
    assert seen == {0, 1, 2, 3, 4, 5}, seen


def test_zz_report_the_worst_ratios():
    """Prints the worst err / tol per kernel family of this session (pytest -s shows it; the figures of the commit message)."""
    print("\nworst err / tol: " + ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))
    assert all(v <= 1.0 for v in WORST.values())
