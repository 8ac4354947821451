"""The slab-hop tests' own tools (tests/slab_model.py) and the HOST plans they run on, without a GPU: the tier ladders hold what
they claim, SellPlan(device="cpu") sorts their rows into the tiers the row lengths imply and loses or doubles no entry, the named
ballot bitmaps have the property in their name, the layout model round-trips and the masked hop model equals a dense product."""
import numpy as np
import pytest
import torch

import slab_model as sm
from elimrec_amd import slab

PAIRS = [(T, G) for G in (64, 32, 16, 8, 4, 2, 1) for T in (32, 4)]          # every (T, G) of tests/test_slab_hop_gpu.py


@pytest.fixture(scope="module", params=PAIRS, ids=lambda p: "T%d-G%d" % p)
def case(request):
    T, G = request.param
    m, named = sm.tier_ladder(T, G)
    return T, G, m, named, slab.SellPlan(m, "cpu", threshold=T, tiered=True, ipw=G, side_split=m.shape[0] // 3)


def test_ladder_has_the_rows_it_claims(case):
    T, G, m, named, _ = case
    T1, T2 = sm.tiers(T, G)
    lens = sm.row_lengths(m)
    n = m.shape[0]
    assert m.shape == (n, n) and m.dtype == np.float32 and m.has_sorted_indices
    assert all(lens[r] == k for r, k in named.items()) and lens[0] == 0 and lens[-1] == 0
    have = set(named.values())
    want = {0, 1, 2, T - 1, T, T + 1, T + 2, T1 - 1, T1, T1 + 1, T2 - 1, T2, T2 + 1, T2 + T, sm.big_row(T, G)}
    want |= {k for k in (G - 1, G, G + 1) if 0 <= k <= T1} | {k for k in (63, 64, 65, 127, 128, 129) if T < k <= T1}
    assert want <= have, sorted(want - have)
    if T + 1 < G:
        assert any(T < k < G for k in have), "no wave row with empty lane groups"
    q = [k // 4 for k in have if k % 4 == 0 and (k // 4) % G == 0 and {k - 1, 3 * (k // 4) + 1} <= have and T1 < 3 * (k // 4) + 1 and k <= T2]
    assert q, "no workgroup rows of 4q, 4q - 1 and 3q + 1 entries"
    longest = int(lens.max())
    assert longest == sm.big_row(T, G) and -(-longest // T) >= 9 * G and longest + 30 <= n <= longest + 300
    assert (T2 + 1) % T == 1 and (T2 + T) % T == 0
    t = sm.tier_of(lens, T, G)
    assert all(int((t == k).sum()) > 0 for k in range(4))
    c = sm.plan_counts(lens, T, G)
    assert c["n_w1"] % 4 and c["n_w4"] % 4 and c["n_seg"] % (4 * G) and c["n_fin"] % (4 * G)
    assert m.nnz < 150000 and n < 19000
    rows = np.repeat(np.arange(n), lens)
    assert np.all(np.diff(m.indices)[np.diff(rows) == 0] > 0), "columns not sorted and distinct"


def test_host_plan_reports_the_tiers_the_lengths_imply(case):
    T, G, m, _, plan = case
    c = sm.plan_counts(sm.row_lengths(m), T, G)
    for p in (plan, slab.SellPlan(m, "cpu", threshold=T, tiered=True, ipw=G)):
        assert (p.n_w1, p.n_w4, p.n_seg, p.n_long) == (c["n_w1"], c["n_w4"], c["n_seg"], c["n_long"])
        t1, tseg, tfin, n_tiles = sm.tile_bases(p)
        assert t1 == 4 * c["n_w4"] and tseg - t1 == -(-c["n_w1"] // 4) * 4 and tfin - tseg == -(-c["n_seg"] // (4 * G)) * 4
        assert n_tiles - tfin == -(-c["n_fin"] // (4 * G)) * 4 and n_tiles == p.n_tiles
        assert int((p.t["tile_dst"] >= 0).sum()) == G * (4 * c["n_w4"] + c["n_w1"]) + c["n_seg"] + c["n_fin"]
    for make in (sm.tier_ladder_flat, sm.tier_ladder_long):
        md = make(T, G)
        p = slab.SellPlan(md, "cpu", threshold=T, tiered=True, ipw=G)
        cd = sm.plan_counts(sm.row_lengths(md), T, G)
        assert (p.n_w1, p.n_w4, p.n_seg, p.n_long) == (cd["n_w1"], cd["n_w4"], cd["n_seg"], cd["n_long"])
        if make is sm.tier_ladder_flat:
            assert p.n_long == 0 and md.shape == m.shape
        else:
            assert int(p.desc.n_tfin) == 0 and p.n_long == md.shape[0] and p.n_w1 and p.n_w4 and p.n_seg


def test_plan_walks_give_back_every_entry(case):
    T, G, m, _, plan = case
    mats = [m, sm.tier_ladder_flat(T, G), sm.tier_ladder_long(T, G)]
    plans = [plan] + [slab.SellPlan(mat, "cpu", threshold=T, tiered=True, ipw=G) for mat in mats]
    for p, mat in zip(plans, [m] + mats):
        got, want = sm.walk_tiles(p), sm.csr_triples(mat)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), "the wave tiles do not hold the CSR entries"
    for p in (slab.SellPlan(m, "cpu", threshold=T, side_split=m.shape[0] // 3), slab.SellPlan(m, "cpu", threshold=T)):
        assert not p.tiered and p.n_long == int((sm.row_lengths(m) > T).sum())
        got, want = sm.walk_sell(p), sm.csr_triples(m)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), "the SELL items do not hold the CSR entries"


def test_ballot_patterns_have_the_property_in_their_name(case):
    T, G, m, _, plan = case
    n = m.shape[0]
    pats = sm.source_patterns(plan, m)
    assert set(pats) == {"none", "all", "line 0 only", "last line only", "middle line only", "every 64th", "not the row's own"}
    ti, row = sm.longest_wave_tile(plan)
    lens = sm.row_lengths(m)
    assert lens[row] == sm.tiers(T, G)[0] == lens[sm.tier_of(lens, T, G) == sm.WAVE].max()
    lines = sm.tile_lines(plan, ti)
    assert sum(len(l) for l in lines) == lens[row] and len(lines) == -(-int(lens[row]) // 64)
    assert not pats["none"].any() and pats["all"].all() and all(p.shape == (n,) and p.dtype == bool for p in pats.values())
    for name, k in (("line 0 only", 0), ("last line only", len(lines) - 1), ("middle line only", len(lines) // 2)):
        active = [int(pats[name][l].sum()) for l in lines]
        assert active[k] == len(lines[k]) > 0 and sum(active) == active[k], (name, active)
        assert int(pats[name].sum()) == len(lines[k])
    assert np.array_equal(np.nonzero(pats["every 64th"])[0], np.arange(0, n, 64))
    own = m.indices[m.indptr[row]:m.indptr[row + 1]]
    assert not pats["not the row's own"][own].any() and int((~pats["not the row's own"]).sum()) == len(own)
    # the device form: bit r of word r >> 5
    w = sm.bitmap_words(pats["every 64th"]).view(np.uint32)
    assert all(((int(w[r >> 5]) >> (r & 31)) & 1) == int(pats["every 64th"][r]) for r in range(0, n, 7))


@pytest.mark.parametrize("U,I", [(29, 700), (37, 700), (523, 1100)])
def test_sweep_ladder(U, I):
    m = sm.sweep_ladder(U, I)
    lens = sm.row_lengths(m)
    assert U % 32 and m.shape == (U + I, U + I) and m.dtype == np.float32
    assert list(lens[:11]) == list(sm.SWEEP_NAMED) + [I]
    assert m.indices[:m.indptr[U]].min() >= U and (U == m.shape[0] or m[U:].indices.max() < U)
    pat = (m != 0).astype(np.int8)
    assert (pat != pat.T).nnz == 0, "pattern not symmetric"
    assert not np.array_equal(m[:U, U:].toarray(), m[U:, :U].T.toarray()), "Q should carry weights of its own"
    for k in (20, 28, 40):                                          # the one-window rows: consecutive items from item 0
        r = int(np.nonzero(lens[:U] == k)[0][0])
        assert np.array_equal(m.indices[m.indptr[r]:m.indptr[r + 1]], U + np.arange(k))


@pytest.mark.parametrize("n,ns,w", [(5, 1, 4), (37, 3, 16), (64, 8, 32)])
def test_slab_layout_round_trips(n, ns, w):
    X = np.arange(n * ns * w, dtype=np.float32).reshape(n, ns * w)
    flat = sm.slab_layout(X, ns, w)
    assert flat.shape == (ns * n * w,) and np.array_equal(sm.slab_dense(flat, n, ns, w), X)
    for s, r, c in ((0, 0, 0), (ns - 1, n - 1, w - 1), (ns // 2, n // 2, 1)):
        assert flat[(s * n + r) * w + c] == X[r, s * w + c]


def test_masked_hop_model_equals_a_dense_product():
    n, d = 40, 8
    m = sm._from_lengths([0, 1, 2, 5, 9, 33, 40, 17] * 5, n, 3)
    rs = np.random.RandomState(0)
    S, mask, amask = rs.randn(n, d), rs.rand(n) < 0.4, rs.rand(n) < 0.5
    Sn, add = np.where(mask[:, None], S, np.nan), np.where(amask[:, None], rs.randn(n, d), np.nan)
    (r, rscale), (acc, ascale) = sm.hop(m, Sn, add1=add, add1_mask=amask, scale=-0.5, src_mask=mask)
    A = m.toarray().astype(np.float64)
    Sz, Az = S * mask[:, None], np.nan_to_num(add) * amask[:, None]
    assert np.allclose(r.numpy(), A @ Sz, rtol=1e-14, atol=1e-14) and np.allclose(rscale.numpy(), np.abs(A) @ np.abs(Sz), rtol=1e-14, atol=1e-14)
    assert np.allclose(acc.numpy(), (A @ Sz + Az) * -0.5, rtol=1e-14, atol=1e-14)
    assert np.allclose(ascale.numpy(), (np.abs(A) @ np.abs(Sz) + np.abs(Az)) * 0.5, rtol=1e-14, atol=1e-14)
    assert torch.equal(sm.hop_K(m).flatten(), torch.from_numpy(sm.row_lengths(m) + 3.0))
