"""tests/rows_model.py checked on the host: the ladder holds what it promises, the float32 restatement of rows_piece lies inside
the float64 bound, and the bound has teeth: each way the kernel could be subtly wrong is rejected on a named row. No GPU."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import rows_model as rm
import slab_model as sm
from fp64_tools import within

T, G, D = 64, 8, 8
LAYERS = [1, 2, 3, 4, 8]


def _tables(N, L, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(N, D, generator=g).numpy() for _ in range(L)]


def _ok(got, ref):
    """Rows of (out0, narrow) inside the bound of rows_ref's tuple."""
    o, so, n, sn, K = ref
    return (within(torch.from_numpy(got[0]), o, so, K).all(1) & within(torch.from_numpy(got[1]), n, sn, K).all(1)).numpy()


@pytest.mark.parametrize("T,G", [(64, 8), (32, 8), (64, 2), (64, 4), (64, 16), (32, 1)])
def test_ladder_holds_every_named_length_and_every_tier(T, G):
    m, U, named = rm.rows_ladder(T, G)
    lens = sm.row_lengths(m)
    N = m.shape[0]
    assert m.shape == (N, N) and N % 2 == 1 and 0 < U < N
    want = [n for n in rm.UNSPLIT_LENGTHS if n <= T]
    assert want == list(rm.UNSPLIT_LENGTHS)[:len(want)] and (T < 64 or len(want) == 14)
    for side in ("user", "item"):
        for n in want:
            r = named[(side, n)]
            assert lens[r] == n and (r < U) == (side == "user"), (side, n)
        tiers = sm.tier_of([n for (s, n) in named if s == side], T, G)
        assert set(tiers.tolist()) == {sm.UNSPLIT, sm.WAVE, sm.WORKGROUP, sm.SEGMENTED}, side
    assert all(lens[r] == n for (_, n), r in named.items()) and len(set(named.values())) == len(named)
    assert lens[U - 1] > 0 and lens[U] > 0 and lens[0] == 0 and lens[-1] == 0
    c = sm.plan_counts(lens, T, G)
    assert min(c["n_w1"], c["n_w4"], c["n_seg"], c["n_long"]) > 0, c
    for s in (0, 1):            # both sides of the boundary hold a row of every upper tier
        side_t = sm.tier_of(lens[:U] if s == 0 else lens[U:], T, G)
        assert all((side_t == k).any() for k in (sm.WAVE, sm.WORKGROUP, sm.SEGMENTED))
    rows = rm.listed_rows(m, U, named, 50, seed=1)
    assert len(np.unique(rows)) == len(rows) and set(named.values()) <= set(rows.tolist()) and {U - 1, U} <= set(rows.tolist())


@pytest.mark.parametrize("L", LAYERS)
def test_fp32_restatement_lies_inside_the_bound(L):
    m, U, named = rm.rows_ladder(T, G)
    N = m.shape[0]
    X = _tables(N, L, seed=L)
    rows = rm.listed_rows(m, U, named, 300, seed=L)
    ref = rm.rows_ref(m, X, None, rows, U)
    tab = rm.long_table_fp32(m, X[L - 1], T)
    assert _ok(rm.rows_fp32(m, X, None, rows, U, T=T, long_tab=tab), ref).all()
    short = rows[sm.row_lengths(m)[rows] <= 600]                       # no table: one chain per row, the wave rows too
    assert _ok(rm.rows_fp32(m, X, None, short, U), rm.rows_ref(m, X, None, short, U)).all()
    # X^L given: the bound without the row's length
    XL = (sp.csr_matrix(m, dtype=np.float64) @ X[L - 1].astype(np.float64)).astype(np.float32)
    ref_g = rm.rows_ref(m, X, XL, rows, U)
    assert float(ref_g[4].max()) == L + 2.0
    assert _ok(rm.rows_fp32(m, X, XL, rows, U), ref_g).all()


def _without_entry(m, r, j):
    """m without the j-th entry (CSR order) of row r."""
    m = sp.csr_matrix(m).copy()
    keep = np.ones(m.nnz, dtype=bool)
    keep[m.indptr[r] + j] = False
    rows = np.repeat(np.arange(m.shape[0]), np.diff(m.indptr))
    return sp.csr_matrix((m.data[keep], (rows[keep], m.indices[keep])), shape=m.shape)


@pytest.mark.parametrize("L", LAYERS)
def test_bound_rejects_every_mutant_on_a_named_row(L):
    m, U, named = rm.rows_ladder(T, G)
    N = m.shape[0]
    X = _tables(N, L, seed=10 + L)
    rows = np.sort(rm.listed_rows(m, U, named, 100, seed=L))
    at = {k: int(np.nonzero(rows == r)[0][0]) for k, r in named.items()}
    at_U = int(np.nonzero(rows == U)[0][0])
    ref = rm.rows_ref(m, X, None, rows, U)
    tab = rm.long_table_fp32(m, X[L - 1], T)
    run = lambda mm=m, XL=None, u=U, t=tab: rm.rows_fp32(mm, X, XL, rows, u, T=T, long_tab=t)
    assert _ok(run(), ref).all()
    for side in ("user", "item"):
        # the 17th neighbour of the 17-long row (the one lane of the second 16-wide round), the last of the 64-long row
        for n, j in ((17, 16), (64, 63)):
            bad = _ok(run(mm=_without_entry(m, named[(side, n)], j)), ref)
            assert not bad[at[(side, n)]] and bad.sum() == len(rows) - 1, (side, n)
    # the parity of narrow swapped: every row evaluated as the other side's
    swapped = np.where((rows < U)[:, None], run(u=0)[1], run(u=N)[1])
    bad = _ok((run()[0], swapped), ref)
    assert not bad[[at[k] for k in named]].any()
    # 1 / L in place of 1 / (L + 1)
    o, n = run()
    f = np.float32((L + 1.0) / L)
    assert not _ok((o * f, n * f), ref)[[at[("user", 1)], at[("item", 33)]]].any()
    # layer L - 1 in place of layer L
    bad = _ok(run(XL=X[L - 1]), ref)
    assert not bad[at[("user", 16)]] and not bad[at[("item", 2)]]
    # the user / item test off by one: row U taken for a user row (out0 does not change, narrow does)
    got = run(u=U + 1)
    assert np.array_equal(got[0], o) and not _ok(got, ref)[at_U] and _ok(got, ref).sum() == len(rows) - 1
    # a long row's table entry taken from the neighbouring long row
    bad = _ok(run(t=np.roll(tab, 1, axis=0)), ref)
    lens = sm.row_lengths(m)[rows]
    assert not bad[lens > T].any() and bad[lens <= T].all()
