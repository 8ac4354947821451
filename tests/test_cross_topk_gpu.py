"""Dot-product / cosine top-K of one table's rows against another's (ops.cross_topk, csrc/knn.hip) against knn_model.topk64.

Exact cases: tables of small integers (|entry| <= 8) make every fp32 dot product exact (at most 128 * 64 = 8192), so ids AND
values are compared bit for bit, the id order among the many ties included. Random float tables: |fp32 dot - float64 dot| <=
knn_model.tol(d) max|q| max|c| (the cosine bound scaled by the largest row norms of the two sides: dot products are not
bounded by 1), lists by the near-tie rule of the cosine tests."""
import numpy as np
import pytest
import torch

import knn_model as km

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NQ = 37


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _cases():
    from elimrec_amd import ops
    C = ops.KNN_CHUNK
    return [  # K, n, Q, d
        (1, 1, 1, 64), (10, C - 1, 16, 64), (64, C, 17, 32), (65, C + 1, 65, 128), (256, 2 * C + 3, 17, 20), (10, 2 * C + 3, 65, 64),
        (256, C - 1, 1, 64), (64, 1, 16, 32), (65, C, 16, 20), (1, C + 1, 1, 128),
    ]


def test_cases_cover_the_issue():
    from elimrec_amd import ops
    C = ops.KNN_CHUNK
    cases = _cases()
    assert {c[0] for c in cases} == {1, 10, 64, 65, 256} and {c[1] for c in cases} == {1, C - 1, C, C + 1, 2 * C + 3}
    assert {c[2] for c in cases} == {1, 16, 17, 65} and {c[3] for c in cases} == {32, 64, 128, 20}


def _excl(rng, Q, n, K):
    """Query 0: an empty list; query 1: a list that repeats ids; the last query: fewer than K candidates are left."""
    excl = [[] for _ in range(Q)]
    if Q > 1:
        e = rng.integers(0, n, size=5).tolist()
        excl[1] = e + e[::-1]
    keep = set(rng.permutation(n)[:min(3, K - 1)].tolist())
    excl[Q - 1] = [i for i in range(n) if i not in keep]
    return excl


def _run(Tq, sqq, T, sq, rows, K, excl=None):
    from elimrec_amd import ops
    Q = len(rows)
    idx = torch.full((Q, K), -7, dtype=torch.int32, device=DEV)
    val = torch.full((Q, K), 7.0, dtype=torch.float32, device=DEV)
    ptr, flat = km.csr(excl) if excl is not None else (None, None)
    ops.cross_topk(Tq, sqq, T, sq, np.asarray(rows, dtype=np.int32), K, idx, val, excl_ptr=ptr, excl_rows=flat)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), val.cpu().numpy()


def test_integer_tables_are_exact():
    for ci, (K, n, Q, d) in enumerate(_cases()):
        rng = np.random.default_rng(ci)
        Tq = rng.integers(-8, 9, size=(NQ, d)).astype(np.float32)
        T = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
        rows = rng.integers(0, NQ, size=Q)
        excl = _excl(rng, Q, n, K)
        ids, vals = _run(_t(Tq), None, _t(T), None, rows, K, excl)
        s = km.masked(Tq[rows].astype(np.float64) @ T.astype(np.float64).T, rows, False, excl)
        want_ids, want_vals = km.topk64(s, K)
        assert np.array_equal(ids, want_ids), (K, n, Q, d)
        assert np.array_equal(vals.view(np.int32), want_vals.astype(np.float32).view(np.int32)), (K, n, Q, d)
        assert (ids[Q - 1] == -1).sum() >= 1 or n > K + 3


def _check_lists(ids, vals, s, K, tol, what):
    """test_knn_gpu's criteria (a)-(e) with the tolerance of this test."""
    n = s.shape[1]
    order, _ = km.topk64(s, K)
    for b in range(s.shape[0]):
        r, v, o = ids[b].astype(np.int64), vals[b], order[b]
        m = min(K, int((s[b] > -np.inf).sum()))
        assert (r[:m] >= 0).all() and (r[:m] < n).all() and (r[m:] == -1).all() and np.isneginf(v[m:]).all(), (what, b)
        assert len(set(r[:m].tolist())) == m and (s[b, r[:m]] > -np.inf).all(), (what, b)
        if not m:
            continue
        assert np.abs(v[:m].astype(np.float64) - s[b, r[:m]]).max() <= tol, (what, b, np.abs(v[:m] - s[b, r[:m]]).max(), tol)
        assert np.abs(s[b, r[:m]] - s[b, o[:m]]).max() <= 2 * tol, (what, b)
        if m == K:
            assert np.isin(np.flatnonzero(s[b] > s[b, o[K - 1]] + 2 * tol), r).all(), (what, b)
        assert (v[1:m] <= v[:m - 1]).all(), (what, b)
        same = v[1:m].view(np.int32) == v[:m - 1].view(np.int32)
        assert (r[1:m][same] > r[:m - 1][same]).all(), (what, b)


@pytest.mark.parametrize("d,K", [(64, 10), (20, 65), (128, 256)])
def test_random_tables_against_float64(d, K):
    from elimrec_amd import ops
    n, Q = ops.KNN_CHUNK + 9, 33
    rng = np.random.default_rng(d)
    Tq = (3.0 * rng.standard_normal((NQ, d))).astype(np.float32)
    T = (0.5 * rng.standard_normal((n, d))).astype(np.float32)
    wide = np.full((n + 3, d + 7), np.nan, dtype=np.float32)              # a column block, rows not 16-byte aligned
    wide[2:2 + n, 3:3 + d] = T
    rows = rng.integers(0, NQ, size=Q)
    excl = _excl(rng, Q, n, K)
    ids, vals = _run(_t(Tq), None, _t(wide)[2:2 + n, 3:3 + d], None, rows, K, excl)
    s = km.masked(Tq[rows].astype(np.float64) @ T.astype(np.float64).T, rows, False, excl)
    tol = km.tol(d) * float(np.sqrt((Tq.astype(np.float64) ** 2).sum(1)).max() * np.sqrt((T.astype(np.float64) ** 2).sum(1)).max())
    _check_lists(ids, vals, s, K, tol, (d, K))


def test_with_both_norms_it_is_cosine_topk():
    from elimrec_amd import ops
    n, d, K = ops.KNN_CHUNK + 40, 64, 50
    rng = np.random.default_rng(5)
    T = rng.standard_normal((n, d)).astype(np.float32)
    Td, sq = _t(T), _t((T.astype(np.float64) ** 2).sum(1).astype(np.float32))
    rows = rng.integers(0, n, size=70).astype(np.int32)
    idx = torch.full((70, K), -7, dtype=torch.int32, device=DEV)
    val = torch.full((70, K), 7.0, dtype=torch.float32, device=DEV)
    ops.cosine_topk(Td, sq, rows, K, idx, val, exclude_self=True)
    ids, vals = _run(Td, sq, Td, sq, rows, K, [[int(q)] for q in rows])
    assert np.array_equal(ids, idx.cpu().numpy()) and np.array_equal(vals.view(np.int32), val.cpu().numpy().view(np.int32))


def test_torch_entry_point_gives_the_same_lists():
    from elimrec_amd import torch_ops
    rng = np.random.default_rng(6)
    Tq = rng.integers(-8, 9, size=(NQ, 32)).astype(np.float32)
    T = rng.integers(-8, 9, size=(500, 32)).astype(np.float32)
    rows = rng.integers(0, NQ, size=20).astype(np.int32)
    excl = _excl(rng, 20, 500, 10)
    ptr, flat = km.csr(excl)
    ids, vals = _run(_t(Tq), None, _t(T), None, rows, 10, excl)
    got_i, got_v = torch_ops.load().cross_topk(_t(Tq), None, _t(T), None, _t(rows), _t(ptr), _t(flat), 10)
    assert np.array_equal(got_i.cpu().numpy(), ids) and np.array_equal(got_v.cpu().numpy().view(np.int32), vals.view(np.int32))
