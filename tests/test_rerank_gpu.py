"""The MMR re-ranking kernel on the device (csrc/rerank.hip) against the float64 model of tests/rerank_model.py, and what is built
on it: EliMRec.rerank_device / recommend_diverse, evaluator.DiversifyReport, --diversify_report.

Tolerance of an objective, tol(d) = 4 (d + 8) 2^-24, a worst-case fp32 bound, not a measurement (u = 2^-24):
  * a cosine formed from an fp32 dot product (d products, d - 1 additions, |dot| <= |a| |b|: off by at most about d u of
    |a| |b|), fp32 squared norms (each off by u relatively: u / 2 in the norm), a square root, a reciprocal and two
    multiplications (half an ulp each, twice for the two rows) is off by at most about (2 d + 8) u of a value <= 1;
  * the normalised relevance (one subtraction each, one division, values in [0, 1]) is off by a few u, as are the two products
    and the subtraction of the objective lambda rel - (1 - lambda) pen, whose weights sum to 1: an objective is off by at most
    about (2 d + 16) u = tol / 2;
  * a pick compares two objectives: the kernel's pick can fall short of the step's float64 maximum by at most tol, and where the
    float64 margin to the runner-up exceeds tol the kernel must make the float64 pick.
The table is a column block of a wider matrix whose other columns and neighbouring rows hold NaN, and the squared norms are a
strided column of a NaN matrix: a read outside the slice shows up as NaN."""
import functools

import numpy as np
import pytest
import torch

import rerank_model as rm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = ((1, 1, 4), (17, 5, 4), (37, 37, 20), (64, 10, 64), (65, 10, 64), (100, 10, 64), (256, 50, 64), (256, 256, 256))   # N, K, d
WHOLE = ((17, 5, 4), (37, 37, 20), (100, 10, 64))
LAMBDAS = (0.3, 0.7)
ROWS, LISTS, SEED = 2000, 200, 7
CANARY_I, CANARY_F = 77, 7.0


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def tol(d):
    return 4.0 * (d + 8) * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _table(d, col0=4):
    """2000 rows of N(0, 1) + 1.5 x one of 8 random centres, fp32, at row 2, column col0 of a wider NaN matrix (col0 = 3: the
    base is not 16-byte aligned); the squared norms as column 1 of a [n + 2 x 3] NaN matrix. -> (T, sq, table view, sqnorm view)"""
    rng = np.random.default_rng(SEED + d)
    centres = rng.standard_normal((8, d))
    T = (rng.standard_normal((ROWS, d)) + 1.5 * centres[rng.integers(0, 8, ROWS)]).astype(np.float32)
    T[11] = 0.0                                                              # a zero row: cosine 0, not a division by zero
    sq = (T.astype(np.float64) ** 2).sum(1).astype(np.float32)
    wide = np.full((ROWS + 3, d + col0 + 4), np.nan, dtype=np.float32)
    wide[2:2 + ROWS, col0:col0 + d] = T
    sqw = np.full((ROWS + 2, 3), np.nan, dtype=np.float32)
    sqw[1:1 + ROWS, 1] = sq
    return T, sq, _t(wide)[2:2 + ROWS, col0:col0 + d], _t(sqw)[1:1 + ROWS, 1]


def _pools(N, B, rng):
    """Distinct random ids with descending uniform scores."""
    ids = np.stack([rng.permutation(ROWS)[:N] for _ in range(B)]).astype(np.int32)
    vals = -np.sort(-rng.uniform(size=(B, N)).astype(np.float32), axis=1)
    return ids, vals


def _run(table, sqn, ids, vals, K, lam):
    """One launch with canaries in front of and behind the [B x K] outputs -> (idx, pos, val) numpy [B x K]."""
    from elimrec_amd import ops
    ids, vals = np.ascontiguousarray(ids, dtype=np.int32), np.ascontiguousarray(vals, dtype=np.float32)
    B = ids.shape[0]
    flat = [torch.full(((B + 3) * K,), c, dtype=dt, device=DEV)
            for c, dt in ((CANARY_I, torch.int32), (CANARY_I, torch.int32), (CANARY_F, torch.float32))]
    views = [f[K:] for f in flat]
    ops.mmr_rerank(table, sqn, _t(ids).reshape(B, -1), _t(vals).reshape(B, -1), K, lam, views[0], views[1], views[2])
    torch.cuda.synchronize()
    out = []
    for f, c in zip(flat, (CANARY_I, CANARY_I, CANARY_F)):
        a = f.cpu().numpy()
        assert (a[:K] == c).all() and (a[(B + 1) * K:] == c).all(), "entries outside [B x K] were written"
        out.append(a[K:(B + 1) * K].reshape(B, K))
    return out


def _verify(P, ids, got, K, d, lam, what):
    """The certificate and the clear prefix of one launch against the float64 model -> bool [B]: the lists whose every float64
    step is clear (margin > tol)."""
    idx, pos, val = got
    B, N = ids.shape
    n_listed = P.mask.sum(1)
    filled = pos >= 0
    assert (filled.sum(1) == np.minimum(K, n_listed)).all(), (what, "number of picks")
    assert (filled[:, :-1] >= filled[:, 1:]).all(), (what, "a filler in front of a pick")
    assert (idx[~filled] == -1).all() and (pos[~filled] == -1).all() and np.isneginf(val[~filled]).all(), (what, "fillers")
    assert (pos[filled] < N).all()
    assert (idx[filled] == np.take_along_axis(ids, np.maximum(pos, 0), 1)[filled]).all(), (what, "out_pos does not index out_idx's id")
    objs, bests, ok = P.replay(pos, lam)
    assert ok.all(), (what, "a pick that is unlisted or was picked before")
    short = float((bests - objs)[filled].max()) if filled.any() else 0.0
    off = float(np.abs(val.astype(np.float64) - objs)[filled].max()) if filled.any() else 0.0
    want, _, margins = P.greedy(K, lam)
    unclear = margins <= tol(d)
    first = np.where(unclear.any(1), unclear.argmax(1), K)
    prefix = np.arange(K)[None, :] < first[:, None]
    print("mmr_rerank %s: pick below the float64 maximum by <= %.3e (bound %.3e), |out_val - float64| <= %.3e (bound %.3e), "
          "%d of %d lists with an unclear step" % (what, short, tol(d), off, tol(d) / 2, int(unclear.any(1).sum()), B))
    assert short <= tol(d), (what, short, tol(d))
    assert off <= tol(d) / 2, (what, off, tol(d) / 2)
    assert (pos[prefix] == want[prefix]).all(), (what, "the list differs from the float64 greedy list before its first unclear step")
    return ~unclear.any(1)


@functools.lru_cache(maxsize=None)
def _shape(N, K, d):
    """The issue's inputs for one shape, run once at both lambdas and shared by the tests."""
    T, sq, table, sqn = _table(d)
    ids, vals = _pools(N, LISTS, np.random.default_rng(SEED))
    P = rm.Pools64(T, sq, ids, vals)
    return P, ids, vals, {lam: _run(table, sqn, ids, vals, K, lam) for lam in LAMBDAS}


def test_forms():
    from elimrec_amd import ops
    assert ops.MMR_MAX_POOL == 256
    want = {(1, 4): True, (17, 4): True, (37, 20): True, (64, 64): True, (65, 64): True, (100, 64): True, (256, 64): False,
            (256, 256): False}
    assert {(N, d): ops.mmr_rows_in_lds(N, d) for N, _, d in SHAPES} == want            # both forms, one and four waves
    assert ops.mmr_rows_in_lds(256, 56) and not ops.mmr_rows_in_lds(256, 60)
    assert ops.mmr_rows_in_lds(56, 256) and not ops.mmr_rows_in_lds(60, 256)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d_K%d_d%d" % s)
def test_certificate_and_clear_prefix(shape):
    N, K, d = shape
    P, ids, _, got = _shape(N, K, d)
    for lam in LAMBDAS:
        clear = _verify(P, ids, got[lam], K, d, lam, (N, K, d, lam))
        if shape in WHOLE:
            idx, pos, _ = got[lam]
            want = P.greedy(K, lam)[0]
            assert clear.mean() >= 0.9, (shape, lam, "more than 10 % of the lists have an unclear step", clear.mean())
            assert (pos[clear] == want[clear]).all() and (idx[clear] == np.take_along_axis(ids, want, 1)[clear]).all()


EDGE_SHAPES = ((17, 5, 4), (100, 10, 64), (256, 12, 64))          # one wave; four waves, rows in LDS; rows in global memory


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: "N%d_K%d_d%d" % s)
@pytest.mark.parametrize("col0", (4, 3), ids=("aligned", "unaligned"))
def test_edges(shape, col0):
    N, K, d = shape
    T, sq, table, sqn = _table(d, col0)
    assert (table.data_ptr() % 16 == 0) == (col0 == 4) and table.stride(0) > d and table.storage_offset() > 0
    rng = np.random.default_rng(SEED + 1)
    ids, vals = _pools(N, 8, rng)
    ids[0, [3, 5, 6]] = (-1, ROWS, 2 ** 31 - 1)                              # ids outside the table in the middle of a pool
    vals[0, [2, 4, 7, 8]] = (np.nan, np.inf, -np.inf, np.nan)                # scores that are not finite
    ids[1, 3:] = -1                                                          # fewer listed entries than K
    vals[1, 1] = np.nan                                                      # (two are left)
    ids[2, 1] = 11                                                           # the zero row
    ids[3, 2], ids[3, 6] = ids[3, 0], ids[3, 1]                              # duplicate ids
    vals[4] = 0.5                                                            # all scores equal
    ids[5] = -7                                                              # nothing listed
    vals[6, :] = vals[6, 0]                                                  # equal scores and unlisted entries together
    ids[6, 0] = ROWS + 3
    P = rm.Pools64(T, sq, ids, vals)
    assert P.mask[0].sum() == N - 7 and P.mask[1].sum() == 2 and P.mask[5].sum() == 0
    for lam in (0.0, 0.3, 0.7, 1.0):
        got = _run(table, sqn, ids, vals, K, lam)
        _verify(P, ids, got, K, d, lam, (shape, col0, lam))
        idx, pos, val = got
        assert (pos[1] == [0, 2] + [-1] * (K - 2)).all() and (pos[5] == -1).all() and np.isneginf(val[5]).all()
        assert (pos[:, 0] == [0, 0, 0, 0, 0, -1, 1, 0]).all()               # step 0 has no penalty: the best listed score
        if lam == 1.0:                                                       # the pool order over the listed positions
            for b in range(8):
                order = np.flatnonzero(P.mask[b])[:K]
                assert (pos[b, :order.size] == order).all(), (b, pos[b], order)
            assert (pos[7] == np.arange(K)).all() and (pos[4] == np.arange(K)).all()
        if lam == 0.0:
            assert (val[:, 0][pos[:, 0] >= 0] == 0.0).all()


@pytest.mark.parametrize("shape", ((64, 10, 64), (100, 10, 64), (256, 50, 64)), ids=lambda s: "N%d_K%d_d%d" % s)
def test_a_list_alone_and_in_a_batch_give_identical_bits(shape):
    N, K, d = shape
    _, _, table, sqn = _table(d)
    ids, vals = _pools(N, 300, np.random.default_rng(SEED + 2))
    batch = _run(table, sqn, ids, vals, K, 0.3)
    alone = _run(table, sqn, ids[150:151], vals[150:151], K, 0.3)
    for a, b in zip(alone, batch):
        assert a[0].tobytes() == b[150].tobytes()


def test_empty_batch_and_torch_op():
    from elimrec_amd import ops, torch_ops
    T, sq, table, sqn = _table(20)
    idx = torch.full((2, 5), CANARY_I, dtype=torch.int32, device=DEV)
    ops.mmr_rerank(table, sqn, torch.zeros(0, 9, dtype=torch.int32, device=DEV), torch.zeros(0, 9, device=DEV), 5, 0.5, idx)
    torch.cuda.synchronize()
    assert (idx == CANARY_I).all()
    ids, vals = _pools(37, 6, np.random.default_rng(SEED + 3))
    want = _run(table, sqn, ids, vals, 9, 0.6)
    got = torch_ops.load().mmr_rerank(table, sqn, _t(ids), _t(vals), 9, 0.6)
    assert [tuple(g.shape) for g in got] == [(6, 9)] * 3
    for g, w in zip(got, want):
        assert g.cpu().numpy().tobytes() == w.tobytes()
    with pytest.raises(RuntimeError):
        torch_ops.load().mmr_rerank(table, sqn, _t(ids), _t(vals), 38, 0.6)


# --------------------------------------------------------------------------- the model and the report on the fixtures
def _forward(name, extra=()):
    from helpers import build_model_from_fixture, load_golden
    g = load_golden(name)
    model, _ = build_model_from_fixture(g, DEV, extra_argv=extra)
    model.bpr_loss(_t(g["step1/users"]), _t(g["step1/pos"]), _t(g["step1/neg"]))
    return model


def _train_csr(train, users):
    tl = [train.get(u, []) for u in users]
    return _t(np.cumsum([0] + [len(x) for x in tl]).astype(np.int64)), _t(np.asarray([i for x in tl for i in x], dtype=np.int32))


def test_recommend_diverse():
    from helpers import build_model_from_fixture, load_golden
    from elimrec_amd.evaluator import CandidateScoringError
    fresh, _ = build_model_from_fixture(load_golden("ml3"), DEV)
    with pytest.raises(RuntimeError):
        fresh.recommend_diverse([0, 1], 3)
    model = _forward("ml3")
    I, k = model.num_items, 4
    pool = min(12, I)
    users = list(range(min(model.num_users, 24)))
    train = model.dataset.get_user_train_dict()
    exclude = {u: train.get(u, []) for u in users}
    tptr, titems = _train_csr(train, users)
    pidx, pval = [x.cpu().numpy() for x in model.predict_device(users, top_k=pool, train_ptr=tptr, train_items=titems)]
    ids, scores = model.recommend_diverse(users, k, pool=pool, lam=1.0, exclude=exclude)
    assert ids.dtype == torch.int32 and scores.dtype == torch.float32 and ids.device.type == scores.device.type == "cpu"
    top, top_val = model.predict_device(users, top_k=k, train_ptr=tptr, train_items=titems)
    assert torch.equal(ids, top.cpu()) and scores.numpy().tobytes() == top_val.cpu().numpy().tobytes()   # lam = 1: the plain top-k
    for space in ("fused",) + tuple(model._mods):
        ids, scores = model.recommend_diverse(users, k, pool=pool, lam=0.5, space=space, exclude=exclude)
        ids, scores = ids.numpy(), scores.numpy()
        assert ids.shape == scores.shape == (len(users), k)
        for b, u in enumerate(users):
            got = ids[b][ids[b] >= 0]
            assert got.size == min(k, int((pidx[b] >= 0).sum())) and len(set(got.tolist())) == got.size
            assert set(got.tolist()) <= set(pidx[b].tolist()) and not set(got.tolist()) & set(exclude[u])
            at = [pidx[b].tolist().index(i) for i in got]
            assert scores[b][:got.size].tobytes() == pval[b][at].tobytes()      # the model's scores of the picked items
            assert ids[b, 0] == pidx[b, 0]                                      # step 0 has no penalty
    assert tuple(model.recommend_diverse(users, k)[0].shape) == (len(users), k)  # the default pool
    assert tuple(model.recommend_diverse([], k)[0].shape) == (0, k)
    model._eval_shard = object()
    try:
        with pytest.raises(CandidateScoringError):
            model.recommend_diverse(users, k)
    finally:
        model._eval_shard = None


@pytest.mark.parametrize("view", [None, [2, 4]])
def test_diversify_report(view):
    import lists_model as lm
    from elimrec_amd import ops
    from elimrec_amd.evaluator import (DIVERSIFY_COLUMNS, CandidateScoringError, DiversifyReport, DiversifyTables, ListReport,
                                       exposure_summary, group_table)
    model = _forward("ml3")
    train, test = model.dataset.get_user_train_dict(), model.dataset.get_user_test_dict()
    K, I = 4, model.num_items
    pool, lambdas = min(12, I), (1.0, 0.3)
    report = DiversifyReport(model.dataset, train, test, K, pool=pool, lambdas=lambdas, group_view=view)
    plain = ListReport(model.dataset, train, test, K, group_view=view)
    report.block_users = plain.block_users = (len(report.users) + 1) // 2       # two user blocks
    model.predict_type = "TIE"
    final, buf = report.evaluate(model)
    rows, lists, counts = report.rerank_rows(model)
    L, G, n = len(lambdas), len(report.group_labels), len(report.users)
    assert isinstance(final, DiversifyTables) and final.columns == DIVERSIFY_COLUMNS and final.table.shape == (G * L, 9)
    assert final.labels == [g for g in report.group_labels for _ in lambdas] and (G > 1) == (view is not None)
    assert tuple(rows.shape) == (L, n, 5) and tuple(lists.shape) == (L, n, K) and tuple(counts.shape) == (L, I)
    assert final.table[:, 0].tolist() == list(lambdas) * G
    # lambda = 1: the plain lists and their numbers
    tptr, titems = _train_csr(train, report.users)
    users_t = _t(np.asarray(report.users, dtype=np.int64))
    top = model.predict_device(users_t, top_k=K, train_ptr=tptr, train_items=titems)[0]
    assert torch.equal(lists[0], top)
    truth = [sorted(set(test[u])) for u in report.users]
    met = torch.empty(n, 2, K, dtype=torch.float32, device=DEV)
    ops.rank_metrics(top, _t(np.cumsum([0] + [len(x) for x in truth]).astype(np.int64)),
                     _t(np.asarray([i for x in truth for i in x], dtype=np.int32)), (2, 4), met)
    want = group_table(met[:, :, K - 1].contiguous(), report._resident(rows.device)["groups"], G)
    list_final = plain.evaluate(model)[0]
    for g in range(G):
        row = final.table[g * L]
        assert row[1:3].tolist() == want[g].astype(np.float64).tolist(), ("recall / ndcg", g)
        assert row[3] == float(list_final.users[g, 0]) and row[4] == float(list_final.users[g, -1]), ("ils_fused / pop", g)
        assert row[5] == 1.0
        print("diversify %s ils_fused: lambda 1 %.6f, lambda 0.3 %.6f" % (report.group_labels[g].strip(), row[3], final.table[g * L + 1, 3]))
        assert g or final.table[1, 3] < row[3], "ils_fused at lambda 0.3 is not below lambda 1 over all test users"
        assert 0.0 < final.table[g * L + 1, 5] <= 1.0
    lists_h = lists.cpu().numpy()
    every = [np.arange(I)]
    for li in range(L):
        assert counts[li].cpu().tolist() == lm.exposure(lists_h[li], I).tolist()
        assert final.table[li, 6:9].tolist() == exposure_summary(lm.exposure(lists_h[li], I), every)[0, 1:4].tolist()
        for g in range(1, G):
            own = lm.exposure(lists_h[li][report._positions[g]], I)
            assert final.table[g * L + li, 6:9].tolist() == exposure_summary(own, every)[0, 1:4].tolist()
    assert final.table[0, 6:9].tolist() == list_final.items[0, 1:4].tolist()     # ListReport's coverage / gini / entropy
    lines = buf.split("\n")
    assert len(lines) == 1 + G * L and lines[0].startswith("columns:") and all(c in lines[0] for c in DIVERSIFY_COLUMNS)
    assert [ln[:12] for ln in lines[1:]] == [x[:12] for x in final.labels]
    assert report.evaluate(model, (rows, lists, counts))[1] == buf
    model._eval_shard = object()
    try:
        with pytest.raises(CandidateScoringError):
            report.evaluate(model)
    finally:
        model._eval_shard = None


def test_driver_switch(tmp_path):
    from test_lists_gpu import _driver
    off, ev0, te0 = _driver(tmp_path / "a", ["--group_view=[10,30]", "--list_report=5"])
    assert not any("by MMR" in ln for ln in off)
    on, ev1, te1 = _driver(tmp_path / "b", ["--group_view=[10,30]", "--list_report=5", "--diversify_report=5", "--diversify_lambda=[1.0,0.5]"])
    added = [k for k, ln in enumerate(on) if ln.startswith("  [TE] top-5 of the top-20 pools by MMR, per lambda:\n")
             or ln.startswith("  [TIE] top-5 of the top-20 pools by MMR, per lambda:\n")]
    assert len(added) == 2 and [ln for k, ln in enumerate(on) if k not in added] == off      # with the switch off: the log as it was
    te, tie = added
    assert on[te].startswith("  [TE]") and on[te - 1].startswith("  [TE] top-5 lists") and on[te + 1].startswith("  [TIE]\t")
    assert on[tie - 1].startswith("  [TIE] top-5 lists") and on[tie + 1].startswith("  [TE->TIE] list shift")
    for k in added:
        assert all(c in on[k] for c in ("lambda", "recall", "ndcg", "ils_fused", "overlap", "coverage", "gini", "entropy"))
        assert on[k].count("\nall:") == 2
    assert ev0.tobytes() == ev1.tobytes() and te0.tobytes() == te1.tobytes()
