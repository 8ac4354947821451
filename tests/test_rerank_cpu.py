"""Diversified re-ranking, host side (no GPU): the float64 model of tests/rerank_model.py on hand-worked pools, the host-only entry
points of csrc/rerank.hip, and the argument checks of ops.mmr_rerank, DiversifyReport and the --diversify_* switches that run
before anything touches the device."""
import types

import numpy as np
import pytest
import torch

import rerank_model as rm
from helpers import build_model_from_fixture, load_golden

# rows 0 and 1 are identical, row 2 is orthogonal to them, row 3 lies between, row 4 is zero
T = np.asarray([[1, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0]], dtype=np.float64)
SQ = (T ** 2).sum(1)


def test_two_identical_rows_the_second_is_deferred():
    picks, objs, margins = rm.greedy(T, SQ, [0, 1, 2], [0.9, 0.8, 0.1], 3, 0.5)
    # rel = 1, 0.875, 0; step 0: 0.5 rel -> position 0; step 1: 0.5 * 0.875 - 0.5 * 1 = -0.0625 against 0 - 0: the orthogonal row
    assert picks == [0, 2, 1]
    assert np.allclose(objs, [0.5, 0.0, -0.0625], rtol=0, atol=1e-15) and np.allclose(margins[:2], [0.0625, 0.0625], rtol=0, atol=1e-15)
    assert margins[2] == np.inf                                               # the only candidate left
    assert rm.greedy_loops(T, SQ, [0, 1, 2], [0.9, 0.8, 0.1], 3, 0.5) == picks


def test_lambda_one_gives_the_pool_order_and_lambda_zero_the_least_similar():
    ids, vals = [0, 3, 1, 2], [0.9, 0.7, 0.7, 0.2]
    assert rm.greedy(T, SQ, ids, vals, 4, 1.0)[0] == [0, 1, 2, 3]             # equal scores: the lower position first
    picks, objs, _ = rm.greedy(T, SQ, ids, vals, 4, 0.0)
    # step 0: every objective is 0 -> position 0 (row 0); then the orthogonal row 2 (cos 0), then row 3 (cos 1 / sqrt 2 to both),
    # then the copy of row 0
    assert picks == [0, 3, 1, 2] and np.allclose(objs, [0.0, 0.0, -np.sqrt(0.5), -1.0], rtol=0, atol=1e-15)
    for lam in (0.0, 0.3, 1.0):
        assert rm.greedy_loops(T, SQ, ids, vals, 4, lam) == rm.greedy(T, SQ, ids, vals, 4, lam)[0]


def test_equal_scores_give_zero_relevance():
    P = rm.Pools64(T, SQ, [[0, 1, 2, 3]], [[0.4, 0.4, 0.4, 0.4]])
    assert (P.rel == 0.0).all()
    picks, objs, _ = P.greedy(3, 0.7)
    assert picks[0].tolist() == [0, 2, 3] and np.allclose(objs[0], [0.0, 0.0, -0.3 * np.sqrt(0.5)], rtol=0, atol=1e-15)
    assert rm.Pools64(T, SQ, [[2]], [[0.1]]).rel.tolist() == [[0.0]]          # a pool of one


def test_unlisted_entries_and_the_zero_row():
    ids = [0, -1, 5, 2, 1, 4, 3]
    vals = [0.5, 0.99, 0.98, np.nan, -np.inf, 0.3, np.inf]
    P = rm.Pools64(T, SQ, [ids], [vals])
    assert P.mask[0].tolist() == [True, False, False, False, False, True, False]
    assert P.rel[0].tolist() == [1.0, 0, 0, 0, 0, 0.0, 0]                     # s_min, s_max over the listed positions only
    picks, objs, margins = P.greedy(4, 0.5)
    assert picks[0].tolist() == [0, 5, -1, -1] and objs[0].tolist() == [0.5, 0.0, -np.inf, -np.inf]    # the zero row: cosine 0
    assert margins[0].tolist() == [0.5, np.inf, np.inf, np.inf]
    o, best, ok = P.replay([[5, 0, -1, -1]], 0.5)
    assert ok.all() and o[0, :2].tolist() == [0.0, 0.5] and best[0, :2].tolist() == [0.5, 0.5] and np.isnan(o[0, 2:]).all()
    for bad in ([[1, 0, -1, -1]], [[0, 0, -1, -1]], [[0, 9, -1, -1]]):        # unlisted, picked twice, outside the pool
        assert not P.replay(bad, 0.5)[2].all()
    picks, _, _ = rm.Pools64(T, SQ, [[0, 0, 2]], [[0.9, 0.8, 0.1]]).greedy(3, 0.5)
    assert picks[0].tolist() == [0, 2, 1]                                     # duplicate ids are positions like any other
    assert rm.greedy(T, SQ, [-1, 7], [0.1, 0.2], 2, 0.5) == ([], [], [])


def test_batched_model_against_loops():
    rng = np.random.default_rng(2)
    Tr = rng.standard_normal((40, 8))
    sq = (Tr ** 2).sum(1)
    ids = np.stack([rng.permutation(40)[:12] for _ in range(6)])
    ids[1, 4], ids[2, 0] = -1, 40
    vals = -np.sort(-rng.uniform(size=(6, 12)), axis=1)
    vals[3, 5] = np.nan
    P = rm.Pools64(Tr, sq, ids, vals)
    for lam in (0.0, 0.4, 1.0):
        picks, objs, _ = P.greedy(12, lam)
        for b in range(6):
            want = rm.greedy_loops(Tr, sq, ids[b], vals[b], 12, lam)
            assert picks[b, :len(want)].tolist() == want and (picks[b, len(want):] == -1).all()
        o, best, ok = P.replay(picks, lam)
        filled = picks >= 0
        assert ok.all() and np.array_equal(o[filled], objs[filled]) and np.array_equal(o[filled], best[filled])


def test_host_entry_points_without_a_gpu():
    from elimrec_amd import _lib, ops
    lib = _lib.load()
    assert lib.elimrec_abi_version() == 2
    assert ops.MMR_MAX_POOL == lib.elimrec_mmr_max_pool() == 256
    for N in (1, 17, 64, 65, 100, 255, 256):
        for d in (4, 20, 56, 60, 64, 128, 256):
            fits = N * (d + 4) * 4 <= 60 * 1024                              # lists.hip's row budget at row stride d + 4
            assert ops.mmr_rows_in_lds(N, d) == fits
            assert (N if fits else 1) * (d + 4) * 4 + N * 8 + 64 <= 64 * 1024  # the workgroup's LDS stays within the default limit
    for bad in ((0, 64), (257, 64), (10, 6), (10, 260), (10, 0)):
        assert lib.elimrec_mmr_rows_in_lds(*bad) == -1
        with pytest.raises(ValueError):
            ops.mmr_rows_in_lds(*bad)
    # the C entry point refuses what lies outside the limits before it looks at a pointer or launches anything
    for kw in (dict(K=0), dict(K=11), dict(N=257, K=257), dict(N=0, K=0), dict(d=6), dict(d=260), dict(d=0), dict(lam=-0.1),
               dict(lam=1.5), dict(lam=float("nan")), dict(B=-1), dict(ld=60)):
        a = dict(N=10, K=5, d=64, lam=0.5, B=2, ld=64)
        a.update(kw)
        rc = lib.elimrec_mmr_rerank(None, a["ld"], 100, a["d"], None, 1, None, None, a["B"], a["N"], a["K"], a["lam"], None, None, None, None)
        assert rc == 10001 and b"mmr_rerank" in lib.elimrec_last_error(), (kw, rc)        # ELIMREC_E_BADARG
    assert lib.elimrec_mmr_rerank(None, 64, 100, 64, None, 1, None, None, 0, 10, 5, 0.5, None, None, None, None) == 0   # B == 0


def test_argument_errors_that_need_no_device():
    from elimrec_amd import ops
    table, sq = torch.zeros(8, 4), torch.zeros(8)
    idx, val = torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 3)
    out = torch.zeros(2, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.mmr_rerank(table, sq, idx, val, 2, 0.5, out)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.mmr_rerank(table, sq, idx.tolist(), val, 2, 0.5, out)
    for K, lam in ((0, 0.5), (4, 0.5), (2.5, 0.5), (True, 0.5), (2, -0.01), (2, 1.01), (2, float("nan"))):
        with pytest.raises(ValueError):
            ops.mmr_rerank(table, sq, idx, val, K, lam, out)
    for bad_table in (torch.zeros(8, 6), torch.zeros(8, 260), torch.zeros(8, 8)[:, ::2], torch.zeros(8)):
        with pytest.raises(ValueError):
            ops.mmr_rerank(bad_table, sq, idx, val, 2, 0.5, out)
    for bad_sq in (torch.zeros(7), torch.zeros(8, 1)):
        with pytest.raises(ValueError):
            ops.mmr_rerank(table, bad_sq, idx, val, 2, 0.5, out)
    for bad_idx, bad_val in ((idx, torch.zeros(2, 4)), (idx[:, :2], val[:, :2]), (idx.reshape(-1), val.reshape(-1)),
                             (torch.zeros(2, 257, dtype=torch.int32), torch.zeros(2, 257))):
        with pytest.raises(ValueError):
            ops.mmr_rerank(table, sq, bad_idx, bad_val, 2, 0.5, out)


def test_torch_op_is_registered():
    from elimrec_amd import torch_ops
    assert hasattr(torch_ops.load(), "mmr_rerank") and "mmr_rerank" in torch_ops.OPS


def test_diversify_report_checks():
    from elimrec_amd import ops
    from elimrec_amd.evaluator import DIVERSIFY_COLUMNS, DiversifyReport
    assert DIVERSIFY_COLUMNS == ("lambda", "recall", "ndcg", "ils_fused", "pop", "overlap", "coverage", "gini", "entropy")
    ds = types.SimpleNamespace(num_items=6, num_users=3)
    train = {0: [1, 2], 1: [2], 2: []}
    test = {0: [3], 2: [4, 5]}
    for bad in (0, 1, -1, 7, ops.LIST_MAX_K + 1, 2.5, True, None):
        with pytest.raises(ValueError):
            DiversifyReport(ds, train, test, bad)
    for k, pool in ((3, 2), (3, 7), (2, 2.0), (2, True)):
        with pytest.raises(ValueError):
            DiversifyReport(ds, train, test, k, pool=pool)
    for lambdas in ([], [1.1], [0.5, -0.1], "0.5", [0.5, "x"], 0.5, [True], [float("nan")]):
        with pytest.raises(ValueError):
            DiversifyReport(ds, train, test, 2, lambdas=lambdas)
    with pytest.raises((TypeError, ValueError)):
        DiversifyReport(ds, train, test, 2, group_view=[3, 3])
    with pytest.raises(TypeError):
        DiversifyReport(ds, [1, 2], test, 2)
    rep = DiversifyReport(ds, train, test, 2, group_view=[1])
    assert (rep.top_k, rep.pool, rep.lambdas) == (2, 6, (1.0, 0.9, 0.7, 0.5))   # the default pool: min(4 K, 256, the catalogue)
    assert rep.users == [0, 2] and rep.name == "diversify" and rep.needs == "rerank_device" and rep.item_counts.tolist() == [0, 1, 2, 0, 0, 0]
    assert rep.group_labels[0].strip() == "all:" and len(rep.group_labels) >= 2
    rep = DiversifyReport(ds, train, test, 3, pool=5, lambdas=(1, 0.25))
    assert (rep.top_k, rep.pool, rep.lambdas) == (3, 5, (1.0, 0.25))
    big = types.SimpleNamespace(num_items=5000, num_users=3)
    assert DiversifyReport(big, train, test, 10).pool == 40 and DiversifyReport(big, train, test, 100).pool == 256
    with pytest.raises(TypeError):
        rep.evaluate(object())


def test_basic_model_switches():
    from elimrec_amd import ops
    g = load_golden("ml3")
    model, _ = build_model_from_fixture(g, "cpu")
    assert model.diversify_reporter is None
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--diversify_report=0", "--diversify_pool=1"])
    assert model.diversify_reporter is None
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--diversify_report=3", "--group_view=[2,4]"])
    rep = model.diversify_reporter
    assert (rep.top_k, rep.pool, rep.lambdas) == (3, min(12, model.num_items), (1.0, 0.9, 0.7, 0.5)) and len(rep.group_labels) >= 2
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--diversify_report=3", "--diversify_pool=5", "--diversify_lambda=[1.0,0.3]"])
    rep = model.diversify_reporter
    assert (rep.top_k, rep.pool, rep.lambdas) == (3, 5, (1.0, 0.3)) and rep.num_items == model.num_items
    for bad in (["--diversify_report=1"], ["--diversify_report=-2"], ["--diversify_report=%d" % (model.num_items + 1)],
                ["--diversify_report=3", "--diversify_pool=2"], ["--diversify_report=3", "--diversify_pool=%d" % (model.num_items + 1)],
                ["--diversify_report=3", "--diversify_pool=%d" % (ops.LIST_MAX_K + 1)], ["--diversify_report=3", "--diversify_lambda=[1.2]"],
                ["--diversify_report=3", "--diversify_lambda=[]"], ["--diversify_report=3", "--diversify_lambda=0.5"]):
        with pytest.raises(ValueError):
            build_model_from_fixture(g, "cpu", extra_argv=bad)
    for kw in (dict(k=0), dict(k=3, pool=2), dict(k=3, pool=model.num_items + 1), dict(k=3, lam=1.5), dict(k=3, lam=-0.5), dict(k=3, space="x")):
        with pytest.raises(ValueError):
            model.recommend_diverse([0, 1], **kw)
    with pytest.raises(IndexError):
        model.recommend_diverse([0], 3, exclude={0: [model.num_items]})
