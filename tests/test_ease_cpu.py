"""EASE without a device: the numpy model of the block sweep against np.linalg.inv, the ranking comparer, and the parameter,
catalogue-size and switch checks that come before anything touches the device."""
import os

import numpy as np
import pytest
import torch

import ease_model as em
from helpers import ROOT


def _binary(U, I, seed):
    X = (np.random.default_rng(seed).random((U, I)) < 0.15).astype(np.float64)
    if I > 1:
        X[:, -1] = X[:, 0]
    X[:, I // 3] = 0.0
    return X


@pytest.mark.parametrize("l2", [0.5, 5.0, 500.0])
@pytest.mark.parametrize("n", [1, 17, 64, 65, 129, 200])
def test_sweep_model_equals_inv(n, l2):
    """The sweep in numpy stays within 2 units of 64 n kappa 2^-53 / 64 on these matrices; the GPU tests allow 64."""
    G = em.gram(_binary(max(8, n // 2), n, seed=n), l2)
    P, ref = em.sweep_inverse(G), np.linalg.inv(G)
    bound = em.inverse_bound(n, em.kappa(G))
    assert np.abs(P - ref).max() / np.abs(ref).max() <= bound / 32 and np.abs(G @ P - np.eye(n)).max() <= bound / 32
    assert abs(P[n // 3, n // 3] - 1.0 / l2) <= 1e-15 / l2


def test_dense_ease_and_the_score_rule():
    X = _binary(30, 20, seed=1)
    P = em.ease_P(X, 5.0)
    B = -P / np.diagonal(P)[None, :]
    B[np.diag_indices(20)] = 0.0
    h = np.flatnonzero(X[3])
    assert np.allclose(em.scores(P, h), X[3] @ B, rtol=1e-6, atol=1e-7)
    assert em.scores(P, h)[20 // 3] == 0.0                   # a cold item scores exactly 0
    ids, vals, s = em.topk(P, h, h, 25)
    assert (ids[20 - h.size:] == -1).all() and np.isneginf(vals[20 - h.size:]).all() and not set(ids[:20 - h.size]) & set(h)
    assert (np.diff(vals[:20 - h.size]) <= 0).all()


def test_rank_comparer():
    s = np.array([5.0, 4.0, 4.0 + 1e-9, 1.0, 3.0])
    order = em.full_order(s, [])
    assert order.tolist() == [0, 2, 1, 4, 3]
    assert em.rank_equal_up_to([0, 2, 1], order, s, 0.0) == (True, 0)
    assert em.rank_equal_up_to([0, 1, 2], order, s, 0.0)[0] is False
    assert em.rank_equal_up_to([0, 1, 2], order, s, 1e-6) == (True, 2)
    assert em.rank_equal_up_to([0, 1], order, s, 1e-6) == (True, 1)          # the run crosses the end of the list
    assert em.rank_equal_up_to([0, 4], order, s, 1e-6)[0] is False
    assert em.rank_equal_up_to([0, 2, 1, 4, 3, -1], order, s, 0.0) == (True, 0)
    assert em.rank_equal_up_to([0, 2, 1, 4, 3, 0], order, s, 0.0)[0] is False


def test_reference_alone_stays_within_the_cap():
    """The generated split of the end-to-end GPU tests (test_ease_gpu: U = 150, I = 130, l2 = 5, seed 7): the share of list slots
    whose reference score lies within tol = 64 I kappa 2^-53 max|s| of a neighbour's is 0.0067 over all 150 users at K = 20 -- the
    20 slots of user 0, who has no history and scores 0 everywhere --, below the cap of 2 %. Seeds 1 .. 5 give the same share."""
    _, split = em.generated_split()
    P, kap = em.reference(split)
    users = np.arange(em.E2E_U)
    lists = np.stack([em.topk(P, split["train"].get(u, []), split["train"].get(u, []), em.E2E_K)[0] for u in users])
    share = em.compare(lists, users, split, P, kap)
    assert 0.0 < share <= 0.02, share
    lists[3, 0], lists[3, 1] = lists[3, 1], lists[3, 0]      # two slots exchanged across distinct scores are not excused
    with pytest.raises(AssertionError):
        em.compare(lists, users, split, P, kap)


def test_parameters_and_catalogue_bound():
    from elimrec_amd import ops
    assert ops._ease_params("x") == 500.0 and ops._ease_params("x", 5, 100) == 5.0
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), True, "5", None):
        with pytest.raises(ValueError, match="l2"):
            ops._ease_params("x", bad)
    assert 8 * ops.EASE_MAX_ITEMS ** 2 + 2 * 64 * ops.EASE_MAX_ITEMS * 8 <= 201 * 2 ** 30 and ops.EASE_MAX_K == 256
    ops._ease_params("x", 5.0, ops.EASE_MAX_ITEMS)
    with pytest.raises(ValueError, match="EASE_MAX_ITEMS"):
        ops._ease_params("x", 5.0, ops.EASE_MAX_ITEMS + 1)


def test_ops_checks_come_before_the_device():
    from elimrec_amd import ops
    P = torch.zeros(4, 4, dtype=torch.float64)
    with pytest.raises(ValueError, match="square"):
        ops.spd_inverse(torch.zeros(3, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="n >= 1"):
        ops.spd_inverse(torch.zeros(0, 0, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.spd_inverse(P)
    with pytest.raises(TypeError, match="CooccurIndex"):
        ops.gram_counts(None, 1.0, P)
    with pytest.raises(ValueError, match="1 <= K"):
        ops.ease_topk(P, None, [0], 0, None)
    with pytest.raises(ValueError, match="1 <= K"):
        ops.ease_topk(P, None, [0], 257, None)
    with pytest.raises(TypeError, match="HistoryIndex"):
        ops.ease_topk(P, None, [0], 5, None)
    hist = ops.HistoryIndex([0, 1, 2], [0, 3], "cpu", n_items=4)
    with pytest.raises(IndexError, match="users span"):
        ops.ease_topk(P, hist, [2], 5, None)
    with pytest.raises(IndexError, match="catalogue"):
        ops.ease_topk(P, ops.HistoryIndex([0, 1], [0], "cpu"), [0], 5, None)
    with pytest.raises(ValueError, match="same users"):
        ops.ease_topk(P, hist, [0], 5, None, excl=ops.HistoryIndex([0, 1], [0], "cpu", n_items=4))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.ease_topk(P, hist, [0], 5, None)


def test_switches_model_and_report_refuse_before_the_device(monkeypatch):
    from elimrec_amd import ops
    from elimrec_amd.basic_model import baseline_sources
    from helpers import build_model_from_fixture, load_golden
    assert baseline_sources("[co,ease]") == ("co", "ease")
    g = load_golden("ml3")
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--baseline_report=10", "--baseline_sources=[co,ease]", "--baseline_l2=20.5"])
    assert model.baseline_reporter.sources == ("co", "ease") and model.baseline_reporter.l2 == 20.5
    with pytest.raises(ValueError, match="'ease'"):
        build_model_from_fixture(g, "cpu", extra_argv=["--baseline_report=10", "--baseline_sources=[co,easy]"])
    for switch in ("--baseline_l2=0", "--baseline_l2=-3.0"):
        with pytest.raises(ValueError, match="baseline_l2"):
            build_model_from_fixture(g, "cpu", extra_argv=[switch])
    with pytest.raises(ValueError, match="l2"):
        model.fit_ease(l2=0.0)
    with pytest.raises(ValueError, match="l2"):
        model.recommend_ease([0], 5, l2=float("nan"))
    with pytest.raises(ValueError, match="K must be"):
        model.recommend_ease([0], 257)
    with pytest.raises(IndexError):
        model.recommend_ease([model.num_users], 5)
    with pytest.raises(IndexError):
        model.recommend_ease([0], 5, history={0: [model.num_items]})
    assert tuple(model.recommend_ease([], 5).ids.shape) == (0, 5)
    assert model.drop_ease() == 0 and model.drop_ease(5.0) == 0
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.fit_ease()
    monkeypatch.setattr(ops, "EASE_MAX_ITEMS", model.num_items - 1)
    with pytest.raises(ValueError, match="EASE_MAX_ITEMS"):
        model.fit_ease()
    with pytest.raises(ValueError, match="EASE_MAX_ITEMS"):
        model.recommend_ease([0], 5)


def test_exports():
    from elimrec_amd import _lib, ops, torch_ops
    header = open(os.path.join(ROOT, "include", "elimrec_hip.h")).read()
    for name in ("elimrec_gram_counts", "elimrec_spd_inverse", "elimrec_spd_inverse_workspace", "elimrec_ease_topk",
                 "elimrec_ease_topk_workspace", "elimrec_ease_block", "elimrec_ease_hist_stage"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name) and name + "(" in header
    assert "ease.hip" in open(os.path.join(ROOT, "elimrec_amd", "csrc", "Makefile")).read()
    assert ops.EASE_BLOCK == 64 and ops.EASE_HIST_STAGE >= 16
    assert ops.spd_inverse_workspace(65) == 64 * 64 * 8 + 2 * 64 * 128 * 8
    ns = torch_ops.load()
    assert all(hasattr(ns, x) for x in ("gram_counts", "spd_inverse", "ease_topk")) and {"gram_counts", "spd_inverse", "ease_topk"} <= set(torch_ops.OPS)
