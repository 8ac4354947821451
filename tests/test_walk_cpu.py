"""The host side of the weighted two-step walk (no GPU): ops.rp3_weights and ops.WalkWeights by hand, every argument error of
ops.walk_topk that is raised before the device is needed -- the overflow bound among them --, the exact model of tests/walk_model.py
against a dense float64 RP3beta, the --baseline_* switches with the source rp3, and the new entries in the header and the binding."""
import os

import numpy as np
import pytest
import torch

import cooccur_model as cm
import walk_model as wm
from helpers import build_model_from_fixture, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND_USERS = [[0, 1, 2], [1, 2], [0, 2], [3], []]             # 5 users x 5 items: user 4 holds nothing, item 4 has no user


def _index(user_lists, n_query, side="item"):
    from elimrec_amd import ops
    o_ptr, o_nbr = cm.csr_of(user_lists)
    q_ptr, q_nbr = cm.transpose_csr(o_ptr, o_nbr, n_query)
    if side == "item":
        return ops.CooccurIndex(q_ptr, q_nbr, o_ptr, o_nbr, n_query, len(user_lists), "cpu")
    return ops.CooccurIndex(o_ptr, o_nbr, q_ptr, q_nbr, len(user_lists), n_query, "cpu")


def test_rp3_weights_by_hand():
    from elimrec_amd import ops
    assert (ops.WALK_FRAC_BITS, ops.WALK_MAX_K) == (40, 256)
    index = _index(HAND_USERS, 5)
    assert index.deg.tolist() == [2, 2, 3, 1, 0] and index.deg_other.tolist() == [3, 2, 2, 1, 0]
    w = ops.rp3_weights(index, 1.0, 0.6)
    assert w.mid_weight.dtype == torch.int64 and w.row_scale.dtype == torch.float64 and w.col_scale.dtype == torch.float64
    assert w.mid_weight.tolist() == [int(np.rint(2.0 ** 40 / 3.0)), 2 ** 39, 2 ** 39, 2 ** 40, 0]     # the degree-0 user: 0
    assert w.row_scale.tolist() == [0.5, 0.5, 1.0 / 3.0, 1.0, 0.0]                                     # the degree-0 item: 0
    assert w.col_scale.tolist() == [2.0 ** -0.6, 2.0 ** -0.6, 3.0 ** -0.6, 1.0, 0.0]
    assert (w.n_other, w.n_query, w.max_weight) == (5, 5, 2 ** 40)
    want = wm.rp3_weights(index.deg, index.deg_other, 1.0, 0.6)
    assert all(np.array_equal(a.numpy(), b) for a, b in zip((w.mid_weight, w.row_scale, w.col_scale), want))
    # alpha = beta = 0: the walks are counted -- every weight 2^40, every scale 1, but for the rows of degree 0
    w = ops.rp3_weights(index, 0, 0.0)
    assert w.mid_weight.tolist() == [2 ** 40] * 4 + [0] and w.row_scale.tolist() == w.col_scale.tolist() == [1.0] * 4 + [0.0]
    # the user side
    w = ops.rp3_weights(_index(HAND_USERS, 5, "user"), 0.5, 4)
    assert w.row_scale.tolist() == [3.0 ** -0.5, 2.0 ** -0.5, 2.0 ** -0.5, 1.0, 0.0] and w.col_scale[0].item() == 3.0 ** -4.0
    assert w.mid_weight.tolist() == [int(np.rint(2.0 ** -0.5 * 2.0 ** 40))] * 2 + [int(np.rint(3.0 ** -0.5 * 2.0 ** 40)), 2 ** 40, 0]
    for bad in (-0.1, 4.5, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="alpha"):
            ops.rp3_weights(index, bad, 0.6)
        with pytest.raises(ValueError, match="beta"):
            ops.rp3_weights(index, 1.0, bad)
    with pytest.raises(TypeError):
        ops.rp3_weights(None, 1.0, 0.6)


def test_walk_weights_are_checked_on_the_host():
    from elimrec_amd import ops
    ok = (np.asarray([1, 0, 5]), np.asarray([1.0, 0.0]), np.asarray([0.5, 2.0]))
    w = ops.WalkWeights(*ok, "cpu")
    assert (w.n_other, w.n_query, w.max_weight, w.max_scale) == (3, 2, 5, 2.0) and w.mid_weight.dtype == torch.int64
    w = ops.WalkWeights(np.zeros(0, np.int64), np.zeros(0), np.zeros(0), "cpu")
    assert (w.n_other, w.n_query, w.max_weight, w.max_scale) == (0, 0, 0, 0.0)
    for bad in ((np.asarray([1, -1, 5]), ok[1], ok[2]),                       # a negative weight
                (np.asarray([1.0, 0.0, 5.0]), ok[1], ok[2]),                  # wrong dtypes
                (ok[0], ok[1].astype(np.float32), ok[2]),
                (ok[0], ok[1], np.asarray([1, 2])),
                (ok[0].reshape(3, 1), ok[1], ok[2]),                          # wrong shapes and lengths
                (ok[0], ok[1], np.asarray([0.5, 2.0, 1.0])),
                (ok[0], np.asarray([1.0, np.nan]), ok[2]),                    # scales that are not finite or negative
                (ok[0], ok[1], np.asarray([np.inf, 1.0])),
                (ok[0], np.asarray([1.0, -1e-300]), ok[2])):
        with pytest.raises(ValueError):
            ops.WalkWeights(*bad, "cpu")


def test_walk_topk_refuses_before_the_device():
    """Every one of these is raised on a CPU index: nothing has touched a device yet."""
    from elimrec_amd import ops
    index = _index(HAND_USERS, 5)
    assert index.walk.tolist() == [5, 5, 7, 1, 0]
    out = torch.empty(2, 3, dtype=torch.int32)
    rows = [0, 2]
    good = ops.rp3_weights(index, 1.0, 0.6)
    for K in (0, 257, 2.0, True):
        with pytest.raises(ValueError, match="K must be"):
            ops.walk_topk(index, rows, K, good, out)
    with pytest.raises(IndexError):
        ops.walk_topk(index, [5], 3, good, out)
    with pytest.raises(TypeError):
        ops.walk_topk(index, rows, 3, (good.mid_weight, good.row_scale, good.col_scale), out)
    with pytest.raises(ValueError, match="the index has"):                    # lengths that do not fit the index
        ops.walk_topk(index, rows, 3, ops.WalkWeights(np.ones(4, np.int64), np.ones(5), np.ones(5), "cpu"), out)
    with pytest.raises(ValueError, match="the index has"):
        ops.walk_topk(index, rows, 3, ops.WalkWeights(np.ones(5, np.int64), np.ones(4), np.ones(4), "cpu"), out)
    # the overflow bound: (the longest walk of the rows) x (the largest weight) >= 2^62; rows [0, 2] walk 7 at most, row 3 walks 1
    at = -(-2 ** 62 // 7)                                                     # the least weight with 7 x weight >= 2^62
    heavy = lambda m: ops.WalkWeights(np.asarray([1, 1, m, 1, 1]), np.ones(5), np.ones(5), "cpu")
    with pytest.raises(ValueError, match="overflow"):
        ops.walk_topk(index, rows, 3, heavy(at), out)
    with pytest.raises(ValueError, match="overflow"):
        ops.walk_topk(index, [3], 3, heavy(2 ** 62), out[:1])
    with pytest.raises(RuntimeError):                                          # one below the bound: the next stop is the device
        ops.walk_topk(index, rows, 3, heavy(at - 1), out)
    with pytest.raises(RuntimeError):
        ops.walk_topk(index, [3], 3, heavy(at), out[:1])
    with pytest.raises(ValueError, match="float64"):                          # finite scales whose product is not
        ops.walk_topk(index, rows, 3, ops.WalkWeights(np.full(5, 2 ** 40), np.full(5, 1e200), np.full(5, 1e200), "cpu"), out)
    # the form rule and the workspace, host arithmetic
    assert [ops.walk_rows_in_lds(W) for W in (0, 2047, 2048, 2049)] == [True, True, True, False]
    with pytest.raises(ValueError):
        ops.walk_rows_in_lds(-1)
    assert ops.walk_workspace(0, 1000) == 0 and ops.walk_workspace(3, 1000) == 3 * 1000 * 8 and ops.walk_workspace(5000, 7) == 512 * 7 * 8
    with pytest.raises(ValueError):
        ops.walk_workspace(-1, 10)
    assert "elimrec_walk_topk(" in open(os.path.join(ROOT, "include", "elimrec_hip.h")).read()
    assert "walk.hip" in open(os.path.join(ROOT, "elimrec_amd", "csrc", "Makefile")).read()


def _random_graph(seed, n_users, n_items, max_deg):
    """User lists without a repeated edge, every degree <= max_deg on BOTH sides, some users and items without an edge."""
    rng = np.random.default_rng(seed)
    room = np.full(n_items, max_deg)
    room[-1] = 0                                             # the last item has no user
    users = []
    for _ in range(n_users):
        free = np.flatnonzero(room > 0)
        held = rng.choice(free, size=min(free.size, int(rng.integers(0, max_deg + 1))), replace=False)
        room[held] -= 1
        users.append(held.tolist())
    return users


@pytest.mark.parametrize("alpha, beta", [(1.0, 0.6), (0.5, 0.0), (1.0, 0.0), (0.0, 0.0), (0.7, 1.3), (1.0, 4.0)])
def test_the_model_against_dense_float64_rp3beta(alpha, beta):
    """Degrees <= 64 and alpha <= 1. A weight is rint(deg^-alpha 2^40) with deg^-alpha >= 2^-6, so its rounding is at most 2^-41 x
    64 = 2^-35 relative per term, and so is the sum's (the terms are positive); the reference's own float64 sums and the model's
    three multiplies add a few 2^-53. All of it is far below half an fp32 ulp (2^-24), so after the one rounding to fp32 the two
    differ by one fp32 ulp at most: |val - ref| <= 2^-23 |ref|, the values compared in fp32."""
    worst = 0.0
    for seed, (U, I, D) in enumerate(((60, 40, 8), (300, 200, 64), (500, 120, 64))):
        users = _random_graph(30 + seed, U, I, D)
        o_ptr, o_nbr = cm.csr_of(users)
        q_ptr, q_nbr = cm.transpose_csr(o_ptr, o_nbr, I)
        deg_q, deg_o = np.diff(q_ptr), np.diff(o_ptr)
        assert deg_q.max() <= 64 and deg_o.max() <= 64 and deg_q.min() == 0
        ref = wm.rp3_dense(q_ptr, q_nbr, U, alpha, beta).astype(np.float32).astype(np.float64)
        idx, val = wm.topk(q_ptr, q_nbr, U, np.arange(I), I, *wm.rp3_weights(deg_q, deg_o, alpha, beta))
        reach = (cm.incidence(q_ptr, q_nbr, U) @ cm.incidence(q_ptr, q_nbr, U).T).toarray() > 0
        np.fill_diagonal(reach, False)
        for q in range(I):
            listed = idx[q] >= 0
            assert sorted(idx[q][listed].tolist()) == np.flatnonzero(reach[q]).tolist()        # the rows one walk reaches, q left out
            got, want = val[q][listed].astype(np.float64), ref[q, idx[q][listed]]
            assert (np.abs(got - want) <= 2.0 ** -23 * np.abs(want)).all(), (alpha, beta, seed, q)
            worst = max(worst, float((np.abs(got - want) / want).max()) if got.size else 0.0)
            v = val[q][listed]
            assert (v[:-1] >= v[1:]).all() and (idx[q][listed][:-1][v[:-1] == v[1:]] < idx[q][listed][1:][v[:-1] == v[1:]]).all()
    print("alpha %g beta %g: worst relative difference %.3g (bound %.3g)" % (alpha, beta, worst, 2.0 ** -23))


def test_the_switches_and_the_report_arguments():
    from elimrec_amd.basic_model import baseline_sources
    from elimrec_amd.evaluator import BaselineReport
    assert baseline_sources("[co,rp3]") == ("co", "rp3") and baseline_sources(["rp3"]) == ("rp3",)
    g = load_golden("ml3")
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--baseline_report=10", "--baseline_sources=[co,rp3]"])
    rep = model.baseline_reporter
    assert rep.sources == ("co", "rp3") and (rep.alpha, rep.beta) == (1.0, 0.6) and rep.labels[len(rep.group_labels)].startswith("rp3 all:")
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--baseline_report=10", "--baseline_sources=[rp3]", "--baseline_alpha=0.5",
                                                              "--baseline_beta=0"])
    rep = model.baseline_reporter
    assert rep.sources == ("rp3",) and (rep.alpha, rep.beta) == (0.5, 0.0) and isinstance(rep.beta, float)
    for bad in (["--baseline_alpha=-1"], ["--baseline_beta=4.5"], ["--baseline_alpha=nan"], ["--baseline_beta=inf"], ["--baseline_alpha=x"],
                ["--baseline_report=10", "--baseline_sources=[rp3]", "--baseline_beta=1e999"], ["--baseline_alpha=True"]):
        with pytest.raises(ValueError):                                      # at start-up, whether or not the report is on
            build_model_from_fixture(g, "cpu", extra_argv=bad)
    train, test = model.dataset.get_user_train_dict(), model.dataset.get_user_test_dict()
    for bad in (dict(alpha=-0.5), dict(beta=5), dict(alpha=float("nan")), dict(beta="0.6")):
        with pytest.raises(ValueError):
            BaselineReport(model.dataset, train, test, [10], sources=("rp3",), **bad)
    rep = BaselineReport(model.dataset, train, test, [10], sources=("rp3",))
    assert (rep.alpha, rep.beta, rep.rp3_info) == (1.0, 0.6, None)
    with pytest.raises(RuntimeError):                                        # a CPU model
        rep.evaluate(model)
    # the model's own checks, before the device
    for bad in (-1.0, 4.01, float("nan"), None):
        with pytest.raises(ValueError, match="alpha"):
            model.rp3_items([0], 3, alpha=bad)
        with pytest.raises(ValueError, match="beta"):
            model.recommend_knn([0], 3, source="rp3", beta=bad)
        with pytest.raises(ValueError, match="beta"):
            model.neighbour_lists("rp3", 5, beta=bad)
    assert [tuple(t.shape) for t in model.recommend_knn([], 5, source="rp3")] == [(0, 5)] * 3
    with pytest.raises(ValueError, match="source must be"):
        model.recommend_knn([0], 3, source="rp4", alpha=-1.0)               # alpha and beta are read by "rp3" alone
    with pytest.raises(RuntimeError):
        model.recommend_knn([0], 3, source="co", alpha=-1.0)                # ... and ignored by the other sources (a CPU model)
    with pytest.raises(ValueError):
        model.rp3_items([0], 257)
    with pytest.raises(IndexError):
        model.rp3_users([model.num_users], 3)
    for call in (lambda: model.rp3_items([0], 3), lambda: model.rp3_users([0], 3), lambda: model.neighbour_lists("rp3"),
                 lambda: model.recommend_knn([0], 3, source="rp3")):
        with pytest.raises(RuntimeError):                                    # a CPU model
            call()
    assert "not tuned" in " ".join(model.rp3_items.__doc__.lower().split()) and "untrained" in model.rp3_items.__doc__
    assert "not tuned" in " ".join(model.rp3_users.__doc__.lower().split())


def test_the_binding_and_the_registry():
    from elimrec_amd import _lib, ops, torch_ops
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "elimrec_hip.h")).read()
    for name in ("elimrec_walk_topk", "elimrec_walk_workspace", "elimrec_walk_slots", "elimrec_walk_max_k", "elimrec_walk_groups",
                 "elimrec_walk_frac_bits", "elimrec_walk_rows_in_lds"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name + "(" in header
    assert lib.elimrec_walk_frac_bits() == ops.WALK_FRAC_BITS and lib.elimrec_walk_max_k() == ops.WALK_MAX_K
    assert lib.elimrec_walk_slots() == ops.WALK_SLOTS == ops.COOCCUR_SLOTS    # one W, one form rule
    assert tuple(ops.COOCCUR_MEASURES) == ("count", "cosine", "jaccard")
    torch_ops.load()
    assert hasattr(torch.ops.elimrec, "walk_topk")
