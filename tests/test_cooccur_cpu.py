"""The host side of the co-interaction neighbours (no GPU): the exact model of tests/cooccur_model.py by hand, every argument error
of ops.CooccurIndex / cooccur_topk, of EliMRec.co_items / co_users and of CoNeighbourReport before the device is needed, the form
rule at its edge, the --co_report switch, and the new entries in the header, the binding and the torch registry."""
import inspect
import os

import numpy as np
import pytest
import torch

import cooccur_model as cm
from helpers import build_model_from_fixture, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND_USERS = [[0, 1, 2], [1, 2], [0, 2], [3]]


def _hand():
    o_ptr, o_nbr = cm.csr_of(HAND_USERS)
    q_ptr, q_nbr = cm.transpose_csr(o_ptr, o_nbr, 5)
    return q_ptr, q_nbr, o_ptr, o_nbr


def test_the_model_by_hand():
    """4 users x 5 items: user 0 took {0, 1, 2}, user 1 {1, 2}, user 2 {0, 2}, user 3 {3}; nobody took item 4.
    Degrees a = (2, 2, 3, 1, 0). Co-counts: c(0, 1) = 1 (user 0), c(0, 2) = 2 (users 0, 2), c(1, 2) = 2 (users 0, 1); item 3's only
    user has degree 1 and item 4 has no user: both rows are fillers.
      count    row 0: (2: 2, 1: 1)                 row 2: (0: 2, 1: 2) -- a tie, the lower id first
      cosine   row 0: (2: 2 / sqrt(6), 1: 1 / 2)   row 2: (0: 2 / sqrt(6), 1: 2 / sqrt(6))
      jaccard  row 0: (2: 2 / 3, 1: 1 / 3)         row 2: (0: 2 / 3, 1: 2 / 3)
    W = (3 + 2, 3 + 2, 3 + 2 + 2, 1, 0)."""
    q_ptr, q_nbr, o_ptr, o_nbr = _hand()
    assert q_ptr.tolist() == [0, 2, 4, 7, 8, 8] and q_nbr.tolist() == [0, 2, 0, 1, 0, 1, 2, 3]
    assert cm.walk(q_ptr, q_nbr, 4).tolist() == [5, 5, 7, 1, 0]
    f32 = lambda xs: np.asarray(xs, dtype=np.float64).astype(np.float32).tolist()
    want = {"count": (f32([2, 1]), f32([2, 2])), "cosine": (f32([2 / np.sqrt(6.0), 0.5]), f32([2 / np.sqrt(6.0)] * 2)),
            "jaccard": (f32([2 / 3.0, 1 / 3.0]), f32([2 / 3.0] * 2))}
    for measure, (row0, row2) in want.items():
        idx, val, cnt = cm.topk(q_ptr, q_nbr, 4, [0, 1, 2, 3, 4], 3, measure)
        assert idx.tolist() == [[2, 1, -1], [2, 0, -1], [0, 1, -1], [-1] * 3, [-1] * 3]
        assert cnt.tolist() == [[2, 1, 0], [2, 1, 0], [2, 2, 0], [0] * 3, [0] * 3]
        assert val[0, :2].tolist() == row0 and val[2, :2].tolist() == row2 and np.isneginf(val[:, 2]).all() and np.isneginf(val[3:]).all()
        assert cm.topk(q_ptr, q_nbr, 4, [2], 1, measure)[0].tolist() == [[0]]
    # a repeated edge is an edge of its own: user 0 lists item 1 twice, so c(0, 1) = 1 x 2 and deg(1) = 2
    o_ptr, o_nbr = cm.csr_of([[0, 1, 1]])
    q_ptr, q_nbr = cm.transpose_csr(o_ptr, o_nbr, 2)
    idx, val, cnt = cm.topk(q_ptr, q_nbr, 1, [0, 1], 1, "cosine")
    assert cnt.tolist() == [[2], [2]] and val.tolist() == f32([[2 / np.sqrt(2.0)]] * 2)
    # the report's columns: two listed co-neighbours, one of them in the space's list
    rows = cm.report_rows(np.asarray([[2, 1, -1], [-1, -1, -1]]), np.asarray([[0.5, 0.25, -np.inf]] * 2, dtype=np.float32), [2, 2, 3],
                          [np.asarray([[1, 0, -1], [0, 2, 1]])])
    assert rows[0].tolist() == [2.0, 0.375, 2.5, 0.5] and rows[1, 0] == 0 and np.isnan(rows[1, 1:]).all()


def test_index_checks_and_host_arithmetic():
    from elimrec_amd import ops
    q_ptr, q_nbr, o_ptr, o_nbr = _hand()
    index = ops.CooccurIndex(q_ptr, q_nbr, o_ptr, o_nbr, 5, 4, "cpu")
    assert (index.n_query, index.n_other, index.n_edges) == (5, 4, 8)
    assert index.deg.tolist() == [2, 2, 3, 1, 0] and index.walk.tolist() == [5, 5, 7, 1, 0]
    assert index.has_neighbour.tolist() == [True, True, True, False, False]
    for bad in ((q_ptr[:-1], q_nbr, o_ptr, o_nbr), (q_ptr, q_nbr, o_ptr[1:], o_nbr),                       # entry counts
                ([0, 4, 2, 7, 8, 8], q_nbr, o_ptr, o_nbr), ([1, 2, 4, 7, 8, 8], q_nbr, o_ptr, o_nbr),      # not ascending from 0
                (q_ptr, q_nbr[:-1], o_ptr, o_nbr), (q_ptr, q_nbr, [0, 3, 5, 7, 7], o_nbr[:-1])):           # the edges
        with pytest.raises(ValueError):
            ops.CooccurIndex(*bad, 5, 4, "cpu")
    for bad in ((q_ptr, [0, 2, 0, 1, 0, 1, 2, 4], o_ptr, o_nbr), (q_ptr, q_nbr, o_ptr, [0, 1, 2, 1, 2, 0, 5, 3]),
                (q_ptr, [-1, 2, 0, 1, 0, 1, 2, 3], o_ptr, o_nbr)):
        with pytest.raises(IndexError):
            ops.CooccurIndex(*bad, 5, 4, "cpu")
    with pytest.raises(TypeError):
        ops.CooccurIndex(q_ptr, q_nbr.astype(np.float32), o_ptr, o_nbr, 5, 4, "cpu")
    # from_train: both sides of one dict
    train = {u: items for u, items in enumerate(HAND_USERS)}
    item = ops.CooccurIndex.from_train(train, 4, 5, "item", "cpu")
    user = ops.CooccurIndex.from_train(train, 4, 5, "user", "cpu")
    assert item.q_ptr.tolist() == q_ptr.tolist() and item.q_nbr.tolist()[:8] == q_nbr.tolist() and item.o_nbr.tolist() == o_nbr.tolist()
    assert user.q_ptr.tolist() == o_ptr.tolist() and (user.n_query, user.n_other) == (4, 5) and user.walk.tolist() == [7, 5, 5, 1]
    with pytest.raises(ValueError):
        ops.CooccurIndex.from_train(train, 4, 5, "items", "cpu")
    with pytest.raises(IndexError):
        ops.CooccurIndex.from_train({0: [5]}, 4, 5, "item", "cpu")
    with pytest.raises(IndexError):
        ops.CooccurIndex.from_train({4: [0]}, 4, 5, "item", "cpu")


def test_op_argument_errors_fire_without_a_gpu():
    from elimrec_amd import ops
    index = ops.CooccurIndex(*_hand(), 5, 4, "cpu")
    out = torch.zeros(2, 3, dtype=torch.int32)
    for bad in (0, 257, -1, 2.0, True, "3"):
        with pytest.raises(ValueError, match="1 <= K <= 256"):
            ops.cooccur_topk(index, [0, 1], bad, out)
    for bad in ("dice", "Cosine", None, 1):
        with pytest.raises(ValueError, match="measure is one of"):
            ops.cooccur_topk(index, [0, 1], 3, out, measure=bad)
    for bad in ([5], [-1], [0, 7]):
        with pytest.raises(IndexError):
            ops.cooccur_topk(index, bad, 3, out)
        with pytest.raises(IndexError):
            ops.cooccur_walk(index, bad)
    with pytest.raises(TypeError):
        ops.cooccur_topk(index, [0.5], 3, out)
    with pytest.raises(TypeError):
        ops.cooccur_topk((1, 2), [0], 3, out)
    with pytest.raises(RuntimeError, match="HIP device tensor"):             # no CPU path
        ops.cooccur_topk(index, [0, 1], 3, out)
    assert ops.COOCCUR_MAX_K == 256 and sorted(ops.COOCCUR_MEASURES) == ["cosine", "count", "jaccard"]


def test_the_form_rule_at_its_edge():
    from elimrec_amd import _lib, ops
    S = ops.COOCCUR_SLOTS
    assert S == 4096 and S & (S - 1) == 0
    assert ops.cooccur_rows_in_lds(0) and ops.cooccur_rows_in_lds(S // 2) and not ops.cooccur_rows_in_lds(S // 2 + 1)
    assert not ops.cooccur_rows_in_lds(2 ** 40)
    with pytest.raises(ValueError):
        ops.cooccur_rows_in_lds(-1)
    assert _lib.load().elimrec_cooccur_rows_in_lds(-1) == -1 and _lib.load().elimrec_cooccur_max_k() == ops.COOCCUR_MAX_K
    # the workspace: one int32 counter row of n entries per dense-form workgroup, COOCCUR_GROUPS of them at most (host arithmetic)
    G = ops.COOCCUR_GROUPS
    assert ops.cooccur_workspace(0, 1000) == 0 and ops.cooccur_workspace(3, 1000) == 12000
    assert ops.cooccur_workspace(G, 1000) == ops.cooccur_workspace(10 * G, 1000) == G * 4000 and ops.cooccur_workspace(1, 3) == 16
    with pytest.raises(ValueError):
        ops.cooccur_workspace(-1, 10)
    with pytest.raises(ValueError):
        ops.cooccur_workspace(1, 2 ** 31)
    assert ops.cooccur_workspace(G, 2 ** 24) > ops.COOCCUR_WORKSPACE_BUDGET    # such a catalogue is an error, not a third form


def test_model_argument_errors_fire_without_a_gpu():
    g = load_golden("ml3")
    model, _ = build_model_from_fixture(g, "cpu")
    for call, n in ((model.co_items, model.num_items), (model.co_users, model.num_users)):
        for bad in (0, 257, 1.5):
            with pytest.raises(ValueError, match="1 <= K <= 256"):
                call([0], bad)
        with pytest.raises(ValueError, match="measure is one of"):
            call([0], 3, measure="dice")
        with pytest.raises(IndexError):
            call([0, n], 3)
        with pytest.raises(IndexError):
            call([-1], 3)
        with pytest.raises(RuntimeError):                                    # a CPU model
            call([0], 3)
    with pytest.raises(ValueError, match="side must be"):
        model.co_neighbours_device("items", [0], 3, "cosine", None, None)
    with pytest.raises(ValueError, match="1 <= K <= 256"):
        model.co_neighbours_device("item", [0], 0, "cosine", None, None)
    assert "untrained" in model.co_items.__doc__ and "untrained" in model.co_users.__doc__
    assert "untrained" in model.co_neighbours_device.__doc__


def test_report_arguments_and_the_switch():
    from elimrec_amd.evaluator import CoNeighbourReport, co_neighbour_columns
    assert co_neighbour_columns("va") == ("n", "co_n", "co_score", "co_pop", "co_overlap_fused", "co_overlap_v", "co_overlap_a")
    g = load_golden("ml3")
    model, _ = build_model_from_fixture(g, "cpu")
    assert model.co_reporter is None
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--co_report=0", "--co_measure=jaccard"])
    assert model.co_reporter is None                                          # 0 means off
    train = model.dataset.get_user_train_dict()
    with pytest.raises(TypeError):
        CoNeighbourReport(model.dataset, [], 3)
    for bad in (0, 257, 2.5, True):
        with pytest.raises(ValueError):
            CoNeighbourReport(model.dataset, train, bad)
    with pytest.raises(ValueError, match="measure is one of"):
        CoNeighbourReport(model.dataset, train, 3, measure="dice")
    with pytest.raises(ValueError):
        CoNeighbourReport(model.dataset, train, 3, item_group_view=[0])
    with pytest.raises(IndexError):
        CoNeighbourReport(model.dataset, {0: [0, model.num_items]}, 3)
    for bad in (["--co_report=-1"], ["--co_report=300"], ["--co_report=3", "--co_measure=dice"], ["--co_measure=dice"]):
        with pytest.raises(ValueError):
            build_model_from_fixture(g, "cpu", extra_argv=bad)
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--co_report=7", "--co_measure=count", "--item_group_view=[1,4]"])
    rep = model.co_reporter
    assert isinstance(rep, CoNeighbourReport) and (rep.k, rep.measure, rep.num_items) == (7, "count", model.num_items)
    assert build_model_from_fixture(g, "cpu", extra_argv=["--co_report=2"])[0].co_reporter.measure == "cosine"
    # an item has a co-neighbour iff one of its users has degree >= 2: the report's host rule against the model's lists
    u_ptr, u_items = cm.csr_of([list(train.get(u, [])) for u in range(model.num_users)])
    i_ptr, i_users = cm.transpose_csr(u_ptr, u_items, model.num_items)
    has = cm.topk(i_ptr, i_users, model.num_users, np.arange(model.num_items), 1, "count")[0][:, 0] >= 0
    assert rep.has_neighbour.tolist() == has.tolist()
    assert rep.group_labels[0] == "all:".ljust(12) and len(rep.group_labels) > 1
    assert rep._positions[0].tolist() == np.flatnonzero(has).tolist()
    assert sum(p.size for p in rep._positions[1:]) == has.sum()
    with pytest.raises(RuntimeError):                                        # a CPU model
        rep.evaluate(model)
    import main
    src = inspect.getsource(main.Net.__init__)
    assert "--co_report needs the whole cached item table on one rank: it is single-GPU" in src
    assert "[co-neighbours]" in inspect.getsource(main.Net)


def test_cooccur_entries_are_declared_bound_and_registered():
    from elimrec_amd import _lib, torch_ops
    header = open(os.path.join(ROOT, "include", "elimrec_hip.h")).read()
    for name in ("elimrec_cooccur_topk", "elimrec_cooccur_walk", "elimrec_cooccur_workspace", "elimrec_cooccur_slots",
                 "elimrec_cooccur_max_k", "elimrec_cooccur_groups", "elimrec_cooccur_rows_in_lds"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name) and name + "(" in header
    assert hasattr(torch_ops.load(), "cooccur_topk") and "cooccur_topk" in torch_ops.OPS
    assert "cooccur.hip" in open(os.path.join(ROOT, "elimrec_amd", "csrc", "Makefile")).read()
    assert _lib.load().elimrec_abi_version() == 2
