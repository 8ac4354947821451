"""The host side of the co-interaction neighbours (no GPU): the exact model of tests/cooccur_model.py by hand, every argument error
of ops.CooccurIndex / cooccur_topk, of EliMRec.co_items / co_users and of CoNeighbourReport before the device is needed, the form
rule at its edge, the --co_report switch, and the new entries in the header, the binding and the torch registry."""
import inspect
import os

import numpy as np
import pytest
import torch

import cooccur_cases as cc
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


def test_the_model_keeps_one_workspace_for_the_two_form_calls():
    """EliMRec._kept_workspace, which co_neighbours_device, walk_neighbours_device and knn_recommend_device share (host logic only:
    CPU and meta tensors): the same zeroed buffer while the need fits, a new one when the need grows or the device asked for is
    another one, nothing for a need of 0, and past the budget a ValueError that names the caller before anything is allocated."""
    from elimrec_amd import ops
    model, _ = build_model_from_fixture(load_golden("ml3"), "cpu")
    cpu, meta = torch.device("cpu"), torch.device("meta")
    assert model._kept_workspace("co_neighbours_device", 0, cpu) is None
    a = model._kept_workspace("co_neighbours_device", 4096, cpu)
    assert a.dtype == torch.uint8 and a.numel() >= 4096 and a.device == cpu and not a.any()
    assert model._kept_workspace("walk_neighbours_device", 4096, cpu) is a and model._kept_workspace("knn_recommend_device", 64, cpu) is a
    assert model._kept_workspace("knn_recommend_device", 0, cpu) is None and model._kept_workspace("co_neighbours_device", 16, cpu) is a
    b = model._kept_workspace("walk_neighbours_device", 4097, cpu)              # the need grows
    assert b is not a and b.numel() >= 4097 and not b.any() and model._kept_workspace("co_neighbours_device", 4096, cpu) is b
    c = model._kept_workspace("co_neighbours_device", 64, meta)                 # the model moved: every family asks for the new device
    assert c is not b and c.device == meta and model._kept_workspace("knn_recommend_device", 64, meta) is c
    assert model._kept_workspace("co_neighbours_device", 64, cpu).device == cpu
    kept = model._kept_workspace("co_neighbours_device", 64, cpu)
    for who in ("co_neighbours_device", "walk_neighbours_device", "knn_recommend_device"):
        with pytest.raises(ValueError, match=who):
            model._kept_workspace(who, ops.COOCCUR_WORKSPACE_BUDGET + 1, meta)
    assert model._kept_workspace("co_neighbours_device", 64, cpu) is kept      # the refusal allocated and replaced nothing
    assert model._kept_workspace("walk_neighbours_device", ops.COOCCUR_WORKSPACE_BUDGET, meta).numel() == ops.COOCCUR_WORKSPACE_BUDGET


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


# --------------------------------------------------------------------------- the inputs of tests/test_cooccur_dense_gpu.py
# Conditions on the graphs of tests/cooccur_cases.py, not on the kernel: each case reaches the mechanism it is named for.
def _schedule(name, K, measure):
    case = cc.case(name)
    return cm.dense_schedule(cc.csrs(case), case.rows[0], K, measure, cc.cap(), cc.USERS_PER_PASS, cc.ENTRIES_PER_STEP)


def _n_candidates(case):
    q_ptr, q_nbr, _, _ = cc.csrs(case)
    B = cm.incidence(q_ptr, q_nbr, len(case.users))
    C = (B[case.rows] @ B.T).toarray()
    C[np.arange(len(case.rows)), case.rows] = 0
    return (C > 0).sum(1)


def test_the_schedule_model_on_a_small_list():
    """Item 0 held by three users, walked 2 users at a time and 2 entries a step with a list of 7 (cut once longer than 3), K = 2,
    "count"; c = 2 for items 1, 3, 4 and 1 for items 2, 5, 6. Users 0 and 1: step (1, 2 | 0, 5) appends 1, 2, 5; step (3, 4 | 1)
    appends 3, 4 (1 is claimed): 5 kept, cut to ids 1 and 3, the threshold is (2, id 3); step (0 | -). User 2 alone: step (6, 3)
    drops 6 (c = 1), 3 is claimed; step (0, 4): 4 is claimed."""
    o_ptr, o_nbr = cm.csr_of([[1, 2, 3, 4, 0], [0, 5, 1], [6, 3, 0, 4]])
    graph = cm.transpose_csr(o_ptr, o_nbr, 7) + (o_ptr, o_nbr)
    s = cm.dense_schedule(graph, 0, 2, "count", 7, users=2, entries=2)
    assert (s.cuts, s.appended, s.dropped, s.longest, s.ids) == (1, 5, 1, 5, [1, 3])
    assert cm.topk(graph[0], graph[1], 3, [0], 2, "count")[0].tolist() == [s.ids]


def test_dense_cases_put_several_rows_on_one_workgroup():
    G, H = cc.groups(), cc.cap()
    case = cc.case("many_rows")
    walk = cc.walk_of_rows(case)
    assert len(case.rows) > 2 * G and (walk > H).all() and len(set(case.rows)) == case.n_query < len(case.rows)
    for lds in (True, False):
        served = cm.dense_groups(walk, lds, H, G)
        assert len(served) == G and max(len(s) for s in served) >= 3 and sum(len(s) for s in served) == len(case.rows)
    print("many_rows: Q %d, n %d, edges %d, rows per workgroup %d..%d" % (len(case.rows), case.n_query, sum(map(len, case.users)),
                                                                         min(map(len, served)), max(map(len, served))))
    s = cm.dense_schedule(cc.csrs(case), case.rows[0], 65, "cosine", H, cc.USERS_PER_PASS, cc.ENTRIES_PER_STEP)
    assert s.cuts >= 1 and s.longest <= H                                    # every row leaves a raised threshold behind

    case = cc.case("interleaved")
    walk = cc.walk_of_rows(case)
    assert (walk > H).tolist() == [True, False, False, True, False, False, True, False] and (walk > 1).all()
    served = cm.dense_groups(walk, True, H, G)
    assert [[p for _, p in s] for s in served] == [[0, 3, 6], [], []]
    assert [len(s) for s in cm.dense_groups(walk, False, H, G)] == [1] * 8
    q_ptr, q_nbr, _, _ = cc.csrs(case)
    lists = cm.topk(q_ptr, q_nbr, len(case.users), [0, 1, 2], H + 200, "count")[0]
    shared = [np.intersect1d(lists[a][lists[a] >= 0], lists[b][lists[b] >= 0]).size for a, b in ((0, 1), (1, 2))]
    assert min(shared) > 100                                                 # a counter left dirty by one row is met by the next
    for q in range(3):
        s = cm.dense_schedule(cc.csrs(case), q, 5, "jaccard", H, cc.USERS_PER_PASS, cc.ENTRIES_PER_STEP)
        assert s.cuts >= 1 and s.longest <= H
    print("interleaved: walks %s, shared candidates %s" % (walk.tolist(), shared))

    case = cc.case("second_pass")
    walk = cc.walk_of_rows(case)
    at = np.flatnonzero(walk > H).tolist()
    served = cm.dense_groups(walk, True, H, G)
    assert len(case.rows) > cc.CO_THREADS and len(at) == 1 and at[0] >= cc.CO_THREADS and served == [[(1, at[0])]]
    assert (walk == 0).sum() == 12 and len(cm.dense_groups(walk, False, H, G)) == len(case.rows)
    print("second_pass: Q %d, the dense row at %d, walks up to %d elsewhere" % (len(case.rows), at[0], walk[walk <= H].max()))


@pytest.mark.parametrize("K", [1, 64, 256])
def test_dense_cases_cut_their_list_as_named(K):
    H, per = cc.cap(), cc.USERS_PER_PASS * cc.ENTRIES_PER_STEP
    for name in ("rising", "falling", "flat_desc", "flat_asc"):
        case = cc.case(name)
        assert cc.walk_of_rows(case).tolist() == [5 * cc.USERS_PER_PASS * (cc.ENTRIES_PER_STEP + 1)] and _n_candidates(case).tolist() == [5 * per]
    # scores strictly rising / falling from block to block in arrival order, c = 1 everywhere
    for name, sign in (("rising", 1), ("falling", -1)):
        case = cc.case(name)
        q_ptr = cc.csrs(case)[0]
        where, deg = cc.block_of(case), np.diff(q_ptr)
        for measure in ("cosine", "jaccard"):
            per_block = [np.unique(cm.scores(1, deg[0], deg[where == t], measure)) for t in range(5)]
            assert all(b.size == 1 for b in per_block) and (sign * np.diff(np.concatenate(per_block)) > 0).all()
    for measure in ("cosine", "jaccard"):
        s = _schedule("rising", K, measure)
        print("rising K=%d %s: %s" % (K, measure, s[:4]))
        assert s.cuts >= 3 and s.dropped == 0 and s.appended == 5 * per and s.longest <= H
        s = _schedule("falling", K, measure)
        print("falling K=%d %s: %s" % (K, measure, s[:4]))
        assert s.cuts == 1 and s.appended == 2 * per and s.dropped == 3 * per and s.longest <= H
    s = _schedule("flat_desc", K, "count")
    print("flat_desc K=%d: %s" % (K, s[:4]))
    assert s.cuts >= 3 and s.dropped == 0 and s.longest <= H and s.ids == sorted(s.ids) and s.ids[0] == 1
    s = _schedule("flat_asc", K, "count")
    print("flat_asc K=%d: %s" % (K, s[:4]))
    assert s.cuts == 1 and s.appended == 2 * per and s.dropped == 3 * per and s.longest <= H and s.ids == list(range(1, K + 1))


def test_lds_cases_reach_the_table_and_list_edges():
    S, H = cc.slots(), cc.cap()
    case = cc.case("wrap")
    q_ptr, q_nbr, _, _ = cc.csrs(case)
    idx, _, cnt = cm.topk(q_ptr, q_nbr, 2, case.rows, H, "count")
    keys = idx[0][idx[0] >= 0]
    assert cc.walk_of_rows(case)[0] <= H and keys.size == 48 and set(cnt[0][:48].tolist()) == {1, 2} and case.rows[0] not in keys
    # a host table under the kernel's rule (home slot id mod SLOTS, the next slot mod SLOTS when taken), in three insertion orders
    for order in (keys, keys[::-1], np.sort(keys)):
        table = {}
        for j in order.tolist():
            s = j % S
            while s in table:
                s = (s + 1) % S
            table[s] = j
        wrapped = [j for s, j in table.items() if s < j % S]
        assert len(wrapped) >= 28 and set(table) == set(range(S - 4, S)) | set(range(44))
    for name, n in (("full_list", [H - 1]), ("sort_sizes", [cc.SORT_SIZES[r] for r in cc.case("sort_sizes").rows])):
        case = cc.case(name)
        assert _n_candidates(case).tolist() == n and (cc.walk_of_rows(case) <= H).all()
        print("%s: candidates %s, walks %s" % (name, n, cc.walk_of_rows(case).tolist()))
    assert cc.walk_of_rows(cc.case("full_list")).tolist() == [H] and sorted(cc.SORT_SIZES) == [63, 64, 65, 128, 129, 1024, 1025]
    # the same rows through the dense form (lds=False) stay within the list
    for name in ("full_list", "sort_sizes", "wrap"):
        case = cc.case(name)
        for q in case.rows:
            assert cm.dense_schedule(cc.csrs(case), q, 5, "count", H, cc.USERS_PER_PASS, cc.ENTRIES_PER_STEP).longest <= H
    assert all(sum(map(len, cc.case(name).users)) < 40000 for name in cc.BUILDERS)


def test_cooccur_entries_are_declared_bound_and_registered():
    from elimrec_amd import _lib, torch_ops
    header = open(os.path.join(ROOT, "include", "elimrec_hip.h")).read()
    for name in ("elimrec_cooccur_topk", "elimrec_cooccur_walk", "elimrec_cooccur_workspace", "elimrec_cooccur_slots",
                 "elimrec_cooccur_max_k", "elimrec_cooccur_groups", "elimrec_cooccur_rows_in_lds"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name) and name + "(" in header
    assert hasattr(torch_ops.load(), "cooccur_topk") and "cooccur_topk" in torch_ops.OPS
    assert "cooccur.hip" in open(os.path.join(ROOT, "elimrec_amd", "csrc", "Makefile")).read()
    assert _lib.load().elimrec_abi_version() == 2
