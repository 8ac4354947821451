"""The host side of the neighbour votes (no GPU): the exact model of tests/vote_model.py by hand, every argument error of
ops.NeighbourLists / neighbour_vote_topk, of EliMRec.recommend_knn / neighbour_lists and of BaselineReport before the device is
needed, the overflow bound and the form rule at their edges, the --baseline_* switches, the new entries in the header, the binding
and the torch registry, and the conditions on the inputs of tests/test_vote_gpu.py."""
import inspect
import os

import numpy as np
import pytest
import torch

import vote_cases as vc
import vote_model as vm
from helpers import build_model_from_fixture, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = -np.inf
# 6 items, Kn = 2: item -> (neighbour, value)
HAND_IDX = np.asarray([[1, 2], [0, 2], [0, 1], [4, -1], [3, 9], [0, 0]], dtype=np.int32)
HAND_VAL = np.asarray([[0.5, 0.25], [0.5, 0.75], [0.25, 0.75], [1.0, NINF], [1.0, 2.0], [-0.5, 0.125]], dtype=np.float32)


def test_the_model_by_hand():
    """History {0, 1}: votes 0 -> (1: 0.5, 2: 0.25), 1 -> (0: 0.5, 2: 0.75). S(2) = 1.0 with c = 2; items 0 and 1 are the history's own
    and left out: the list is (2). Without exclude_history: (2: 1.0, c 2), then 0 and 1 at 0.5 by id. History {5}: 0 gets -0.5 + 0.125
    with c = 2. History {3, 4}: 3 -> 4 (1.0; the -1 / -inf slot is skipped), 4 -> 3 (1.0; id 9 is outside the table): both are the
    history's own: fillers. History {5, 5}: a repeated id votes again: c = 4, S = -0.75. History {7, -1}: outside the table."""
    hist = [[0, 1], [5], [3, 4], [5, 5], [7, -1], []]
    idx, val, cnt = vm.topk(HAND_IDX, HAND_VAL, hist, range(6), 3)
    assert idx.tolist() == [[2, -1, -1], [0, -1, -1], [-1] * 3, [0, -1, -1], [-1] * 3, [-1] * 3]
    assert val[:, 0].tolist() == [1.0, -0.375, NINF, -0.75, NINF, NINF] and cnt[:, 0].tolist() == [2, 2, 0, 4, 0, 0]
    idx, val, cnt = vm.topk(HAND_IDX, HAND_VAL, hist, [0, 2], 3, exclude_history=False)
    assert idx.tolist() == [[2, 0, 1], [3, 4, -1]] and val.tolist() == [[1.0, 0.5, 0.5], [1.0, 1.0, NINF]] and cnt.tolist() == [[2, 1, 1], [1, 1, 0]]
    idx, _, _ = vm.topk(HAND_IDX, HAND_VAL, hist, [0, 1], 3, excl=[[2], [9, -3], [], [], [], []])
    assert idx.tolist() == [[-1] * 3, [0, -1, -1]]                          # the second CSR: item 2 left out; ids outside the table
    # fixed point: round half even, the sum of the rounded votes, rounded once to fp32
    assert vm.fixed(np.float32([2.0 ** -25, 3 * 2.0 ** -25, -2.0 ** -25, -3 * 2.0 ** -25, 1.0])).tolist() == [0, 2, 0, -2, 2 ** 24]
    assert vm.score_of([2 ** 34 + 1, 2 ** 34 + 2, -3]).tolist() == [1024.0, 1024.0, -3 * 2.0 ** -24]
    assert vm.votes(2, hist).tolist() == [6, 3, 6, 6, 6, 0] and vm.votes(2, hist, [[1]] * 6, False).tolist() == [5, 3, 5, 5, 5, 1]
    # the report's columns
    rows = vm.metric_rows(np.asarray([[3, -1, 1], [-1, -1, -1]]), [[1, 3], [0]], [1, 2, 4]).reshape(2, 3, 3)
    f32 = lambda xs: np.asarray(xs, dtype=np.float32).tolist()
    assert rows[0, 0].tolist() == f32([1, 0.5, 2 / 3.0]) and rows[0, 1].tolist() == f32([0.5, 0.5, 1.0]) and not rows[1].any()
    assert rows[0, 2, 0] == 1.0 and rows[0, 2, 2] == np.float32(1.5) / np.float32(np.float64(np.float32(1.0)) + 1 / np.log2(3.0))
    assert vm.list_columns(np.asarray([[3, -1], [-1, -1]]), np.asarray([[3, 1], [2, 0]]), [1, 2, 3, 4]).tolist() == [[0.5, 4.0, 0.5], [0, 0, 0]]


def test_lists_checks_and_host_arithmetic():
    from elimrec_amd import ops
    lists = ops.NeighbourLists(HAND_IDX, HAND_VAL, "cpu")
    assert (lists.n, lists.Kn, lists.max_abs) == (6, 2, 2.0) and lists.idx.dtype == torch.int32
    assert ops.NeighbourLists(torch.from_numpy(HAND_IDX), torch.from_numpy(HAND_VAL), "cpu").max_abs == 2.0
    assert ops.NeighbourLists(HAND_IDX[:1], np.float32([[NINF, np.nan]]), "cpu").max_abs == 0.0      # no finite value
    for bad in ((HAND_IDX, HAND_VAL[:5]), (HAND_IDX.reshape(-1), HAND_VAL.reshape(-1)), (HAND_IDX[:, :0], HAND_VAL[:, :0]),
                (HAND_IDX[:, ::2], HAND_VAL[:, ::2]), (HAND_IDX.T, HAND_VAL.T)):
        with pytest.raises(ValueError):
            ops.NeighbourLists(*bad, "cpu")
    for bad in ((HAND_IDX.astype(np.int64), HAND_VAL), (HAND_IDX, HAND_VAL.astype(np.float64))):
        with pytest.raises(TypeError):
            ops.NeighbourLists(*bad, "cpu")
    hist = ops.HistoryIndex([0, 2, 3, 3], [0, 1, 5], "cpu")
    excl = ops.HistoryIndex([0, 0, 2, 3], [9, -3, 2], "cpu")
    assert ops.vote_votes(lists, hist).tolist() == [6, 3, 0] and ops.vote_votes(lists, hist, excl).tolist() == [6, 5, 1]
    assert ops.vote_votes(lists, hist, excl, exclude_history=False).tolist() == [4, 4, 1]
    with pytest.raises(ValueError, match="same users"):
        ops.vote_votes(lists, hist, ops.HistoryIndex([0, 1], [0], "cpu"))
    with pytest.raises(TypeError):
        ops.vote_votes((HAND_IDX, HAND_VAL), hist)


def test_op_argument_errors_fire_without_a_gpu():
    from elimrec_amd import ops
    lists = ops.NeighbourLists(HAND_IDX, HAND_VAL, "cpu")
    hist = ops.HistoryIndex([0, 2, 3, 3], [0, 1, 5], "cpu")
    out = torch.zeros(2, 3, dtype=torch.int32)
    for bad in (0, 257, -1, 2.0, True, "3"):
        with pytest.raises(ValueError, match="1 <= K <= 256"):
            ops.neighbour_vote_topk(lists, hist, [0, 1], bad, out)
    for bad in ([3], [-1], [0, 7]):
        with pytest.raises(IndexError):
            ops.neighbour_vote_topk(lists, hist, bad, 3, out)
    with pytest.raises(TypeError):
        ops.neighbour_vote_topk(lists, hist, [0.5], 3, out)
    with pytest.raises(TypeError):
        ops.neighbour_vote_topk(lists, (1, 2), [0], 3, out)
    with pytest.raises(TypeError):
        ops.neighbour_vote_topk(lists, hist, [0], 3, out, excl=[[1]])
    with pytest.raises(ValueError, match="same users"):
        ops.neighbour_vote_topk(lists, hist, [0], 3, out, excl=ops.HistoryIndex([0, 1], [0], "cpu"))
    with pytest.raises(RuntimeError, match="HIP device tensor"):             # no CPU path
        ops.neighbour_vote_topk(lists, hist, [0, 1], 3, out)
    assert ops.VOTE_MAX_K == 256 and ops.VOTE_FRAC_BITS == vm.FRAC_BITS == 24


def test_the_overflow_bound_at_its_edge():
    """ceil(max|val| * 2^24) x (longest history) x Kn >= 2^62 is refused before any launch: with max|val| = 2^14 and Kn = 256 a
    history of 2^16 entries is exactly at the bound, one of 2^16 - 1 just below it (that call goes on to the device check)."""
    from elimrec_amd import ops
    idx = np.zeros((3, 256), dtype=np.int32)
    val = np.full((3, 256), 1.0, dtype=np.float32)
    val[1, 7] = -2.0 ** 14
    val[2, 0] = np.inf                                                       # not finite: not part of max_abs
    lists = ops.NeighbourLists(idx, val, "cpu")
    assert lists.max_abs == 2.0 ** 14
    out = torch.zeros(1, 3, dtype=torch.int32)
    at = ops.HistoryIndex([0, 1, 1 + 2 ** 16], np.zeros(1 + 2 ** 16, dtype=np.int32), "cpu")
    with pytest.raises(ValueError, match="could overflow"):
        ops.neighbour_vote_topk(lists, at, [0], 3, out)                      # the longest segment counts, not the called user's
    below = ops.HistoryIndex([0, 1, 2 ** 16], np.zeros(2 ** 16, dtype=np.int32), "cpu")
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        ops.neighbour_vote_topk(lists, below, [0], 3, out)
    val[1, 7] = 2.0 ** 14 + 0.5                                              # (2^38 + 2^23) x (2^16 - 1) x 2^8 > 2^62
    with pytest.raises(ValueError, match="could overflow"):
        ops.neighbour_vote_topk(ops.NeighbourLists(idx, val, "cpu"), below, [0], 3, out)
    with pytest.raises(ValueError, match="fewer than 2\\^30"):               # the count's mark bit
        ops.neighbour_vote_topk(ops.NeighbourLists(idx, np.zeros_like(val), "cpu"),
                                ops.HistoryIndex([0, 2 ** 22], np.zeros(2 ** 22, dtype=np.int32), "cpu"), [0], 3, out)


def test_the_form_rule_at_its_edge():
    from elimrec_amd import _lib, ops
    S = ops.VOTE_SLOTS
    assert S == vc.SLOTS == 2048 and S & (S - 1) == 0 and vc.CAP == S // 2 and ops.VOTE_GROUPS == vc.GROUPS
    assert ops.vote_rows_in_lds(0) and ops.vote_rows_in_lds(S // 2) and not ops.vote_rows_in_lds(S // 2 + 1) and not ops.vote_rows_in_lds(2 ** 40)
    with pytest.raises(ValueError):
        ops.vote_rows_in_lds(-1)
    lib = _lib.load()
    assert lib.elimrec_vote_rows_in_lds(-1) == -1 and lib.elimrec_vote_max_k() == ops.VOTE_MAX_K and lib.elimrec_vote_frac_bits() == 24
    assert S * 16 + (S // 2) * 12 <= 64 * 1024                                # the table and the list within 64 KiB of LDS
    # the workspace: n int64 sums and n int32 counts per dense-form workgroup, VOTE_GROUPS of them at most (host arithmetic)
    G = ops.VOTE_GROUPS
    assert ops.vote_workspace(0, 1000) == 0 and ops.vote_workspace(3, 1000) == 36000 and ops.vote_workspace(1, 3) == 48
    assert ops.vote_workspace(G, 1000) == ops.vote_workspace(10 * G, 1000) == G * 12000
    with pytest.raises(ValueError):
        ops.vote_workspace(-1, 10)
    with pytest.raises(ValueError):
        ops.vote_workspace(1, 2 ** 31)
    assert ops.vote_workspace(G, 2 ** 24) > ops.COOCCUR_WORKSPACE_BUDGET
    # the case at the cap
    case = vc.case("at_the_cap")
    assert vm.votes(3, case.hist, case.excl).tolist() == [S // 2, 8, S // 2 + 1, S // 2 + 1]


def test_model_argument_errors_fire_without_a_gpu():
    g = load_golden("ml3")
    model, _ = build_model_from_fixture(g, "cpu")
    for bad in (0, 257, 1.5, True):
        with pytest.raises(ValueError, match="1 <= K <= 256"):
            model.recommend_knn([0], bad)
        with pytest.raises(ValueError, match="neighbours must be"):
            model.recommend_knn([0], 3, neighbours=bad)
        with pytest.raises(ValueError, match="neighbours must be"):
            model.neighbour_lists("co", bad)
    with pytest.raises(ValueError, match="measure is one of"):
        model.recommend_knn([0], 3, measure="dice")
    for bad in ("x", "items", None, 3):
        with pytest.raises(ValueError, match="source must be"):
            model.recommend_knn([0], 3, source=bad)
        with pytest.raises(ValueError, match="source must be"):
            model.neighbour_lists(bad)
    for bad in ([model.num_users], [-1]):
        with pytest.raises(IndexError):
            model.recommend_knn(bad, 3)
    with pytest.raises(IndexError):
        model.recommend_knn([0], 3, history={0: [model.num_items]})
    with pytest.raises(IndexError):
        model.recommend_knn([0], 3, exclude={0: [-1]})
    with pytest.raises(TypeError):
        model.recommend_knn([0], 3, history=[[1]])
    empty = model.recommend_knn([], 5)                                       # no launch: a CPU model answers
    assert [tuple(t.shape) for t in empty] == [(0, 5)] * 3 and [t.dtype for t in empty] == [torch.int32, torch.float32, torch.int32]
    for source in ("co", "v", "fused"):
        with pytest.raises(RuntimeError):                                    # a CPU model
            model.recommend_knn([0], 3, source=source)
        with pytest.raises(RuntimeError):
            model.neighbour_lists(source)
    assert "untrained" in model.neighbour_lists.__doc__


def test_report_arguments_and_the_switches():
    from elimrec_amd.basic_model import baseline_sources
    from elimrec_amd.evaluator import BASELINE_LIST_COLUMNS, BaselineReport
    assert BASELINE_LIST_COLUMNS == ("filled", "pop", "overlap", "coverage", "gini", "entropy")
    assert baseline_sources("[co,fused,v]") == ("co", "fused", "v") and baseline_sources(["co"]) == ("co",) and baseline_sources("[ 'v' ]") == ("v",)
    for bad in ("co", "[]", "[co,co]", [], [1], 3):
        with pytest.raises(ValueError):
            baseline_sources(bad)
    g = load_golden("ml3")
    model, _ = build_model_from_fixture(g, "cpu")
    assert model.baseline_reporter is None
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--baseline_report=0", "--baseline_sources=[co,v]", "--baseline_measure=jaccard"])
    assert model.baseline_reporter is None                                    # 0 means off
    train, test = model.dataset.get_user_train_dict(), model.dataset.get_user_test_dict()
    with pytest.raises(TypeError):
        BaselineReport(model.dataset, [], test, [10])
    for bad in dict(sources=(), neighbours=0, measure="dice", list_k=9, sources_=("co", "co"), neighbours_=257, list_k_=257, sources__="co").items():
        with pytest.raises(ValueError):
            BaselineReport(model.dataset, train, test, [10], **{bad[0].rstrip("_"): bad[1]})
    for bad in (["--baseline_report=-1"], ["--baseline_report=300"], ["--baseline_report=5"], ["--baseline_report=10", "--baseline_measure=dice"],
                ["--baseline_measure=dice"], ["--baseline_neighbours=0"], ["--baseline_report=10", "--baseline_sources=[co,x]"],
                ["--baseline_sources=co"], ["--baseline_report=2.5"]):
        with pytest.raises(ValueError):
            build_model_from_fixture(g, "cpu", extra_argv=bad)
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--baseline_report=20", "--baseline_sources=[co,v]", "--baseline_neighbours=7",
                                                              "--baseline_measure=count", "--group_view=[2,4]"])
    rep = model.baseline_reporter
    assert isinstance(rep, BaselineReport) and (rep.k, rep.sources, rep.neighbours, rep.measure) == (20, ("co", "v"), 7, "count")
    assert rep.columns[-6:] == BASELINE_LIST_COLUMNS and rep.columns[:-6] == rep.metric_columns and rep.users == list(test.keys())
    assert len(rep.labels) == 2 * len(rep.group_labels) and rep.labels[0].startswith("co all:") and len(rep.group_labels) > 1
    assert build_model_from_fixture(g, "cpu", extra_argv=["--baseline_report=10"])[0].baseline_reporter.sources == ("co",)
    with pytest.raises(RuntimeError):                                        # a CPU model
        rep.evaluate(model)
    with pytest.raises(ValueError, match="source is one of"):
        rep.knn_lists(model, "a")
    import main
    assert "--baseline_report needs the whole cached item table on one rank: it is single-GPU" in inspect.getsource(main.Net.__init__)
    src = inspect.getsource(main.Net)
    assert "[baselines]" in src and "[{} - {}] metric difference, paired bootstrap:" in src


# --------------------------------------------------------------------------- the inputs of tests/test_vote_gpu.py
# Conditions on the cases of tests/vote_cases.py, not on the kernel: each case reaches the mechanism it is named for.
def test_dense_cases_put_several_rows_on_one_workgroup():
    case = vc.case("dense_rows")
    V = vm.votes(case.idx.shape[1], case.hist, case.excl)
    served = vm.dense_groups(V, False, vc.CAP, 2)
    assert [[p for _, p in s] for s in served] == [[0, 2, 4, 6], [1, 3, 5]] and (V <= vc.CAP).all()
    lists = vm.topk(case.idx, case.val, case.hist, case.users, 256, case.excl)[0]
    for a, b in ((0, 2), (2, 6), (1, 3), (3, 5)):                            # an entry left dirty by one row is met by the next
        assert np.intersect1d(case.idx[case.hist[a]].reshape(-1), case.idx[case.hist[b]].reshape(-1)).size >= 1
    assert (lists[[1, 2, 5]] == 50).any(1).all() and not (lists[[0, 3, 6]] == 50).any()
    case = vc.case("at_the_cap")
    V = vm.votes(3, case.hist, case.excl)
    assert [[p for _, p in s] for s in vm.dense_groups(V, True, vc.CAP, vc.GROUPS)] == [[2], [3]]
    assert len(vm.dense_groups(V, False, vc.CAP, vc.GROUPS)) == 4


@pytest.mark.parametrize("K", vc.KS)
def test_cut_cases_overflow_the_list_as_named(K):
    touched = vc.CUT_H * vc.CUT_KN
    assert touched > vc.CAP and 64 + touched <= vc.CUT_N
    per_step = vc.CUT_H * vc.SLOTS_PER_STEP
    for name in ("cut_rising", "cut_falling", "cut_flat"):
        case = vc.case(name)
        assert vm.votes(vc.CUT_KN, case.hist).tolist() == [touched + vc.CUT_H, 2 * vc.CUT_KN + 2]
        assert (vm.topk(case.idx, case.val, case.hist, [0], 256)[0] >= 0).all()
        s = vm.dense_schedule(case.idx, case.val, case.hist[0], [], K, vc.CAP, vc.POSITIONS, vc.SLOTS_PER_STEP)
        print("%s K=%d: %s" % (name, K, s[:4]))
        assert s.cuts >= 1 and s.longest <= vc.CAP and s.appended + s.dropped == touched
        assert s.ids == vm.topk(case.idx, case.val, case.hist, [0], K)[0][0].tolist()
        if name == "cut_rising":                                             # every cut raises the threshold, (almost) nothing is dropped
            assert s.cuts >= 2 and s.dropped <= 1
        else:                                                                # one cut; the threshold then drops what arrives later
            assert s.cuts == 1 and s.appended >= 2 * per_step and s.dropped >= touched - vc.CAP + 64


def test_lds_cases_reach_the_probe_chain():
    S = vc.SLOTS
    case = vc.case("hash_chain")
    assert case.idx.shape[0] > 2 * S and (vm.votes(3, case.hist, case.excl) <= vc.CAP).all()
    # a host table under the kernel's rule (home slot id mod SLOTS, the next slot mod SLOTS when taken), left-out ids first
    for u in case.users:
        table = {}
        voted = [int(i) for j in case.hist[u] for i in case.idx[j]]
        for j in [x for x in case.hist[u] + case.excl[u] if 0 <= x < case.idx.shape[0]] + voted:
            s = j % S
            while s in table and table[s] != j:
                s = (s + 1) % S
            table[s] = j
        moved = [j for s, j in table.items() if s != j % S]
        assert len(moved) >= 2, (u, table)
    assert any(s < j % S for s, j in table.items())                          # user 2's chain wraps around the table's end
    want = vm.topk(case.idx, case.val, case.hist, case.users, 8, case.excl)[0]
    assert 5 in want[0] and 5 + 2 * S in want[0] and 6 not in want[0] and 5 + S not in want[0] and 6 + S in want[0]


def test_vote_entries_are_declared_bound_and_registered():
    from elimrec_amd import _lib, torch_ops
    header = open(os.path.join(ROOT, "include", "elimrec_hip.h")).read()
    for name in ("elimrec_neighbour_vote_topk", "elimrec_vote_workspace", "elimrec_vote_slots", "elimrec_vote_groups", "elimrec_vote_max_k",
                 "elimrec_vote_frac_bits", "elimrec_vote_rows_in_lds"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name) and name + "(" in header
    assert hasattr(torch_ops.load(), "neighbour_vote_topk") and "neighbour_vote_topk" in torch_ops.OPS
    makefile = open(os.path.join(ROOT, "elimrec_amd", "csrc", "Makefile")).read()
    assert "vote.hip" in makefile and "co_select.h" in makefile
    for name in ("cooccur.hip", "vote.hip"):                                 # the selection is shared, not copied
        src = open(os.path.join(ROOT, "elimrec_amd", "csrc", name)).read()
        assert '#include "co_select.h"' in src and "void co_sort(" not in src and "uint64_t co_key(" not in src
    assert _lib.load().elimrec_abi_version() == 2
