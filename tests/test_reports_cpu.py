"""The pieces the reports and table readers share, host side (no GPU): the ragged-list builder, the one checked CSR behind
GroupIndex / TargetIndex / NeighbourQuery (every failure keeps its exception type and its words), the table formatter, the group
index and the item counts."""
import numpy as np
import pytest
import torch

from elimrec_amd import ops

CPU = torch.device("cpu")


def test_ragged_builder():
    ptr, flat, lens = ops.ragged([])
    assert ptr.tolist() == [0] and ptr.dtype == np.int64 and flat.size == 0 and flat.dtype == np.int64 and lens.size == 0
    assert ops.ragged_padded(flat, lens).shape == (0, 0)
    ptr, flat, lens = ops.ragged([[], [], []], dtype=np.int32)
    assert ptr.tolist() == [0, 0, 0, 0] and flat.size == 0 and flat.dtype == np.int32 and lens.tolist() == [0, 0, 0]
    assert ops.ragged_padded(flat, lens).shape == (3, 0) and ops.ragged_padded(flat, lens, 2).tolist() == [[-1, -1]] * 3
    lists = [[4, 1], [], (7,), np.asarray([2, 2, 9])]
    ptr, flat, lens = ops.ragged(lists, check=(10, "ids must lie in [0, 10)"), cast=int)
    assert ptr.tolist() == [0, 2, 2, 3, 6] and flat.tolist() == [4, 1, 7, 2, 2, 9] and lens.tolist() == [2, 0, 1, 3]
    assert ptr.dtype == lens.dtype == flat.dtype == np.int64
    padded = ops.ragged_padded(flat, lens)
    assert padded.dtype == np.int32 and padded.tolist() == [[4, 1, -1], [-1, -1, -1], [7, -1, -1], [2, 2, 9]]
    assert ops.ragged_padded(flat, lens, 4)[:, 3].tolist() == [-1] * 4
    for bad in ([[0, 10]], [[3], [-1]]):                                   # an id equal to the bound, a negative id
        with pytest.raises(IndexError, match=r"^ids must lie in \[0, 10\)$"):
            ops.ragged(bad, check=(10, "ids must lie in [0, 10)"))
    assert ops.ragged([[0, 10], [-5]])[1].tolist() == [0, 10, -5]          # no bound: nothing is checked
    # arrays go in whole; a Python integer beyond the dtype is an error under cast=int, not a wrapped id
    assert ops.ragged([np.arange(3), np.arange(2)], dtype=np.int32)[1].tolist() == [0, 1, 2, 0, 1]
    with pytest.raises(OverflowError):
        ops.ragged([[1 << 40]], dtype=np.int32, cast=int)


def _raises(exc, prefix, fn):
    with pytest.raises(exc) as e:
        fn()
    assert type(e.value) is exc and str(e.value).startswith(prefix), (str(e.value), prefix)


def test_group_index_failures_keep_their_words():
    who = "elimrec_amd.ops.GroupIndex: "
    _raises(ValueError, who + "group_ptr needs G + 1 >= 2 entries", lambda: ops.GroupIndex([0], [], 3, CPU))
    _raises(TypeError, who + "group_rows must hold integers, got float64", lambda: ops.GroupIndex([0, 1], [0.5], 3, CPU))
    _raises(ValueError, who + "group_ptr must ascend from 0 to len(group_rows) = 2", lambda: ops.GroupIndex([0, 2, 1], [0, 1], 3, CPU))
    _raises(ValueError, who + "group_ptr must ascend from 0 to len(group_rows) = 2", lambda: ops.GroupIndex([0, 3], [0, 1], 3, CPU))
    _raises(IndexError, who + "row indices span [0, 3], the block has 3 rows", lambda: ops.GroupIndex([0, 2], [0, 3], 3, CPU))
    _raises(IndexError, who + "row indices span [-1, 2], the block has 3 rows", lambda: ops.GroupIndex([0, 2], [-1, 2], 3, CPU))
    idx = ops.GroupIndex([0, 2, 2, 3], [2, 0, 2], 3, CPU)
    assert (idx.n_rows, idx.n_groups, idx.n_listed) == (3, 3, 3) and idx.sizes.tolist() == [2, 0, 1]
    assert idx.ptr.dtype == torch.int64 and idx.rows.dtype == torch.int32 and idx.rows.tolist() == [2, 0, 2]
    assert ops.GroupIndex([0, 0], [], 3, CPU).rows.numel() == 1               # never an empty tensor


def test_target_index_failures_keep_their_words():
    who = "elimrec_amd.ops.TargetIndex: "
    _raises(ValueError, who + "ptr needs B + 1 = 3 entries, got 2", lambda: ops.TargetIndex([0, 1], [0], 2, 5, CPU))
    _raises(TypeError, who + "items must hold integers, got float64", lambda: ops.TargetIndex([0, 1, 1], [0.5], 2, 5, CPU))
    _raises(ValueError, who + "ptr must ascend from 0 to len(items) = 2", lambda: ops.TargetIndex([0, 2, 1], [0, 1], 2, 5, CPU))
    _raises(ValueError, who + "ptr must ascend from 0 to len(items) = 2", lambda: ops.TargetIndex([1, 1, 2], [0, 1], 2, 5, CPU))
    _raises(IndexError, who + "item ids span [0, 5], the catalogue has 5 items", lambda: ops.TargetIndex([0, 1, 2], [0, 5], 2, 5, CPU))
    idx = ops.TargetIndex([0, 1, 3], [4, 0, 0], 2, 5, CPU)
    assert (idx.n_rows, idx.n_items, idx.n_targets) == (2, 5, 3) and idx.sizes.tolist() == [1, 2] and idx.items.tolist() == [4, 0, 0]
    assert ops.TargetIndex([0, 0], [], 1, 5, CPU).items.numel() == 1


def test_neighbour_query_failures_keep_their_words():
    who = "elimrec_amd.ops.NeighbourQuery: "
    _raises(TypeError, who + "rows must hold integers, got float64", lambda: ops.NeighbourQuery([0.5], 5, CPU))
    _raises(IndexError, who + "query rows span [0, 5], the table has 5 rows", lambda: ops.NeighbourQuery([0, 5], 5, CPU))
    _raises(ValueError, who + "the exclusion CSR needs excl_ptr and excl_rows, or neither", lambda: ops.NeighbourQuery([0, 1], 5, CPU, [0, 0, 0], None))
    _raises(ValueError, who + "excl_ptr needs Q + 1 = 3 entries, got 2", lambda: ops.NeighbourQuery([0, 1], 5, CPU, [0, 1], [0]))
    _raises(TypeError, who + "excl_rows must hold integers, got float64", lambda: ops.NeighbourQuery([0, 1], 5, CPU, [0, 1, 1], [0.5]))
    _raises(ValueError, who + "excl_ptr must ascend from 0 to len(excl_rows) = 1", lambda: ops.NeighbourQuery([0, 1], 5, CPU, [0, 2, 1], [0]))
    _raises(IndexError, who + "excluded rows span [0, 5], the table has 5 rows", lambda: ops.NeighbourQuery([0, 1], 5, CPU, [0, 1, 2], [0, 5]))
    q = ops.NeighbourQuery([3, 0], 5, CPU, [0, 0, 2], [4, 4])
    assert (q.n_rows, q.n_queries) == (5, 2) and q.rows.tolist() == [3, 0] and q.excl_ptr.tolist() == [0, 0, 2] and q.excl_rows.tolist() == [4, 4]
    q = ops.NeighbourQuery([], 5, CPU)
    assert q.n_queries == 0 and q.rows.numel() == 1 and q.excl_ptr is None and q.excl_rows is None


def test_format_table_is_the_one_formatter():
    from elimrec_amd import reports
    from elimrec_amd.evaluator import GroupedEvaluator, ListReport, RankReport
    labels = ["all:".ljust(12), "(0,2]:".ljust(12)]
    table = np.asarray([[float("nan"), 1.5], [0.25, -2.0]], dtype=np.float32)
    want = ("columns:\ta           \tb           "
            "\nall:        \tnan         \t1.50000000  "
            "\n(0,2]:      \t0.25000000  \t-2.00000000 ")
    assert reports.format_table(("a", "b"), labels, table) == want
    assert reports.format_table(("rank",), labels[:1], table[:1, 1:]) == "columns:\trank        \nall:        \t1.50000000  "   # one row
    assert reports.format_rows(labels, table) == want[want.index("\n"):]
    assert RankReport._format is reports.format_table and ListReport._format is reports.format_table
    ge = GroupedEvaluator.__new__(GroupedEvaluator)
    ge.group_labels = labels
    assert ge.format_groups(table) == want[want.index("\n"):]                  # the header-less form


def test_group_index_and_item_counts():
    from elimrec_amd import reports
    positions = [np.arange(4, dtype=np.int64), np.asarray([3, 1], dtype=np.int64), np.asarray([2], dtype=np.int64)]
    idx = reports.group_index(positions, 4, CPU)
    assert isinstance(idx, ops.GroupIndex) and (idx.n_rows, idx.n_groups, idx.n_listed) == (4, 3, 7)
    assert idx.ptr.tolist() == [0, 4, 6, 7] and idx.rows.tolist() == [0, 1, 2, 3, 3, 1, 2] and idx.rows.dtype == torch.int32
    with pytest.raises(IndexError):
        reports.group_index(positions, 3, CPU)
    train = {0: [1, 3, 3], 5: [], 2: (3, 0), 9: np.asarray([4])}           # a repeated item, a user without items
    want = np.zeros(6, dtype=np.int64)
    for items in train.values():
        for i in items:
            want[int(i)] += 1
    got = reports.item_train_counts(train, 6)
    assert got.dtype == np.int64 and got.tolist() == want.tolist() == [1, 1, 0, 3, 1, 0]
    ptr, items = reports.lists_csr([0, 7, 2], train, CPU)
    assert ptr.tolist() == [0, 3, 3, 5] and items.tolist() == [1, 3, 3, 3, 0] and items.dtype == torch.int32
    assert reports.lists_csr([0, 2], train, CPU, unique=True)[1].tolist() == [1, 3, 0, 3]


def test_moved_names_stay_importable_from_the_evaluator():
    from elimrec_amd import evaluator, reports
    for name in ("EffectReport", "RankReport", "NeighbourReport", "ListReport", "assign_user_groups", "assign_item_groups",
                 "exposure_summary", "EXPOSURE_COLUMNS", "RankTables", "ListTables", "CandidateScoringError"):
        assert getattr(evaluator, name) is getattr(reports, name), name
