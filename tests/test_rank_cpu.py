"""Exact catalogue ranks, host side (no GPU): the item groups, the report's pairs / blocks / format, TargetIndex's checks -- all of
which run before anything touches the device -- and the numpy model of the kernels (rank_model) on cases worked by hand."""
import types

import numpy as np
import pytest

import rank_model as rm
from helpers import build_model_from_fixture, load_golden


def _labels(names):
    return [n.ljust(12) for n in names]


def test_assign_item_groups_boundaries():
    from elimrec_amd.evaluator import assign_item_groups
    counts = np.asarray([0, 1, 2, 4, 5, 100, 0, 3])
    ids = [0, 1, 2, 3, 4, 5, 6, 7, 3]
    labels, pos = assign_item_groups(ids, counts, [1, 4])
    assert labels == _labels(["cold:", "(0,1]:", "(1,4]:", "(4,inf):"])
    assert [p.tolist() for p in pos] == [[0, 6], [1], [2, 3, 7, 8], [4, 5]]              # 4 is in (1,4], 5 opens the last bucket
    assert all(p.dtype == np.int64 for p in pos)
    # empty groups are omitted, the order of the rest is kept
    labels, pos = assign_item_groups([5, 0, 5], counts, [1, 4])
    assert labels == _labels(["cold:", "(4,inf):"]) and [p.tolist() for p in pos] == [[1], [0, 2]]
    labels, pos = assign_item_groups([1, 2], counts, [2])
    assert labels == _labels(["(0,2]:"]) and pos[0].tolist() == [0, 1]
    for bad in ([], [0, 3], [3, 3], [4, 2], [1.5], [True]):
        with pytest.raises((TypeError, ValueError)):
            assign_item_groups(ids, counts, bad)
    with pytest.raises(TypeError):
        assign_item_groups(ids, counts, (1, 4))
    with pytest.raises(IndexError):
        assign_item_groups([8], counts, [1])


def _report(**kw):
    from elimrec_amd.evaluator import RankReport
    train = {0: [1, 2], 1: [2, 3, 4], 2: [], 3: [0, 1, 2, 3, 4, 5, 6, 7], 4: [9]}
    test = {1: [5, 3, 0], 0: [3], 3: [2], 2: [9, 8], 4: [0, 1, 2, 3, 4, 5, 6, 7, 8]}
    return RankReport(types.SimpleNamespace(num_items=10), train, test, kw.pop("top_k", [1, 5]), **kw), train, test


def test_pairs_follow_the_test_dict_and_drop_train_overlaps():
    rep, train, test = _report()
    # user 1 loses item 3 (in its train list); user 3's only test item is a train item; user 4's test items are every candidate
    assert rep.users == [1, 0, 2] and rep.num_dropped == 2 and rep.num_skipped_users == 2
    assert rep.pair_ptr.tolist() == [0, 2, 3, 5] and rep.pair_items.tolist() == [5, 0, 3, 9, 8] and rep.pair_items.dtype == np.int32
    assert rep.pair_user.tolist() == [0, 0, 1, 2, 2] and rep.num_pairs == 5
    assert rep.user_n_cand.tolist() == [7, 8, 10] and rep.pair_n_cand.tolist() == [7, 7, 8, 10, 10]
    assert rep.ks == [1, 5] and rep.pair_labels == _labels(["all:"]) and rep.user_labels == _labels(["all:"])
    from elimrec_amd.evaluator import RankReport
    with pytest.raises(ValueError):
        RankReport(types.SimpleNamespace(num_items=10), train, test, 0)
    with pytest.raises(ValueError):
        RankReport(types.SimpleNamespace(num_items=10), train, {3: [2]}, 5)            # nothing left to rank
    with pytest.raises(IndexError):
        RankReport(types.SimpleNamespace(num_items=10), train, {0: [10]}, 5)


def test_report_groups():
    rep, train, _ = _report(group_view=[2, 3], item_group_view=[1])
    # users 1 (3 train items), 0 (2), 2 (0 -> the first group, as the evaluator's groups have it)
    assert rep.user_labels == _labels(["all:", "(0,2]:", "(2,3]:"])
    assert [p.tolist() for p in rep._user_pos] == [[0, 1, 2], [1, 2], [0]]
    # item training counts: 0:1 1:2 2:3 3:2 4:2 5:1 6:1 7:1 8:0 9:1 -> pairs (5, 0, 3, 9, 8)
    assert rep.pair_labels == _labels(["all:", "(0,2]:", "(2,3]:", "item cold:", "item (0,1]:", "item (1,inf):"])
    assert [p.tolist() for p in rep._pair_pos] == [[0, 1, 2, 3, 4], [2, 3, 4], [0, 1], [4], [0, 1, 3], [2]]


def test_block_sizing_from_block_bytes():
    rep, _, _ = _report()
    assert rep.block_bytes == 2 << 30
    assert rep.block_users == (2 << 30) // (12 * 4)                                    # rows of 10 items padded to 12 floats
    rep.block_bytes = 2 * 48
    assert rep.block_users == 2
    rep.block_bytes = 2 * 48 + 47
    assert rep.block_users == 2
    rep.block_bytes = 1
    assert rep.block_users == 1                                                        # never less than one user


def test_buf_format():
    from elimrec_amd.evaluator import RankReport
    table = np.asarray([[1.5, 0.25], [3.0, 1.0 / 3.0]], dtype=np.float32)
    buf = RankReport._format(("rank", "hit@10"), _labels(["all:", "item cold:"]), table)
    assert buf.split("\n") == ["columns:\t" + "rank".ljust(12) + "\t" + "hit@10".ljust(12),
                               "all:".ljust(12) + "\t" + "1.50000000".ljust(12) + "\t" + "0.25000000".ljust(12),
                               "item cold:".ljust(12) + "\t" + "3.00000000".ljust(12) + "\t" + "0.33333334".ljust(12)]


def test_target_index_rejections():
    from elimrec_amd import ops
    ok = ops.TargetIndex([0, 2, 2, 3], np.asarray([4, 0, 4], dtype=np.int32), 3, 5, "cpu")
    assert (ok.n_rows, ok.n_items, ok.n_targets) == (3, 5, 3) and ok.sizes.tolist() == [2, 0, 1]
    assert ok.ptr.dtype.is_floating_point is False and ok.items.tolist() == [4, 0, 4]
    with pytest.raises(ValueError):
        ops.TargetIndex([0, 2, 1, 3], [4, 0, 4], 3, 5, "cpu")                          # not monotone
    with pytest.raises(ValueError):
        ops.TargetIndex([0, 2, 3], [4, 0, 4], 3, 5, "cpu")                             # B entries, not B + 1
    with pytest.raises(ValueError):
        ops.TargetIndex([0, 2, 2, 2], [4, 0, 4], 3, 5, "cpu")                          # does not end at len(items)
    with pytest.raises(ValueError):
        ops.TargetIndex([1, 2, 2, 3], [4, 0, 4], 3, 5, "cpu")                          # does not start at 0
    with pytest.raises(IndexError):
        ops.TargetIndex([0, 2, 2, 3], [4, 5, 4], 3, 5, "cpu")                          # id = I
    with pytest.raises(IndexError):
        ops.TargetIndex([0, 2, 2, 3], [4, -1, 4], 3, 5, "cpu")                         # negative id
    with pytest.raises(TypeError):
        ops.TargetIndex([0, 2, 2, 3], [4.0, 1.0, 4.0], 3, 5, "cpu")
    empty = ops.TargetIndex([0, 0], [], 1, 5, "cpu")
    assert empty.n_targets == 0 and empty.items.numel() == 1


def test_rank_entries_are_declared_bound_and_registered():
    from elimrec_amd import _lib, ops, torch_ops
    for name in ("elimrec_rank_targets", "elimrec_rank_pair_rows", "elimrec_rank_user_rows", "elimrec_rank_segment",
                 "elimrec_rank_targets_per_pass"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    assert hasattr(torch_ops.load(), "rank_targets") and "rank_targets" in torch_ops.OPS
    SEG, P = ops.RANK_SEGMENT, ops.RANK_TARGETS_PER_PASS
    assert SEG >= 1024 and SEG % 4 == 0 and P >= 1
    assert ops.rank_pair_columns([10, 50]) == ("rank", "rr", "pct", "hit@10", "hit@50")
    assert ops.RANK_USER_COLUMNS == ("auc", "mrr_full", "first_rank")


def test_rank_items_argument_errors_fire_without_a_gpu():
    g = load_golden("ml3")
    model, _ = build_model_from_fixture(g, "cpu")
    with pytest.raises(ValueError, match="one item list per user"):
        model.rank_items([0, 1], [[1]])
    with pytest.raises(IndexError):
        model.rank_items([0, 1], [[1], [model.num_items]])
    with pytest.raises(IndexError):
        model.rank_items([0, 1], [[1], [-1]])
    with pytest.raises(IndexError):
        model.rank_items([0, 1], [[1], [2]], exclude={0: [model.num_items]})
    assert model.rank_reporter is None
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--rank_report=1", "--group_view=[1,3,5]", "--item_group_view=[1,4]"])
    rep = model.rank_reporter
    assert rep is not None and rep.num_items == model.num_items and rep.pair_labels[0] == "all:".ljust(12)
    assert any(x.startswith("item ") for x in rep.pair_labels)


# --------------------------------------------------------------------------- the numpy model, by hand
def test_model_ranks_by_hand():
    ninf = -np.inf
    block = np.asarray([[0.5, 0.9, 0.5, ninf, 0.1, 0.5],
                        [0.0, -0.0, 1.0, 0.0, ninf, ninf]], dtype=np.float32)
    ptr, items = rm.csr([[0, 2, 5, 1, 4, 3, 2], [1, 0, 3, 4, 2]])
    got = rm.ranks(block, ptr, items)
    # row 0: 0.9 first, then the 0.5s by id (0, 2, 5), then 0.1; the masked item -1; the repeated target its rank again
    assert got[:7].tolist() == [1, 2, 3, 0, 4, -1, 2]
    # row 1: -0.0 == 0.0: ids 0, 1, 3 follow 1.0 in id order
    assert got[7:].tolist() == [2, 1, 3, -1, 0]
    assert got.dtype == np.int32


def test_model_rows_by_hand():
    rows = rm.pair_rows([0, 4, -1, 9], [10, 10, 10, 1], [1, 5])
    assert rows.dtype == np.float64 and rows.shape == (4, 5)
    assert rows[0].tolist() == [0.0, 1.0, 0.0, 1.0, 1.0]
    assert rows[1].tolist() == [4.0, 0.2, 4.0 / 9.0, 0.0, 1.0]
    assert np.isnan(rows[2]).all()
    assert rows[3].tolist() == [9.0, 0.1, 0.0, 0.0, 0.0]
    # user 0: targets at ranks 0 and 3 among 10 candidates: 8 negatives, the second target has 2 negatives above it
    # user 1: no valid target; user 2: its one target is the only candidate; user 3: two targets at the same rank (a repeat)
    ptr = np.asarray([0, 2, 3, 4, 6])
    users = rm.user_rows([0, 3, -1, 0, 2, 2], ptr, [10, 10, 1, 6])
    assert users[0].tolist() == [1.0 - 2.0 / 16.0, 1.0, 0.0]
    assert np.isnan(users[1]).all() and np.isnan(users[2]).all()
    assert users[3].tolist() == [1.0 - 4.0 / 8.0, 1.0 / 3.0, 2.0]
