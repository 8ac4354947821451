"""Grouped evaluation (group_view) without a GPU: the group assignment against a literal restatement of the reference's
evaluator/grouped_evaluator.py:63-80, the fixtures' groups, construction through the configuration, the string format."""
from collections import OrderedDict

import numpy as np
import pytest

from helpers import build_model_from_fixture, csr_dict, load_golden, make_config


def _reference_groups(user_train_dict, user_test_dict, group_view):
    """grouped_evaluator.py:63-80 line for line, the pandas groupby (ascending group index, the users of a group in their
    original order) written out; a user without training items counts 0 interactions."""
    group_list = [0] + group_view
    group_info = [("(%d,%d]:" % (g_l, g_h)).ljust(12) for g_l, g_h in zip(group_list[:-1], group_list[1:])]
    all_test_user = list(user_test_dict.keys())
    num_interaction = [len(user_train_dict.get(u, [])) for u in all_test_user]
    group_idx = np.searchsorted(group_list[1:], num_interaction)
    grouped_user = OrderedDict()
    for idx in sorted(set(group_idx.tolist())):
        if idx < len(group_info):
            grouped_user[group_info[idx]] = [u for u, g in zip(all_test_user, group_idx) if g == idx]
    if not grouped_user:
        raise ValueError("The splitting of user groups is not suitable!")
    return grouped_user


def test_assign_user_groups_is_the_references_rule():
    """n_train of 0, exactly on a bound, one above a bound and beyond the last bound; an empty middle group is omitted; labels
    and order."""
    from elimrec_amd.evaluator import assign_user_groups
    view = [2, 4, 6, 9]
    n_train = {10: 0, 11: 2, 12: 3, 13: 9, 14: 10, 15: 1, 16: 7, 17: 30, 18: 2, 19: 8}      # nobody in (4,6]
    train = {u: list(range(n)) for u, n in n_train.items() if u != 10}                       # user 10: absent from the dict
    test = OrderedDict((u, [0]) for u in (14, 10, 13, 12, 11, 15, 16, 17, 18, 19))
    users = list(test.keys())
    labels, positions, discarded = assign_user_groups(users, train, view)
    want = _reference_groups(train, test, view)
    assert labels == list(want.keys()) == ["(0,2]:".ljust(12), "(2,4]:".ljust(12), "(6,9]:".ljust(12)]
    assert [[users[i] for i in at] for at in positions] == list(want.values()) == [[10, 11, 15, 18], [12], [13, 16, 19]]
    assert discarded == 2                                                                    # users 14 and 17
    assert all(at.dtype == np.int64 for at in positions)
    # a single bound, every user inside
    labels, positions, discarded = assign_user_groups(users, train, [30])
    assert labels == ["(0,30]:".ljust(12)] and positions[0].tolist() == list(range(10)) and discarded == 0


def test_assign_user_groups_errors():
    from elimrec_amd.evaluator import assign_user_groups
    train = {0: [1, 2, 3], 1: [1, 2, 3, 4]}
    for bad in (7, (1, 3), None, "[1,3]"):
        with pytest.raises(TypeError, match="must be `list`"):
            assign_user_groups([0, 1], train, bad)
    with pytest.raises(ValueError, match="The splitting of user groups is not suitable!"):
        assign_user_groups([0, 1], train, [1, 2])                  # both users beyond the last bound
    with pytest.raises(ValueError, match="not suitable"):
        assign_user_groups([0, 1], train, [])
    for bad in ([3, 3], [5, 3], [0, 3], [-1, 3], [1.5, 3], [True, 3]):
        with pytest.raises(ValueError, match="strictly ascending positive integers"):
            assign_user_groups([0, 1], train, bad)


@pytest.mark.parametrize("name, sizes", [("ml3", [25, 30]), ("kwai", [16, 19])])
def test_fixture_groups(name, sizes):
    """group_view = [1, 3, 5] on the fixtures: (0,1] has no user and is absent, 15 users have more than 5 training items."""
    from elimrec_amd import ProxyEvaluator
    from elimrec_amd.evaluator import GroupedEvaluator
    g = load_golden(name)
    train, test = csr_dict(g, "train"), csr_dict(g, "test")
    ev = ProxyEvaluator(None, train, test, metric=["Recall"], group_view=[1, 3, 5], top_k=[10]).evaluator
    assert isinstance(ev, GroupedEvaluator)
    assert ev.group_labels == ["(1,3]:".ljust(12), "(3,5]:".ljust(12)]
    assert ev.group_sizes == sizes and ev.num_discarded == 15
    assert sum(sizes) + 15 == len(test)
    assert ev.grouped_user == dict(_reference_groups(train, test, [1, 3, 5]))
    assert ev.metrics_info() == ev.evaluator.metrics_info() == "metrics:\t" + "Recall@10".ljust(12)


def test_group_view_constructs_through_the_configuration():
    """--group_view=[1,3,5] reaches both evaluators of the model (it raised NotImplementedError before); the --tie_order
    plumbing reaches the evaluator that ranks; a scalar is a TypeError."""
    from elimrec_amd.evaluator import GroupedEvaluator, UniEvaluator
    assert make_config(["--group_view=[1,3,5]"])["group_view"] == [1, 3, 5]
    g = load_golden("ml3")
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--group_view=[1,3,5]", "--tie_order=id"])
    for facade in (model.valid_evaluator, model.test_evaluator):
        assert isinstance(facade.evaluator, GroupedEvaluator) and isinstance(facade.evaluator.evaluator, UniEvaluator)
        assert facade.evaluator.evaluator.tie_order == "id" and facade.evaluator.tie_order == "id"
        assert facade.metrics_info().startswith("metrics:\tPrecision@10")
    assert model.test_evaluator.evaluator.group_sizes == [25, 30]
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--group_view=[1,3,5]"])
    assert model.test_evaluator.evaluator.evaluator.tie_order == "reference"
    with pytest.raises(TypeError, match="must be `list`"):
        build_model_from_fixture(g, "cpu", extra_argv=["--group_view=7"])
    plain, _ = build_model_from_fixture(g, "cpu")
    assert isinstance(plain.test_evaluator.evaluator, UniEvaluator)


def test_group_table_string_format():
    """Per group "\\n" + label + "\\t" + the tab-joined "%.8f".ljust(12) fields (grouped_evaluator.py:107-112 around the
    evaluator's own line format)."""
    from elimrec_amd.evaluator import GroupedEvaluator
    train = {0: [1], 1: [1, 2, 3], 2: [4, 5, 6, 7]}
    test = {0: [9], 1: [9], 2: [9]}
    ev = GroupedEvaluator(None, train, test, metric=["Recall", "NDCG"], group_view=[1, 3, 5], top_k=[5])
    final = np.asarray([[0.5, 0.25], [1.0, 0.0], [0.123456789, 2.0 / 3.0]], dtype=np.float32)
    buf = ev.format_groups(final)
    assert buf == ("\n(0,1]:      \t0.50000000  \t0.25000000  "
                   "\n(1,3]:      \t1.00000000  \t0.00000000  "
                   "\n(3,5]:      \t0.12345679  \t0.66666669  ")
    lines = buf.split("\n")
    assert lines[0] == "" and len(lines) == 4
    # the host-side index check of the device reduction: an index outside the block never reaches a kernel
    from elimrec_amd import ops
    with pytest.raises(IndexError, match="the block has 3 rows"):
        ops.GroupIndex([0, 2], [0, 3], 3, "cpu")
    with pytest.raises(IndexError):
        ops.GroupIndex([0, 2], [-1, 2], 3, "cpu")
    with pytest.raises(ValueError, match="must ascend from 0"):
        ops.GroupIndex([0, 2, 1], [0, 1], 3, "cpu")
    with pytest.raises(ValueError, match="must ascend from 0"):
        ops.GroupIndex([0, 3], [0, 1], 3, "cpu")
    idx = ops.GroupIndex([0, 2, 2, 3], [2, 0, 2], 3, "cpu")
    assert (idx.n_groups, idx.n_listed, idx.sizes.tolist()) == (3, 3, [2, 0, 1])
