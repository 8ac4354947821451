"""The list report, host side (no GPU): the numpy model's self-checks, exposure_summary's known answers, the host-only entry points
of csrc/lists.hip, the column names and the argument checks that run before anything touches the device."""
import types

import numpy as np
import pytest
import torch

import lists_model as lm
from helpers import build_model_from_fixture, load_golden


def test_model_against_triple_loops():
    rng = np.random.default_rng(5)
    for n, d, blocks, K in ((3, 4, 1, 2), (6, 8, 2, 5), (7, 4, 3, 9)):
        T = rng.standard_normal((n, blocks * d))
        T[1] = 0.0                                                    # a zero row: the floor, not a division by zero
        sq = np.stack([(T[:, h * d:(h + 1) * d] ** 2).sum(1) for h in range(blocks)], 1).astype(np.float32)
        lists = rng.integers(-2, n + 2, size=(6, K))
        lists[0] = np.arange(K) % n                                   # duplicates once K > n
        lists[1] = -1
        lists[2, 1:] = n
        a, b = lm.pair_cosine64(T, sq, lists, blocks), lm.pair_cosine64_loops(T, sq, lists.tolist(), blocks)
        assert np.isnan(a[1]).all() and np.isnan(a[2]).all() and not np.isnan(a[0]).any()
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.allclose(a, b, rtol=0, atol=1e-14, equal_nan=True)
    same = np.tile(rng.standard_normal((1, 8)), (4, 1))
    got = lm.pair_cosine64(same, (same ** 2).sum(1, keepdims=True), [[0, 1, 2, 3], [2, 2, -1, 2]], 1)
    assert np.allclose(got, 1.0, rtol=0, atol=1e-7)                   # (the squared norms are float32)
    assert lm.exposure([[0, 2, 2], [5, -1, 4]], 5).tolist() == [1, 0, 2, 0, 1]


def test_exposure_summary_known_answers():
    from elimrec_amd.evaluator import EXPOSURE_COLUMNS, exposure_summary
    assert EXPOSURE_COLUMNS == ("items", "coverage", "gini", "entropy", "slot_share")
    for n in (1, 2, 7, 64):
        every = np.arange(n)
        equal = exposure_summary(np.full(n, 3), [every])
        assert equal.dtype == np.float64 and equal.shape == (1, 5)
        assert equal[0, 0] == n and equal[0, 1] == 1.0 and abs(equal[0, 2]) < 1e-15 and abs(equal[0, 3] - np.log2(n)) < 1e-12
        assert equal[0, 4] == 1.0
        hot = np.zeros(n, dtype=np.int32)
        hot[n // 2] = 11
        one = exposure_summary(hot, [every])
        assert abs(one[0, 1] - 1.0 / n) < 1e-15 and abs(one[0, 2] - (n - 1.0) / n) < 1e-15 and one[0, 3] == 0.0
        assert not np.signbit(one[0, 3])
    counts = np.asarray([4, 0, 0, 1, 3, 0])
    groups = [np.arange(6), np.asarray([], dtype=np.int64), np.asarray([1, 2, 5]), np.asarray([0, 3, 4])]
    got = exposure_summary(counts, groups)
    assert got[1].tolist() == [0.0, 0.0, 0.0, 0.0, 0.0]                # an empty group
    assert got[2].tolist() == [3.0, 0.0, 0.0, 0.0, 0.0]                # an all-zero group
    assert got[3, 4] == 1.0 and got[0, 4] == 1.0 and got[0, 1] == 0.5
    assert exposure_summary(np.zeros(4), [np.arange(4)])[0].tolist() == [4.0, 0.0, 0.0, 0.0, 0.0]
    rng = np.random.default_rng(3)
    counts = rng.integers(0, 9, size=40)
    groups = [np.arange(40), rng.permutation(40)[:13], np.asarray([7]), np.asarray([], dtype=np.int64)]
    assert np.allclose(exposure_summary(counts, groups), lm.exposure_summary_loops(counts, groups), rtol=0, atol=1e-12)
    assert ((exposure_summary(counts, groups)[:, 2] >= 0) & (exposure_summary(counts, groups)[:, 2] < 1)).all()


def test_model_rows_means_and_shift():
    ils = np.asarray([[0.5, 0.25], [np.nan, np.nan], [1.0, 0.0]], dtype=np.float32)
    lists = np.asarray([[1, 2], [-1, -1], [0, -1]])
    rows = lm.rows(ils, lists, [4, 0, 3])
    assert rows.dtype == np.float32 and rows.shape == (3, 3)
    assert rows[0].tolist() == [0.5, 0.25, 1.5] and np.isnan(rows[1]).all() and rows[2].tolist() == [1.0, 0.0, 4.0]
    assert lm.means(rows, [np.asarray([0, 2]), np.asarray([2])]).tolist() == [[0.75, 0.125, 2.75], [1.0, 0.0, 4.0]]
    sh = lm.shift_rows(rows, lists, rows[::-1], np.asarray([[2, 5], [-1, -1], [-1, 0]]))
    assert sh[:, 0].tolist() == [0.5, 0.0, 0.5] and sh[0, 1:].tolist() == [0.5, -0.25, 2.5]


def test_host_entry_points_without_a_gpu():
    from elimrec_amd import _lib, ops
    lib = _lib.load()
    assert ops.LIST_MAX_K == lib.elimrec_list_max_k() == 256 and ops.LIST_SMALL_K == lib.elimrec_list_pair_cosine_small_k()
    assert 16 <= ops.LIST_SMALL_K < ops.LIST_MAX_K and ops.LIST_SMALL_K % 16 == 0
    for K in (1, 16, 17, 50, 255, 256):
        KP = 16 * ((K + 15) // 16)
        for d in (4, 36, 64, 128, 256):
            dc = ops.list_chunk_cols(K, d)
            assert 4 <= dc <= d and dc % 4 == 0
            assert KP * (dc + 4) * 4 + KP * 8 + 64 <= 64 * 1024         # the workgroup's LDS stays within the default limit
            assert dc == d or KP * (dc + 8) * 4 > 60 * 1024              # all of d, or the widest chunk that fits
    assert ops.list_chunk_cols(10, 64) == 64 and ops.list_chunk_cols(256, 256) < 256
    for bad in ((0, 64), (257, 64), (10, 6), (10, 260), (10, 0)):
        assert ops.list_chunk_cols(*bad) == 0


def test_cpu_tensors_are_refused():
    from elimrec_amd import ops
    lists = torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.list_pair_cosine(torch.zeros(8, 4), torch.zeros(8, 1), lists, torch.zeros(2, 1))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.list_exposure(lists, torch.zeros(8, dtype=torch.int32))


def test_list_columns():
    from elimrec_amd import ops
    assert ops.list_columns(("v", "a", "t")) == ("ils_fused", "ils_v", "ils_a", "ils_t", "pop")
    assert ops.list_columns(("v",)) == ("ils_fused", "ils_v", "pop")
    assert ops.list_columns(()) == ("ils_fused", "pop")


def test_list_report_checks():
    from elimrec_amd import ops
    from elimrec_amd.evaluator import ListReport
    ds = types.SimpleNamespace(num_items=6, num_users=3)
    train = {0: [1, 2], 1: [2], 2: []}
    test = {0: [3], 2: [4, 5]}
    for bad in (0, 1, -1, ops.LIST_MAX_K + 1, 2.5, True):
        with pytest.raises(ValueError):
            ListReport(ds, train, test, bad)
    for bad in ([], [0, 3], [3, 3], (1, 4)):
        with pytest.raises((TypeError, ValueError)):
            ListReport(ds, train, test, 3, item_group_view=bad)
    with pytest.raises((TypeError, ValueError)):
        ListReport(ds, train, test, 3, group_view=[3, 3])
    with pytest.raises(TypeError):
        ListReport(ds, [1, 2], test, 3)
    with pytest.raises(TypeError):
        ListReport(ds, train, [1], 3)
    rep = ListReport(ds, train, test, 3, group_view=[1], item_group_view=[1])
    assert rep.users == [0, 2] and rep.top_k == 3 and rep.block_users == 8192 and rep.item_counts.tolist() == [0, 1, 2, 0, 0, 0]
    assert [x.strip() for x in rep.item_labels] == ["all:", "item cold:", "item (0,1]:", "item (1,inf):"]
    assert [p.tolist() for p in rep._item_positions] == [[0, 1, 2, 3, 4, 5], [0, 3, 4, 5], [1], [2]]
    assert rep.group_labels[0].strip() == "all:" and rep._positions[0].tolist() == [0, 1] and len(rep.group_labels) >= 2
    plain = ListReport(ds, train, test, ops.LIST_MAX_K)
    assert len(plain.group_labels) == 1 and len(plain.item_labels) == 1
    with pytest.raises(TypeError):
        plain.list_rows(object())


def test_basic_model_switch():
    from elimrec_amd import ops
    g = load_golden("ml3")
    model, _ = build_model_from_fixture(g, "cpu")
    assert model.list_reporter is None
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--list_report=0"])
    assert model.list_reporter is None
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--list_report=5", "--group_view=[2,4]", "--item_group_view=[1,4]"])
    rep = model.list_reporter
    assert rep.top_k == 5 and len(rep.item_labels) >= 2 and len(rep.group_labels) >= 2 and rep.num_items == model.num_items
    for bad in (-1, 1, ops.LIST_MAX_K + 1, model.num_items + 1):
        with pytest.raises(ValueError):
            build_model_from_fixture(g, "cpu", extra_argv=["--list_report=%d" % bad])
    with pytest.raises(ValueError):
        model.list_similarity([[0, 1]], space="x")
    with pytest.raises(ValueError):
        model.list_similarity([list(range(ops.LIST_MAX_K + 1))])
    with pytest.raises(IndexError):
        model.list_similarity([[0, model.num_items]])
    with pytest.raises(IndexError):
        model.list_similarity([[0, 1], [-1]])
