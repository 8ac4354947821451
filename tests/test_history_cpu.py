"""History support without a GPU: the float64 model of tests/history_model.py against brute force, the model's own share of
unclear slots on the GPU test's inputs, and the argument errors of the entry point, the wrappers, the model front, the report and
the switch, all raised before anything touches a device."""
import ctypes
import types

import numpy as np
import pytest
import torch

import history_model as hm
from helpers import build_model_from_fixture, load_golden

R = 1.0 / np.sqrt(2.0)


def test_model_on_a_hand_worked_example():
    T = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [0.0, 0.0], [-1.0, 0.0]])           # item 3: a zero row, cosine 0
    ptr = [0, 5, 5, 8]
    items = [1, 2, 2, 4, 0,   3, 1, 7]                 # segment 0: a repeated id and the target itself; 1: empty; 2: an id outside
    users = [0, 1, 2, 3, -1]
    lists = [[0, 2], [0, 2], [0, 9], [0, 1], [0, 1]]
    for excl in (True, False):
        idx, val, cnt, mean, margin = hm.support(T, [1.0], users, lists, ptr, items, 3, excl)
        # user 0, target 0: scores 0, R, R, -1 and -- not excluded -- 1 for itself
        assert idx[0, 0].tolist() == ([2, 2, 1] if excl else [0, 2, 2])
        np.testing.assert_allclose(val[0, 0], [R, R, 0.0] if excl else [1.0, R, R], atol=1e-15)
        assert cnt[0, 0] == (4 if excl else 5)
        np.testing.assert_allclose(mean[0, 0], (2 * R - 1.0) / 4 if excl else 2 * R / 5, atol=1e-15)
        # the copies of id 2 tie among themselves only: the gap to the nearest score under another id
        np.testing.assert_allclose(margin[0, 0], [R, R, R] if excl else [1.0 - R, 1.0 - R, 1.0 - R], atol=1e-15)
        # user 0, target 2: 1 and 2 x itself (excluded or not), 4, 0
        assert idx[0, 1].tolist() == ([1, 0, 4] if excl else [2, 2, 1]) and cnt[0, 1] == (3 if excl else 5)
        # an empty history, a target outside the table, users outside the index
        for b, k in ((1, 0), (1, 1), (2, 1), (3, 0), (3, 1), (4, 0), (4, 1)):
            assert idx[b, k].tolist() == [-1] * 3 and np.isneginf(val[b, k]).all() and cnt[b, k] == 0 and np.isnan(mean[b, k])
            assert np.isposinf(margin[b, k]).all()
        # user 2, target 0: the zero row scores 0, item 1 scores 0, id 7 is not listed: a tie, the lower position first
        assert idx[2, 0].tolist() == [3, 1, -1] and val[2, 0, :2].tolist() == [0.0, 0.0] and np.isneginf(val[2, 0, 2])
        assert cnt[2, 0] == 2 and mean[2, 0] == 0.0 and margin[2, 0, :2].tolist() == [0.0, 0.0]
        full = hm.support_full(T, [1.0], users, lists, ptr, items, 3, excl)
        assert full.pos[2, 0].tolist() == [0, 1, -1] and full.flat[2, 0] and not full.flat[0, 0]
        assert full.pos[0, 0].tolist() == ([1, 2, 0] if excl else [4, 1, 2])


@pytest.mark.parametrize("excl", [True, False])
def test_model_against_brute_force(excl):
    rng = np.random.default_rng(5)
    T = rng.standard_normal((30, 12))
    T[4] = 0.0
    ptr, items = hm.segments(3, rng)
    items = np.where((items >= 0) & (items < hm.ITEMS), items % 30, np.where(items < 0, -1, 30)).astype(np.int32)
    Rn = ptr.size - 1
    users = np.array(list(range(Rn)) + [-1, Rn])
    lists = rng.integers(-1, 31, (users.size, 6))
    lists[:, 0] = 4
    for w in ([1.0, 0.0, 0.5], [0.0, 2.0, 0.0]):
        for top in (1, 4):
            idx, val, cnt, mean, _ = hm.support(T, w, users, lists, ptr, items, top, excl)
            bi, bv, bc, bm = hm.brute_force(T, w, users, lists, ptr, items, top, excl)
            assert np.array_equal(cnt, bc) and np.array_equal(np.isnan(mean), np.isnan(bm))
            np.testing.assert_allclose(np.nan_to_num(mean), np.nan_to_num(bm), atol=1e-14)
            assert np.array_equal(np.isneginf(val), np.isneginf(bv))
            np.testing.assert_allclose(np.where(np.isneginf(val), 0.0, val), np.where(np.isneginf(bv), 0.0, bv), atol=1e-14)
            assert np.array_equal(idx < 0, bi < 0)
            clear = np.ones_like(idx, dtype=bool)                      # ids agree wherever the two orders cannot differ by rounding
            clear[:, :, 1:] &= np.abs(np.diff(np.where(np.isneginf(bv), 0.0, bv), axis=2)) > 1e-12
            clear[:, :, :-1] &= clear[:, :, 1:] | (top == 1)
            assert np.array_equal(idx[clear], bi[clear])


@pytest.mark.parametrize("case", hm.CASES, ids=lambda c: "d%d_b%d_K%d_top%d_B%d" % (c[0], c[1], c[3], c[4], c[5]))
def test_the_models_own_share_of_unclear_slots_stays_under_the_caps(case):
    d, w = case[0], case[2]
    for excl in (True, False):
        res = hm.case_model(case, excl)
        share = hm.unclear_share(res, hm.tol(d, w))
        print("history model %s exclude_self %d: %.4f of the returned slots unclear (cap %.2f)" % (case, excl, share, hm.unclear_cap(d)))
        assert share <= hm.unclear_cap(d), (case, excl, share)
        assert (res.idx >= 0).any()


def test_columns_and_limits():
    from elimrec_amd import _lib, ops
    assert ops.history_columns(("v", "a")) == ("sup_max_fused", "sup_max_v", "sup_max_a", "sup_mean_fused", "sup_mean_v", "sup_mean_a",
                                               "unexpected_fused", "unexpected_v", "unexpected_a", "hist_n")
    assert ops.history_columns(()) == ("sup_max_fused", "sup_mean_fused", "unexpected_fused", "hist_n")
    lib = _lib.load()
    assert lib.elimrec_abi_version() == 2
    assert ops.HISTORY_MAX_TOP == lib.elimrec_history_max_top() == 16


def test_history_index_rejects_bad_csrs():
    from elimrec_amd import ops
    ok = ops.HistoryIndex([0, 2, 2, 5], [1, 7, -1, 3, 3], "cpu")
    assert (ok.n_rows, ok.n_entries, ok.n_items, ok.sizes.tolist()) == (3, 5, None, [2, 0, 3])
    assert ok.ptr.dtype == torch.int64 and ok.items.dtype == torch.int32 and ok.items.tolist() == [1, 7, -1, 3, 3]
    empty = ops.HistoryIndex([0, 0], [], "cpu", n_items=4)
    assert (empty.n_rows, empty.n_entries, empty.n_items) == (1, 0, 4) and empty.items.numel() == 1
    for ptr, items in (([0], []), ([], []), ([1, 2], [0, 1]), ([0, 3], [0, 1]), ([0, 2, 1, 3], [0, 1, 2]), ([0, 1], [0, 1])):
        with pytest.raises(ValueError):
            ops.HistoryIndex(ptr, items, "cpu")
    with pytest.raises(TypeError):
        ops.HistoryIndex([0, 2], [0.5, 1.0], "cpu")
    for items in ([0, 4], [-1, 2]):
        with pytest.raises(IndexError):
            ops.HistoryIndex([0, 2], items, "cpu", n_items=4)
    with pytest.raises(IndexError):
        ops.HistoryIndex([0, 1], [2 ** 31], "cpu")


def test_entry_point_refuses_bad_arguments_before_it_looks_at_a_pointer():
    from elimrec_amd import _lib
    lib = _lib.load()
    w = (ctypes.c_float * 8)(*([1.0] * 8))
    for kw in (dict(K=0), dict(K=257), dict(top=0), dict(top=17), dict(d=6), dict(d=260), dict(d=0), dict(blocks=0), dict(blocks=9),
               dict(B=-1), dict(ld=100), dict(ld_sq=1), dict(n_items=-1), dict(n_items=2 ** 31), dict(rows=-1), dict(excl=2),
               dict(w=None)):
        a = dict(K=5, top=3, d=64, blocks=2, B=2, ld=128, ld_sq=2, n_items=100, rows=4, excl=1, w=w)
        a.update(kw)
        rc = lib.elimrec_history_support(None, a["ld"], a["n_items"], a["blocks"], a["d"], None, a["ld_sq"], a["w"], None, None, a["B"],
                                         a["K"], None, None, a["rows"], a["top"], a["excl"], None, None, None, None, None)
        assert rc == 10001 and b"history_support" in lib.elimrec_last_error(), (kw, rc)          # ELIMREC_E_BADARG
    rc = lib.elimrec_history_support(None, 128, 100, 2, 64, None, 2, w, None, None, 2, 5, None, None, 4, 3, 1, None, None, None, None, None)
    assert rc == 10001 and b"null pointer" in lib.elimrec_last_error()                          # good numbers, no pointers, B > 0
    assert lib.elimrec_history_support(None, 128, 100, 2, 64, None, 2, None, None, None, 0, 5, None, None, 4, 3, 1, None, None, None, None,
                                       None) == 0                                               # B == 0


def test_wrapper_errors_that_need_no_device():
    from elimrec_amd import ops
    table, sq = torch.zeros(8, 8), torch.zeros(8, 2)
    users, lists = torch.zeros(2, dtype=torch.int64), torch.zeros(2, 3, dtype=torch.int32)
    hist = ops.HistoryIndex([0, 1], [0], "cpu")
    oi, ov = torch.zeros(2, 3, 2, dtype=torch.int32), torch.zeros(2, 3, 2)
    for w in ([], [1.0] * 9):
        with pytest.raises(ValueError, match="blocks"):
            ops.history_support(table, sq, w, users, lists, hist, 2, oi, ov)
    with pytest.raises(ValueError, match="equal blocks"):
        ops.history_support(table, sq, [1.0] * 3, users, lists, hist, 2, oi, ov)
    with pytest.raises(ValueError, match="d % 4"):
        ops.history_support(torch.zeros(8, 6), torch.zeros(8, 1), [1.0], users, lists, hist, 2, oi, ov)
    for top in (0, 17, -1, 2.5, True):
        with pytest.raises(ValueError, match="top"):
            ops.history_support(table, sq, [1.0, 0.0], users, lists, hist, top, oi, ov)
    with pytest.raises(TypeError, match="HistoryIndex"):
        ops.history_support(table, sq, [1.0, 0.0], users, lists, ([0, 1], [0]), 2, oi, ov)
    with pytest.raises(RuntimeError, match="HIP device"):                       # everything host-checkable is fine: no CPU path
        ops.history_support(table, sq, [1.0, 0.0], users, lists, hist, 2, oi, ov)


def test_torch_op_is_registered():
    from elimrec_amd import torch_ops
    assert hasattr(torch_ops.load(), "history_support") and "history_support" in torch_ops.OPS


def test_model_front_errors():
    from elimrec_amd import HistorySupport
    model, _ = build_model_from_fixture(load_golden("ml3"), "cpu")
    I = model.num_items
    assert HistorySupport._fields == ("items", "history", "scores", "count", "mean")
    for kw in (dict(), dict(items=[[0], [1]], top_k=2), dict(items=[[0], [1]], top=0), dict(top_k=2, top=17), dict(top_k=2, top=2.5),
               dict(top_k=0), dict(top_k=I + 1), dict(top_k=257), dict(items=[[0]]), dict(items=[[0] * 257, [1]]),
               dict(top_k=2, space="x"), dict(items=[[0], [1]], exclude={0: [1]})):
        with pytest.raises(ValueError):
            model.explain_history([0, 1], **kw)
    for kw in (dict(items=[[0], [I]]), dict(items=[[-1], [0]]), dict(top_k=2, history={0: [I]}), dict(top_k=2, exclude={1: [-1]})):
        with pytest.raises(IndexError):
            model.explain_history([0, 1], **kw)
    with pytest.raises(TypeError):
        model.explain_history([0, 1], top_k=2, history=[[0], [1]])
    with pytest.raises(RuntimeError):                                             # good arguments on a CPU model: no CPU path
        model.explain_history([0, 1], top_k=2)
    users, lists = torch.zeros(2, dtype=torch.int64), torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match="space"):
        model.history_support_device(users, lists, None, space="x")
    with pytest.raises(RuntimeError):
        model.history_support_device(users, lists, None)


def test_history_report_checks():
    from elimrec_amd import ops
    from elimrec_amd.evaluator import HistoryReport
    ds = types.SimpleNamespace(num_items=6, num_users=4)
    train = {0: [1, 2], 1: [2], 2: [], 3: [0, 1, 2, 3]}
    test = {0: [3], 2: [4, 5], 3: [5]}
    for bad in (0, -1, 7, ops.LIST_MAX_K + 1, 2.5, True, None):
        with pytest.raises(ValueError):
            HistoryReport(ds, train, test, bad)
    for bad in (0, 17, -1, 2.5, True, None):
        with pytest.raises(ValueError):
            HistoryReport(ds, train, test, 2, top=bad)
    with pytest.raises((TypeError, ValueError)):
        HistoryReport(ds, train, test, 2, group_view=[3, 3])
    with pytest.raises(TypeError):
        HistoryReport(ds, [1, 2], test, 2)
    big = types.SimpleNamespace(num_items=5000, num_users=4)
    assert HistoryReport(big, train, test, 256).top_k == 256
    with pytest.raises(ValueError):
        HistoryReport(big, train, test, 257)
    rep = HistoryReport(ds, train, test, 2, group_view=[2, 10])
    assert (rep.top_k, rep.top, rep.users, rep.name, rep.needs) == (2, 3, [0, 2, 3], "history", "history_support_device")
    assert [x.strip() for x in rep.group_labels] == ["all:", "(0,2]:", "(2,10]:"]
    assert [p.tolist() for p in rep._positions] == [[0, 2], [0], [2]]            # user 2 has no history: in no group's rows
    with pytest.raises(TypeError):
        rep.evaluate(object())


def test_basic_model_switches():
    g = load_golden("ml3")
    model, _ = build_model_from_fixture(g, "cpu")
    assert model.history_reporter is None
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--history_report=0", "--history_top=99"])
    assert model.history_reporter is None
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--history_report=3", "--group_view=[2,4]"])
    rep = model.history_reporter
    assert (rep.top_k, rep.top, rep.num_items) == (3, 3, model.num_items) and len(rep.group_labels) >= 2
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--history_report=1", "--history_top=16"])
    assert (model.history_reporter.top_k, model.history_reporter.top) == (1, 16)
    for bad in (["--history_report=-2"], ["--history_report=%d" % (model.num_items + 1)], ["--history_report=257"],
                ["--history_report=3", "--history_top=0"], ["--history_report=3", "--history_top=17"]):
        with pytest.raises(ValueError):
            build_model_from_fixture(g, "cpu", extra_argv=bad)
