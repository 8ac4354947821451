"""Calibrated re-ranking, host side (no GPU): the float64 model of tests/calibrate_model.py on hand-worked pools and against its
plain-loops form, the bindings of csrc/calibrate.hip, the argument checks of the ops wrappers, EliMRec.recommend_calibrated,
CalibrationReport and the --calibrate_* switches that run before anything touches the device -- and the model's own statement
about the device test's inputs: nearly every list's every step is clear."""
import math
import types

import numpy as np
import pytest
import torch

import calibrate_cases as cc
import calibrate_model as cm
from helpers import build_model_from_fixture, load_golden


def test_bindings_are_present():
    from elimrec_amd import _lib, ops, torch_ops
    lib = _lib.load()
    for name in ("elimrec_calibrate_rerank", "elimrec_class_shares_csr", "elimrec_list_calibration", "elimrec_calibrate_max_classes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    ns = torch_ops.load()
    for name in ("calibrate_rerank", "list_calibration"):
        assert hasattr(ns, name) and name in torch_ops.OPS
    assert ops.CALIBRATE_MAX_CLASSES == lib.elimrec_calibrate_max_classes() == 16
    assert lib.elimrec_abi_version() == 2


def test_c_entry_points_refuse_bad_arguments_before_any_launch():
    from elimrec_amd import _lib
    lib = _lib.load()
    for kw in (dict(K=0), dict(K=11), dict(N=257, K=257), dict(N=0, K=0), dict(C=0), dict(C=17), dict(lam=-0.1), dict(lam=1.5),
               dict(lam=float("nan")), dict(smooth=0.0), dict(smooth=1.0), dict(smooth=float("nan")), dict(B=-1), dict(ld=2)):
        a = dict(N=10, K=5, C=3, lam=0.5, smooth=0.01, B=2, ld=3)
        a.update(kw)
        rc = lib.elimrec_calibrate_rerank(None, None, a["B"], a["N"], a["K"], None, 100, None, a["ld"], a["C"], a["lam"], a["smooth"],
                                          None, None, None, None)
        assert rc == 10001 and b"calibrate_rerank" in lib.elimrec_last_error(), (kw, rc)         # ELIMREC_E_BADARG
    assert lib.elimrec_calibrate_rerank(None, None, 0, 10, 5, None, 100, None, 3, 3, 0.5, 0.01, None, None, None, None) == 0   # B == 0
    for C in (0, 17):
        assert lib.elimrec_class_shares_csr(None, None, 0, 2, None, 100, C, None, None) == 10001
        assert lib.elimrec_list_calibration(None, 2, 4, None, 100, C, None, None, 0, 0.01, None, None) == 10001
    assert b"list_calibration" in lib.elimrec_last_error()
    assert lib.elimrec_list_calibration(None, 2, 0, None, 100, 3, None, None, 0, 0.01, None, None) == 10001      # K == 0
    assert lib.elimrec_class_shares_csr(None, None, 0, 0, None, 100, 3, None, None) == 0
    assert lib.elimrec_list_calibration(None, 0, 4, None, 100, 3, None, None, 0, 0.01, None, None) == 0


def test_hand_checked_pool():
    """p = (1/2, 1/2), classes 0 0 0 1, lam = 0, K = 2, smooth = 0.01. Step 0: a candidate of class 0 gives q = (1, 0), one of class
    1 gives q = (0, 1): the same two terms in the other order -- a tie, position 0 wins. Step 1 (n = (1, 0)): class 1 gives
    q = (1/2, 1/2) = p, so q~ = p and KL = 0; class 0 gives q = (1, 0) again: position 3 wins."""
    ids, vals, class_of, p = [0, 1, 2, 3], [0.9, 0.8, 0.7, 0.6], [0, 0, 0, 1], [0.5, 0.5]
    picks, objs, margins = cm.greedy(ids, vals, class_of, p, 2, 0.0)
    kl_10 = 0.5 * math.log(0.5 / (0.99 * 1.0 + 0.01 * 0.5)) + 0.5 * math.log(0.5 / (0.99 * 0.0 + 0.01 * 0.5))
    assert abs(kl_10 - (0.5 * math.log(0.5 / 0.995) + 0.5 * math.log(100.0))) < 1e-15 and 1.95 < kl_10 < 1.96
    assert picks == [0, 3]
    assert abs(objs[0] + kl_10) <= 1e-15 and abs(objs[1]) <= 1e-15
    assert margins[0] == 0.0 and abs(margins[1] - kl_10) <= 1e-15           # step 0: the other class ties exactly
    assert cm.greedy_loops(ids, vals, class_of, p, 2, 0.0) == picks
    # with some weight on relevance the tie of step 0 is still position 0's (rel = 1), and step 1 weighs 0.3 * 1/3 against KL
    picks, objs, _ = cm.greedy(ids, vals, class_of, p, 4, 0.3)
    assert picks[:2] == [0, 3] and abs(objs[0] - (0.3 - 0.7 * kl_10)) <= 1e-15
    assert sorted(picks) == [0, 1, 2, 3]


def test_orders_that_keep_the_pool():
    rng = np.random.default_rng(3)
    ids = rng.permutation(30)[:12]
    vals = -np.sort(-rng.uniform(size=12))
    vals[5] = vals[4]                                                         # equal scores: the lower position first
    class_of = rng.integers(0, 4, 30)
    p = [0.1, 0.0, 0.6, 0.3]
    for lam in (0.0, 0.4, 1.0):
        assert cm.greedy(ids, vals, np.zeros(30, dtype=int), [1.0], 12, lam)[0] == list(range(12))       # C = 1
        assert cm.greedy(ids, vals, class_of, [0.0, 0.0, 0.0, 0.0], 12, lam)[0] == list(range(12))       # a zero target row
        assert cm.greedy(ids, vals, class_of, [-1.0, np.nan, np.inf, 0.0], 12, lam)[0] == list(range(12))
    assert cm.greedy(ids, vals, class_of, p, 12, 1.0)[0] == list(range(12))                              # lam = 1
    assert cm.greedy(ids, vals, class_of, p, 7, 0.0)[0] != list(range(7))


def test_unlisted_entries():
    class_of = [0, 1, 2, 0, 5, -1]
    ids = [0, -1, 6, 1, 2, 4, 5, 3]
    vals = [0.9, 0.8, 0.7, np.nan, 0.5, 0.4, 0.3, np.inf]
    P = cm.Pools64([ids], [vals], class_of, [[0.5, 0.25, 0.25]])
    # id -1, id 6 (outside), NaN score, class 5 and class -1 (outside [0, 3)), inf score
    assert P.mask[0].tolist() == [True, False, False, False, True, False, False, False]
    picks, objs, margins = P.greedy(4, 0.5)
    assert picks[0].tolist() == [0, 4, -1, -1] and np.isneginf(objs[0, 2:]).all() and margins[0, 1] == np.inf
    o, best, ok = P.replay([[4, 0, -1, -1]], 0.5)
    assert ok.all() and np.isnan(o[0, 2:]).all() and o[0, 0] <= best[0, 0]
    for bad in ([[1, 0, -1, -1]], [[0, 0, -1, -1]], [[0, 9, -1, -1]]):        # unlisted, picked twice, outside the pool
        assert not P.replay(bad, 0.5)[2].all()
    assert cm.greedy([-1, 7], [0.1, 0.2], class_of, [1.0, 0.0, 0.0], 2, 0.5) == ([], [], [])
    assert cm.greedy([0, 0, 1], [0.9, 0.8, 0.1], class_of, [0.5, 0.5, 0.0], 3, 0.0)[0] == [0, 2, 1]     # duplicates are positions


def test_batched_model_against_loops():
    rng = np.random.default_rng(2)
    class_of = rng.integers(0, 5, 40)
    class_of[7] = 5
    ids = np.stack([rng.permutation(40)[:12] for _ in range(6)])
    ids[1, 4], ids[2, 0] = -1, 40
    vals = -np.sort(-rng.uniform(size=(6, 12)), axis=1)
    vals[3, 5] = np.nan
    p = rng.dirichlet(np.ones(5), 6)
    p[0, 2], p[4] = 0.0, 0.0
    P = cm.Pools64(ids, vals, class_of, p)
    for lam in (0.0, 0.4, 1.0):
        picks, objs, _ = P.greedy(12, lam)
        for b in range(6):
            want = cm.greedy_loops(ids[b], vals[b], class_of, p[b], 12, lam)
            assert picks[b, :len(want)].tolist() == want and (picks[b, len(want):] == -1).all()
        o, best, ok = P.replay(picks, lam)
        filled = picks >= 0
        assert ok.all() and np.array_equal(o[filled], objs[filled]) and np.array_equal(o[filled], best[filled])


def test_class_shares_and_c_kl_model():
    class_of = [0, 1, 1, 2, 7]
    lists = [[0, 1, 2, 2], [3, -1, 9, 4], [-1, -1, -1, -1]]
    assert cm.class_counts(lists, class_of, 3).tolist() == [[1, 3, 0], [0, 0, 1], [0, 0, 0]]
    sh = cm.class_shares(lists, class_of, 3)
    assert sh.dtype == np.float32 and sh.tolist() == [[0.25, 0.75, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, 0.0]]
    third = cm.class_shares([[0, 1, 3]], class_of, 3)[0, 0]
    assert third == np.float32(1) / np.float32(3)
    p = cm.targets([0.5, np.nan, -2.0, 0.5])
    assert p.tolist() == [0.5, 0.0, 0.0, 0.5]
    assert abs(cm.c_kl(p, [0.5, 0.0, 0.0, 0.5])) <= 1e-15                     # q = p: q~ = p
    want = 0.5 * math.log(0.5 / (0.99 * 0.25 + 0.005)) + 0.5 * math.log(0.5 / (0.99 * 0.0 + 0.005))
    assert abs(cm.c_kl(p, [0.25, 0.75, 0.0, 0.0]) - want) <= 1e-15
    assert cm.c_kl([0.0, 0.0], [0.3, 0.7]) == 0.0
    kl = cm.list_kl(lists, class_of, 3, [[0.25, 0.75, 0.0]] * 3)
    assert abs(kl[0]) <= 1e-15 and abs(kl[2] - math.log(100.0)) <= 1e-14      # nothing listed: q = 0, every term is p log(1 / smooth)


@pytest.mark.parametrize("shape", cc.SHAPES, ids=lambda s: "N%d_K%d_C%d" % s)
def test_the_device_tests_inputs_are_clear(shape):
    """What the device test relies on: on its pools every step of at least 99 % of the lists has a float64 margin above TOL, at
    every lambda -- so "equal up to the first unclear step" there means "equal" for nearly every list."""
    N, K, C = shape
    P = cc.pools(N, K, C)
    assert P.mask.all() and (cc.case(N, K, C)[3] == 0).any() == (C > 1)
    for lam in cc.LAMBDAS:
        picks, _, margins = cc.greedy(N, K, C, lam)
        assert (picks >= 0).all()
        clear = (margins > cc.TOL).all(axis=1)
        assert clear.mean() >= 0.99, (shape, lam, clear.mean())


def test_ops_argument_errors_that_need_no_device():
    from elimrec_amd import ops
    idx, val = torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 3)
    class_of, target = torch.zeros(8, dtype=torch.int32), torch.zeros(2, 4)
    out = torch.zeros(2, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.calibrate_rerank(idx, val, class_of, target, 2, 0.5, out)        # everything is in order but the device
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.calibrate_rerank(idx.tolist(), val, class_of, target, 2, 0.5, out)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.calibrate_rerank(idx, val, class_of, target, 2, 0.5, None)
    for K, lam, smooth in ((0, 0.5, 0.01), (4, 0.5, 0.01), (2.5, 0.5, 0.01), (True, 0.5, 0.01), (2, -0.01, 0.01), (2, 1.01, 0.01),
                           (2, float("nan"), 0.01), (2, 0.5, 0.0), (2, 0.5, 1.0), (2, 0.5, float("nan"))):
        with pytest.raises(ValueError, match="calibrate_rerank"):
            ops.calibrate_rerank(idx, val, class_of, target, K, lam, out, smooth=smooth)
    for bad_idx, bad_val in ((idx, torch.zeros(2, 4)), (idx[:, :2], val[:, :2]), (idx.reshape(-1), val.reshape(-1)), (idx.long(), val),
                             (idx, val.double()), (torch.zeros(2, 257, dtype=torch.int32), torch.zeros(2, 257))):
        with pytest.raises(ValueError, match="calibrate_rerank"):
            ops.calibrate_rerank(bad_idx, bad_val, class_of, target, 2, 0.5, out)
    for bad_cls in (class_of.long(), class_of.reshape(2, 4), torch.zeros(16, dtype=torch.int32)[::2]):
        with pytest.raises(ValueError, match="calibrate_rerank"):
            ops.calibrate_rerank(idx, val, bad_cls, target, 2, 0.5, out)
    for bad_target in (torch.zeros(3, 4), torch.zeros(2, 17), torch.zeros(2, 0), torch.zeros(2, 4).double(), torch.zeros(8),
                       torch.zeros(2, 8)[:, ::2]):
        with pytest.raises(ValueError, match="calibrate_rerank"):
            ops.calibrate_rerank(idx, val, class_of, bad_target, 2, 0.5, out)
    assert ops.calibrate_rerank.__doc__.count("RELEVANCE") == 1 and "Steck" in ops.calibrate_rerank.__doc__

    ptr, items, shares = torch.zeros(3, dtype=torch.int64), torch.zeros(5, dtype=torch.int32), torch.zeros(2, 4)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.class_shares(ptr, items, class_of, 4, shares)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.class_shares(ptr.tolist(), items, class_of, 4, shares)
    for C in (0, 17, 2.5, True):
        with pytest.raises(ValueError, match="class_shares"):
            ops.class_shares(ptr, items, class_of, C, shares)
    for bad_ptr, bad_items in ((ptr.int(), items), (ptr, items.long()), (ptr.reshape(1, 3), items), (torch.zeros(0, dtype=torch.int64), items),
                               (ptr, items.reshape(1, 5))):
        with pytest.raises(ValueError, match="class_shares"):
            ops.class_shares(bad_ptr, bad_items, class_of, 4, shares)
    with pytest.raises(ValueError, match="class_shares"):
        ops.class_shares(ptr, items, class_of.long(), 4, shares)

    lists, kl = torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.list_calibration(lists, class_of, 4, shares)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.list_calibration(lists, class_of, 4, shares, target=target, out_kl=kl)
    for bad in (lists.long(), lists.reshape(-1), torch.zeros(2, 0, dtype=torch.int32), torch.zeros(2, 6, dtype=torch.int32)[:, ::2]):
        with pytest.raises(ValueError, match="list_calibration"):
            ops.list_calibration(bad, class_of, 4, shares)
    for C in (0, 17):
        with pytest.raises(ValueError, match="list_calibration"):
            ops.list_calibration(lists, class_of, C, shares)
    with pytest.raises(ValueError, match="go together"):
        ops.list_calibration(lists, class_of, 4, shares, target=target)
    with pytest.raises(ValueError, match="go together"):
        ops.list_calibration(lists, class_of, 4, shares, out_kl=kl)
    for bad_target, bad_kl, smooth in ((torch.zeros(2, 5), kl, 0.01), (torch.zeros(3, 4), kl, 0.01), (target, torch.zeros(1), 0.01),
                                       (target, kl.double(), 0.01), (target, kl, 0.0), (target, kl, float("nan"))):
        with pytest.raises(ValueError, match="list_calibration"):
            ops.list_calibration(lists, class_of, 4, shares, target=bad_target, smooth=smooth, out_kl=bad_kl)


def test_item_classes_and_columns():
    from elimrec_amd.evaluator import assign_item_groups, calibration_columns, item_classes
    counts = np.asarray([0, 1, 2, 5, 5, 40, 0, 3])
    class_of, names = item_classes(8, counts, [1, 4])
    labels, positions = assign_item_groups(np.arange(8), counts, [1, 4])
    assert names == labels == [x.ljust(12) for x in ("cold:", "(0,1]:", "(1,4]:", "(4,inf):")]
    assert class_of.dtype == np.int32 and class_of.tolist() == [0, 1, 2, 3, 3, 3, 0, 2]
    for c, at in enumerate(positions):
        assert (class_of[at] == c).all()
    class_of, names = item_classes(8, counts, [100])                          # empty buckets are no classes
    assert [n.strip() for n in names] == ["cold:", "(0,100]:"] and class_of.tolist() == [0, 1, 1, 1, 1, 1, 0, 1]
    sub, sub_names = item_classes([5, 0, 3], counts, [1, 4])
    assert sub.tolist() == [1, 0, 1] and [n.strip() for n in sub_names] == ["cold:", "(4,inf):"]
    with pytest.raises(ValueError, match="16"):
        item_classes(40, np.arange(40), list(range(1, 30)))
    with pytest.raises(TypeError):
        item_classes(8, counts, None)
    with pytest.raises(ValueError):
        item_classes(8, counts, [4, 1])
    assert calibration_columns(names) == ("lambda", "recall", "ndcg", "ckl", "pop", "overlap", "share_cold", "share_(0,100]", "coverage",
                                          "gini", "entropy")
    assert calibration_columns(()) == ("lambda", "recall", "ndcg", "ckl", "pop", "overlap", "coverage", "gini", "entropy")


def test_calibration_report_checks():
    from elimrec_amd import ops
    from elimrec_amd.evaluator import CalibrationReport
    ds = types.SimpleNamespace(num_items=6, num_users=3)
    train = {0: [1, 2], 1: [2], 2: []}
    test = {0: [3], 2: [4, 5]}
    for bad in (0, 1, -1, 7, ops.LIST_MAX_K + 1, 2.5, True, None):
        with pytest.raises(ValueError):
            CalibrationReport(ds, train, test, bad, [1])
    for k, pool in ((3, 2), (3, 7), (2, 2.0), (2, True)):
        with pytest.raises(ValueError):
            CalibrationReport(ds, train, test, k, [1], pool=pool)
    for lambdas in ([], [1.1], [0.5, -0.1], "0.5", [0.5, "x"], 0.5, [True], [float("nan")]):
        with pytest.raises(ValueError):
            CalibrationReport(ds, train, test, 2, [1], lambdas=lambdas)
    for smooth in (0.0, 1.0, -0.1, float("nan"), "x", True):
        with pytest.raises(ValueError):
            CalibrationReport(ds, train, test, 2, [1], smooth=smooth)
    with pytest.raises((TypeError, ValueError)):
        CalibrationReport(ds, train, test, 2, [1], group_view=[3, 3])
    with pytest.raises(TypeError):
        CalibrationReport(ds, [1, 2], test, 2, [1])
    with pytest.raises(TypeError):
        CalibrationReport(ds, train, test, 2, None)
    with pytest.raises(ValueError):
        CalibrationReport(ds, train, test, 2, [2, 1])
    big = types.SimpleNamespace(num_items=5000, num_users=3)
    with pytest.raises(ValueError, match="16"):
        CalibrationReport(big, {0: [i for i in range(40) for _ in range(i)]}, test, 2, list(range(1, 30)))
    rep = CalibrationReport(ds, train, test, 2, [1], group_view=[1])
    assert (rep.top_k, rep.pool, rep.lambdas, rep.smooth) == (2, 6, (1.0, 0.9, 0.7, 0.5), 0.01)
    assert rep.users == [0, 2] and rep.name == "calibrate" and rep.needs == "predict_device" and rep.item_counts.tolist() == [0, 1, 2, 0, 0, 0]
    assert rep.class_of.tolist() == [0, 1, 2, 0, 0, 0] and [n.strip() for n in rep.class_names] == ["cold:", "(0,1]:", "(1,inf):"]
    assert rep.num_classes == 3 and rep.columns[6:9] == ("share_cold", "share_(0,1]", "share_(1,inf)") and len(rep.columns) == 12
    assert rep.group_labels[0].strip() == "all:" and len(rep.group_labels) >= 2
    rep = CalibrationReport(ds, train, test, 3, [1], pool=5, lambdas=(1, 0.25), smooth=0.1)
    assert (rep.top_k, rep.pool, rep.lambdas, rep.smooth) == (3, 5, (1.0, 0.25), 0.1)
    assert CalibrationReport(big, train, test, 10, [1]).pool == 40 and CalibrationReport(big, train, test, 100, [1]).pool == 256
    with pytest.raises(TypeError):
        rep.evaluate(object())


def test_basic_model_switches_and_recommend_calibrated_checks():
    from elimrec_amd import ops
    g = load_golden("ml3")
    model, _ = build_model_from_fixture(g, "cpu")
    assert model.calibrate_reporter is None
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--calibrate_report=0", "--calibrate_pool=1"])
    assert model.calibrate_reporter is None
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--calibrate_report=3", "--item_group_view=[2,4]", "--group_view=[2,4]"])
    rep = model.calibrate_reporter
    assert (rep.top_k, rep.pool, rep.lambdas) == (3, min(12, model.num_items), (1.0, 0.9, 0.7, 0.5)) and len(rep.group_labels) >= 2
    assert 2 <= rep.num_classes <= 4 and rep.class_of.shape == (model.num_items,)
    view = ["--item_group_view=[2,4]"]
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=view + ["--calibrate_report=3", "--calibrate_pool=5", "--calibrate_lambda=[1.0,0.3]"])
    rep = model.calibrate_reporter
    assert (rep.top_k, rep.pool, rep.lambdas) == (3, 5, (1.0, 0.3)) and rep.num_items == model.num_items
    with pytest.raises(ValueError, match="item_group_view"):
        build_model_from_fixture(g, "cpu", extra_argv=["--calibrate_report=3"])
    for bad in (["--calibrate_report=1"], ["--calibrate_report=-2"], ["--calibrate_report=%d" % (model.num_items + 1)],
                ["--calibrate_report=3", "--calibrate_pool=2"], ["--calibrate_report=3", "--calibrate_pool=%d" % (model.num_items + 1)],
                ["--calibrate_report=3", "--calibrate_pool=%d" % (ops.LIST_MAX_K + 1)], ["--calibrate_report=3", "--calibrate_lambda=[1.2]"],
                ["--calibrate_report=3", "--calibrate_lambda=[]"], ["--calibrate_report=3", "--calibrate_lambda=0.5"]):
        with pytest.raises(ValueError):
            build_model_from_fixture(g, "cpu", extra_argv=view + bad)
    classes = rep.class_of
    I = model.num_items
    for kw in (dict(k=0), dict(k=3, pool=2), dict(k=3, pool=I + 1), dict(k=3, lam=1.5), dict(k=3, lam=-0.5), dict(k=3, lam=float("nan")),
               dict(k=3, smooth=0.0), dict(k=3, smooth=1.0), dict(k=3, smooth=float("nan")), dict(k=3, classes=classes[:-1]),
               dict(k=3, classes=classes.astype(np.float32)), dict(k=3, classes=classes - 1), dict(k=3, classes=classes + 16),
               dict(k=3, classes=classes.reshape(1, -1)), dict(k=3, targets=np.zeros((3, rep.num_classes))),
               dict(k=3, targets=np.zeros((2, 17))), dict(k=3, targets=np.zeros(2)), dict(k=3, targets=np.zeros((2, 1)), classes=classes * 0 + 1)):
        a = dict(classes=classes)
        a.update(kw)
        with pytest.raises(ValueError):
            model.recommend_calibrated([0, 1], **a)
    with pytest.raises(IndexError):
        model.recommend_calibrated([0], 3, classes, exclude={0: [I]})
    with pytest.raises(RuntimeError, match="no CPU fallback|There is no CPU"):
        model.recommend_calibrated([0, 1], 3, classes)
    with pytest.raises(RuntimeError, match="no CPU fallback|There is no CPU"):
        model.calibrate_device(torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 4), 2, 0.5, torch.from_numpy(classes), torch.zeros(1, 3))
    for fn in (model.calibrate_device, model.recommend_calibrated):
        assert "RELEVANCE" in fn.__doc__ and "Steck" in fn.__doc__


def test_main_refuses_the_switch_on_several_ranks():
    import inspect
    import main
    src = inspect.getsource(main.Net.__init__)
    assert "--calibrate_report needs the whole cached item table on one rank: it is single-GPU" in src
