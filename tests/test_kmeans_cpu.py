"""Spherical k-means, host side (no GPU): the float64 model of tests/kmeans_model.py on a hand-worked example and against its
plain-loops form, the bindings of csrc/kmeans.hip, the argument checks of the C entry points, the ops wrappers,
EliMRec.cluster_items / cluster_users, ClusterReport and the --cluster_* switches that run before anything touches the device -- and
the model's own statement about the device test's inputs: nearly every row of every case is clear."""
import math
import types

import numpy as np
import pytest
import torch

import kmeans_cases as kc
import kmeans_model as km
from helpers import build_model_from_fixture, load_golden


def test_bindings_are_present():
    from elimrec_amd import _lib, ops, torch_ops
    lib = _lib.load()
    for name in ("elimrec_kmeans_assign", "elimrec_kmeans_update", "elimrec_kmeans_max_clusters", "elimrec_kmeans_segment",
                 "elimrec_kmeans_workspace"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    ns = torch_ops.load()
    for name in ("kmeans_assign", "kmeans_update"):
        assert hasattr(ns, name) and name in torch_ops.OPS
    assert ops.KMEANS_MAX_CLUSTERS == lib.elimrec_kmeans_max_clusters() == 256
    seg = ops.KMEANS_SEGMENT
    assert seg == lib.elimrec_kmeans_segment() and seg >= 64
    assert lib.elimrec_abi_version() == 2
    # the workspace: per segment a [C x d] float64 partial and C int32 counts, rounded up to 16 bytes
    for n, d, C in ((1, 4, 1), (seg, 64, 16), (seg + 1, 64, 16), (76085, 64, 256)):
        segs = -(-n // seg)
        assert ops.kmeans_workspace(n, d, C) == -(-(segs * C * d * 8 + segs * C * 4) // 16) * 16
    assert ops.kmeans_workspace(0, 64, 16) == 0
    for n, d, C in ((-1, 64, 16), (10, 2, 16), (10, 260, 16), (10, 64, 0), (10, 64, 257)):
        assert ops.kmeans_workspace(n, d, C) == 0


def test_c_entry_points_refuse_bad_arguments_before_any_launch():
    from elimrec_amd import _lib
    lib = _lib.load()
    one = 8                                                        # any non-null address: nothing is launched, nothing dereferenced
    for kw in (dict(C=0), dict(C=257), dict(d=6), dict(d=260), dict(d=0), dict(n=-1), dict(ld=60), dict(ld_sq=0), dict(T=None),
               dict(sq=None), dict(cen=None), dict(csq=None), dict(out=None), dict(changed=None), dict(n=2 ** 31)):
        a = dict(T=one, ld=64, n=100, d=64, sq=one, ld_sq=1, cen=one, csq=one, C=16, out=one, changed=one)
        a.update(kw)
        rc = lib.elimrec_kmeans_assign(a["T"], a["ld"], a["n"], a["d"], a["sq"], a["ld_sq"], a["cen"], a["csq"], a["C"], None, a["out"],
                                       None, a["changed"], None)
        assert rc == 10001 and b"kmeans_assign" in lib.elimrec_last_error(), (kw, rc)            # ELIMREC_E_BADARG
    assert lib.elimrec_kmeans_assign(None, 64, 0, 64, None, 1, None, None, 16, None, None, None, None, None) == 0        # n == 0
    for kw in (dict(C=0), dict(C=257), dict(d=6), dict(d=260), dict(n=-1), dict(ld=60), dict(ld_sq=0), dict(T=None), dict(sq=None),
               dict(cen=None), dict(csq=None), dict(assign=None), dict(ws=None), dict(ws_bytes=16), dict(ws=one + 4)):
        a = dict(T=one, ld=64, n=100, d=64, sq=one, ld_sq=1, assign=one, C=16, cen=one, csq=one, ws=16, ws_bytes=1 << 20)
        a.update(kw)
        rc = lib.elimrec_kmeans_update(a["T"], a["ld"], a["n"], a["d"], a["sq"], a["ld_sq"], a["assign"], a["C"], a["cen"], a["csq"],
                                       None, None, a["ws"], a["ws_bytes"], None)
        assert rc == 10001 and b"kmeans_update" in lib.elimrec_last_error(), (kw, rc)
    assert lib.elimrec_kmeans_update(None, 64, 0, 64, None, 1, None, 16, None, None, None, None, None, 0, None) == 0


def test_hand_worked_example():
    """Four rows, two centroids (1, 0, 0, 0) and (0, 1, 0, 0). Row 0 = (2, 0, 0, 0): cosines 1, 0 -> 0. Row 1 = (3, 3, 0, 0): cosines
    1/sqrt 2 twice, an exact tie -> the lower id, 0. Row 2 = 0: no norm -> -1 / -inf. Row 3 = (4, 0, 3, 0): cosines 0.8, 0 -> 0.
    Cluster 1 is empty and keeps its centroid; cluster 0 sums the unit rows (1, 0, 0, 0) + (1, 1, 0, 0) / sqrt 2 + (0.8, 0, 0.6, 0)."""
    T = np.asarray([[2, 0, 0, 0], [3, 3, 0, 0], [0, 0, 0, 0], [4, 0, 3, 0]], dtype=np.float32)
    Cen = np.asarray([[1, 0, 0, 0], [0, 1, 0, 0]], dtype=np.float32)
    r = 1.0 / math.sqrt(2.0)
    for fn in (km.assign64, km.assign64_loops):
        assign, cos, margin = fn(T, Cen)
        assert assign.tolist() == [0, 0, -1, 0]
        assert cos[2] == -np.inf and np.allclose(cos[[0, 1, 3]], [1.0, r, 0.8], rtol=0, atol=1e-15)
        assert margin[1] == 0.0 and margin[2] == np.inf and abs(margin[0] - 1.0) < 1e-15 and abs(margin[3] - 0.8) < 1e-15
    for fn in (km.update64, km.update64_loops):
        sums, counts, cen = fn(T, [0, 0, -1, 0], Cen, 2)
        assert counts.tolist() == [3, 0]
        want = np.asarray([1.0 + r + 0.8, r, 0.6, 0.0])
        assert np.allclose(sums[0], want, rtol=0, atol=1e-15) and (sums[1] == 0).all()
        assert np.allclose(cen[0], want / math.sqrt((want ** 2).sum()), rtol=0, atol=1e-15)
        assert cen[1].tolist() == [0.0, 1.0, 0.0, 0.0]             # the empty cluster keeps its centroid
    # a member row without a norm adds nothing; assignments outside [0, C) belong nowhere
    sums, counts, _ = km.update64(T, [0, 5, 0, -3], Cen, 2)
    assert counts.tolist() == [1, 0] and sums[0].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert km.assign64(T, Cen[:1])[2].tolist() == [np.inf] * 4      # C = 1: no second best


def test_model_against_its_loops():
    rng = np.random.default_rng(0)
    for n, d, C in ((9, 4, 1), (20, 8, 5), (33, 12, 7)):
        T, Cen = rng.standard_normal((n, d)), rng.standard_normal((C, d))
        T[n // 2] = 0.0
        T[1, 0] = np.nan
        Cen[C - 1] = 0.0
        if C > 3:
            Cen[3] = Cen[1]
        a, c, m = km.assign64(T, Cen)
        la, lc, lm = km.assign64_loops(T, Cen)
        assert a.tolist() == la.tolist() and np.allclose(c, lc, rtol=0, atol=1e-14) and np.allclose(m, lm, rtol=0, atol=1e-14)
        assert a[n // 2] == a[1] == -1 and (a != C - 1).all() and (C <= 3 or (a != 3).all())
        assign = rng.integers(-1, C + 1, n)
        s, k, cen = km.update64(T, assign, Cen, C)
        ls, lk, lcen = km.update64_loops(T, assign, Cen, C)
        assert k.tolist() == lk.tolist() and np.allclose(s, ls, rtol=0, atol=1e-13) and np.allclose(cen, lcen, rtol=0, atol=1e-13)


def test_the_device_tests_inputs_are_clear():
    """A condition on the inputs of tests/test_kmeans_gpu.py, not a measurement: at least 99 % of the rows of every case have a
    margin above the cosine tolerance, and Lloyd's loop on the planted case has every margin clear along its whole trajectory."""
    for case in kc.ASSIGN_CASES:
        T, Cen = kc.gaussian(*case)
        margin = km.assign64(T, Cen)[2]
        assert (margin > km.tol(case[1])).mean() >= 0.99, case
    for case, seed in (((65, 64, 33), 1), ((130, 68, 17), 1), ((333, 64, 17), 4), ((130, 68, 17), 9)):
        T, Cen = kc.gaussian(*case, seed=seed)
        assert (km.assign64(T, Cen)[2] > km.tol(case[1])).mean() >= 0.99, case
    T, init, truth = kc.planted()
    run = km.lloyd64(T, init, 25)
    assert run["converged"] and 2 <= run["n_iter"] < 25
    for assign, cos, margin, _ in run["trail"]:
        assert (margin > km.tol(T.shape[1])).all() and (assign >= 0).all()
    cohesion = [t[3] for t in run["trail"]]
    assert all(b >= a for a, b in zip(cohesion, cohesion[1:]))
    assert run["counts"].sum() == T.shape[0] and len(set(init.tolist())) == len(init) and truth[init].tolist() == list(range(len(init)))
    again = km.lloyd64(T, init, 1)
    assert again["n_iter"] == 1 and not again["converged"] and again["assign"].tolist() == run["trail"][0][0].tolist()


def test_ops_argument_errors_need_no_device():
    from elimrec_amd import ops
    T, sq = torch.zeros(10, 8), torch.ones(10)
    cen, csq = torch.zeros(3, 8), torch.ones(3)
    out = torch.zeros(10, dtype=torch.int32)
    for call in (lambda: ops.kmeans_assign(T, sq, cen, csq, out), lambda: ops.kmeans_update(T, sq, out, cen, csq),
                 lambda: ops.spherical_kmeans(T, sq, 3), lambda: ops.kmeans_assign(None, sq, cen, csq, out)):
        with pytest.raises(RuntimeError, match="HIP device tensor"):
            call()
    for C, iters in ((0, 5), (257, 5), (-1, 5), (2.5, 5), (True, 5), (3, 0), (3, -1), (3, 1.5), (3, None)):
        with pytest.raises(ValueError, match="spherical_kmeans"):
            ops.spherical_kmeans(T, sq, C, iters=iters)
    assert "PREDECESSORS" in ops.spherical_kmeans.__doc__ and "IN PLACE" in ops.kmeans_update.__doc__
    assert ops.KMeans._fields == ("assign", "cos", "centroids", "counts", "n_iter", "converged", "cohesion")


def test_cluster_rows_against_loops():
    from elimrec_amd.evaluator import CLUSTER_COLUMNS, CLUSTER_USER_COLUMNS, cluster_rows, cluster_user_rows
    assert CLUSTER_COLUMNS == ("size", "pop", "cohesion", "train_share", "test_share", "slot_share")
    assert CLUSTER_USER_COLUMNS == ("distinct", "ckl")
    rng = np.random.default_rng(1)
    I, C = 40, 5
    assign = rng.integers(-1, C - 1, I)                            # the last cluster is empty, some items have none
    cos = rng.uniform(-1, 1, I)
    train, test, seen = rng.integers(0, 9, I), rng.integers(0, 3, I), rng.integers(0, 6, I)
    got = cluster_rows(assign, cos, train, test, seen, C)
    assert np.allclose(got, km.cluster_rows_loops(assign, cos, train, test, seen, C), rtol=1e-13, atol=0, equal_nan=True)
    assert got[C - 1, 0] == 0 and np.isnan(got[C - 1, 1:3]).all() and (got[C - 1, 3:] == 0).all()
    assert got[:, 0].sum() == (assign >= 0).sum() and got[:, 3].sum() < 1.0
    assert (cluster_rows(assign, cos, train * 0, test * 0, seen * 0, C)[:, 3:] == 0).all()
    # hand-checked user rows: clusters 0 0 1 -1; the list (0, 2, 3, -1) holds clusters 0 and 1 once each (item 3 has none)
    classes = np.asarray([0, 0, 1, -1])
    rows = cluster_user_rows([[0, 2, 3, -1], [-1, -1, -1, -1]], classes, 2, [[0.5, 0.5], [1.0, 0.0]], smooth=0.01)
    assert rows[0].tolist() == [2.0, 0.0]                          # q = p: q~ = p, C_KL = 0
    assert rows[1, 0] == 0.0 and abs(rows[1, 1] - math.log(100.0)) < 1e-12      # nothing listed: q = 0, q~ = 0.01 p


def test_cluster_report_checks():
    from elimrec_amd import ops
    from elimrec_amd.evaluator import ClusterReport
    ds = types.SimpleNamespace(num_items=6, num_users=3)
    train = {0: [1, 2], 1: [2], 2: []}
    test = {0: [3], 2: [4, 5, 5]}
    for bad in (0, -1, ops.LIST_MAX_K + 1, 2.5, True, None):
        with pytest.raises(ValueError):
            ClusterReport(ds, train, test, bad)
    for kw in (dict(n_clusters=1), dict(n_clusters=17), dict(n_clusters=0), dict(n_clusters=2.0), dict(n_clusters=True), dict(iters=0),
               dict(iters=2.5), dict(space=""), dict(space=3), dict(seed=1.5), dict(smooth=0.0), dict(smooth=1.0), dict(smooth="x")):
        with pytest.raises(ValueError):
            ClusterReport(ds, train, test, 2, **kw)
    with pytest.raises((TypeError, ValueError)):
        ClusterReport(ds, train, test, 2, group_view=[3, 3])
    with pytest.raises(TypeError):
        ClusterReport(ds, [1, 2], test, 2)
    rep = ClusterReport(ds, train, test, 2, group_view=[1])
    assert (rep.top_k, rep.num_classes, rep.space, rep.iters, rep.seed, rep.smooth) == (2, 8, "fused", 25, 2022, 0.01)
    assert rep.users == [0, 2] and rep.name == "cluster" and rep.needs == "clusters_device"
    assert rep.item_counts.tolist() == [0, 1, 2, 0, 0, 0] and rep.test_counts.tolist() == [0, 0, 0, 1, 1, 1]
    assert [x.strip() for x in rep.cluster_labels] == ["cluster %d:" % c for c in range(8)]
    assert rep.group_labels[0].strip() == "all:" and len(rep.group_labels) >= 2
    with pytest.raises(TypeError):
        rep.evaluate(object())
    with pytest.raises(ValueError):
        rep.shift(None, None)


def test_basic_model_switches_and_cluster_items_checks():
    g = load_golden("ml3")
    model, _ = build_model_from_fixture(g, "cpu")
    assert model.cluster_reporter is None
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--cluster_report=0", "--cluster_count=99"])
    assert model.cluster_reporter is None
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--cluster_report=3", "--group_view=[2,4]"])
    rep = model.cluster_reporter
    assert (rep.top_k, rep.num_classes, rep.space) == (3, 8, "fused") and len(rep.group_labels) >= 2
    head = model._mods[0]
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--cluster_report=4", "--cluster_count=3", "--cluster_space=" + head])
    rep = model.cluster_reporter
    assert (rep.top_k, rep.num_classes, rep.space, rep.num_items) == (4, 3, head, model.num_items)
    for bad in (["--cluster_report=-2"], ["--cluster_report=3", "--cluster_count=1"], ["--cluster_report=3", "--cluster_count=17"]):
        with pytest.raises(ValueError):
            build_model_from_fixture(g, "cpu", extra_argv=bad)
    for kw in (dict(n_clusters=0), dict(n_clusters=257), dict(n_clusters=2.5), dict(n_clusters=True), dict(n_clusters=3, iters=0),
               dict(n_clusters=3, space="nope"), dict(n_clusters=3, space=None)):
        for fn in (model.cluster_items, model.cluster_users):
            with pytest.raises(ValueError):
                fn(**kw)
    with pytest.raises(ValueError):
        model.clusters_device("row", 3)
    with pytest.raises(RuntimeError, match="no CPU fallback|There is no CPU"):
        model.cluster_items(3)
    assert "classes_from_clusters" in model.cluster_items.__doc__ and "recommend_calibrated" in model.cluster_items.__doc__
    from elimrec_amd.model import classes_from_clusters
    assert classes_from_clusters(np.asarray([2, -1, 0]), 3).tolist() == [2, 3, 0]
    assert classes_from_clusters(torch.tensor([1, 0], dtype=torch.int32), 2).dtype == np.int32


def test_main_refuses_the_switch_on_several_ranks():
    import inspect
    import main
    src = inspect.getsource(main.Net.__init__)
    assert "--cluster_report needs the whole cached item table on one rank: it is single-GPU" in src
