"""The spherical k-means kernels on the device (csrc/kmeans.hip) against the float64 model of tests/kmeans_model.py, and what is
built on them: ops.spherical_kmeans, EliMRec.clusters_device / cluster_items / cluster_users, evaluator.ClusterReport,
--cluster_report.

Tolerances are derived, not measured. A cosine: knn_model.tol(d) = 2 (d + 8) 2^-24 (derived there); the assignment must equal the
model's wherever the model's margin between the best and the second-best cosine exceeds it (tests/test_kmeans_cpu.py shows that
this holds for at least 99 % of the rows of every case). The update: a unit row's component x * (1 / max(sqrt(sq), 1e-12)) is
formed in fp32 from sq rounded once (0.5 u relative, a quarter of it after the root), a root, a division and a product of half an
ulp each: below 3 u = 3 * 2^-24 in absolute value since the component is at most 1; the float64 sum of count_c such terms adds
nothing visible, so a sum's component is within 4 u count_c of the model's, and a centroid's within 4 u count_c / |sum_c| plus the
one rounding to fp32 (2^-24 for a component of at most 1)."""
import numpy as np
import pytest
import torch

import kmeans_cases as kc
import kmeans_model as km

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _sq(T):
    """Squared norms rounded once to fp32."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(T, dtype=np.float64) ** 2).sum(1).astype(np.float32)


def _table(T, form="plain"):
    """T [n x d] on the device: plain, as a column slice of a wider NaN table, with a row stride that is no multiple of 4 (no
    vector load), or at a base pointer that is not 16-byte aligned."""
    n, d = T.shape
    if form == "plain":
        return _t(T)
    if form == "slice":
        wide = np.full((n + 2, d + 12), np.nan, dtype=np.float32)
        wide[1:1 + n, 8:8 + d] = T
        view = _t(wide)[1:1 + n, 8:8 + d]
    elif form == "stride":
        wide = np.full((n, d + 3), np.nan, dtype=np.float32)
        wide[:, :d] = T
        view = _t(wide)[:, :d]
        assert view.stride(0) % 4 != 0 or n == 1
    else:
        flat = np.full(n * d + 1, np.nan, dtype=np.float32)
        flat[1:] = T.reshape(-1)
        view = _t(flat)[1:].view(n, d)
        assert view.data_ptr() % 16 != 0
    assert view.stride(1) == 1
    return view


def _assign(T, Cen, prev=None, form="plain", sq=None, csq=None):
    """One launch with canaries round the outputs -> (assign, cos, changed)."""
    from elimrec_amd import ops
    n = T.shape[0]
    sq = _sq(T) if sq is None else sq
    sq_wide = _t(np.stack([np.full(n, np.nan, dtype=np.float32), sq], 1))[:, 1]          # any stride
    out_a = torch.full((n + 2,), 77, dtype=torch.int32, device=DEV)
    out_c = torch.full((n + 2,), 7.0, dtype=torch.float32, device=DEV)
    changed = ops.kmeans_assign(_table(T, form), sq_wide if n > 1 else _t(sq), _t(Cen), _t(_sq(Cen) if csq is None else csq),
                                out_a[1:1 + n], out_c[1:1 + n], prev=None if prev is None else _t(prev.astype(np.int32)))
    a, c = out_a.cpu().numpy(), out_c.cpu().numpy()
    assert a[0] == a[-1] == 77 and c[0] == c[-1] == 7.0
    return a[1:-1], c[1:-1], changed


def _check_assign(T, Cen, a, c):
    d = T.shape[1]
    want_a, want_c, margin = km.assign64(T, Cen)
    clear = margin > km.tol(d)
    assert (a[clear] == want_a[clear]).all()
    listed = want_a >= 0
    assert ((a >= 0) == listed).all() and (c[~listed] == -np.inf).all()
    # the device's pick, scored by the model, stands within the tolerance of the best
    err = np.abs(c[listed].astype(np.float64) - want_c[listed])
    print("assign n %d d %d C %d: max |cos - cos64| %.3g (bound %.3g), clear %.4f" % (T.shape[0], d, Cen.shape[0],
                                                                                    err.max() if err.size else 0.0, km.tol(d), clear.mean()))
    assert (err <= km.tol(d)).all()


@pytest.mark.parametrize("case", kc.ASSIGN_CASES, ids=kc.case_id)
def test_assign_against_model(case):
    T, Cen = kc.gaussian(*case)
    a, c, changed = _assign(T, Cen)
    _check_assign(T, Cen, a, c)
    assert changed == T.shape[0]                                   # without prev every row counts


@pytest.mark.parametrize("form", ["slice", "stride", "unaligned"])
@pytest.mark.parametrize("case", [(65, 64, 33), (130, 68, 17)], ids=kc.case_id)
def test_assign_table_forms(case, form):
    T, Cen = kc.gaussian(*case, seed=1)
    plain = _assign(T, Cen)
    a, c, _ = _assign(T, Cen, form=form)
    _check_assign(T, Cen, a, c)
    assert a.tobytes() == plain[0].tobytes() and c.tobytes() == plain[1].tobytes()        # the load form changes no bit


def test_exact_ties():
    T, Cen = kc.gaussian(150, 64, 40, seed=2)
    Cen[33] = Cen[5]                                               # two identical centroids, in different LDS stages
    Cen[17] = Cen[16]                                              # ... and in one MFMA tile
    a, c, _ = _assign(T, Cen)
    assert not np.isin(a, (33, 17)).any() and np.isin(a, (5, 16)).any()
    only = np.repeat(Cen[5:6], 2, 0)
    assert (_assign(T, only)[0] == 0).all()
    # centroids taken from table rows (row 3 twice): cosine 1, the row's own centroid or the lowest-id duplicate of it
    rows = np.asarray([70, 3, 149, 3, 0, 64], dtype=np.int64)
    a, c, _ = _assign(T, T[rows].copy())
    assert a[rows].tolist() == [0, 1, 2, 1, 4, 5]
    assert (np.abs(c[rows].astype(np.float64) - 1.0) <= km.tol(64)).all()
    _check_assign(T, T[rows].copy(), a, c)


def test_rows_and_centroids_without_a_norm():
    T, Cen = kc.gaussian(70, 8, 20, seed=3)
    T[0] = 0.0
    T[17, 3] = np.nan
    T[64, 0] = np.inf
    T[69] = 0.0
    Cen[0] = 0.0
    Cen[19, 1] = np.nan
    Cen[7] = np.inf
    a, c, changed = _assign(T, Cen)
    gone = [0, 17, 64, 69]
    assert (a[gone] == -1).all() and (c[gone] == -np.inf).all() and changed == 70
    keep = np.setdiff1d(np.arange(70), gone)
    assert (a[keep] >= 0).all() and not np.isin(a, (0, 7, 19)).any() and np.isfinite(c[keep]).all()
    _check_assign(T, Cen, a, c)
    # no usable centroid at all
    a, c, _ = _assign(T, Cen[[0, 19, 7]].copy())
    assert (a == -1).all() and (c == -np.inf).all()


def test_prev_and_changed():
    T, Cen = kc.gaussian(333, 64, 17, seed=4)
    a, _, changed = _assign(T, Cen)
    assert changed == 333
    assert _assign(T, Cen, prev=a)[2] == 0
    prev = a.copy()
    prev[::7] = (prev[::7] + 1) % 17
    prev[5] = -1
    got = _assign(T, Cen, prev=prev)
    assert got[2] == int((got[0] != prev).sum()) == int((a != prev).sum()) and got[0].tobytes() == a.tobytes()


def test_independence_of_n_place_and_grid():
    for d, C in ((64, 256), (68, 33)):
        T, Cen = kc.gaussian(1000, d, C)
        a, c, _ = _assign(T, Cen)
        rows = np.arange(37, 37 + 130)
        sa, sc, _ = _assign(T[rows].copy(), Cen)                   # a subset alone: other tiles, another grid
        assert sa.tobytes() == a[rows].tobytes() and sc.tobytes() == c[rows].tobytes()
        ra, rc, _ = _assign(T[::-1].copy(), Cen)                   # the rows reversed
        assert ra[::-1].tobytes() == a.tobytes() and rc[::-1].tobytes() == c.tobytes()
        pad = np.concatenate([T[900:941], T, T[:5]])               # padded to another n: every row at another place in its tile
        pa, pc, _ = _assign(pad, Cen)
        assert pa[41:1041].tobytes() == a.tobytes() and pc[41:1041].tobytes() == c.tobytes()
        assert pa[:41].tobytes() == a[900:941].tobytes()           # equal rows, equal results


def _update(T, assign, Cen, form="plain", with_outputs=True):
    from elimrec_amd import ops
    C, d = Cen.shape
    cen, csq = _t(Cen.copy()), _t(_sq(Cen))
    sums = torch.full((C, d), 7.0, dtype=torch.float64, device=DEV) if with_outputs else None
    counts = torch.full((C,), 77, dtype=torch.int32, device=DEV) if with_outputs else None
    out = ops.kmeans_update(_table(T, form), _t(_sq(T)), _t(assign.astype(np.int32)), cen, csq, out_sums=sums, out_counts=counts)
    assert out is cen
    return (cen.cpu().numpy(), csq.cpu().numpy(), sums.cpu().numpy() if with_outputs else None,
            counts.cpu().numpy() if with_outputs else None)


def _check_update(T, assign, Cen, got):
    C, d = Cen.shape
    cen, csq, sums, counts = got
    want_sums, want_counts, want_cen = km.update64(T, assign, Cen, C)
    assert counts.tolist() == want_counts.tolist()
    bound = 4 * U * np.maximum(want_counts, 0)[:, None]
    err = np.abs(sums - want_sums)
    assert (err <= bound).all(), float((err - bound).max())
    norm = np.sqrt((want_sums ** 2).sum(1))
    moved = (want_counts > 0) & (norm > 0)
    cerr = np.abs(cen[moved].astype(np.float64) - want_cen[moved])
    cbound = (4 * U * want_counts[moved] / norm[moved] + U)[:, None]
    print("update n %d d %d C %d: sums err/bound %.3g, centroids err/bound %.3g" % (
        T.shape[0], d, C, float((err / np.maximum(bound, 1e-300)).max()), float((cerr / cbound).max()) if cerr.size else 0.0))
    assert (cerr <= cbound).all()
    assert cen[~moved].tobytes() == Cen[~moved].tobytes() and csq[~moved].tobytes() == _sq(Cen)[~moved].tobytes()    # kept bit for bit
    want_sq = (cen[moved].astype(np.float64) ** 2).sum(1)
    assert np.abs(csq[moved] - want_sq).max(initial=0.0) <= U + 1e-12      # the rounded centroid's squared norm (below 2), rounded once


@pytest.mark.parametrize("case", kc.UPDATE_CASES, ids=kc.case_id)
def test_update_against_model(case):
    n, d, C = case
    T, Cen = kc.gaussian(n, d, C, seed=5)
    assign = kc.random_assign(n, C)
    assign[n // 2] = -1                                            # skipped, never dereferenced
    assign[n // 3] = C
    assign[n - 1] = 2 ** 31 - 1
    if C > 2:
        assign[assign == C - 2] = 0                                # an empty cluster keeps its centroid
    got = _update(T, assign, Cen)
    _check_update(T, assign, Cen, got)
    again = _update(T, assign, Cen, form="stride")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again))                    # two runs: identical bits
    bare = _update(T, assign, Cen, with_outputs=False)
    assert bare[0].tobytes() == got[0].tobytes() and bare[1].tobytes() == got[1].tobytes()


def test_update_one_cluster_and_one_row_per_cluster():
    T, Cen = kc.gaussian(1100, 64, 16, seed=6)
    T[7] = 0.0                                                     # a row without a norm belongs to no cluster
    T[600, 2] = np.nan
    assign = np.full(1100, 3, dtype=np.int32)                      # all rows in one cluster
    got = _update(T, assign, Cen)
    _check_update(T, assign, Cen, got)
    assert got[3][3] == 1098 and got[3].sum() == 1098
    T, Cen = kc.gaussian(256, 64, 256, seed=6)
    assign = np.random.default_rng(0).permutation(256).astype(np.int32)          # one row per cluster
    got = _update(T, assign, Cen)
    _check_update(T, assign, Cen, got)
    unit = T.astype(np.float64) / np.sqrt((T.astype(np.float64) ** 2).sum(1))[:, None]
    assert np.abs(got[0][assign] - unit).max() <= 6 * U            # a single row's centroid is its unit row: 4 u / (1 - 3 u) + u


def _lloyd(T, init, iters, C=None, seed=2022):
    from elimrec_amd import ops
    return ops.spherical_kmeans(_t(T), _t(_sq(T)), len(init) if init is not None else C, iters=iters, seed=seed, init=init)


def test_lloyd_follows_the_model():
    T, init, truth = kc.planted()
    want = km.lloyd64(T, init, 25)
    got = _lloyd(T, init, 25)
    assert got.n_iter == want["n_iter"] and got.converged == want["converged"] is True
    assert got.assign.cpu().tolist() == want["assign"].tolist() and got.counts.cpu().tolist() == want["counts"].tolist()
    assert abs(got.cohesion - want["cohesion"]) <= km.tol(T.shape[1])
    sums, counts, cen = km.update64(T, want["assign"], T[init], len(init))          # equal assignments: the update's own bound
    bound = (4 * U * counts / np.sqrt((sums ** 2).sum(1)) + U)[:, None]
    assert (np.abs(got.centroids.cpu().numpy() - cen) <= bound).all()
    assert got.assign.dtype == torch.int32 and got.cos.dtype == got.centroids.dtype == torch.float32 and got.assign.is_cuda
    # iteration for iteration; the cohesion does not decrease
    last = -np.inf
    for it in range(1, want["n_iter"] + 1):
        step = _lloyd(T, init, it)
        assert step.n_iter == it and step.assign.cpu().tolist() == want["trail"][it - 1][0].tolist()
        assert step.converged == (it == want["n_iter"])
        assert step.cohesion >= last - km.tol(T.shape[1])
        last = step.cohesion
    # iters = 1: the first iteration's assignment and the centroids of its update
    first = _lloyd(T, init, 1)
    a1, c1, _ = _assign(T, T[init].copy())
    assert first.assign.cpu().numpy().tobytes() == a1.tobytes() and first.cos.cpu().numpy().tobytes() == c1.tobytes()
    cen1 = _update(T, a1, T[init].copy(), with_outputs=False)[0]
    assert first.centroids.cpu().numpy().tobytes() == cen1.tobytes() and not first.converged
    # the planted groups come back: every cluster lies in one group (the duplicated direction is one group, shared by two clusters)
    fold = np.where(truth == len(init) - 1, 0, truth)
    a = got.assign.cpu().numpy()
    assert all(len(set(fold[a == c].tolist())) == 1 for c in range(len(init)) if (a == c).any())


def test_lloyd_default_init_and_determinism():
    T, _ = kc.gaussian(700, 64, 1, seed=8)
    T[11] = 0.0
    one = _lloyd(T, None, 4, C=9, seed=5)
    two = _lloyd(T, None, 4, C=9, seed=5)
    for x, y in zip(one[:4], two[:4]):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    assert one[4:] == two[4:] and one.assign[11].item() == -1 and int(one.counts.sum()) == 699
    want = km.lloyd64(T, km.default_init(T, 9, 5), 1)
    clear = want["trail"][0][2] > km.tol(64)
    assert (_lloyd(T, None, 1, C=9, seed=5).assign.cpu().numpy()[clear] == want["assign"][clear]).all() and clear.mean() >= 0.99
    with pytest.raises(ValueError):
        _lloyd(np.zeros((5, 8), dtype=np.float32), None, 3, C=2)                          # fewer usable rows than clusters


def test_torch_ops_are_the_same_launches():
    from elimrec_amd import torch_ops
    t = torch_ops.load()
    T, Cen = kc.gaussian(130, 68, 17, seed=9)
    a, c, changed = _assign(T, Cen)
    ta, tc, tch = t.kmeans_assign(_t(T), _t(_sq(T)), _t(Cen), _t(_sq(Cen)), None)
    assert ta.cpu().numpy().tobytes() == a.tobytes() and tc.cpu().numpy().tobytes() == c.tobytes() and int(tch.item()) == changed
    assert int(t.kmeans_assign(_t(T), _t(_sq(T)), _t(Cen), _t(_sq(Cen)), ta)[2].item()) == 0
    cen, csq, sums, counts = _update(T, a, Cen)
    before = _t(Cen)
    got = t.kmeans_update(_t(T), _t(_sq(T)), ta, before, _t(_sq(Cen)))
    assert before.cpu().numpy().tobytes() == Cen.tobytes()                              # the op is functional
    for x, y in zip(got, (cen, csq, sums, counts)):
        assert x.cpu().numpy().tobytes() == y.tobytes()


# ---- the model and the report
def _forward(name, extra=()):
    from helpers import build_model_from_fixture, load_golden
    g = load_golden(name)
    model, _ = build_model_from_fixture(g, DEV, extra_argv=extra)
    model.bpr_loss(_t(g["step1/users"]), _t(g["step1/pos"]), _t(g["step1/neg"]))
    return model


def test_cluster_items_and_users():
    from helpers import build_model_from_fixture, load_golden
    from elimrec_amd import ops
    from elimrec_amd.evaluator import CandidateScoringError
    from elimrec_amd.model import Clusters, classes_from_clusters
    fresh, _ = build_model_from_fixture(load_golden("ml3"), DEV)
    with pytest.raises(RuntimeError):
        fresh.cluster_items(3)
    model = _forward("ml3")
    U_, I, d = model.num_users, model.num_items, model.latent_dim
    C = min(4, I)
    sqn = model._block_sqnorms(model._cached_tables("the test needs"))       # the pending forward made real, then the block norms
    for h, space in enumerate(("fused",) + tuple(model._mods)):
        got = model.cluster_items(C, space=space, iters=6, seed=7)
        assert isinstance(got, Clusters) and got.assign.device.type == got.cos.device.type == got.centroids.device.type == "cpu"
        assert tuple(got.assign.shape) == (I,) and got.assign.dtype == torch.int32 and tuple(got.centroids.shape) == (C, d)
        want = ops.spherical_kmeans(model._ws["Y"][U_:U_ + I, h * d:(h + 1) * d], sqn[U_:U_ + I, h], C, iters=6, seed=7)
        assert torch.equal(got.assign, want.assign.cpu()) and got.cos.numpy().tobytes() == want.cos.cpu().numpy().tobytes()
        assert got.centroids.numpy().tobytes() == want.centroids.cpu().numpy().tobytes()
        assert torch.equal(got.counts, want.counts.cpu()) and (got.n_iter, got.converged) == (want.n_iter, want.converged)
    users = model.cluster_users(min(3, U_), iters=3)
    assert tuple(users.assign.shape) == (U_,) and int(users.counts.sum()) == int((users.assign >= 0).sum())
    # the assignment as the classes of recommend_calibrated
    got = model.cluster_items(C, iters=6, seed=7)
    classes = classes_from_clusters(got.assign, C)
    assert classes.dtype == np.int32 and classes.min() >= 0 and classes.max() <= C
    assert (classes[got.assign.numpy() < 0] == C).all() and (classes[got.assign.numpy() >= 0] == got.assign.numpy()[got.assign.numpy() >= 0]).all()
    ids, scores, kl = model.recommend_calibrated(list(range(min(U_, 8))), 3, classes, pool=min(8, I))
    assert tuple(ids.shape) == (min(U_, 8), 3) and np.isfinite(kl.numpy()).all()
    model._eval_shard = object()
    try:
        with pytest.raises(CandidateScoringError):
            model.cluster_items(C)
    finally:
        model._eval_shard = None


@pytest.mark.parametrize("view", [None, [2, 4]])
def test_cluster_report(view):
    import lists_model as lm
    from elimrec_amd.evaluator import ClusterReport, ClusterTables, cluster_rows, cluster_user_rows
    model = _forward("ml3")
    train, test = model.dataset.get_user_train_dict(), model.dataset.get_user_test_dict()
    K, I = 4, model.num_items
    C = min(3, I)
    report = ClusterReport(model.dataset, train, test, K, n_clusters=C, iters=5, group_view=view)
    report.block_users = (len(report.users) + 1) // 2              # two user blocks
    model.predict_type = "TIE"
    final, buf = report.evaluate(model)
    assert isinstance(final, ClusterTables)
    clusters = report.clusters(model)
    assert clusters is report.clusters(model)                      # once per table version
    want = model.cluster_items(C, iters=5)
    assert torch.equal(clusters.assign.cpu(), want.assign)
    rows, lists, counts = report.cluster_lists(model)
    lists_h = lists.cpu().numpy()
    assign, cos = want.assign.numpy(), want.cos.numpy()
    exposure = lm.exposure(lists_h, I)
    assert counts.cpu().tolist() == exposure.tolist()
    test_counts = np.bincount(np.asarray([i for u in report.users for i in set(test[u])], dtype=np.int64), minlength=I)
    got_rows = cluster_rows(assign, cos, report.item_counts, test_counts, exposure, C)
    assert np.allclose(got_rows, km.cluster_rows_loops(assign, cos, report.item_counts, test_counts, exposure, C), rtol=1e-12, atol=0, equal_nan=True)
    assert final.clusters.tobytes() == got_rows.tobytes()
    assert got_rows[:, 0].sum() == (assign >= 0).sum() and abs(got_rows[:, 5].sum() - float((assign[lists_h[lists_h >= 0]] >= 0).mean())) < 1e-12
    # the user rows: distinct clusters in a list, ckl against the user's own training mix over the clusters (+ the class of no cluster)
    classes = report.classes(model).cpu().numpy()
    n_cls = report.num_classes
    cnt = np.stack([np.bincount(classes[np.asarray(train.get(u, []), dtype=np.int64)].clip(-1) + 1, minlength=n_cls + 1)[1:]
                    for u in report.users])
    with np.errstate(invalid="ignore", divide="ignore"):
        targets = np.where(cnt.sum(1, keepdims=True) > 0, cnt.astype(np.float32) / cnt.sum(1, keepdims=True).astype(np.float32),
                           np.float32(0)).astype(np.float32)
    want_users = cluster_user_rows(lists_h, classes, n_cls, targets, report.smooth)
    rows_h = rows.cpu().numpy()
    assert rows_h[:, 0].tolist() == want_users[:, 0].tolist()
    assert np.abs(rows_h[:, 1].astype(np.float64) - want_users[:, 1]).max() <= 2.0 ** -22
    G = len(report.group_labels)
    assert final.users.shape == (G, 2) and (G > 1) == (view is not None)
    for g in range(G):
        assert np.allclose(final.users[g], rows_h[report._positions[g]].astype(np.float64).mean(0), rtol=1e-6, atol=1e-6)
    lines = buf.split("\n")
    assert lines[0].startswith("columns:") and all(c in lines[0] for c in ("size", "pop", "cohesion", "train_share", "test_share", "slot_share"))
    assert sum(ln.startswith("cluster") for ln in lines) == C and any("distinct" in ln and "ckl" in ln for ln in lines)
    assert report.evaluate(model)[1] == buf
    # TE -> TIE
    model.predict_type = "TE"
    te = report.evaluate(model)[0]
    shift, sbuf = report.shift(te, final)
    assert np.allclose(shift.clusters[:, 0], final.clusters[:, 5] - te.clusters[:, 5]) and np.allclose(shift.users, final.users - te.users)
    assert "d_slot_share" in sbuf and "d_distinct" in sbuf and "d_ckl" in sbuf


def test_driver_switch(tmp_path):
    from test_lists_gpu import _driver
    view = ["--group_view=[10,30]", "--list_report=5"]
    off, ev0, te0 = _driver(tmp_path / "a", view)
    assert not any("content clusters" in ln for ln in off)
    on, ev1, te1 = _driver(tmp_path / "b", view + ["--cluster_report=5", "--cluster_count=3"])
    added = [k for k, ln in enumerate(on) if "content clusters" in ln]
    assert len(added) == 3 and [ln for k, ln in enumerate(on) if k not in added] == off      # with the switch off: the log as it was
    assert on[added[0]].startswith("  [TE]") and on[added[1]].startswith("  [TIE]") and on[added[2]].startswith("  [TE->TIE]")
    for k in added[:2]:
        assert all(c in on[k] for c in ("size", "pop", "cohesion", "train_share", "test_share", "slot_share", "distinct", "ckl"))
        assert on[k].count("\ncluster") == 3
    assert all(c in on[added[2]] for c in ("d_slot_share", "d_distinct", "d_ckl"))
    assert ev0.tobytes() == ev1.tobytes() and te0.tobytes() == te1.tobytes()
