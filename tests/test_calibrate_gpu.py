"""The calibrated re-ranking kernel and the class-share kernel on the device (csrc/calibrate.hip) against the float64 model of
tests/calibrate_model.py, and what is built on them: EliMRec.calibrate_device / recommend_calibrated, evaluator.CalibrationReport,
--calibrate_report.

TOL = 1e-12 bounds how far the kernel's float64 objective may stand from the model's; it is a bound, not a measurement. An
objective is lam * rel - (1 - lam) * KL. rel and lam * rel are the same IEEE operations on the same fp32 scores in both. KL is a
sum of at most C = 16 terms p log(p / q~): per term two products and a sum for q~, a division, a log (within an ulp in either
library) and a product, then C - 1 additions, one product and one subtraction -- at most C + 3 float64 operations and C logs on
values of magnitude below 8 (KL <= log(1 / smooth) = log 100 < 8). Each is off by at most 2^-53 relatively (2^-52 for a log), so
an objective is off by the order of 16 * 8 * 2^-52 ~ 3e-14 on either side, well inside TOL:
  * the kernel's pick can fall short of the step's float64 maximum by at most TOL;
  * where the float64 margin to the best candidate not tied to the pick by construction (calibrate_model: same class -- or both
    without a target share -- and the same lam * rel) exceeds TOL, the kernel must make the float64 pick;
  * out_val is that objective rounded once to fp32: a value in [-log(1 / smooth), 1], below 8 in magnitude, so half an fp32 ulp
    is at most 2^-22.
tests/test_calibrate_cpu.py checks on the host that at least 99 % of the lists of every shape are clear at every step.
The targets are a strided column block of a NaN matrix and class_of has guard entries of a valid class in front of and behind it:
a read outside shows up as a target of 0 or as a listed position that should not be."""
import functools

import numpy as np
import pytest
import torch

import calibrate_cases as cc
import calibrate_model as cm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY_I, CANARY_F = 77, 7.0
SMOOTH, TOL = cc.SMOOTH, cc.TOL
HALF_ULP = 2.0 ** -22


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _guarded_classes(class_of):
    """class_of [n] as a view into a longer tensor whose entries in front of and behind it hold class 0."""
    wide = np.zeros(len(class_of) + 6, dtype=np.int32)
    wide[3:3 + len(class_of)] = class_of
    return _t(wide)[3:3 + len(class_of)]


def _strided_targets(targets):
    """targets [B x C] as a column block of a wider NaN matrix."""
    B, C = targets.shape
    wide = np.full((B + 2, C + 5), np.nan, dtype=np.float32)
    wide[1:1 + B, 2:2 + C] = targets
    view = _t(wide)[1:1 + B, 2:2 + C]
    assert view.stride(0) == C + 5 and view.storage_offset() > 0
    return view


def _run(ids, vals, class_of, targets, K, lam, smooth=SMOOTH):
    """One launch with canaries in front of and behind the [B x K] outputs -> (idx, pos, val) numpy [B x K]."""
    from elimrec_amd import ops
    ids, vals = np.ascontiguousarray(ids, dtype=np.int32), np.ascontiguousarray(vals, dtype=np.float32)
    B = ids.shape[0]
    flat = [torch.full(((B + 3) * K,), c, dtype=dt, device=DEV)
            for c, dt in ((CANARY_I, torch.int32), (CANARY_I, torch.int32), (CANARY_F, torch.float32))]
    views = [f[K:] for f in flat]
    ops.calibrate_rerank(_t(ids).reshape(B, -1), _t(vals).reshape(B, -1), _guarded_classes(class_of),
                         _strided_targets(np.asarray(targets, dtype=np.float32)), K, lam, views[0], views[1], views[2], smooth=smooth)
    torch.cuda.synchronize()
    out = []
    for f, c in zip(flat, (CANARY_I, CANARY_I, CANARY_F)):
        a = f.cpu().numpy()
        assert (a[:K] == c).all() and (a[(B + 1) * K:] == c).all(), "entries outside [B x K] were written"
        out.append(a[K:(B + 1) * K].reshape(B, K))
    return out


def _verify(P, ids, got, K, lam, what, want=None):
    """The certificate and the clear prefix of one launch against the float64 model -> bool [B]: the lists whose every float64
    step is clear (margin > TOL)."""
    idx, pos, val = got
    B, N = ids.shape
    n_listed = P.mask.sum(1)
    filled = pos >= 0
    assert (filled.sum(1) == np.minimum(K, n_listed)).all(), (what, "number of picks")
    assert (filled[:, :-1] >= filled[:, 1:]).all(), (what, "a filler in front of a pick")
    assert (idx[~filled] == -1).all() and (pos[~filled] == -1).all() and np.isneginf(val[~filled]).all(), (what, "fillers")
    assert (pos[filled] < N).all()
    assert (idx[filled] == np.take_along_axis(ids, np.maximum(pos, 0), 1)[filled]).all(), (what, "out_pos does not index out_idx's id")
    objs, bests, ok = P.replay(pos, lam)
    assert ok.all(), (what, "a pick that is unlisted or was picked before")
    short = float((bests - objs)[filled].max()) if filled.any() else 0.0
    off = float(np.abs(val.astype(np.float64) - objs)[filled].max()) if filled.any() else 0.0
    picks, _, margins = P.greedy(K, lam) if want is None else want
    unclear = margins <= TOL
    first = np.where(unclear.any(1), unclear.argmax(1), K)
    prefix = np.arange(K)[None, :] < first[:, None]
    print("calibrate_rerank %s: pick below the float64 maximum by <= %.3e (bound %.1e), |out_val - float64| <= %.3e (bound %.3e), "
          "%d of %d lists with an unclear step" % (what, short, TOL, off, HALF_ULP, int(unclear.any(1).sum()), B))
    assert short <= TOL, (what, short, TOL)
    assert off <= HALF_ULP, (what, off, HALF_ULP)
    assert (pos[prefix] == picks[prefix]).all(), (what, "the list differs from the float64 greedy list before its first unclear step")
    return ~unclear.any(1)


@pytest.mark.parametrize("shape", cc.SHAPES, ids=lambda s: "N%d_K%d_C%d" % s)
def test_certificate_and_clear_prefix(shape):
    N, K, C = shape
    ids, vals, class_of, targets = cc.case(N, K, C)
    P = cc.pools(N, K, C)
    for lam in cc.LAMBDAS:
        got = _run(ids, vals, class_of, targets, K, lam)
        clear = _verify(P, ids, got, K, lam, (N, K, C, lam), want=cc.greedy(N, K, C, lam))
        assert clear.mean() >= 0.99                                          # (the host test's statement about these inputs)
        if lam == 1.0 or C == 1:                                             # bit for bit the pool's order
            idx, pos, val = got
            assert (pos == np.arange(K)[None, :]).all() and (idx == ids[:, :K]).all()
            lo, hi = vals[:, -1:].astype(np.float64), vals[:, :1].astype(np.float64)
            if lam == 1.0 and N > 1:
                assert val.tobytes() == ((vals[:, :K].astype(np.float64) - lo) / (hi - lo)).astype(np.float32).tobytes()


def test_exact_cases():
    N, K, C = 100, 10, 5
    ids, vals, class_of, targets = (np.array(a[:40]) if a.shape[0] == cc.LISTS else np.array(a) for a in cc.case(N, K, C))
    targets[3] = 0.0                                                         # a zero target row: the pool's order at any lambda
    targets[4] = (np.nan, -1.0, np.inf, 0.0, -0.0)                           # ... and one whose every entry counts as 0
    vals[5, 10:30] = vals[5, 10]                                             # equal scores: within a class the lower position
    vals[6] = 0.5                                                            # all scores equal: rel = 0
    P = cm.Pools64(ids, vals, class_of, targets, SMOOTH)
    for lam in (0.0, 0.3, 1.0):
        idx, pos, val = got = _run(ids, vals, class_of, targets, K, lam)
        _verify(P, ids, got, K, lam, ("exact", lam))
        for b in (3, 4):
            assert (pos[b] == np.arange(K)).all() and (idx[b] == ids[b, :K]).all()
        want = P.greedy(K, lam)[0]
        assert (pos[5] == want[5]).all() and (pos[6] == want[6]).all()       # ties within a class: exact in any arithmetic
        cls = class_of[ids[6]]
        for c in range(C):                                                   # all scores equal: every class in position order
            mine = pos[6][cls[pos[6]] == c]
            assert (np.diff(mine) > 0).all()
    # a row alone, in a batch of one and at another place in the batch: identical bits
    batch = _run(ids, vals, class_of, targets, K, 0.3)
    alone = _run(ids[17:18], vals[17:18], class_of, targets[17:18], K, 0.3)
    order = np.r_[np.arange(20, 40), np.arange(0, 20)]
    moved = _run(ids[order], vals[order], class_of, targets[order], K, 0.3)
    for a, m, b in zip(alone, moved, batch):
        assert a[0].tobytes() == b[17].tobytes() == m[37].tobytes()
    # four waves, K = N and C at its limit
    N, K, C = 256, 256, 16
    ids, vals, class_of, targets = cc.case(N, K, C)
    batch = _run(ids[:30], vals[:30], class_of, targets[:30], K, 0.7)
    alone = _run(ids[29:30], vals[29:30], class_of, targets[29:30], K, 0.7)
    for a, b in zip(alone, batch):
        assert a[0].tobytes() == b[29].tobytes()


@pytest.mark.parametrize("shape", ((17, 5, 3), (100, 10, 5), (256, 12, 16)), ids=lambda s: "N%d_K%d_C%d" % s)
def test_malformed_batch(shape):
    N, K, C = shape
    ids, vals, class_of, targets = (np.array(a[:9]) if a.shape[0] == cc.LISTS else np.array(a) for a in cc.case(N, K, C))
    I = cc.ITEMS
    ids[0, [3, 5, 6]] = (-1, I, 2 ** 31 - 1)                                 # ids outside the catalogue in the middle of a pool
    vals[0, [2, 4, 7, 8]] = (np.nan, np.inf, -np.inf, np.nan)                # scores that are not finite
    ids[1, 3:] = -1                                                          # fewer listed entries than K
    vals[1, 1] = np.nan                                                      # (two are left)
    class_of[ids[2, 1]], class_of[ids[2, 2]] = -1, C                         # classes outside [0, C)
    ids[3, 2], ids[3, 6] = ids[3, 0], ids[3, 1]                              # duplicate ids
    ids[4] = -7                                                              # nothing listed
    ids[5, 0] = I + 1                                                        # (behind class_of's guard entries)
    targets[6] = 0.0
    targets[6, :2] = (-0.5, np.nan)                                          # negative / NaN target entries: a row of zeros
    gone = int(class_of[ids[7, 0]])                                          # a class that is absent from the pool but wanted
    for k in range(N):
        if class_of[ids[7, k]] == gone:
            ids[7, k] = -1
    targets[7] = 0.0
    targets[7, gone] = 1.0
    P = cm.Pools64(ids, vals, class_of, targets, SMOOTH)
    assert P.mask[1].sum() == 2 and P.mask[4].sum() == 0 and not P.mask[5, 0] and P.mask[0].sum() <= N - 7
    assert not P.mask[2, 1] and not P.mask[2, 2] and P.mask[6].sum() >= K and P.mask[7].sum() >= K
    for lam in cc.LAMBDAS:
        idx, pos, val = got = _run(ids, vals, class_of, targets, K, lam)
        _verify(P, ids, got, K, lam, (shape, "malformed", lam))
        assert sorted(pos[1, :2].tolist()) == [0, 2] and (pos[1, 2:] == -1).all() and (pos[4] == -1).all() and np.isneginf(val[4]).all()
        assert (pos[6] == np.flatnonzero(P.mask[6])[:K]).all() and (pos[7] == np.flatnonzero(P.mask[7])[:K]).all()
        if lam == 1.0:                                                       # the pool order over the listed positions
            for b in range(9):
                order = np.flatnonzero(P.mask[b])[:K]
                assert (pos[b, :order.size] == order).all(), (b, pos[b], order)


def test_class_shares_and_list_calibration():
    from elimrec_amd import ops, torch_ops
    rng = np.random.default_rng(5)
    I, C, B = 500, 7, 41
    class_of = rng.integers(0, C, I).astype(np.int32)
    class_of[[3, 4]] = (-1, C)
    lens = rng.integers(0, 200, B)
    lens[[0, 7, B - 1]] = 0                                                  # empty segments, the last one too
    lens[[2, 5, 9, 11]] = (10, 64, 20, 5)
    segs = [rng.integers(0, I, n).astype(np.int32) for n in lens]
    segs[2][:4] = (-1, I, 3, 4)                                              # skipped entries
    segs[9][:] = 10                                                          # a repeated id counts each time
    segs[11][:] = 3                                                          # listed ids, no listed class: zeros
    ptr = np.cumsum([0] + [len(s) for s in segs]).astype(np.int64)
    flat = np.concatenate(segs).astype(np.int32)
    cls = _guarded_classes(class_of)
    out = torch.full((B + 2, C), CANARY_F, device=DEV)
    ops.class_shares(_t(ptr), _t(flat), cls, C, out[1:].reshape(-1))
    want = cm.class_shares(segs, class_of, C)
    got = out.cpu().numpy()
    assert (got[0] == CANARY_F).all() and (got[B + 1:] == CANARY_F).all()
    assert got[1:B + 1].tobytes() == want.tobytes()
    assert (want[[0, 7, 11, B - 1]] == 0).all() and want[9].max() == 1.0
    bad_ptr = ptr.copy()
    bad_ptr[0], bad_ptr[-1] = -5, len(flat) + 100                            # a segment never leaves the items it is given
    out2 = torch.empty(B, C, device=DEV)
    ops.class_shares(_t(bad_ptr), _t(flat), cls, C, out2)
    assert out2.cpu().numpy()[1:B - 1].tobytes() == want[1:B - 1].tobytes()
    # the list form, with and without the miscalibration
    for K in (1, 10, 64, 65, 200):
        lists = rng.integers(-1, I + 1, (B, K)).astype(np.int32)
        lists[1] = -1
        targets = rng.dirichlet(np.ones(C), B).astype(np.float32)
        targets[rng.uniform(size=(B, C)) < 0.2] = 0.0
        targets[2] = 0.0
        targets[3, :2] = (np.nan, -1.0)
        shares = torch.full((B + 1, C), CANARY_F, device=DEV)
        ops.list_calibration(_t(lists), cls, C, shares)
        want = cm.class_shares(lists, class_of, C)
        assert shares[:B].cpu().numpy().tobytes() == want.tobytes() and (shares[B] == CANARY_F).all()
        kl = torch.full((B + 1,), CANARY_F, device=DEV)
        shares2 = torch.empty(B, C, device=DEV)
        ops.list_calibration(_t(lists), cls, C, shares2, target=_strided_targets(targets), smooth=SMOOTH, out_kl=kl)
        assert torch.equal(shares2, shares[:B]) and float(kl[B]) == CANARY_F
        want_kl = cm.list_kl(lists, class_of, C, targets, SMOOTH)
        err = np.abs(kl[:B].cpu().numpy().astype(np.float64) - want_kl).max()
        print("list_calibration K %d: |kl - float64| <= %.3e (bound %.3e)" % (K, err, HALF_ULP))
        assert err <= HALF_ULP and kl[2] == 0.0
        t_shares, t_kl = torch_ops.load().list_calibration(_t(lists), cls, C, _strided_targets(targets), SMOOTH)
        assert torch.equal(t_shares, shares2) and t_kl.cpu().numpy().tobytes() == kl[:B].cpu().numpy().tobytes()


def test_empty_batch_and_torch_op():
    from elimrec_amd import ops, torch_ops
    ids, vals, class_of, targets = cc.case(37, 37, 2)
    cls = _guarded_classes(class_of)
    idx = torch.full((2, 5), CANARY_I, dtype=torch.int32, device=DEV)
    ops.calibrate_rerank(torch.zeros(0, 9, dtype=torch.int32, device=DEV), torch.zeros(0, 9, device=DEV), cls,
                         torch.zeros(0, 2, device=DEV), 5, 0.5, idx)
    torch.cuda.synchronize()
    assert (idx == CANARY_I).all()
    want = _run(ids[:6], vals[:6], class_of, targets[:6], 9, 0.6, smooth=0.05)
    got = torch_ops.load().calibrate_rerank(_t(ids[:6]), _t(vals[:6]), cls, _strided_targets(targets[:6]), 9, 0.6, 0.05)
    assert [tuple(g.shape) for g in got] == [(6, 9)] * 3
    for g, w in zip(got, want):
        assert g.cpu().numpy().tobytes() == w.tobytes()
    with pytest.raises(RuntimeError):
        torch_ops.load().calibrate_rerank(_t(ids[:6]), _t(vals[:6]), cls, _t(targets[:6]), 38, 0.6, 0.05)
    with pytest.raises(RuntimeError):
        torch_ops.load().calibrate_rerank(_t(ids[:6]), _t(vals[:6]), cls, _t(targets[:6]), 9, 0.6, 0.0)


# --------------------------------------------------------------------------- the model and the report on the fixtures
def _forward(name, extra=()):
    from helpers import build_model_from_fixture, load_golden
    g = load_golden(name)
    model, _ = build_model_from_fixture(g, DEV, extra_argv=extra)
    model.bpr_loss(_t(g["step1/users"]), _t(g["step1/pos"]), _t(g["step1/neg"]))
    return model


def _train_csr(train, users):
    tl = [train.get(u, []) for u in users]
    return _t(np.cumsum([0] + [len(x) for x in tl]).astype(np.int64)), _t(np.asarray([i for x in tl for i in x], dtype=np.int32))


def _classes(model, view):
    from elimrec_amd.evaluator import item_classes
    from elimrec_amd.reports import item_train_counts
    return item_classes(model.num_items, item_train_counts(model.dataset.get_user_train_dict(), model.num_items), view)


def test_recommend_calibrated():
    from helpers import build_model_from_fixture, load_golden
    from elimrec_amd.evaluator import CandidateScoringError
    fresh, _ = build_model_from_fixture(load_golden("ml3"), DEV)
    classes, names = _classes(fresh, [2, 4])
    C = len(names)
    with pytest.raises(RuntimeError):
        fresh.recommend_calibrated([0, 1], 3, classes)
    model = _forward("ml3")
    I, k = model.num_items, 4
    pool = min(12, I)
    users = list(range(min(model.num_users, 24)))
    train = model.dataset.get_user_train_dict()
    exclude = {u: train.get(u, []) for u in users}
    tptr, titems = _train_csr(train, users)
    pidx, pval = [x.cpu().numpy() for x in model.predict_device(users, top_k=pool, train_ptr=tptr, train_items=titems)]
    ids, scores, kl = model.recommend_calibrated(users, k, classes, pool=pool, lam=1.0, exclude=exclude)
    assert ids.dtype == torch.int32 and scores.dtype == kl.dtype == torch.float32 and tuple(kl.shape) == (len(users),)
    assert ids.device.type == scores.device.type == kl.device.type == "cpu"
    top, top_val = model.predict_device(users, top_k=k, train_ptr=tptr, train_items=titems)
    assert torch.equal(ids, top.cpu()) and scores.numpy().tobytes() == top_val.cpu().numpy().tobytes()   # lam = 1: the plain top-k
    # the default targets: the class shares of the users' training items; the model composition at lam = 0.5
    want_t = cm.class_shares([train.get(u, []) for u in users], classes, C)
    P = cm.Pools64(pidx, pval, classes, want_t, 0.01)
    for lam, targets in ((0.5, None), (0.0, None), (0.5, np.roll(want_t, 1, axis=1))):
        ids, scores, kl = [x.numpy() for x in model.recommend_calibrated(users, k, classes, pool=pool, lam=lam, targets=targets,
                                                                        exclude=exclude)]
        Pm = P if targets is None else cm.Pools64(pidx, pval, classes, targets, 0.01)
        pos = np.asarray([[pidx[b].tolist().index(i) if i >= 0 else -1 for i in ids[b]] for b in range(len(users))])
        objs, bests, ok = Pm.replay(pos, lam)
        assert ok.all() and ((bests - objs)[pos >= 0] <= TOL).all()             # every pick is the step's float64 maximum
        picks, _, margins = Pm.greedy(k, lam)
        clear = (margins > TOL).all(1)
        want_ids = np.where(picks >= 0, np.take_along_axis(pidx, np.maximum(picks, 0), 1), -1)
        assert (ids[clear] == want_ids[clear]).all() and ((pos >= 0).sum(1) == (picks >= 0).sum(1)).all()
        for b, u in enumerate(users):
            got = ids[b][ids[b] >= 0]
            assert got.size == min(k, int((pidx[b] >= 0).sum())) and len(set(got.tolist())) == got.size
            assert set(got.tolist()) <= set(pidx[b].tolist()) and not set(got.tolist()) & set(exclude[u])
            at = [pidx[b].tolist().index(i) for i in got]
            assert scores[b][:got.size].tobytes() == pval[b][at].tobytes()      # the model's scores of the picked items
        want_kl = cm.list_kl(ids, classes, C, want_t if targets is None else targets, 0.01)
        assert np.abs(kl.astype(np.float64) - want_kl).max() <= HALF_ULP
    assert tuple(model.recommend_calibrated(users, k, classes)[0].shape) == (len(users), k)  # the default pool
    empty = model.recommend_calibrated([], k, classes)
    assert [tuple(x.shape) for x in empty] == [(0, k), (0, k), (0,)]
    model._eval_shard = object()
    try:
        with pytest.raises(CandidateScoringError):
            model.recommend_calibrated(users, k, classes)
    finally:
        model._eval_shard = None


@pytest.mark.parametrize("view", [None, [2, 4]])
def test_calibration_report(view):
    import lists_model as lm
    from elimrec_amd import ops
    from elimrec_amd.evaluator import (CalibrationReport, CalibrationTables, CandidateScoringError, ListReport, calibration_columns,
                                       exposure_summary, group_table)
    model = _forward("ml3")
    train, test = model.dataset.get_user_train_dict(), model.dataset.get_user_test_dict()
    K, I = 4, model.num_items
    pool, lambdas = min(12, I), (1.0, 0.3)
    report = CalibrationReport(model.dataset, train, test, K, [2, 4], pool=pool, lambdas=lambdas, group_view=view)
    plain = ListReport(model.dataset, train, test, K, group_view=view)
    report.block_users = plain.block_users = (len(report.users) + 1) // 2       # two user blocks
    model.predict_type = "TIE"
    final, buf = report.evaluate(model)
    rows, lists, counts = report.calibrate_rows(model)
    L, G, n, C = len(lambdas), len(report.group_labels), len(report.users), report.num_classes
    assert isinstance(final, CalibrationTables) and final.columns == calibration_columns(report.class_names) == report.columns
    assert final.table.shape == (G * L, 9 + C) and C >= 2
    assert final.labels == [g for g in report.group_labels for _ in lambdas] and (G > 1) == (view is not None)
    assert tuple(rows.shape) == (L, n, 5 + C) and tuple(lists.shape) == (L, n, K) and tuple(counts.shape) == (L, I)
    assert final.table[:, 0].tolist() == list(lambdas) * G
    # lambda = 1: the plain lists and their numbers
    tptr, titems = _train_csr(train, report.users)
    users_t = _t(np.asarray(report.users, dtype=np.int64))
    top = model.predict_device(users_t, top_k=K, train_ptr=tptr, train_items=titems)[0]
    assert torch.equal(lists[0], top)
    truth = [sorted(set(test[u])) for u in report.users]
    met = torch.empty(n, 2, K, dtype=torch.float32, device=DEV)
    ops.rank_metrics(top, _t(np.cumsum([0] + [len(x) for x in truth]).astype(np.int64)),
                     _t(np.asarray([i for x in truth for i in x], dtype=np.int32)), (2, 4), met)
    want = group_table(met[:, :, K - 1].contiguous(), report._resident(rows.device)["groups"], G)
    list_final = plain.evaluate(model)[0]
    # ckl and the shares: the numpy model on the lists the report returns, against the targets of the users' training items
    targets = cm.class_shares([train.get(u, []) for u in report.users], report.class_of, C)
    assert report.targets(rows.device).cpu().numpy().tobytes() == targets.tobytes()
    lists_h, rows_h = lists.cpu().numpy(), rows.cpu().numpy()
    for li in range(L):
        assert rows_h[li, :, 5:].tobytes() == cm.class_shares(lists_h[li], report.class_of, C).tobytes()
        assert np.abs(rows_h[li, :, 2].astype(np.float64) - cm.list_kl(lists_h[li], report.class_of, C, targets, report.smooth)).max() <= HALF_ULP
    for g in range(G):
        row = final.table[g * L]
        assert row[1:3].tolist() == want[g].astype(np.float64).tolist(), ("recall / ndcg", g)
        assert row[4] == float(list_final.users[g, -1]) and row[5] == 1.0, ("pop / overlap", g)
        at = report._positions[g]
        for li in range(L):
            mean = rows_h[li][at].astype(np.float64).mean(0)
            assert np.allclose(final.table[g * L + li, 1:6 + C], mean, rtol=1e-6, atol=1e-6)
        print("calibrate %s ckl: lambda 1 %.6f, lambda 0.3 %.6f" % (report.group_labels[g].strip(), row[3], final.table[g * L + 1, 3]))
        assert g or final.table[1, 3] < row[3], "ckl at lambda 0.3 is not below lambda 1 over all test users"
        assert 0.0 < final.table[g * L + 1, 5] <= 1.0
    every = [np.arange(I)]
    for li in range(L):
        assert counts[li].cpu().tolist() == lm.exposure(lists_h[li], I).tolist()
        assert final.table[li, 6 + C:].tolist() == exposure_summary(lm.exposure(lists_h[li], I), every)[0, 1:4].tolist()
        for g in range(1, G):
            own = lm.exposure(lists_h[li][report._positions[g]], I)
            assert final.table[g * L + li, 6 + C:].tolist() == exposure_summary(own, every)[0, 1:4].tolist()
    assert final.table[0, 6 + C:].tolist() == list_final.items[0, 1:4].tolist()     # ListReport's coverage / gini / entropy
    lines = buf.split("\n")
    assert len(lines) == 2 + G * L and lines[0].startswith("columns:") and all(c in lines[0] for c in final.columns)
    assert [ln[:12] for ln in lines[1:-1]] == [x[:12] for x in final.labels]
    assert lines[-1].startswith("target:") and len(lines[-1].split("\t")) == 1 + C
    assert [float(x) for x in lines[-1].split("\t")[1:]] == [float("%.8f" % x) for x in targets.astype(np.float64).mean(0)]
    assert report.evaluate(model, (rows, lists, counts))[1] == buf
    model._eval_shard = object()
    try:
        with pytest.raises(CandidateScoringError):
            report.evaluate(model)
    finally:
        model._eval_shard = None


def test_driver_switch(tmp_path):
    from test_lists_gpu import _driver
    view = ["--group_view=[10,30]", "--item_group_view=[1,4]", "--list_report=5"]
    off, ev0, te0 = _driver(tmp_path / "a", view)
    assert not any("calibrated" in ln for ln in off)
    on, ev1, te1 = _driver(tmp_path / "b", view + ["--calibrate_report=5", "--calibrate_lambda=[1.0,0.5]"])
    head = " top-5 of the top-20 pools calibrated to the users' popularity mix, per lambda:\n"
    added = [k for k, ln in enumerate(on) if ln.startswith("  [TE]" + head) or ln.startswith("  [TIE]" + head)]
    assert len(added) == 2 and [ln for k, ln in enumerate(on) if k not in added] == off      # with the switch off: the log as it was
    te, tie = added
    assert on[te].startswith("  [TE]") and on[te - 1].startswith("  [TE] top-5 lists") and on[te + 1].startswith("  [TIE]\t")
    assert on[tie - 1].startswith("  [TIE] top-5 lists") and on[tie + 1].startswith("  [TE->TIE] list shift")
    for k in added:
        assert all(c in on[k] for c in ("lambda", "recall", "ndcg", "ckl", "pop", "overlap", "share_", "coverage", "gini", "entropy"))
        assert on[k].count("\nall:") == 2 and on[k].count("\ntarget:") == 1
    assert ev0.tobytes() == ev1.tobytes() and te0.tobytes() == te1.tobytes()
