"""The iALS half-sweep on the device (csrc/als.hip, ops.als_solve) against the float64 model of tests/als_model.py, and the fit
and its readers built on it (EliMRec.fit_ials, recommend_ials, the `ials` source of the baseline report).

The solve's bound per row (derived, not measured -- als_model.solve_bound):
    |got - x64| <= 2^-24 |x64| + 64 d cond(A_r) 2^-53 max|x64|
the one rounding to float32 plus the Cholesky backward-error bound with a loose constant; the test asserts from the model that
every cond(A_r) <= 1e6, so the second term stays below 64 * 64 * 1e6 * 2^-53 = 4.5e-7 max|x64|."""
import numpy as np
import pytest
import torch

import als_model as am
import knn_model as km
from helpers import build_model_from_fixture, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_FIXED = am.N_FIXED
SENTINEL = 7.0


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _case(d, seed=0, col0=4):
    """als_model.solve_case: (ptr, nbr, F float32 [N_FIXED x d], its device view as a column block of a wider NaN matrix; col0 = 3:
    rows not 16-byte aligned, the scalar loads; 4: aligned, the vector loads)."""
    from elimrec_amd import ops
    ptr, nbr, F = am.solve_case(d, ops.ALS_CHUNK, seed)
    wide = np.full((N_FIXED + 3, d + 12), np.nan, dtype=np.float32)
    wide[2:2 + N_FIXED, col0:col0 + d] = F
    return ptr, nbr, F, _t(wide)[2:2 + N_FIXED, col0:col0 + d]


def _gram(Fd):
    from elimrec_amd import ops
    n = Fd.shape[0]
    return ops.row_gram(Fd, torch.ones(n, dtype=torch.float32, device=DEV), torch.arange(n, dtype=torch.int32, device=DEV))[0]


def _reg(kind, ptr):
    return am.solve_reg(kind, ptr)


def _solve(index, Fd, A0, reg, conf, rows=None):
    from elimrec_amd import ops
    out = torch.full((index.n, Fd.shape[1]), SENTINEL, dtype=torch.float32, device=DEV)
    ops.als_solve(index, Fd, A0, reg, conf, out, rows=rows)
    return out.cpu().numpy()


@pytest.mark.parametrize("d", [16, 48, 64])
def test_solve_against_float64(d):
    """Largest observed |got - x64| / bound over all cases on an MI355X: 0.974 (d = 16, conf = 0, constant reg; the first
    term alone is half an ulp of float32, which a correctly rounded result can reach)."""
    from elimrec_amd import ops
    ptr, nbr, F, Fd = _case(d)
    assert Fd.stride(0) > d
    n = ptr.size - 1
    index = ops.AlsIndex(ptr, nbr, n, N_FIXED, DEV)
    A0 = _gram(Fd)
    assert np.abs(A0.cpu().numpy() - F.astype(np.float64).T @ F.astype(np.float64)).max() <= 1e-12
    rows = np.arange(n)
    worst = 0.0
    for conf in am.SOLVE_CONFS:
        for kind in am.SOLVE_REGS:
            reg = _reg(kind, ptr)
            cnd = am.cond(ptr, nbr, F, reg, conf, rows)
            assert cnd.max() <= 1e6, (d, conf, kind, cnd.max())
            x64 = am.solve_rows(ptr, nbr, F, reg, conf, rows)
            got = _solve(index, Fd, A0, reg, conf).astype(np.float64)
            ratio = float((np.abs(got - x64) / np.maximum(am.solve_bound(x64, cnd, d), 1e-300)).max())
            worst = max(worst, ratio)
            print("als_solve d=%d conf=%g reg=%s: cond <= %.3g, err / bound = %.3g" % (d, conf, kind, cnd.max(), ratio))
            assert (np.abs(got - x64) <= am.solve_bound(x64, cnd, d)).all(), (d, conf, kind, ratio)
            assert (got[np.diff(ptr) == 0] == 0).all()
    print("als_solve d=%d: largest err / bound = %.3g" % (d, worst))


def test_solve_is_deterministic_and_leaves_other_rows_alone():
    from elimrec_amd import ops
    d, conf = 64, 1.0
    ptr, nbr, F, Fd = _case(d, seed=1)
    n = ptr.size - 1
    index = ops.AlsIndex(ptr, nbr, n, N_FIXED, DEV)
    A0, reg = _gram(Fd), _reg("per row", ptr)
    every = _solve(index, Fd, A0, reg, conf)
    listed = np.asarray([6, 1, 7, 3, 0])
    some = _solve(index, Fd, A0, reg, conf, rows=listed)
    back = _solve(index, Fd, A0, reg, conf, rows=listed[::-1].copy())
    others = np.setdiff1d(np.arange(n), listed)
    assert (some[others] == SENTINEL).all() and (back[others] == SENTINEL).all()
    for r in listed:
        alone = _solve(index, Fd, A0, reg, conf, rows=np.asarray([r]))
        assert (alone[np.arange(n) != r] == SENTINEL).all()
        for other in (some, back, every):
            assert np.array_equal(alone[r].view(np.int32), other[r].view(np.int32)), r
    assert np.array_equal(_solve(index, Fd, A0, reg, conf).view(np.int32), every.view(np.int32))


def test_not_positive_definite_is_reported_and_the_process_carries_on():
    from elimrec_amd import ops
    d = 16
    ptr, nbr, F, Fd = _case(d, seed=2, col0=3)
    n = ptr.size - 1
    index = ops.AlsIndex(ptr, nbr, n, N_FIXED, DEV)
    rows = np.asarray([5, 2, 3, 6])                      # every one with a list of its own
    out = torch.full((n, d), SENTINEL, dtype=torch.float32, device=DEV)
    A_bad = -4.0 * torch.eye(d, dtype=torch.float64, device=DEV)
    with pytest.raises(ArithmeticError, match=r"4 row\(s\), the first is row 2 "):
        ops.als_solve(index, Fd, A_bad, 0.0, 0.0, out, rows=rows)
    got = out.cpu().numpy()
    assert (got[rows] == 0).all() and (got[np.setdiff1d(np.arange(n), rows)] == SENTINEL).all()
    reg = _reg("constant", ptr)
    x64 = am.solve_rows(ptr, nbr, F, reg, 1.0, np.arange(n))
    got = _solve(index, Fd, _gram(Fd), reg, 1.0).astype(np.float64)
    assert (np.abs(got - x64) <= am.solve_bound(x64, am.cond(ptr, nbr, F, reg, 1.0, np.arange(n)), d)).all()


def test_torch_entry_point_gives_the_same_bits():
    from elimrec_amd import ops, torch_ops
    d, conf = 48, 40.0
    ptr, nbr, F, Fd = _case(d, seed=3)
    n = ptr.size - 1
    A0, reg = _gram(Fd), _reg("per row", ptr)
    want = _solve(ops.AlsIndex(ptr, nbr, n, N_FIXED, DEV), Fd, A0, reg, conf)
    ns = torch_ops.load()
    got = ns.als_solve(_t(ptr), _t(nbr), Fd, A0, _t(reg), conf, None).cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    rows = np.asarray([7, 3], dtype=np.int32)
    got = ns.als_solve(_t(ptr), _t(nbr), Fd, A0, _t(reg), conf, _t(rows)).cpu().numpy()
    assert np.array_equal(got[rows].view(np.int32), want[rows].view(np.int32)) and (np.delete(got, rows, 0) == 0).all()
    with pytest.raises(ValueError, match="strictly ascending"):
        bad = nbr.copy()
        bad[int(ptr[2])] = bad[int(ptr[2]) + 1]
        ns.als_solve(_t(ptr), _t(bad), Fd, A0, _t(reg), conf, None)
    # not positive definite: the dispatcher's error is a RuntimeError (ops.als_solve raises ArithmeticError), with the same words
    with pytest.raises(RuntimeError, match=r"not positive definite for 2 row\(s\), the first is row 3 "):
        ns.als_solve(_t(ptr), _t(nbr), Fd, -4.0 * torch.eye(d, dtype=torch.float64, device=DEV), _t(np.zeros(n)), 0.0, _t(rows))
    assert np.array_equal(ns.als_solve(_t(ptr), _t(nbr), Fd, A0, _t(reg), conf, None).cpu().numpy().view(np.int32), want.view(np.int32))


# --------------------------------------------------------------------------- the fit, its readers and the report
def _fixture(forward=False, extra=()):
    g = load_golden("ml3")
    model, _ = build_model_from_fixture(g, DEV, extra_argv=list(extra))
    if forward:
        model.bpr_loss(_t(g["step1/users"]), _t(g["step1/pos"]), _t(g["step1/neg"]))
    return model


def _train_lists(model):
    train = model.dataset.get_user_train_dict()
    return [list(train.get(u, [])) for u in range(model.num_users)]


def test_fit_ials_against_the_model_half_sweep_by_half_sweep():
    """The bound used: every one of the 6 half-sweeps of fit_ials(factors=16, iters=3) is held to the solve bound of its own
    normal equations, the model being fed the DEVICE's float32 factors of the half-sweep before (fits are bit-identical and kept
    per parameter tuple, so the fit with iters = k is the state after 2 k half-sweeps). That chain is the accumulated bound: no
    half-sweep may add more than its own solve bound to what it was given. (Compounding the bounds through first-order
    perturbation theory, tol_h = b_h + 3 cond_h tol_(h-1), gives a factor of 75^5 at the condition numbers of this fixture and
    says nothing.) End to end, against als_model.fit's own trajectory Xm / Ym, every half-sweep is asserted as well:
        |got - model(model's previous factors)| <= solve bound + |model(device's previous factors) - model(model's previous factors)|
    the second term being the MODEL's own sensitivity to the difference of the inputs, computed in float64 by the model and not
    taken from the device (it is 0 for as long as the earlier half-sweeps matched bit for bit -- on an MI355X all 6 did, and the
    final factors equalled Xm and Ym exactly). The objective is compared with the model's."""
    model = _fixture()                                   # untrained, no forward: the training graph alone
    lists, I, U, d = _train_lists(model), model.num_items, model.num_users, 16
    ptr, nbr, t_ptr, t_nbr = am.graph(lists, I)
    reg_u, reg_i = am.ridge(ptr, 0.01, 0.0), am.ridge(t_ptr, 0.01, 0.0)
    Y = (0.01 * np.random.default_rng(2022).standard_normal((I, d))).astype(np.float32)
    worst, end_to_end, trail = 0.0, [], [Y.copy(), None]     # trail: the model's own (items, users) as als_model.fit walks them
    for k in (1, 2, 3):
        fit = model.fit_ials(factors=d, iters=k)
        Xd, Yd = fit.users.cpu().numpy(), fit.items.cpu().numpy()
        for got, (p, n_, F, reg) in ((Xd, (ptr, nbr, Y, reg_u)), (Yd, (t_ptr, t_nbr, Xd, reg_i))):
            rows = np.arange(p.size - 1)
            cnd = am.cond(p, n_, F, reg, 1.0, rows)
            assert cnd.max() <= 1e6
            x64 = am.solve_rows(p, n_, F, reg, 1.0, rows)
            bound = am.solve_bound(x64, cnd, d)
            worst = max(worst, float((np.abs(got - x64) / np.maximum(bound, 1e-300)).max()))
            assert (np.abs(got.astype(np.float64) - x64) <= bound).all(), (k, worst)
            # end to end against als_model.fit's own trajectory: the solve bound plus the model's own sensitivity to the input
            Fm = trail[0] if p is ptr else trail[1]
            xm = am.solve_rows(p, n_, Fm, reg, 1.0, rows)
            moved = np.abs(x64 - xm)
            assert (np.abs(got.astype(np.float64) - xm) <= bound + moved).all(), (k, float(moved.max()))
            end_to_end.append(float(np.abs(got - xm.astype(np.float32)).max()))
            if p is ptr:
                trail[1] = xm.astype(np.float32)             # the model's users, from the model's items
            else:
                trail[0] = xm.astype(np.float32)             # the model's items, from the model's users
        Y = Yd
    Xm, Ym, obj, _ = am.fit(lists, I, factors=d, iters=3)
    assert end_to_end, "no half-sweep was compared end to end"
    assert np.array_equal(trail[1], Xm) and np.array_equal(trail[0], Ym)                   # the trail IS als_model.fit's trajectory
    print("fit_ials: largest half-sweep err / bound %.3g; end to end |X - Xm| %.3g, |Y - Ym| %.3g; per half-sweep %s" % (
        worst, np.abs(Xd - Xm).max(), np.abs(Yd - Ym).max(), end_to_end))
    assert fit.objective.dtype == np.float64 and fit.objective.shape == (6,)
    assert (np.diff(fit.objective) <= 1e-9 * np.abs(fit.objective[:-1])).all(), fit.objective
    assert np.abs(fit.objective - obj).max() <= 1e-6 * np.abs(obj).max(), (fit.objective, obj)
    assert fit.params == (16, 3, 1.0, 0.01, 0.0, 2022) and fit.users.is_cuda and fit.users.dtype == torch.float32
    assert model.fit_ials(factors=d, iters=3) is fit                                       # kept per parameter tuple
    again = _fixture().fit_ials(factors=d, iters=3)
    assert again.users.cpu().numpy().tobytes() == Xd.tobytes() and again.items.cpu().numpy().tobytes() == Yd.tobytes()
    assert again.objective.tobytes() == fit.objective.tobytes()
    scaled = model.fit_ials(factors=d, iters=2, reg_scale=0.5, conf=3.0)
    Xs, Ys, objs, _ = am.fit(lists, I, factors=d, iters=2, conf=3.0, reg_scale=0.5)
    assert np.abs(scaled.objective - objs).max() <= 1e-6 * np.abs(objs).max()


def test_recommend_ials():
    model = _fixture()
    U, I, d, k = model.num_users, model.num_items, 16, 20
    fit = model.fit_ials(factors=d, iters=3)
    X, Y = fit.users.cpu().numpy().astype(np.float64), fit.items.cpu().numpy().astype(np.float64)
    train = model.dataset.get_user_train_dict()
    users = [3, 0, U - 1, 3]
    got = model.recommend_ials(users, k, factors=d, iters=3)
    assert not got.ids.is_cuda and got.ids.dtype == torch.int32 and tuple(got.ids.shape) == (len(users), k)
    excl = [list(train.get(u, [])) for u in users]
    s = km.masked(X[users] @ Y.T, users, False, excl)
    tol = km.tol(d) * float(np.sqrt((X * X).sum(1)).max() * np.sqrt((Y * Y).sum(1)).max())
    from test_cross_topk_gpu import _check_lists
    _check_lists(got.ids.numpy(), got.scores.numpy(), s, k, tol, "recommend_ials")
    for b, u in enumerate(users):
        assert not set(got.ids[b].tolist()) & set(train.get(u, []))
    # an explicit exclude replaces the train dict; a user it leaves nearly nothing gets fillers
    most = {3: list(range(I - 2))}
    got = model.recommend_ials([3], k, exclude=most, factors=d, iters=3)
    assert sorted(got.ids[0, :2].tolist()) == [I - 2, I - 1] and (got.ids[0, 2:] == -1).all() and torch.isneginf(got.scores[0, 2:]).all()
    # a user WITHOUT history (a zero row of the users' factors, as the fit leaves it): every score is exactly 0, the list is all ties and
    # the lowest ids are listed; fillers only where k exceeds the unmasked catalogue
    from elimrec_amd.model import IalsFactors
    Xz = fit.users.clone()
    Xz[5] = 0.0
    blank = IalsFactors(Xz, fit.items, fit.params, fit.objective)
    none = (np.zeros(3, dtype=np.int64), np.zeros(0, dtype=np.int64))
    idx, val = model.ials_recommend_device(np.asarray([5, 3]), blank, k, none)
    assert idx[0].tolist() == list(range(k)) and (val[0] == 0).all() and idx[1].tolist() != list(range(k))
    kk = min(I, 256)
    idx, val = model.ials_recommend_device(np.asarray([5]), blank, kk, (np.asarray([0, 0]), np.zeros(0, dtype=np.int64)))
    assert idx[0].tolist() == list(range(kk)) and (val[0] == 0).all()                          # k <= I: no filler
    idx, val = model.ials_recommend_device(np.asarray([5]), blank, kk, (np.asarray([0, 3]), np.asarray([0, 2, I - 1])))
    left = [i for i in range(I) if i not in (0, 2, I - 1)]
    assert idx[0].tolist() == left[:kk] + [-1] * (kk - len(left[:kk])) and int((idx[0] == -1).sum()) == max(0, kk - (I - 3))
    assert torch.isneginf(val[0, min(kk, I - 3):]).all() and (val[0, :min(kk, I - 3)] == 0).all()
    # and through the fit itself: a copy of the data set in which user 5 has no train item
    lonely = _fixture()
    emptied = dict(lonely.dataset.get_user_train_dict())
    emptied[5] = []
    lonely.dataset._dicts["train"] = emptied
    zero = lonely.fit_ials(factors=d, iters=2)
    assert (zero.users[5] == 0).all() and (zero.users[3] != 0).any()
    got = lonely.recommend_ials([5], k, factors=d, iters=2)
    assert got.ids[0].tolist() == list(range(k)) and (got.scores[0] == 0).all()
    # fillers appear only where k exceeds the unmasked catalogue: nothing masked -> none; the train items masked -> one each
    kk = min(I, 256)
    cold = model.recommend_ials([3], kk, exclude={}, factors=d, iters=3)
    assert (cold.ids >= 0).all() and len(set(cold.ids[0].tolist())) == kk
    seen = len(set(train.get(3, [])))
    warm = model.recommend_ials([3], kk, factors=d, iters=3)
    assert seen > 0 and int((warm.ids[0] == -1).sum()) == max(0, kk - (I - seen))
    assert tuple(model.recommend_ials([], 5, factors=d, iters=3).ids.shape) == (0, 5)


@pytest.mark.parametrize("effect", ["TE", "TIE"])
def test_the_baseline_report_with_ials(effect):
    from elimrec_amd import ops
    args = ["--baseline_report=20", "--baseline_neighbours=7", "--group_view=[2,4]", "--baseline_factors=16", "--baseline_iters=3"]
    model = _fixture(True, args + ["--baseline_sources=[co,ials]", "--significance_report=50"])
    model.predict_type = effect
    rep, sig = model.baseline_reporter, model.significance_reporter
    assert rep.ials_params[:5] == (16, 3, 1.0, 0.01, 0.0)
    final, buf = rep.evaluate(model)
    G = len(rep.group_labels)
    lines = buf.split("\n")
    assert final.table.shape == (2 * G, len(rep.columns)) and final.labels[G].startswith("ials all:")
    assert len(lines) == 1 + 2 * G + 1 and lines[1].startswith("co all:") and lines[1 + G].startswith("ials all:")
    fit = model.fit_ials(factors=16, iters=3)
    assert lines[-1] == "ials: factors=16 iters=3 conf=1 reg=0.01 reg_scale=0 objective=%.8g -> %.8g" % (fit.objective[0], fit.objective[-1])
    want = model.recommend_ials(list(rep.users), 20, factors=16, iters=3).ids.numpy()
    lists = rep.knn_lists(model, "ials")
    assert np.array_equal(lists.cpu().numpy(), want) and (want >= 0).all()
    ev = rep.evaluator
    res = rep._resident(lists.device)
    out = torch.empty(len(rep.users), ev.metrics_num * ev.max_top, dtype=torch.float32, device=DEV)
    first = lists if rep.k == ev.max_top else lists[:, :ev.max_top].contiguous()
    ops.rank_metrics(first, res["truth"][0], res["truth"][1], ev.metrics, out)
    rows, columns = rep.metric_rows(model, "ials")
    assert torch.equal(rows, out.index_select(1, res["shown"])) and columns == rep.metric_columns
    shift, text = sig.shift((rows, columns), sig.metric_rows(model))         # model - ials, paired per user
    assert shift.p is not None and "all: mean" in text
    # the ials row does not depend on the neighbour-vote settings; the co rows do not depend on ials
    other = _fixture(True, ["--baseline_report=20", "--baseline_neighbours=3", "--baseline_measure=count", "--group_view=[2,4]",
                            "--baseline_factors=16", "--baseline_iters=3", "--baseline_sources=[ials]"])
    other.predict_type = effect
    assert other.baseline_reporter.evaluate(other)[0].table.tobytes() == final.table[G:].tobytes()
    alone = _fixture(True, args + ["--baseline_sources=[co]"])
    alone.predict_type = effect
    final0, buf0 = alone.baseline_reporter.evaluate(alone)
    assert buf0.split("\n") == lines[:1 + G] and final0.table.tobytes() == final.table[:G].tobytes()


def test_driver_switch(tmp_path):
    from test_lists_gpu import _driver
    base = ["--baseline_report=10", "--baseline_neighbours=5", "--significance_report=20", "--baseline_factors=16", "--baseline_iters=2"]
    off, ev0, te0 = _driver(tmp_path / "a", base + ["--baseline_sources=[co]"])
    assert not any("ials" in ln for ln in off)
    on, ev1, te1 = _driver(tmp_path / "b", base + ["--baseline_sources=[co,ials]"])
    paired = [k for k, ln in enumerate(on) if ln.startswith("  [TE - ials] metric difference") or ln.startswith("  [TIE - ials] metric difference")]
    tables = [k for k, ln in enumerate(on) if "[baselines]" in ln.split("\n")[0]]
    assert len(paired) == 2 and len(tables) == 2
    for k in tables:
        block = on[k].split("\n")
        ials = [ln for ln in block if ln.startswith("ials")]
        assert len(ials) == 2 and ials[0].startswith("ials all:") and block[-1] == ials[1]
        assert ials[1].startswith("ials: factors=16 iters=2 conf=1 reg=0.01 reg_scale=0 objective=")
        assert block[2].startswith("co all:")
        on[k] = "\n".join(ln for ln in block if not ln.startswith("ials"))   # without the ials row and line: the run without ials
    assert [ln for k, ln in enumerate(on) if k not in paired] == off
    assert ev0.tobytes() == ev1.tobytes() and te0.tobytes() == te1.tobytes()
