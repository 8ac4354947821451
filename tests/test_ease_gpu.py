"""EASE on the device (csrc/ease.hip): the Gram build, the SPD inverse and the ranking pass against tests/ease_model.py, the
readers built on them (EliMRec.fit_ease, recommend_ease, the `ease` source of the baseline report) and the torch.ops forms.

The inverse's bound, the form and constant of als_model.solve_bound: with kappa = max / min eigenvalue of G (eigvalsh)
    max|P - inv(G)| / max|inv(G)| <= 64 n kappa 2^-53   and   max|G P - I| <= 64 n kappa 2^-53.
The numpy sweep measures at most 2 of these units on the matrices below."""
import numpy as np
import pytest
import torch

import ease_model as em

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _binary(U, I, seed, density=0.15):
    """A random binary U x I matrix with one cold column (I // 3) and one duplicated column (the last = the first)."""
    X = (np.random.default_rng(seed).random((U, I)) < density).astype(np.float64)
    if I > 1:
        X[:, -1] = X[:, 0]
    X[:, I // 3] = 0.0
    return X


def _index(X):
    from elimrec_amd import ops
    U, I = X.shape
    return ops.CooccurIndex.from_train({u: np.flatnonzero(X[u]) for u in range(U)}, U, I, "item", DEV)


# ---- inverse
@pytest.mark.parametrize("l2", [0.5, 5.0, 500.0])
@pytest.mark.parametrize("n", [1, 17, 64, 65, 129, 200])
def test_inverse_against_float64(n, l2):
    from elimrec_amd import ops
    X = _binary(max(8, n // 2), n, seed=n)
    G = em.gram(X, l2)
    cold = n // 3
    ref = np.linalg.inv(G)
    bound = em.inverse_bound(n, em.kappa(G))
    A = _t(G)
    pivot = ops.spd_inverse(A)
    P = A.cpu().numpy()
    err = np.abs(P - ref).max() / np.abs(ref).max()
    res = np.abs(G @ P - np.eye(n)).max()
    print("n=%d l2=%g err/bound=%.3g res/bound=%.3g pivot_min=%g" % (n, l2, err / bound, res / bound, pivot))
    assert err <= bound and res <= bound, (err, res, bound)
    assert np.array_equal(P, P.T)
    e = np.zeros(n)
    e[cold] = 1.0
    assert np.array_equal(P[cold], e / l2) and np.array_equal(P[:, cold], e / l2)
    assert 0.0 < pivot <= G.diagonal().max()
    B = _t(G)
    assert ops.spd_inverse(B) == pivot and torch.equal(A, B)


def test_inverse_in_a_wider_matrix_touches_nothing_else():
    from elimrec_amd import ops
    n = 70
    G = em.gram(_binary(40, n, seed=3), 5.0)
    wide = torch.full((n + 2, n + 5), 7.0, dtype=torch.float64, device=DEV)
    view = wide[1:1 + n, 2:2 + n]
    view.copy_(_t(G))
    ops.spd_inverse(view)
    tight = _t(G)
    ops.spd_inverse(tight)
    assert torch.equal(view, tight)
    wide[1:1 + n, 2:2 + n] = 7.0
    assert bool((wide == 7.0).all())


def test_inverse_refuses_a_pivot_that_is_not_positive():
    from elimrec_amd import ops
    n = 130
    G = em.gram(_binary(60, n, seed=5), 5.0)
    G[100, 100] = -1.0                                       # the second pivot block meets it
    with pytest.raises(ArithmeticError):
        ops.spd_inverse(_t(G))
    with pytest.raises(ArithmeticError):
        ops.spd_inverse(_t(np.zeros((3, 3))))


# ---- Gram
def test_gram_counts_bit_for_bit():
    from elimrec_amd import ops
    U, I = 40, 70
    X = _binary(U, I, seed=11)
    X[7, :] = 1.0                                            # a user who holds every item ...
    X[:, I // 3] = 0.0                                       # ... but the empty one
    X[7, I // 3] = 0.0
    for l2 in (0.5, 500.0):
        out = torch.full((I, I + 3), np.nan, dtype=torch.float64, device=DEV)
        ops.gram_counts(_index(X), l2, out[:, :I])
        assert np.array_equal(out[:, :I].cpu().numpy(), em.gram(X, l2))
        assert bool(torch.isnan(out[:, I:]).all())
    assert em.gram(X, 0.5)[I // 3, I // 3] == 0.5


# ---- ranking
RANK_I = (4100, 70)


def _rank_case(I, seed=0):
    """A symmetric table of small integers with a power-of-two diagonal (every score exact), users with histories of length 0, 1,
    a few, and one beyond a history stage; 21 users: a ragged last row group."""
    from elimrec_amd import ops
    rng = np.random.default_rng(seed)
    P = rng.integers(-3, 4, size=(I, I)).astype(np.float64)
    P = np.triu(P, 1)
    P = P + P.T
    P[np.diag_indices(I)] = 2.0 ** rng.integers(0, 3, size=I)
    P[:, I // 3] = 0.0                                       # a cold item: zero off the diagonal
    P[I // 3, :] = 0.0
    P[I // 3, I // 3] = 0.25
    stage = ops.EASE_HIST_STAGE
    lens = [0, 1, stage + 1, 3, 5, stage, 2] + [int(x) for x in rng.integers(0, 12, size=14)]
    hists = [rng.choice(I, size=min(n, I), replace=False) for n in lens]
    return P, hists


@pytest.fixture(scope="module", params=RANK_I)
def rank_case(request):
    from elimrec_amd import ops
    I = request.param
    P, hists = _rank_case(I)
    rng = np.random.default_rng(1)
    excls = [np.unique(np.concatenate([h[:len(h) // 2], rng.choice(I, size=4, replace=False)])) for h in hists]   # differs from the history
    ptr = np.concatenate([[0], np.cumsum([len(h) for h in hists])])
    eptr = np.concatenate([[0], np.cumsum([len(e) for e in excls])])
    hist = ops.HistoryIndex(ptr, np.concatenate(hists), DEV, n_items=I)
    excl = ops.HistoryIndex(eptr, np.concatenate(excls), DEV, n_items=I)
    return I, P, _t(P), hists, excls, hist, excl


@pytest.mark.parametrize("K", [1, 10, 64, 65, 256])
@pytest.mark.parametrize("own_excl", [False, True])
def test_ranking_bit_for_bit(rank_case, K, own_excl):
    from elimrec_amd import ops
    I, P, Pd, hists, excls, hist, excl = rank_case
    B = len(hists)
    users = np.arange(B)[::-1].copy()                        # not the identity: query b is segment users[b]
    idx = torch.full((B, K), -7, dtype=torch.int32, device=DEV)
    val = torch.full((B, K), 9.0, dtype=torch.float32, device=DEV)
    ops.ease_topk(Pd, hist, users, K, idx, val, excl=excl if own_excl else None)
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    for b, u in enumerate(users):
        ids, vals, _ = em.topk(P, hists[u], excls[u] if own_excl else hists[u], K)
        assert np.array_equal(idx[b], ids), (I, K, u, idx[b][:8], ids[:8])
        assert np.array_equal(val[b], vals), (I, K, u)


def test_ranking_more_lists_than_items():
    """K > I: fillers behind the I - |excluded| items; an empty history lists the lowest ids that are not left out, at score 0."""
    from elimrec_amd import ops
    I, K = 70, 100
    P, hists = _rank_case(I)
    ptr = np.concatenate([[0], np.cumsum([len(h) for h in hists])])
    hist = ops.HistoryIndex(ptr, np.concatenate(hists), DEV, n_items=I)
    idx = torch.empty((len(hists), K), dtype=torch.int32, device=DEV)
    val = torch.empty((len(hists), K), dtype=torch.float32, device=DEV)
    ops.ease_topk(_t(P), hist, np.arange(len(hists)), K, idx, val)
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    for u, h in enumerate(hists):
        ids, vals, _ = em.topk(P, h, h, K)
        assert np.array_equal(idx[u], ids) and np.array_equal(val[u], vals)
    assert np.array_equal(idx[0, :I], np.arange(I)) and (val[0, :I] == 0).all() and (idx[0, I:] == -1).all() and np.isneginf(val[0, I:]).all()


# ---- torch.ops forms
def test_torch_ops_equal_the_bindings():
    from elimrec_amd import ops, torch_ops
    torch_ops.load()
    U, I, l2 = 30, 70, 5.0
    X = _binary(U, I, seed=21)
    index = _index(X)
    G = torch.empty((I, I), dtype=torch.float64, device=DEV)
    ops.gram_counts(index, l2, G)
    n_e = index.n_edges
    G2 = torch.ops.elimrec.gram_counts(index.q_ptr, index.q_nbr[:n_e], index.o_ptr, index.o_nbr[:n_e], l2)
    assert torch.equal(G, G2)
    P = G.clone()
    pivot = ops.spd_inverse(P)
    P2, pivot2 = torch.ops.elimrec.spd_inverse(G)
    assert torch.equal(P, P2) and float(pivot2.item()) == pivot
    hists = [np.flatnonzero(X[u]) for u in range(U)]
    ptr = np.concatenate([[0], np.cumsum([len(h) for h in hists])])
    hist = ops.HistoryIndex(ptr, np.concatenate(hists), DEV, n_items=I)
    users = np.arange(U)
    idx = torch.empty((U, 10), dtype=torch.int32, device=DEV)
    val = torch.empty((U, 10), dtype=torch.float32, device=DEV)
    ops.ease_topk(P, hist, users, 10, idx, val)
    idx2, val2 = torch.ops.elimrec.ease_topk(P, hist.ptr, hist.items[:hist.n_entries], None, None, _t(users), 10)
    assert torch.equal(idx, idx2) and torch.equal(val, val2)
    with pytest.raises(RuntimeError):
        torch.ops.elimrec.spd_inverse(-G)


# ---- end to end: the fit, its readers and the report on a generated split
E2E_U, E2E_I, E2E_L2, E2E_SEED, E2E_K = em.E2E_U, em.E2E_I, em.E2E_L2, em.E2E_SEED, em.E2E_K
_generated, _reference, _compare = em.generated_split, em.reference, em.compare


def _model(extra=(), forward=False):
    from elimrec_amd import EliMRec
    from helpers import FixtureDataset, fixture_argv, make_config
    g, split = _generated()
    torch.manual_seed(0)
    model = EliMRec(make_config(fixture_argv(g) + list(extra)), FixtureDataset(g)).to(DEV)
    if forward:                                              # the report's overlap column reads the model's own lists: cached tables
        users = np.arange(1, 65, dtype=np.int64)
        pos = np.asarray([split["train"][u][0] for u in users], dtype=np.int64)
        model.bpr_loss(_t(users), _t(pos), _t((pos + 1) % E2E_I))
    return model, split


def test_recommend_ease_against_dense_numpy():
    model, split = _model()
    P, kap = _reference(split)
    users = np.arange(E2E_U)
    got = model.recommend_ease(users, E2E_K, l2=E2E_L2)
    fit = model.fit_ease(E2E_L2)
    assert fit is model.fit_ease(E2E_L2) and fit.l2 == E2E_L2 and fit.bytes >= 8 * E2E_I ** 2 and 0 < fit.pivot_min
    Pd = fit.P.cpu().numpy()
    assert np.abs(Pd - P).max() / np.abs(P).max() <= em.inverse_bound(E2E_I, kap)
    e = np.zeros(E2E_I)
    e[E2E_I // 3] = 1.0 / E2E_L2
    assert np.array_equal(Pd[E2E_I // 3], e)
    share = _compare(got.ids.numpy(), users, split, P, kap)
    print("excused share: %.4f" % share)
    assert share <= 0.02
    assert np.array_equal(got.ids[0].numpy(), np.arange(E2E_K)) and (got.scores[0] == 0).all()       # user 0 has no history
    for b, u in enumerate(users):                            # the scores are the model's up to the inverse's error
        s = em.scores(P, split["train"].get(int(u), []))
        assert np.abs(got.scores[b].numpy() - s[got.ids[b].numpy()]).max() <= 1e-5 * max(1.0, np.abs(s).max())
    # history and exclude as recommend_knn takes them
    other = model.recommend_ease([5, 6], 10, history={5: split["train"][6], 6: []}, exclude={5: [0, 1]}, l2=E2E_L2)
    s = em.scores(P, split["train"][6])
    ok, _ = em.rank_equal_up_to(other.ids[0].numpy(), em.full_order(s, list(split["train"][6]) + [0, 1]), s, 1e-12)
    assert ok and np.array_equal(other.ids[1].numpy(), np.arange(10))


def test_the_baseline_report_with_ease():
    from elimrec_amd import ops
    args = ["--baseline_report=%d" % E2E_K, "--baseline_neighbours=7", "--group_view=[5,30]", "--baseline_l2=%r" % E2E_L2]
    model, split = _model(args + ["--baseline_sources=[co,ease]"], forward=True)
    rep = model.baseline_reporter
    final, buf = rep.evaluate(model)
    G = len(rep.group_labels)
    lines = buf.split("\n")
    assert final.table.shape == (2 * G, len(rep.columns)) and final.labels[G].startswith("ease all:")
    fit = model.fit_ease(E2E_L2)
    assert lines[-1] == "ease: l2=5 items=%d bytes=%d pivot_min=%.8g" % (E2E_I, fit.bytes, fit.pivot_min) and len(lines) == 1 + 2 * G + 1
    lists = rep.knn_lists(model, "ease")
    want = model.recommend_ease(list(rep.users), E2E_K, l2=E2E_L2).ids.numpy()
    assert np.array_equal(lists.cpu().numpy(), want)
    P, kap = _reference(split)
    assert _compare(want, np.asarray(rep.users), split, P, kap) <= 0.02
    ev = rep.evaluator
    res = rep._resident(lists.device)
    out = torch.empty(len(rep.users), ev.metrics_num * ev.max_top, dtype=torch.float32, device=DEV)
    first = lists if rep.k == ev.max_top else lists[:, :ev.max_top].contiguous()
    ops.rank_metrics(first, res["truth"][0], res["truth"][1], ev.metrics, out)
    rows, columns = rep.metric_rows(model, "ease")
    assert torch.equal(rows, out.index_select(1, res["shown"])) and columns == rep.metric_columns
    Cs = len(rep.metric_columns)
    assert np.allclose(final.table[G, :Cs], rows.double().mean(0).cpu().numpy(), rtol=1e-6, atol=1e-9)
    # without ease among the sources the report's text for ("co",) is what it was
    alone, _ = _model(args + ["--baseline_sources=[co]"], forward=True)
    final0, buf0 = alone.baseline_reporter.evaluate(alone)
    assert buf0.split("\n") == lines[:1 + G] and final0.table.tobytes() == final.table[:G].tobytes() and "ease" not in buf0
