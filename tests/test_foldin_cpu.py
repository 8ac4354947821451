"""The host side of the new-user fold-in: reports.fold_in_weights against the adjacency itself for the five adjacency types, the
identity the definition rests on (the weighted sum of the history's layer means IS the mean of the new row's layers 1 .. L + 1 in
the extended graph), the float64 model against a plain loop on the shared cases, the report's pure table functions, and the
switch's refusals."""
import numpy as np
import pytest

import foldin_cases as fc
import foldin_model as fm
from helpers import build_model_from_fixture, load_golden

ADJ_TYPES = ("plain", "norm", "gcmc", "pre", "mean")
U, I = 3, 4
TRAIN_U, TRAIN_I = [0, 0, 1, 1, 1, 2], [0, 1, 0, 1, 2, 2]                 # item 3 has no training edge
TRAIN = {0: [0, 1], 1: [0, 1, 2], 2: [2]}


@pytest.mark.parametrize("adj_type", ADJ_TYPES)
def test_weights_are_the_adjacency_rows_of_training_users(adj_type):
    """A training user folded in with its own training items gets its own row of create_adj_mat off the diagonal: 2^-23 relative
    (the weights are formed in float64 and rounded once)."""
    from elimrec_amd import reports
    from elimrec_amd.model import create_adj_mat
    A = create_adj_mat(TRAIN_U, TRAIN_I, U, I, adj_type).toarray()
    deg = reports.item_train_counts(TRAIN, I)
    assert deg.tolist() == [2, 2, 2, 0]
    ptr, items = fm.csr([TRAIN[u] for u in range(U)])
    w = reports.fold_in_weights(adj_type, ptr, items, deg)
    assert w.dtype == np.float32 and w.shape == items.shape
    for u in range(U):
        for j in range(int(ptr[u]), int(ptr[u + 1])):
            want = float(A[u, U + int(items[j])])
            assert want > 0 and abs(float(w[j]) - want) <= 2.0 ** -23 * want, (adj_type, u, j, float(w[j]), want)
    assert np.allclose(w, fm.weights(adj_type, ptr, items, deg), rtol=2.0 ** -23, atol=0)


@pytest.mark.parametrize("adj_type", ADJ_TYPES)
def test_weights_rules(adj_type):
    from elimrec_amd import reports
    deg = np.array([2, 2, 2, 0])
    ptr, items = fm.csr([[3, 0, 3], [], [1]])                              # a cold item, twice; an empty history; one item
    w = reports.fold_in_weights(adj_type, ptr, items, deg)
    want = fm.weights(adj_type, ptr, items, deg)
    assert w.dtype == np.float32 and np.allclose(w, want, rtol=2.0 ** -23, atol=0)
    if adj_type == "pre":                                                 # max(deg, 1): the new edge is a cold item's first
        assert w[0] == np.float32(1.0 / np.sqrt(3.0)) and w[1] == np.float32(1.0 / np.sqrt(6.0)) and w[3] == np.float32(1.0 / np.sqrt(2.0))
    if adj_type == "norm":
        assert w[0] == np.float32(0.25) and w[3] == np.float32(0.5)       # 1 / (n + 1): the diagonal is in the row sum
    assert reports.fold_in_weights(adj_type, [0], [], deg).shape == (0,)
    for bad in ([4], [-1]):
        with pytest.raises(IndexError):
            reports.fold_in_weights(adj_type, [0, 1], bad, deg)
    for bad_ptr in ([0, 2], [1, 1], [0, 2, 1]):
        with pytest.raises(ValueError):
            reports.fold_in_weights(adj_type, bad_ptr, [0], deg)
    with pytest.raises(TypeError):
        reports.fold_in_weights(adj_type, [0, 1], [0.5], deg)


def _dense_adj(adj_type):
    """create_adj_mat's definitions in float64 on the dense tiny graph."""
    n = U + I
    A = np.zeros((n, n))
    for u, i in zip(TRAIN_U, TRAIN_I):
        A[u, U + i] = A[U + i, u] = 1.0

    def row_normalised(a):
        deg = a.sum(1)
        inv = np.where(deg > 0, 1.0 / np.where(deg > 0, deg, 1.0), 0.0)
        return inv[:, None] * a

    if adj_type == "plain":
        return A
    if adj_type == "norm":
        return row_normalised(A + np.eye(n))
    if adj_type == "gcmc":
        return row_normalised(A)
    if adj_type == "pre":
        deg = A.sum(1)
        inv = np.where(deg > 0, np.where(deg > 0, deg, 1.0) ** -0.5, 0.0)
        return inv[:, None] * A * inv[None, :]
    return row_normalised(A) + np.eye(n)


@pytest.mark.parametrize("adj_type", ADJ_TYPES)
def test_identity_of_the_definition(adj_type):
    """With every other row frozen, layer l + 1 of the new row is sum_i w_i layer_l[U + i]; the mean of its layers 1 .. L + 1 is
    therefore w . Out_items, Out = the mean of the trained layers 0 .. L. float64, atol 1e-12."""
    L, c = 3, 5
    rng = np.random.default_rng(ADJ_TYPES.index(adj_type))
    A = _dense_adj(adj_type)
    layers = [rng.standard_normal((U + I, c))]
    for _ in range(L):
        layers.append(A @ layers[-1])
    out = sum(layers) / (L + 1)
    deg = np.array([2, 2, 2, 0])
    for hist in ([0], [2, 0, 1], [3, 3, 1], [0, 1, 2, 3, 0]):
        ptr, items = fm.csr([hist])
        w = fm.weights(adj_type, ptr, items, deg)
        new_layers = [sum(w[j] * layers[l][U + i] for j, i in enumerate(hist)) for l in range(L + 1)]        # layers 1 .. L + 1
        want = sum(new_layers) / (L + 1)
        got = fm.segment_row_sum(out, ptr, items, w, row_offset=U)[0][0]
        assert np.allclose(got, want, rtol=0, atol=1e-12), (adj_type, hist)


@pytest.mark.parametrize("family", fc.FAMILIES)
def test_model_equals_a_plain_loop(family):
    rng = np.random.default_rng(fc.FAMILIES.index(family))
    buf, ptr, rows, w = fc.make(family, 8, 4, rng, pad=4, row_offset=3)
    assert np.diff(ptr).tolist() == fc.lengths(4) and np.isnan(buf[:, 8:]).all()
    want, bound, mag = fm.segment_row_sum(buf[:, :8], ptr, rows, w, row_offset=3)
    assert np.isfinite(want).all() and (bound >= 0).all() and not want[2].any() and not bound[2].any()
    for q in range(len(ptr) - 1):
        lo, hi = int(ptr[q]), int(ptr[q + 1])
        ref = (w[lo:hi, None].astype(np.float64) * buf[3 + rows[lo:hi], :8].astype(np.float64)).sum(0) if hi > lo else np.zeros(8)
        assert (np.abs(ref - want[q]) <= (hi - lo) * 2.0 ** -50 * mag[q]).all(), (family, q)
    if family == "cancel":                                                # the pairs cancel: what is left is far below the magnitudes
        assert (np.abs(want[6]) <= 1e-9 * mag[6]).all() and mag[6].min() > 0


def test_report_table_functions():
    from elimrec_amd import reports
    assert reports.NEWUSER_VARIANTS == ("trained", "history", "history+mean_id")
    cols = reports.newuser_columns(("Recall@5", "NDCG@5"))
    assert cols == ("users", "Recall@5", "NDCG@5", "overlap", "cos")
    # the all: row's metric columns: the evaluator's own overall expression (numpy's float32 mean over the users), column by column
    from elimrec_amd.evaluator import UniEvaluator
    rng = np.random.default_rng(0)
    ev = UniEvaluator(None, {}, {}, metric=["Recall", "NDCG"], top_k=[2, 5])
    full = rng.uniform(size=(203, 2 * 5)).astype(np.float32)
    shown = full.reshape(203, 2, 5)[:, :, ev.top_show - 1].reshape(203, -1)
    got = reports.newuser_overall_metrics(shown)
    assert got.dtype == np.float32 and got.tobytes() == ev._summary(full)[0].tobytes()
    assert reports.newuser_overall_metrics(shown[:, ::-1].copy()).tobytes() == got[::-1].tobytes()        # a column's mean is its own
    assert np.allclose(got, shown.astype(np.float64).mean(0), rtol=203 * 2.0 ** -24, atol=0)
    assert np.isnan(reports.newuser_overall_metrics(np.zeros((0, 4), dtype=np.float32))).all()
    # the model of the per-user rows and of the table (what the GPU test holds the report's device path against)
    n, k, d = 7, 4, 6
    own_lists = np.stack([rng.permutation(20)[:k] for _ in range(n)]).astype(np.int32)
    lists = own_lists.copy()
    lists[0] = own_lists[0][::-1]                                         # the same items in another order: overlap 1
    lists[1] = 20 + np.arange(k)                                          # none shared: overlap 0
    a, b = rng.standard_normal((n, d)), rng.standard_normal((n, d))
    b[1] = 0.0                                                            # a zero row: cos 0, not NaN
    b[2] = 3.0 * a[2]                                                     # parallel rows: cos 1
    rows = fm.user_rows(rng.uniform(size=(n, 2)), own_lists, lists, k, a, b)
    assert rows.shape == (n, 4) and rows[0, 2] == 1.0 and rows[1, 2] == 0.0 and rows[1, 3] == 0.0 and abs(rows[2, 3] - 1.0) <= 1e-12
    table = fm.table(rows, [np.arange(n), np.array([0, 2, 5]), np.array([6])])
    assert table.shape == (3, 5) and table[:, 0].tolist() == [7.0, 3.0, 1.0] and np.allclose(table[2, 1:], rows[6])
    buf = reports.format_newuser(cols, [(v + ":").ljust(16) for v in reports.NEWUSER_VARIANTS], np.tile(table[0], (3, 1)))
    assert buf.startswith("columns:") and "history+mean_id:" in buf and "%.8f" % table[0, 1] in buf
    assert "no test user" in reports.format_newuser(None, None, None)


def test_report_front_end_and_the_switch():
    from elimrec_amd.evaluator import NewUserReport
    g = load_golden("ml3")
    model, _ = build_model_from_fixture(g, "cpu")
    assert model.newuser_reporter is None                                 # off by default
    for bad in ("--newuser_report=-1", "--newuser_report=257"):
        with pytest.raises(ValueError, match="newuser_report"):
            build_model_from_fixture(g, "cpu", extra_argv=[bad])
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--newuser_report=7", "--group_view=[1,3,5]"])
    rep = model.newuser_reporter
    topks = [int(k) for k in model.config["topks"]]
    assert isinstance(rep, NewUserReport) and rep.k == 7 and rep.top_k == max(topks + [7])
    assert rep.evaluator.top_show.tolist() == sorted(set(topks + [7])) and rep.tie_order == model.test_evaluator.evaluator.tie_order
    train, test = model.dataset.get_user_train_dict(), model.dataset.get_user_test_dict()
    assert rep.users == [u for u in test if len(train.get(u, []))] and len(rep.group_labels) > 1
    assert rep.columns[0] == "users" and rep.columns[-2:] == ("overlap", "cos") and "Recall@7" in rep.columns
    cold = NewUserReport(model.dataset, {}, test, [5])                    # nobody has a training history
    assert cold.users == [] and cold.group_labels == ["all:".ljust(12)]
    with pytest.raises(TypeError):
        NewUserReport(model.dataset, [], test, [5])
    for bad in ([], [0], [True], [300], 2.5):
        with pytest.raises(ValueError):
            NewUserReport(model.dataset, train, test, bad)
    with pytest.raises(ValueError):
        NewUserReport(model.dataset, train, test, [5, 10], k=11)
    # fold_in_users refuses a bad id and bad id rows on the host: no device is ever asked for (this model lives on the CPU)
    with pytest.raises(IndexError):
        model.fold_in_users([[0, model.num_items]])
    with pytest.raises(IndexError):
        model.fold_in_users([[0], [-1]])
    for bad in (np.zeros((1, model.latent_dim + 1), dtype=np.float32), np.full((1, model.latent_dim), np.nan, dtype=np.float32),
                np.zeros((2, model.latent_dim), dtype=np.float32), np.zeros((1, model.latent_dim), dtype=np.int64), "median"):
        with pytest.raises(ValueError):
            model.fold_in_users([[0]], id_rows=bad)
