"""Cosine top-K lists on the device (csrc/knn.hip) against the float64 model of tests/knn_model.py.

Scores are compared within tol(d) = 2 (d + 8) 2^-24 (derived in knn_model.tol, not measured); lists by criteria (a)-(e) of
_check_lists, which accept any order the fp32 scores can justify and nothing else. The table is a column block of a wider matrix
whose other columns and neighbouring rows hold NaN: a read outside the slice shows up as a wrong list. Shapes are placed from
ops.KNN_TILE / ops.KNN_CHUNK. K <= 256 < KNN_CHUNK, so K > n - 1 (fillers at the tail) is met for every n up to 17; the n around the
chunk edges get their fillers from an exclusion list that leaves query 0 five candidates."""
import os

import numpy as np
import pytest
import torch

import knn_model as km
from helpers import ROOT, build_model_from_fixture, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FAMILIES = ("normal", "scaled", "clustered")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _edges():
    from elimrec_amd import ops
    return ops.KNN_TILE, ops.KNN_CHUNK


def _table(family, n, d, rng):
    x = rng.standard_normal((n, d))
    if family == "scaled":
        x = x * np.exp(rng.uniform(-8, 8, size=(n, 1)))
    elif family == "clustered":
        x = rng.standard_normal((1, d)) + 0.05 * x
    return x.astype(np.float32)


def _place(T, col0):
    """T as a column block at row 2, column col0 of a wider NaN matrix (col0 = 3: rows not 16-byte aligned; 4: aligned), and its
    squared norms as column 1 of a NaN [n x 3] table. -> (table view, sqnorm view) on the device."""
    n, d = T.shape
    wide = np.full((n + 3, d + col0 + 4), np.nan, dtype=np.float32)
    wide[2:2 + n, col0:col0 + d] = T
    sq = np.full((n, 3), np.nan, dtype=np.float32)
    sq[:, 1] = (T.astype(np.float64) ** 2).sum(1).astype(np.float32)
    return _t(wide)[2:2 + n, col0:col0 + d], _t(sq)[:, 1]


def _run(table, sqn, rows, K, exclude_self=True, excl=None, rows_out=None):
    from elimrec_amd import ops
    Q = len(rows)
    idx = torch.full((rows_out or Q, K), -7, dtype=torch.int32, device=DEV)
    val = torch.full((rows_out or Q, K), 7.0, dtype=torch.float32, device=DEV)
    ptr, flat = km.csr(excl) if excl is not None else (None, None)
    ops.cosine_topk(table, sqn, np.asarray(rows, dtype=np.int32), K, idx, val, exclude_self=exclude_self, excl_ptr=ptr, excl_rows=flat)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), val.cpu().numpy()


def _check_lists(ids, vals, s, K, d, what):
    """ids / vals [Q x K] against the masked float64 scores s [Q x n]."""
    tol = km.tol(d)
    n = s.shape[1]
    order, _ = km.topk64(s, K)
    for b in range(s.shape[0]):
        r, v, o = ids[b].astype(np.int64), vals[b], order[b]
        m = min(K, int((s[b] > -np.inf).sum()))
        # (a)
        assert (r[:m] >= 0).all() and (r[:m] < n).all() and (r[m:] == -1).all() and np.isneginf(v[m:]).all(), (what, b, r, m)
        assert len(set(r[:m].tolist())) == m and (s[b, r[:m]] > -np.inf).all(), (what, b)
        if not m:
            continue
        # (b), (c)
        assert np.abs(v[:m].astype(np.float64) - s[b, r[:m]]).max() <= tol, (what, b, np.abs(v[:m] - s[b, r[:m]]).max(), tol)
        assert np.abs(s[b, r[:m]] - s[b, o[:m]]).max() <= 2 * tol, (what, b)
        # (d)
        if m == K:
            must = np.flatnonzero(s[b] > s[b, o[K - 1]] + 2 * tol)
            assert np.isin(must, r).all(), (what, b)
        # (e)
        assert (v[1:m] <= v[:m - 1]).all(), (what, b)
        same = v[1:m].view(np.int32) == v[:m - 1].view(np.int32)
        assert (r[1:m][same] > r[:m - 1][same]).all(), (what, b)


def _cases():
    T, C = _edges()
    return [  # d, n, Q, K, column offset
        (4, 1, 1, 1, 3), (32, 2, 1, 10, 4), (36, 15, T - 1, 50, 3), (64, 16, T, 50, 4), (128, 17, T + 1, 256, 3),
        (4, 17, T, 10, 4), (36, 16, T + 1, 256, 4), (64, C - 1, T + 1, 10, 3), (128, 2, 1, 1, 4), (128, 15, T - 1, 50, 4),
        (32, C, T, 256, 3), (32, C + 1, T - 1, 1, 4), (32, 2 * C + 7, T + 1, 50, 3), (32, 2 * C + 7, 1, 256, 4),
    ]


def test_cases_cover_the_issue():
    T, C = _edges()
    cases = _cases()
    assert {c[0] for c in cases} == {4, 32, 36, 64, 128} and {c[3] for c in cases} == {1, 10, 50, 256}
    assert {c[1] for c in cases} == {1, 2, 15, 16, 17, C - 1, C, C + 1, 2 * C + 7} and {c[2] for c in cases} == {1, T - 1, T, T + 1}
    assert all(c[0] == 32 for c in cases if c[1] >= C)
    for n in (1, 2, 15, 16, 17):
        assert any(c[1] == n and c[3] > n - 1 for c in cases)


@pytest.mark.parametrize("family", FAMILIES)
def test_lists_against_float64(family):
    T_, C = _edges()
    for ci, (d, n, Q, K, col0) in enumerate(_cases()):
        rng = np.random.default_rng(100 * ci + FAMILIES.index(family))
        T = _table(family, n, d, rng)
        table, sqn = _place(T, col0)
        rows = rng.integers(0, n, size=Q)
        excl = None
        if n >= C - 1:                                   # fillers at a large n: query 0 keeps five candidates
            keep = set(rng.permutation(n)[:5].tolist())
            excl = [[i for i in range(n) if i not in keep]] + [[] for _ in range(Q - 1)]
        ids, vals = _run(table, sqn, rows, K, excl=excl)
        s = km.masked(km.cos64(T, rows), rows, True, excl)
        _check_lists(ids, vals, s, K, d, (family, d, n, Q, K))


def test_ties():
    T_, C = _edges()
    d, K = 32, 50
    n = C + 40
    rng = np.random.default_rng(7)
    base = rng.standard_normal((n // 4 + 1, d)).astype(np.float32)
    source = np.full(n, -1, dtype=np.int64)
    forced = {0: [15, 16, C - 1, C], 1: [14, 17, 31, 32, C + 1], 2: [C - 2, C + 16, C + 17]}    # copies either side of tile and chunk edges
    for src, at in forced.items():
        source[at] = src
    free, src = rng.permutation(np.flatnonzero(source < 0)), 3
    while free.size:
        c = min(int(rng.integers(3, 6)), free.size)
        source[free[:c]] = src
        free, src = free[c:], src + 1
    T = base[source]
    table, sqn = _place(T, 4)
    rows = np.asarray([15, C, 14, C - 2, 100, n - 1])
    ids, vals = _run(table, sqn, rows, K)
    s = km.masked(km.cos64(T, rows), rows)
    _check_lists(ids, vals, s, K, d, "ties")
    met = 0
    for b in range(len(rows)):
        by_src = {}
        for r, v in zip(ids[b], vals[b].view(np.int32)):
            by_src.setdefault(int(source[r]), []).append((int(r), int(v)))
        for got in by_src.values():
            assert len({v for _, v in got}) == 1, ("copies of a row carry one value", b, got)
            assert [r for r, _ in got] == sorted(r for r, _ in got)
            met += len(got) > 1
        # the query's own copies lead the list: cosine 1 up to rounding, all with one value, in id order
        own = [int(i) for i in np.flatnonzero(source == source[rows[b]]) if i != rows[b]]
        assert ids[b, :len(own)].tolist() == own
    assert met > 10
    # every row the same vector: ids 0 .. K - 1 without the excluded ones; all zeros: scores exactly 0 in id order
    for fill, n2, K2 in ((None, 40, 10), (0.0, 40, 10), (None, C + 3, 256), (0.0, 20, 50)):
        E = np.tile(rng.standard_normal((1, d)).astype(np.float32) if fill is None else np.zeros((1, d), np.float32), (n2, 1))
        table, sqn = _place(E, 3)
        rows2 = [0, 5, n2 - 1, 5]
        excl = [[1, 1, 3], [], [0], [6, 4]]
        ids, vals = _run(table, sqn, rows2, K2, excl=excl)
        for b, q in enumerate(rows2):
            want = [i for i in range(n2) if i != q and i not in excl[b]][:K2]
            assert ids[b, :len(want)].tolist() == want and (ids[b, len(want):] == -1).all(), (fill, n2, b)
            assert len(set(vals[b, :len(want)].view(np.int32).tolist())) == 1
            if fill is not None:
                assert (vals[b, :len(want)] == 0.0).all()


@pytest.mark.parametrize("exclude_self", [True, False])
def test_exclusions(exclude_self):
    d, n, K = 32, 300, 10
    rng = np.random.default_rng(11)
    T = _table("normal", n, d, rng)
    table, sqn = _place(T, 4)
    rows = [7, 8, 299, 0, 150, 7]
    excl = [rng.integers(0, n, size=40).tolist() + [3, 3, 3], [], [299, 1, 0], list(range(n)), list(range(n - 1, 4, -1)),
            list(range(0, n, 2)) * 2]
    assert not excl[1] and excl[0] and excl[2]
    ids, vals = _run(table, sqn, rows, K, exclude_self=exclude_self, excl=excl)
    s = km.masked(km.cos64(T, rows), rows, exclude_self, excl)
    _check_lists(ids, vals, s, K, d, ("exclusions", exclude_self))
    for b in range(len(rows)):
        assert not set(ids[b].tolist()) & set(excl[b]), b
        assert (rows[b] in ids[b].tolist()) == (not exclude_self and rows[b] not in excl[b]), b
    assert (ids[3] == -1).all() and np.isneginf(vals[3]).all()               # the list that names every row
    assert (ids[4] >= 0).sum() == 5                                          # rows 0 .. 4 are left (the query, row 150, is listed too)


@pytest.mark.parametrize("exclude_self", [True, False])
@pytest.mark.parametrize("K", [1, 64, 65, 256])
def test_rising_scores(K, exclude_self):
    """Every candidate beats the running threshold (knn_model.rising_case): every 16-row tile appends to every live list, the lists
    are cut in mid-chunk, a second chunk of 17 rows and the merge take part. The scores' gaps are far beyond the near-tie allowance
    (test_knn_cpu.py asserts it on the float64 model), so the ids are the model's exactly."""
    T_, C = _edges()
    d, n, Q = 32, C + 17, 17
    T, rows, excl = km.rising_case(n, d, Q)
    table, sqn = _place(T, 4)
    ids, vals = _run(table, sqn, rows, K, exclude_self=exclude_self, excl=excl)
    s = km.masked(km.cos64(T, rows), rows, exclude_self, excl)
    _check_lists(ids, vals, s, K, d, ("rising", K, exclude_self))
    assert np.array_equal(ids, km.topk64(s, K)[0])
    assert (n - 1 in ids[0].tolist()) == (not exclude_self) and not set(ids[1].tolist()) & set(excl[1])


def test_queries():
    from elimrec_amd import ops
    T_, C = _edges()
    d, n, K = 64, C + 100, 10
    rng = np.random.default_rng(13)
    T = _table("clustered", n, d, rng)
    table, sqn = _place(T, 4)
    before = table.clone()
    rows = rng.integers(0, n, size=T_ + 9)
    rows[5] = rows[40] = rows[T_ + 3] = rows[0]                               # a repeated query, in several tiles
    ids, vals = _run(table, sqn, rows, K)
    for b in (5, 40, T_ + 3):
        assert np.array_equal(ids[b], ids[0]) and np.array_equal(vals[b].view(np.int32), vals[0].view(np.int32))
    perm = rng.permutation(len(rows))
    ids_p, vals_p = _run(table, sqn, rows[perm], K)
    assert np.array_equal(ids_p, ids[perm]) and np.array_equal(vals_p.view(np.int32), vals[perm].view(np.int32))
    ids2, vals2 = _run(table, sqn, rows, K)
    assert np.array_equal(ids2, ids) and np.array_equal(vals2.view(np.int32), vals.view(np.int32))
    # a NeighbourQuery gives the same bits; sentinels behind [Q x K] stay
    excl = [[int(r)] if b % 3 == 0 else [] for b, r in enumerate((rows + 1) % n)]
    ids_e, vals_e = _run(table, sqn, rows, K, excl=excl)
    ptr, flat = km.csr(excl)
    query = ops.NeighbourQuery(rows, n, DEV, ptr, flat)
    idx = torch.full((len(rows) + 2, K), -7, dtype=torch.int32, device=DEV)
    val = torch.full((len(rows) + 2, K), 7.0, dtype=torch.float32, device=DEV)
    ws = torch.empty(ops.cosine_topk_workspace(len(rows), n, K) + 64, dtype=torch.uint8, device=DEV)
    ops.cosine_topk(table, sqn, query, K, idx, val, workspace=ws)
    assert np.array_equal(idx[:len(rows)].cpu().numpy(), ids_e) and np.array_equal(val[:len(rows)].cpu().numpy().view(np.int32), vals_e.view(np.int32))
    assert bool((idx[len(rows):] == -7).all()) and bool((val[len(rows):] == 7.0).all())
    flat1 = torch.full((len(rows) * K + 5,), -7, dtype=torch.int32, device=DEV)
    ops.cosine_topk(table, sqn, query, K, flat1)                              # 1-D output, no values
    assert np.array_equal(flat1[:len(rows) * K].cpu().numpy().reshape(-1, K), ids_e) and bool((flat1[len(rows) * K:] == -7).all())
    assert torch.equal(table, before)
    # the registered op: the same lists
    from elimrec_amd import torch_ops
    oi, ov = torch_ops.load().cosine_topk(table, sqn, _t(rows.astype(np.int32)), K, True)
    assert np.array_equal(oi.cpu().numpy(), ids) and np.array_equal(ov.cpu().numpy().view(np.int32), vals.view(np.int32))


def test_argument_checks():
    from elimrec_amd import ops
    n, d, K = 20, 8, 4
    T = _t(np.ones((n, d), np.float32))
    sq = _t(np.full(n, float(d), np.float32))
    idx = torch.full((2, K), -7, dtype=torch.int32, device=DEV)
    val = torch.full((2, K), 7.0, dtype=torch.float32, device=DEV)

    def call(table=T, sqn=sq, rows=(0, 1), k=K, oi=idx, ov=val, **kw):
        return ops.cosine_topk(table, sqn, np.asarray(rows, dtype=np.int32), k, oi, ov, **kw)
    for k in (0, 257):
        with pytest.raises(ValueError):
            call(k=k, oi=torch.empty(2, max(k, 1), dtype=torch.int32, device=DEV), ov=None)
    for bad_d in (6, 260):
        with pytest.raises(ValueError):
            call(table=_t(np.ones((n, bad_d), np.float32)))
    for rows in ((0, n), (-1, 0)):
        with pytest.raises(IndexError):
            call(rows=rows)
    for bad in ([n], [-1]):
        with pytest.raises(IndexError):
            call(excl_ptr=[0, 1, 1], excl_rows=bad)
    with pytest.raises(ValueError):
        call(workspace=torch.empty(16, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        call(oi=torch.empty(2, K + 1, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        call(oi=torch.empty(1, K, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        call(ov=torch.empty(2 * K - 1, dtype=torch.float32, device=DEV))
    with pytest.raises(TypeError):
        call(oi=torch.empty(2, K, dtype=torch.int64, device=DEV))
    with pytest.raises(TypeError):
        call(ov=torch.empty(2, K, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        call(sqn=sq[:-1])
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and bool((val == 7.0).all())               # nothing was launched
    call()
    assert idx.cpu().tolist() == [[1, 2, 3, 4], [0, 2, 3, 4]]


@pytest.mark.parametrize("K", [1, 10, 64, 256])
def test_list_overlap(K):
    from elimrec_amd import ops, torch_ops
    rng = np.random.default_rng(K)
    n = 11
    a = np.stack([rng.permutation(3 * K)[:K] for _ in range(n)]).astype(np.int32)
    b = np.stack([rng.permutation(3 * K)[:K] for _ in range(n)]).astype(np.int32)
    a[1, K // 2:] = -1                                                        # fillers at the tail of either list
    b[2, K // 3:] = -1
    a[3], b[3] = -1, -1                                                       # two empty lists: fillers never match
    b[4] = a[4] + 3 * K                                                       # disjoint
    b[5] = a[5]                                                               # identical
    b[6] = a[6][::-1]                                                         # identical up to order
    out = torch.full((n + 1,), -7, dtype=torch.int32, device=DEV)
    ops.list_overlap(_t(a), _t(b), out)
    want = km.overlap(a, b)
    assert out[:n].cpu().tolist() == want.tolist() and int(out[n]) == -7
    assert want[3] == 0 and want[4] == 0 and want[5] == K and want[6] == K
    assert torch_ops.load().list_overlap(_t(a), _t(b)).cpu().tolist() == want.tolist()


# --------------------------------------------------------------------------- the model on the fixtures
def _forward(name, extra=()):
    g = load_golden(name)
    model, _ = build_model_from_fixture(g, DEV, extra_argv=extra)
    model.bpr_loss(_t(g["step1/users"]), _t(g["step1/pos"]), _t(g["step1/neg"]))
    return model


@pytest.mark.parametrize("name", ["ml3", "kwai", "ablate"])
def test_similar_on_a_fixture(name):
    from elimrec_amd import Neighbours
    from elimrec_amd.evaluator import CandidateScoringError
    g = load_golden(name)
    fresh, _ = build_model_from_fixture(g, DEV)
    with pytest.raises(RuntimeError):
        fresh.similar_items([0], 3)
    model = _forward(name)
    U, I, d = model.num_users, model.num_items, model.latent_dim
    model.similar_items([0], 1)                                               # (the tables are realised before Y is read back)
    Y = model._ws["Y"].cpu().numpy()
    rng = np.random.default_rng(3)
    items = rng.permutation(I)[:min(I, 70)].tolist()
    k = 10
    for h, space in enumerate(["fused"] + list(model._mods)):
        got = model.similar_items(items, k, space=space)
        assert isinstance(got, Neighbours) and got.ids.dtype == torch.int32 and got.scores.dtype == torch.float32
        assert got.ids.device.type == "cpu" and tuple(got.ids.shape) == tuple(got.scores.shape) == (len(items), k)
        block = Y[U:U + I, h * d:(h + 1) * d]
        s = km.masked(km.cos64(block, items), items)
        _check_lists(got.ids.numpy(), got.scores.numpy(), s, k, d, (name, space))
        assert all(q not in row for q, row in zip(items, got.ids.tolist()))
    users = rng.permutation(U)[:min(U, 70)].tolist()
    got = model.similar_users(users, k)
    _check_lists(got.ids.numpy(), got.scores.numpy(), km.masked(km.cos64(Y[:U, :d], users), users), k, d, (name, "users"))
    # exclude: the first neighbours of the plain call are left out of the second
    plain = model.similar_items(items[:5], k)
    exclude = {items[b]: plain.ids[b, :3].tolist() + [items[b]] for b in range(4)}
    got = model.similar_items(items[:5], k, exclude=exclude)
    s = km.masked(km.cos64(Y[U:U + I, :d], items[:5]), items[:5], True, [exclude.get(i, []) for i in items[:5]])
    _check_lists(got.ids.numpy(), got.scores.numpy(), s, k, d, (name, "exclude"))
    for b in range(4):
        assert not set(got.ids[b].tolist()) & set(exclude[items[b]])
    assert torch.equal(got.ids[4], plain.ids[4])
    # errors
    for space in ("x", "fusion", None) + (("a", "t") if name == "kwai" else ()):
        with pytest.raises(ValueError):
            model.similar_items([0], 3, space=space)
    with pytest.raises(IndexError):
        model.similar_items([I], 3)
    with pytest.raises(IndexError):
        model.similar_users([0], 3, exclude={0: [U]})
    with pytest.raises(ValueError):
        model.similar_items([0], 0)
    model._eval_shard = object()
    try:
        with pytest.raises(CandidateScoringError):
            model.similar_items([0], 3)
    finally:
        model._eval_shard = None
    assert tuple(model.similar_items([], 3).ids.shape) == (0, 3)


def _mean_1ulp(got, want, what):
    err = np.abs(got.astype(np.float64) - want)
    ok = (err <= np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)) | (np.isnan(want) & np.isnan(got))
    assert ok.all(), (what, got, want)


@pytest.mark.parametrize("view", [None, [1, 10]])
def test_neighbour_report(view):
    from elimrec_amd import ops
    from elimrec_amd.evaluator import NeighbourReport
    model = _forward("ml3")
    train = model.dataset.get_user_train_dict()
    k, I = 7, model.num_items
    report = NeighbourReport(model.dataset, train, k, item_group_view=view)
    report.block_items = (I + 1) // 2                                         # two item blocks
    final, buf = report.evaluate(model)
    columns = ops.neighbour_columns(model._mods)
    spaces = ["fused"] + list(model._mods)
    lists = [model.similar_items(list(range(I)), k, space=sp) for sp in spaces]
    ids = np.stack([x.ids.numpy() for x in lists])
    vals = np.stack([x.scores.numpy() for x in lists])
    rows = km.report_rows(ids, vals, report.item_counts, k)
    got_rows = report.neighbour_rows(model)[0].cpu().numpy()
    S = len(model._mods)
    assert np.array_equal(got_rows[:, :S], rows[:, :S]) and np.array_equal(got_rows[:, 2 * S + 1:], rows[:, 2 * S + 1:])   # overlap, pop
    want = km.report_means(rows, report._positions)
    assert final.dtype == np.float32 and final.shape == (len(report.group_labels), len(columns)) == want.shape
    assert (len(report.group_labels) > 1) == (view is not None)
    for gi in range(final.shape[0]):
        _mean_1ulp(final[gi], want[gi], report.group_labels[gi])
    lines = buf.split("\n")
    assert len(lines) == 1 + len(report.group_labels) and lines[0].startswith("columns:") and lines[1].startswith("all:")
    assert all(c in lines[0] for c in columns) and [ln[:12] for ln in lines[1:]] == [x[:12] for x in report.group_labels]


# --------------------------------------------------------------------------- the driver's switch
def _net(tmp_path, extra, shape="[60,200,1200]"):
    import importlib
    import sys
    sys.path.insert(0, ROOT)
    main = importlib.import_module("main")
    from elimrec_amd import Configurator, set_seed
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        args = Configurator(os.path.join(ROOT, "NeuRec.properties"), default_section="hyperparameters",
                            argv=["main.py", "--data.input.dataset=synthetic", "--alpha=0.5", "--synthetic_shape=" + shape,
                                  "--synthetic_dims=[16,8,12]", "--recdim=32", "--loss=bpr_loss", "--batch_size=512", "--num_epoch=2",
                                  "--test_step=1", "--verbose=0", "--save_flag=0", "--path=%s" % str(tmp_path / "ck")] + list(extra))
        set_seed(args["seed"])
        return main.Net(args)
    finally:
        os.chdir(cwd)


class _Capture(object):
    def __init__(self):
        self.lines = []

    def log(self, *msg):
        self.lines.append("\t".join(str(m) for m in msg))


def _driver(tmp_path, extra):
    """(lines Net.test_all_effects() logs after a two-epoch synthetic run, evaluate()[0], test()[0])."""
    from elimrec_amd import Logger
    net = _net(tmp_path, extra)
    before = Logger.logger
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        net.run()
        cap = Logger.logger = _Capture()
        net.test_all_effects()
        rec = net.recommender
        rec.predict_type = "TIE"
        return cap.lines, np.asarray(rec.evaluate()[0]), np.asarray(rec.test()[0])
    finally:
        os.chdir(cwd)
        Logger.logger = before


def test_driver_switch(tmp_path):
    from elimrec_amd import ops
    off, ev0, te0 = _driver(tmp_path / "a", [])
    assert len(off) == 2 and not any("[neighbours]" in ln for ln in off)
    on, ev1, te1 = _driver(tmp_path / "b", ["--neighbour_report=5", "--item_group_view=[1,4]"])
    assert on[:2] == off and len(on) == 3
    table = on[2]
    assert table.startswith("  [neighbours] top-5 ") and "columns:" in table and "\nall:" in table
    assert all(c in table for c in ops.neighbour_columns(("v", "a", "t")))
    assert len(table.split("\n")) >= 4                                       # header line, columns, all, at least one item group
    assert ev0.tobytes() == ev1.tobytes() and te0.tobytes() == te1.tobytes()
