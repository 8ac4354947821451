"""The list kernels on the device (csrc/lists.hip) against the float64 model of tests/lists_model.py, and what is built on them:
EliMRec.list_similarity, evaluator.ListReport, --list_report.

Tolerance of a list's mean pairwise cosine: knn_model.tol(d) + 2^-23 -- every pair's fp32 score lies within tol(d) of its float64
value (derived in knn_model.tol), so their mean does; the float64 sum adds nothing visible and the result is rounded once to fp32
(|mean| <= 1 + tol: half an ulp is at most 2^-24, taken twice). Derived, not measured. The table is a column block of a wider
matrix whose other columns and neighbouring rows hold NaN, the squared norms sit inside a NaN matrix too: a read outside the slice
shows up as NaN."""
import os

import numpy as np
import pytest
import torch

import knn_model as km
import lists_model as lm
from helpers import ROOT, build_model_from_fixture, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FAMILIES = ("normal", "scaled", "clustered")
SENTINEL = 7.0


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _tol(d):
    return km.tol(d) + 2.0 ** -23


def _table(family, n, width, rng):
    x = rng.standard_normal((n, width))
    if family == "scaled":
        x = x * np.exp(rng.uniform(-8, 8, size=(n, 1)))
    elif family == "clustered":
        x = rng.standard_normal((1, width)) + 0.05 * x
    return x.astype(np.float32)


def _sq32(T, blocks):
    d = T.shape[1] // blocks
    return np.stack([(T[:, h * d:(h + 1) * d].astype(np.float64) ** 2).sum(1) for h in range(blocks)], 1).astype(np.float32)


def _place(T, blocks, col0):
    """T [n x blocks * d] at row 2, column col0 of a wider NaN matrix (col0 = 3: rows not 16-byte aligned; 4: aligned) and its
    squared norms [n x blocks] at row 1, column 1 of a NaN matrix. -> (table view, sqnorm view, float32 squared norms)."""
    n, width = T.shape
    wide = np.full((n + 3, width + col0 + 4), np.nan, dtype=np.float32)
    wide[2:2 + n, col0:col0 + width] = T
    sq = _sq32(T, blocks)
    sqw = np.full((n + 2, blocks + 2), np.nan, dtype=np.float32)
    sqw[1:1 + n, 1:1 + blocks] = sq
    return _t(wide)[2:2 + n, col0:col0 + width], _t(sqw)[1:1 + n, 1:1 + blocks], sq


def _run(table, sqn, lists, blocks, extra_rows=2):
    from elimrec_amd import ops
    lists = np.ascontiguousarray(lists, dtype=np.int32)
    B = lists.shape[0]
    out = torch.full((B + extra_rows, blocks), SENTINEL, dtype=torch.float32, device=DEV)
    ops.list_pair_cosine(table, sqn, _t(lists), out, blocks=blocks)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert (out[B:] == SENTINEL).all(), "rows beyond B were written"
    return out[:B]


def _check(got, want, d, what):
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    diff = np.abs(got.astype(np.float64) - want)
    err = float(diff[~np.isnan(diff)].max()) if (~np.isnan(diff)).any() else 0.0
    print("list_pair_cosine %s: max |err| %.3e, bound %.3e" % (what, err, _tol(d)))
    assert err <= _tol(d), (what, err, _tol(d))


def _cases():
    from elimrec_amd import ops
    S = ops.LIST_SMALL_K
    return [  # d, blocks, K, B, column offset
        (4, 1, 1, 1, 3), (4, 2, 2, 3, 4), (36, 4, 15, 3, 3), (36, 1, 16, 1, 4), (64, 2, 17, 3, 3), (64, 4, S - 1, 1, 4),
        (128, 1, S, 3, 3), (128, 2, S + 1, 3, 4), (256, 1, 50, 3, 3), (64, 4, 50, 3, 4), (256, 2, 255, 1, 4), (64, 1, 256, 3, 3),
        (128, 4, 256, 1, 4), (36, 2, 256, 3, 3), (256, 1, 256, 3, 4), (4, 4, 33, 3, 3), (64, 1, 31, 3, 4), (36, 1, 32, 3, 3),
    ]


def test_cases_cover_the_issue():
    from elimrec_amd import ops
    cases = _cases()
    S = ops.LIST_SMALL_K
    assert {c[0] for c in cases} == {4, 36, 64, 128, 256} and {c[1] for c in cases} == {1, 2, 4}
    assert {c[2] for c in cases} >= {1, 2, 15, 16, 17, 31, 32, 33, 50, 255, 256, S - 1, S, S + 1} and {c[3] for c in cases} == {1, 3}
    assert {c[4] for c in cases} == {3, 4}
    # the LDS chunking: lists whose rows go in one stage, in several, and in several with a narrower last one
    chunks = {(c[0] == ops.list_chunk_cols(c[2], c[0]), c[0] % ops.list_chunk_cols(c[2], c[0]) == 0) for c in cases}
    assert chunks >= {(True, True), (False, False)}
    assert any(c[0] > 2 * ops.list_chunk_cols(c[2], c[0]) for c in cases)


@pytest.mark.parametrize("family", FAMILIES)
def test_pair_cosine_against_float64(family):
    for ci, (d, blocks, K, B, col0) in enumerate(_cases()):
        rng = np.random.default_rng(100 * ci + FAMILIES.index(family))
        n = 300 if K > 64 else 90
        T = _table(family, n, blocks * d, rng)
        zero = int(rng.integers(0, n))
        T[zero] = 0.0
        table, sqn, sq = _place(T, blocks, col0)
        lists = np.stack([rng.permutation(n)[:K] for _ in range(B)])
        for b in range(B):
            if zero not in lists[b]:
                lists[b, int(rng.integers(0, K))] = zero                  # the all-zero row is listed
        got = _run(table, sqn, lists, blocks)
        _check(got, lm.pair_cosine64(T, sq, lists, blocks), d, (family, d, blocks, K, B))
        assert np.isnan(got).all() == (K == 1)


def test_list_contents():
    d, blocks, K, n = 64, 2, 20, 50
    rng = np.random.default_rng(21)
    T = _table("normal", n, blocks * d, rng)
    T[9] = 0.0
    table, sqn, sq = _place(T, blocks, 3)
    full = rng.permutation(n)[:K]
    full[4] = 9
    tail = full.copy()
    tail[13:] = -1
    middle = full.copy()
    middle[[0, 3, 7, 8, 16]] = -1
    nothing = np.full(K, -1)
    single = nothing.copy()
    single[11] = 5
    dup = full.copy()
    dup[[1, 2, 17]] = dup[0]
    same = np.full(K, 6)
    outside = full.copy()
    outside[[0, 5, 19]] = [n, n + 5, -2]
    huge = full.copy()
    huge[[2, 3]] = [np.iinfo(np.int32).max, np.iinfo(np.int32).min]
    lists = np.stack([full, tail, middle, nothing, single, dup, same, outside, huge])
    got = _run(table, sqn, lists, blocks)
    want = lm.pair_cosine64(T, sq, lists, blocks)
    _check(got, want, d, "contents")
    assert np.isnan(got[3]).all() and np.isnan(got[4]).all() and not np.isnan(np.delete(got, [3, 4], 0)).any()
    assert np.abs(got[6] - 1.0).max() <= _tol(d)                             # a pair of equal ids is a pair
    # not listed = left out, wherever it stands: the same list without those entries
    for row, kept in ((2, middle[middle >= 0]), (7, np.delete(outside, [0, 5, 19]))):
        alone = _run(table, sqn, kept[None, :], blocks)
        assert np.abs(alone[0].astype(np.float64) - got[row]).max() <= 2 * _tol(d)
        _check(alone, want[row:row + 1], d, ("compacted", row))
    # a table of no rows: nothing is listed
    from elimrec_amd import ops
    out = torch.full((2, 1), SENTINEL, dtype=torch.float32, device=DEV)
    ops.list_pair_cosine(torch.empty(0, 8, device=DEV), torch.empty(0, 1, device=DEV), _t(np.asarray([[0, 1, 2]], np.int32)), out)
    assert np.isnan(out[0].cpu().numpy()).all() and float(out[1]) == SENTINEL
    # 1-D squared norms (blocks = 1), 1-D output, B = 0
    t1, s1, q1 = _place(T[:, :d], 1, 4)
    flat = torch.full((len(lists) + 3,), SENTINEL, dtype=torch.float32, device=DEV)
    ops.list_pair_cosine(t1, s1[:, 0], _t(lists.astype(np.int32)), flat)
    assert np.array_equal(flat.cpu().numpy()[:len(lists)].view(np.int32), _run(t1, s1, lists, 1)[:, 0].view(np.int32))
    assert bool((flat[len(lists):] == SENTINEL).all())
    ops.list_pair_cosine(t1, s1, torch.empty(0, K, dtype=torch.int32, device=DEV), flat)
    assert bool((flat[len(lists):] == SENTINEL).all())


@pytest.mark.parametrize("K", [10, 50, 256])
def test_determinism(K):
    d, blocks, n, B = 128, 2, 300, 5
    rng = np.random.default_rng(K)
    T = _table("clustered", n, blocks * d, rng)
    table, sqn, _ = _place(T, blocks, 4)
    lists = np.stack([rng.permutation(n)[:K] for _ in range(B)])
    lists[1, K // 2:] = -1
    lists[3, ::3] = lists[3, 0]
    got = _run(table, sqn, lists, blocks)
    again = _run(table, sqn, lists, blocks)
    assert np.array_equal(got.view(np.int32), again.view(np.int32))
    filler = rng.permutation(n)[:K]
    for b in range(B):
        alone = _run(table, sqn, lists[b:b + 1], blocks)
        assert np.array_equal(alone[0].view(np.int32), got[b].view(np.int32)), b
        moved = _run(table, sqn, np.stack([filler, filler[::-1], lists[b], filler]), blocks)
        assert np.array_equal(moved[2].view(np.int32), got[b].view(np.int32)), b


def test_argument_checks():
    from elimrec_amd import ops
    n, d, K = 20, 8, 4
    T = _t(np.ones((n, 2 * d), np.float32))
    sq = _t(np.full((n, 2), float(d), np.float32))
    lists = _t(np.tile(np.arange(K, dtype=np.int32), (2, 1)))
    out = torch.full((2, 2), SENTINEL, dtype=torch.float32, device=DEV)

    def call(table=T, sqn=sq, ls=lists, o=out, blocks=2):
        return ops.list_pair_cosine(table, sqn, ls, o, blocks=blocks)
    for blocks in (0, 9, 3):
        with pytest.raises(ValueError):
            call(blocks=blocks)
    for bad_d in (6, 260):
        with pytest.raises(ValueError):
            call(table=_t(np.ones((n, bad_d), np.float32)), sqn=sq[:, :1], blocks=1)
    with pytest.raises(ValueError):
        call(ls=torch.zeros(2, ops.LIST_MAX_K + 1, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        call(ls=lists.t())
    with pytest.raises(TypeError):
        call(ls=lists.long())
    with pytest.raises(ValueError):
        call(sqn=sq[:-1])
    with pytest.raises(ValueError):
        call(sqn=sq[:, 0])
    with pytest.raises(ValueError):
        call(o=torch.empty(1, 2, dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        call(o=torch.empty(2, 3, dtype=torch.float32, device=DEV))
    with pytest.raises(TypeError):
        call(o=torch.empty(2, 2, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        ops.list_exposure(lists, torch.zeros(2, 2, dtype=torch.int32, device=DEV))
    with pytest.raises(TypeError):
        ops.list_exposure(lists, torch.zeros(4, dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())                                       # nothing was launched
    call()
    assert np.abs(out.cpu().numpy() - 1.0).max() <= _tol(d)
    # the C entry point refuses what the wrapper refuses, with the library's argument error code
    from elimrec_amd import _lib
    raw = _lib.load().elimrec_list_pair_cosine
    for kw in (dict(K=0), dict(K=257), dict(d=6), dict(d=260), dict(blocks=0), dict(blocks=9), dict(B=-1)):
        a = dict(K=K, d=d, blocks=2, B=2)
        a.update(kw)
        rc = raw(T.data_ptr(), 2 * d, n, a["blocks"], a["d"], sq.data_ptr(), 2, lists.data_ptr(), a["B"], a["K"], out.data_ptr(), None)
        assert rc == 10001, (kw, rc)                                           # ELIMREC_E_BADARG
    assert raw(T.data_ptr(), 2 * d, n, 2, d, sq.data_ptr(), 2, None, 0, K, None, None) == 0   # B == 0 launches nothing


def test_exposure():
    from elimrec_amd import ops
    rng = np.random.default_rng(4)
    n, B, K = 257, 133, 10
    lists = rng.integers(0, n, size=(B, K)).astype(np.int32)
    lists[5, 3:] = -1
    lists[6] = [n, n + 5, -2, 0, 0, 0, n - 1, n - 1, -1, 2 ** 31 - 1]
    counts = torch.zeros(n + 3, dtype=torch.int32, device=DEV)
    counts[n:] = -7
    ops.list_exposure(_t(lists), counts[:n])
    want = lm.exposure(lists, n)
    assert counts[:n].cpu().tolist() == want.tolist() and counts[n:].cpu().tolist() == [-7, -7, -7]
    assert int(want.sum()) == int(((lists >= 0) & (lists < n)).sum()) < B * K
    more = rng.integers(-3, n + 3, size=(40, 3)).astype(np.int32)
    ops.list_exposure(_t(more), counts[:n])                                    # accumulates
    assert counts[:n].cpu().tolist() == (want + lm.exposure(more, n)).tolist() and counts[n:].cpu().tolist() == [-7, -7, -7]
    hot = np.zeros((4096, 1), dtype=np.int32)                                  # contention: every list names item 0
    c2 = torch.zeros(5, dtype=torch.int32, device=DEV)
    ops.list_exposure(_t(hot), c2)
    assert c2.cpu().tolist() == [4096, 0, 0, 0, 0]
    ops.list_exposure(torch.empty(0, 4, dtype=torch.int32, device=DEV), c2)
    assert c2.cpu().tolist() == [4096, 0, 0, 0, 0]


def test_torch_ops():
    from elimrec_amd import torch_ops
    t = torch_ops.load()
    rng = np.random.default_rng(8)
    for d, blocks, K, col0 in ((36, 2, 17, 3), (64, 4, 50, 4), (128, 1, 256, 3)):
        n = 300
        T = _table("normal", n, blocks * d, rng)
        table, sqn, _ = _place(T, blocks, col0)
        lists = np.stack([rng.permutation(n)[:K] for _ in range(3)]).astype(np.int32)
        lists[1, K // 2:] = -1
        lists[2, 0] = n
        got = t.list_pair_cosine(table, sqn, _t(lists), blocks)
        assert tuple(got.shape) == (3, blocks) and got.dtype == torch.float32
        assert np.array_equal(got.cpu().numpy().view(np.int32), _run(table, sqn, lists, blocks).view(np.int32))
        counts = t.list_exposure(_t(lists), n)
        assert counts.dtype == torch.int32 and counts.cpu().tolist() == lm.exposure(lists, n).tolist()
    assert tuple(t.list_pair_cosine(table, sqn, torch.empty(0, 5, dtype=torch.int32, device=DEV), 1).shape) == (0, 1)
    with pytest.raises(RuntimeError):
        t.list_pair_cosine(table, sqn, _t(lists), 3)


# --------------------------------------------------------------------------- the model on the fixtures
def _forward(name, extra=()):
    g = load_golden(name)
    model, _ = build_model_from_fixture(g, DEV, extra_argv=extra)
    model.bpr_loss(_t(g["step1/users"]), _t(g["step1/pos"]), _t(g["step1/neg"]))
    return model


def _item_block(model):
    """(the item rows of the cached Y as float32 [I x (1 + S) d], their float32 squared norms [I x 1 + S])."""
    U, I, d, nb = model.num_users, model.num_items, model.latent_dim, 1 + model.S
    Y = model._ws["Y"].cpu().numpy()[U:U + I, :nb * d]
    return Y, _sq32(Y, nb)


@pytest.mark.parametrize("name", ["ml3", "kwai", "ablate"])
def test_list_similarity_on_a_fixture(name):
    from elimrec_amd.evaluator import CandidateScoringError
    g = load_golden(name)
    fresh, _ = build_model_from_fixture(g, DEV)
    with pytest.raises(RuntimeError):
        fresh.list_similarity([[0, 1]])
    model = _forward(name)
    I, d, nb = model.num_items, model.latent_dim, 1 + model.S
    model.list_similarity([[0, 1]])                                            # (the tables are realised before Y is read back)
    Y, sq = _item_block(model)
    rng = np.random.default_rng(3)
    lists = [rng.permutation(I)[:int(k)].tolist() for k in rng.integers(0, min(I, 40), size=30)] + [[], [3], [2, 2], [0, 1]]
    K = max(len(x) for x in lists)
    padded = np.full((len(lists), K), -1, dtype=np.int64)
    for b, x in enumerate(lists):
        padded[b, :len(x)] = x
    want = lm.pair_cosine64(Y, sq, padded, nb)
    got = model.list_similarity(lists)
    assert got.dtype == torch.float32 and got.device.type == "cpu" and tuple(got.shape) == (len(lists), nb)
    _check(got.numpy(), want, d, (name, "all spaces"))
    for h, space in enumerate(["fused"] + list(model._mods)):
        one = model.list_similarity(lists, space=space)
        assert tuple(one.shape) == (len(lists),)
        assert np.array_equal(one.numpy().view(np.int32), got[:, h].numpy().view(np.int32)), space
    for space in ("x", "fusion") + (("a", "t") if name == "kwai" else ()):
        with pytest.raises(ValueError):
            model.list_similarity(lists, space=space)
    for bad in ([[0, I]], [[-1, 0]], [[0, 1], [I + 5]]):
        with pytest.raises(IndexError):
            model.list_similarity(bad)
    with pytest.raises(ValueError):
        model.list_similarity_device(_t(padded.astype(np.int32)), torch.empty(len(lists), nb, device=DEV), side="items")
    model._eval_shard = object()
    try:
        with pytest.raises(CandidateScoringError):
            model.list_similarity([[0, 1]])
    finally:
        model._eval_shard = None
    assert tuple(model.list_similarity([]).shape) == (0, nb) and tuple(model.list_similarity([], space="fused").shape) == (0,)
    users = model.list_similarity_device(_t(np.asarray([[0, 1, 2]], np.int32)), torch.empty(1, nb, device=DEV), side="user").cpu().numpy()
    Yu = model._ws["Y"].cpu().numpy()[:model.num_users, :nb * d]
    _check(users, lm.pair_cosine64(Yu, _sq32(Yu, nb), [[0, 1, 2]], nb), d, (name, "users"))


def _mean_1ulp(got, want, what):
    err = np.abs(got.astype(np.float64) - want)
    ok = (err <= np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)) | (np.isnan(want) & np.isnan(got))
    assert ok.all(), (what, got, want)


@pytest.mark.parametrize("views", [(None, None), ([2, 4], [1, 10])])
def test_list_report(views):
    from elimrec_amd import ops
    from elimrec_amd.evaluator import EXPOSURE_COLUMNS, CandidateScoringError, ListReport, ListTables, exposure_summary
    model = _forward("ml3")
    train, test = model.dataset.get_user_train_dict(), model.dataset.get_user_test_dict()
    K, I, nb, d = 7, model.num_items, 1 + model.S, model.latent_dim
    report = ListReport(model.dataset, train, test, K, group_view=views[0], item_group_view=views[1])
    report.block_users = (len(report.users) + 1) // 2                          # two user blocks
    assert len(report.users) > 2
    model.predict_type = "TIE"
    rows, columns, lists, counts = report.list_rows(model)
    assert columns == ops.list_columns(model._mods) and rows.dtype == torch.float32 and lists.dtype == counts.dtype == torch.int32
    assert tuple(rows.shape) == (len(report.users), nb + 1) and tuple(lists.shape) == (len(report.users), K) and tuple(counts.shape) == (I,)
    # the lists are predict_device's
    tl = [train.get(u, []) for u in report.users]
    tptr = _t(np.cumsum([0] + [len(x) for x in tl]).astype(np.int64))
    titems = _t(np.asarray([i for x in tl for i in x], dtype=np.int32))
    idx = model.predict_device(_t(np.asarray(report.users, dtype=np.int64)), top_k=K, train_ptr=tptr, train_items=titems)[0]
    assert torch.equal(idx, lists)
    lists_h, rows_h = lists.cpu().numpy(), rows.cpu().numpy()
    Y, sq = _item_block(model)
    _check(rows_h[:, :nb], lm.pair_cosine64(Y, sq, lists_h, nb), d, "report ils")
    want_rows = lm.rows(rows_h[:, :nb], lists_h, report.item_counts)
    assert np.array_equal(rows_h[:, nb], want_rows[:, nb])                     # pop is exact
    assert counts.cpu().tolist() == lm.exposure(lists_h, I).tolist()           # so are the counters
    final, buf = report.evaluate(model)
    assert isinstance(final, ListTables) and final.user_columns == columns and final.item_columns == EXPOSURE_COLUMNS
    assert final.user_labels == report.group_labels and final.item_labels == report.item_labels
    assert (len(final.user_labels) > 1) == (views[0] is not None) and (len(final.item_labels) > 1) == (views[1] is not None)
    want = lm.means(rows_h, report._positions)
    assert final.users.dtype == np.float32 and final.users.shape == want.shape
    for gi in range(want.shape[0]):
        _mean_1ulp(final.users[gi], want[gi], report.group_labels[gi])
    assert final.items.dtype == np.float64
    assert np.array_equal(final.items, exposure_summary(lm.exposure(lists_h, I), report._item_positions))
    assert np.allclose(final.items, lm.exposure_summary_loops(lm.exposure(lists_h, I), report._item_positions), rtol=0, atol=1e-12)
    assert final.items[0, 0] == I and abs(final.items[0, 4] - 1.0) < 1e-15
    lines = buf.split("\n")
    nu, ni = len(report.group_labels), len(report.item_labels)
    assert len(lines) == 2 + nu + ni and lines[0].startswith("columns:") and lines[1].startswith("all:")
    assert all(c in lines[0] for c in columns) and [ln[:12] for ln in lines[1:1 + nu]] == [x[:12] for x in report.group_labels]
    assert lines[1 + nu].startswith("columns:") and all(c in lines[1 + nu] for c in EXPOSURE_COLUMNS)
    assert [ln[:12] for ln in lines[2 + nu:]] == [x[:12] for x in report.item_labels]
    # TE -> TIE
    model.predict_type = "TE"
    rows_a, _, lists_a, _ = report.list_rows(model)
    shift, sbuf = report.shift(rows_a, lists_a, rows, lists)
    assert report.shift_columns == ("overlap",) + tuple("d_" + c for c in columns)
    srows = lm.shift_rows(rows_a.cpu().numpy(), lists_a.cpu().numpy(), rows_h, lists_h)
    swant = lm.means(srows, report._positions)
    assert shift.dtype == np.float32 and shift.shape == swant.shape
    for gi in range(swant.shape[0]):
        _mean_1ulp(shift[gi], swant[gi], ("shift", report.group_labels[gi]))
    same, _ = report.shift(rows, lists, rows, lists)
    assert (same[:, 0] == 1.0).all() and (same[:, 1:] == 0.0).all()
    slines = sbuf.split("\n")
    assert len(slines) == 1 + nu and slines[0].startswith("columns:") and "overlap" in slines[0] and "d_pop" in slines[0]
    with pytest.raises(ValueError):
        report.shift(rows, lists[:, :-1], rows, lists[:, :-1])
    model._eval_shard = object()
    try:
        with pytest.raises(CandidateScoringError):
            report.evaluate(model)
    finally:
        model._eval_shard = None


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
    from elimrec_amd.evaluator import EXPOSURE_COLUMNS
    view = ["--group_view=[10,30]", "--item_group_view=[1,4]"]
    off, ev0, te0 = _driver(tmp_path / "a", view + ["--rank_report=1", "--neighbour_report=3"])
    assert not any("lists" in ln.split("\n")[0] or "list shift" in ln for ln in off)
    on, ev1, te1 = _driver(tmp_path / "b", view + ["--rank_report=1", "--neighbour_report=3", "--list_report=5"])
    added = [k for k, ln in enumerate(on) if ln.startswith("  [TE] top-5 lists: similarity, popularity, exposure:\n")
             or ln.startswith("  [TIE] top-5 lists: similarity, popularity, exposure:\n") or ln.startswith("  [TE->TIE] list shift:\n")]
    assert len(added) == 3 and [ln for k, ln in enumerate(on) if k not in added] == off
    te, tie, shift = added
    assert on[te].startswith("  [TE] top-5") and on[tie].startswith("  [TIE] top-5") and on[shift].startswith("  [TE->TIE] list shift")
    assert "catalogue rank" in on[te - 1] and on[te - 1].startswith("  [TE]") and on[te + 1].startswith("  [TIE]\t")
    assert "catalogue rank" in on[tie - 1] and on[tie - 1].startswith("  [TIE]")
    assert on[shift - 1].startswith("  [TE->TIE] rank shift") and on[shift + 1].startswith("  [neighbours]") and shift == len(on) - 2
    for k in (te, tie):
        assert all(c in on[k] for c in ops.list_columns(("v", "a", "t")) + EXPOSURE_COLUMNS) and "\nall:" in on[k] and "\nitem " in on[k]
    assert "overlap" in on[shift] and "d_ils_fused" in on[shift] and "d_pop" in on[shift]
    assert ev0.tobytes() == ev1.tobytes() and te0.tobytes() == te1.tobytes()
    plain_off, ev2, te2 = _driver(tmp_path / "c", [])
    plain_on, ev3, te3 = _driver(tmp_path / "d", ["--list_report=5"])
    assert len(plain_off) == 2 and len(plain_on) == 5 and [plain_on[0], plain_on[2]] == plain_off
    assert plain_on[1].startswith("  [TE] top-5 lists") and plain_on[3].startswith("  [TIE] top-5 lists") and plain_on[4].startswith("  [TE->TIE] list shift")
    assert ev2.tobytes() == ev3.tobytes() and te2.tobytes() == te3.tobytes()
