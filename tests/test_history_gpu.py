"""History support on the device: the kernel (csrc/history.hip) against the float64 model of tests/history_model.py, and what is
built on it: EliMRec.history_support_device / explain_history, reports.HistoryReport, --history_report.

Tolerance of a score, tol = 4 (d + 8) 2^-24 * sum_b |w_b|: the worst-case fp32 bound derived in test_rerank_gpu.py's header
((2 d + 8) u for one cosine, u = 2^-24; twice that for a comparison of two), times the weight sum. A bound, not a measurement: a
reported score is off by at most tol / 2, the list reaches no more than tol below the float64 top-th score, and where the float64
gap of a slot to every entry under another id exceeds tol the kernel must name the float64 id. The share of slots that gap does
not decide is capped at 0.02 for d <= 64 and 0.10 for d = 256 (test_history_cpu.py holds the model itself to the same caps on
these inputs). The tables are column slices of wider matrices whose other columns and neighbouring rows hold NaN, the squared
norms strided columns of a NaN matrix, and every output lies between canaries: a read or a write outside shows up."""
import functools

import numpy as np
import pytest
import torch

import history_model as hm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY_I, CANARY_F, PAD = 77, 7.0, 5
IDS = lambda c: "d%d_b%d_K%d_top%d_B%d" % (c[0], c[1], c[3], c[4], c[5])     # noqa: E731


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _tables(d, blocks, col0=4):
    """hm.item_rows(d, blocks) at row 2, column col0 of a wider NaN matrix (col0 = 3: the base is not 16-byte aligned and
    ld % 4 != 0), the squared norms at row 1, column 1 of a NaN matrix -> (table view, norms view)."""
    X = hm.item_rows(d, blocks)
    rows = X.shape[0]
    sq = (X.astype(np.float64).reshape(rows, blocks, d) ** 2).sum(2).astype(np.float32)
    wide = np.full((rows + 3, blocks * d + col0 + 4), np.nan, dtype=np.float32)
    wide[2:2 + rows, col0:col0 + blocks * d] = X
    sqw = np.full((rows + 2, blocks + 2), np.nan, dtype=np.float32)
    sqw[1:1 + rows, 1:1 + blocks] = sq
    view, norms = _t(wide)[2:2 + rows, col0:col0 + blocks * d], _t(sqw)[1:1 + rows, 1:1 + blocks]
    assert (view.data_ptr() % 16 == 0) == (col0 == 4) and (view.stride(0) % 4 == 0) == (col0 == 4)
    return view, norms


@functools.lru_cache(maxsize=None)
def _index(case):
    from elimrec_amd import ops
    _, _, ptr, items = hm.case_inputs(case)
    return ops.HistoryIndex(ptr, items, DEV)


def _run(tabs, w, users, lists, hist, top, exclude_self, outputs=4):
    """One launch with canaries in front of and behind every output -> (idx int32 [B x K x top], val, cnt int32 [B x K], mean)."""
    from elimrec_amd import ops
    B, K = lists.shape
    sizes = (B * K * top, B * K * top, B * K, B * K)
    kinds = ((CANARY_I, torch.int32), (CANARY_F, torch.float32), (CANARY_I, torch.int32), (CANARY_F, torch.float32))
    flat = [torch.full((n + 2 * PAD,), c, dtype=dt, device=DEV) for n, (c, dt) in zip(sizes, kinds)]
    views = [f[PAD:PAD + n] for f, n in zip(flat, sizes)]
    ops.history_support(tabs[0], tabs[1], list(w), _t(np.asarray(users, dtype=np.int64)), _t(np.asarray(lists, dtype=np.int32)), hist, top,
                        views[0], views[1], *(views[2:] if outputs == 4 else ()), exclude_self=exclude_self)
    torch.cuda.synchronize()
    out = []
    for f, n, (c, _), shape in zip(flat[:outputs], sizes, kinds, ((B, K, top), (B, K, top), (B, K), (B, K))):
        a = f.cpu().numpy()
        assert (a[:PAD] == c).all() and (a[PAD + n:] == c).all(), "entries outside the output were written"
        out.append(a[PAD:PAD + n].reshape(shape))
    return out


def _verify(case, exclude_self, got, what):
    """Every check of the header for one launch against the case's float64 result."""
    d, blocks, w, K, top, B, _ = case
    users, lists, ptr, items = hm.case_inputs(case)
    res = hm.case_model(case, exclude_self)
    t = hm.tol(d, w)
    idx, val, cnt, mean = got
    # count and mean
    assert np.array_equal(cnt, res.cnt), (what, "cnt")
    assert np.array_equal(np.isnan(mean), np.isnan(res.mean)), (what, "mean: NaN exactly where nothing is listed")
    some = res.cnt > 0
    off_mean = float(np.abs(mean[some].astype(np.float64) - res.mean[some]).max()) if some.any() else 0.0
    # unlisted rows, short lists
    n_ret = np.minimum(res.cnt, top)
    returned = np.arange(top)[None, None, :] < n_ret[:, :, None]
    assert np.array_equal(idx >= 0, returned) and np.array_equal(res.idx >= 0, returned), (what, "how many entries are returned")
    assert (idx[~returned] == -1).all() and np.isneginf(val[~returned]).all(), (what, "the fill is -1 / -inf")
    assert np.isfinite(val[returned]).all()
    # values: the float64 score of the entry each slot names (copies of an id score alike), order, depth
    s64 = hm.scores(hm.item_rows(d, blocks), w, users, lists, ptr, items, exclude_self)
    off, short = 0.0, 0.0
    for b in range(B):
        if not returned[b].any():
            continue
        seg = items[ptr[users[b]]:ptr[users[b] + 1]].astype(np.int64)
        where = np.full(hm.ITEMS + 1, -1, dtype=np.int64)
        where[np.where((seg >= 0) & (seg < hm.ITEMS), seg, hm.ITEMS)] = np.arange(seg.size)
        at = where[np.where(returned[b], idx[b], hm.ITEMS)]
        assert (at[returned[b]] >= 0).all(), (what, b, "a returned id is not in the user's history")
        named = np.take_along_axis(s64[b], np.maximum(at, 0), 1)
        assert not np.isneginf(named[returned[b]]).any(), (what, b, "an unlisted entry was returned")
        off = max(off, float(np.abs(val[b].astype(np.float64) - named)[returned[b]].max()))
        last = np.maximum(n_ret[b] - 1, 0)
        rows = n_ret[b] > 0
        gap = (np.take_along_axis(res.val[b], last[:, None], 1) - np.take_along_axis(named, last[:, None], 1))[:, 0]
        short = max(short, float(gap[rows].max()))
    both = returned[:, :, 1:]
    assert (val[:, :, :-1][both] >= val[:, :, 1:][both]).all(), (what, "returned values are not non-increasing")
    # clear slots, exact ties
    clear = returned & (res.margin > t)
    assert (idx[clear] == res.idx[clear]).all(), (what, "a clear slot does not name the float64 id")
    flat = res.flat[:, :, None] & returned
    assert (idx[flat] == res.idx[flat]).all(), (what, "equal scores: not the lower positions of the segment, in order")
    unclear = float((returned & ~clear & ~flat).sum()) / max(int(returned.sum()), 1)
    print("history_support %s: |out_val - float64| <= %.3e, |out_mean - float64| <= %.3e (bound %.3e), depth short by <= %.3e "
          "(bound %.3e), %.4f of the slots unclear (cap %.2f)" % (what, off, off_mean, t / 2, short, t, unclear, hm.unclear_cap(d)))
    assert off <= t / 2, (what, off, t / 2)
    assert off_mean <= t / 2, (what, off_mean, t / 2)
    assert short <= t, (what, short, t)
    assert unclear <= hm.unclear_cap(d), (what, unclear)


@pytest.mark.parametrize("exclude_self", [True, False], ids=["excl", "keep"])
@pytest.mark.parametrize("case", hm.CASES, ids=IDS)
def test_kernel_against_float64(case, exclude_self):
    d, blocks, w, K, top, B, _ = case
    users, lists, _, _ = hm.case_inputs(case)
    got = _run(_tables(d, blocks), w, users, lists, _index(case), top, exclude_self)
    _verify(case, exclude_self, got, (IDS(case), exclude_self))


def test_self_is_excluded_only_on_request():
    case = hm.CASES[4]
    d, blocks, w, K, top, B, _ = case
    users, lists, ptr, items = hm.case_inputs(case)
    on, off = (_run(_tables(d, blocks), w, users, lists, _index(case), top, e) for e in (True, False))
    inside = np.array([[0 <= users[b] < ptr.size - 1 and 0 <= lists[b, k] < hm.ITEMS and lists[b, k] in items[ptr[users[b]]:ptr[users[b] + 1]] for k in range(K)]
                       for b in range(B)])
    assert inside.any() and (~inside).any()
    assert (off[2][inside] > on[2][inside]).all() and np.array_equal(off[2][~inside], on[2][~inside])
    assert (on[0] != lists[:, :, None])[on[0] >= 0].all(), "exclude_self returned the target itself"
    nonzero = inside & (lists != 11)
    assert (off[0][nonzero][:, 0] == lists[nonzero]).all() and np.abs(off[1][nonzero][:, 0] - sum(x for x in w)).max() <= hm.tol(d, w) / 2
    for a, b in zip(on, off):                                                     # a pair without its target in the history: the same bits
        assert a[~inside].tobytes() == b[~inside].tobytes()


@pytest.mark.parametrize("case", [hm.CASES[5], hm.CASES[9]], ids=IDS)
def test_misaligned_base_takes_the_scalar_row_load(case):
    d, blocks, w, K, top, B, _ = case
    users, lists, _, _ = hm.case_inputs(case)
    got = _run(_tables(d, blocks, col0=3), w, users, lists, _index(case), top, True)
    _verify(case, True, got, (IDS(case), "col0 = 3"))
    aligned = _run(_tables(d, blocks), w, users, lists, _index(case), top, True)   # the same rows through the 16-byte loads: the same bits
    for a, b in zip(got, aligned):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("d", (4, 64, 68, 128, 132, 192, 196, 256))
def test_width_edges(d):
    """Both sides of every boundary of NQ = ceil(d / 64), the float4s a lane holds: B = 2, K = 3, top = 3 over histories of 0, 1 and
    65 entries (65: a second chunk at NQ = 1), two blocks with one zero weight, through the 16-byte and the scalar row loads."""
    from elimrec_amd import ops
    blocks, w, K, top = 2, (0.0, 1.0), 3, 3
    rng = np.random.default_rng(hm.SEED + d)
    items = rng.integers(0, hm.ITEMS, 66).astype(np.int32)
    ptr = np.array([0, 0, 1, 66], dtype=np.int64)
    hist, t = ops.HistoryIndex(ptr, items, DEV), hm.tol(d, w)
    for users in ((0, 2), (1, 2)):
        users = np.array(users, dtype=np.int64)
        lists = rng.integers(0, hm.ITEMS, (2, K)).astype(np.int32)
        lists[1, 0], lists[0, 1] = items[40], items[0]                       # targets inside the histories
        res = hm.support_full(hm.item_rows(d, blocks), w, users, lists, ptr, items, top, True)
        got = _run(_tables(d, blocks, col0=3), w, users, lists, hist, top, True)
        idx, val, cnt, mean = got
        assert np.array_equal(cnt, res.cnt) and np.array_equal(idx >= 0, res.idx >= 0) and np.array_equal(np.isnan(mean), res.cnt == 0)
        back = idx >= 0
        assert (idx[~back] == -1).all() and np.isneginf(val[~back]).all()
        assert np.abs(val[back].astype(np.float64) - res.val[back]).max() <= t / 2       # the k-th largest moves by no more than a score
        assert np.abs(mean[cnt > 0].astype(np.float64) - res.mean[cnt > 0]).max() <= t / 2
        clear = back & (res.margin > t)
        assert (idx[clear] == res.idx[clear]).all()
        for a, b in zip(got, _run(_tables(d, blocks), w, users, lists, hist, top, True)):
            assert a.tobytes() == b.tobytes()


def test_optional_outputs_and_empty_calls():
    from elimrec_amd import ops
    case = hm.CASES[2]
    d, blocks, w, K, top, B, _ = case
    users, lists, _, _ = hm.case_inputs(case)
    tabs, hist = _tables(d, blocks), _index(case)
    full = _run(tabs, w, users, lists, hist, top, True)
    two = _run(tabs, w, users, lists, hist, top, True, outputs=2)
    assert two[0].tobytes() == full[0].tobytes() and two[1].tobytes() == full[1].tobytes()
    e_i, e_f = torch.empty(0, dtype=torch.int32, device=DEV), torch.empty(0, device=DEV)
    ops.history_support(tabs[0], tabs[1], list(w), torch.empty(0, dtype=torch.int64, device=DEV),
                        torch.empty(0, K, dtype=torch.int32, device=DEV), hist, top, e_i, e_f)      # B == 0
    zero = _run(tabs, [0.0, 0.0], users, lists, hist, top, True)                 # no active block: every score is 0, ties by position
    res = hm.support_full(hm.item_rows(d, blocks), [0.0, 0.0], *hm.case_inputs(case), top, True)
    assert np.array_equal(zero[0], res.idx) and np.array_equal(zero[2], res.cnt) and (zero[1][zero[0] >= 0] == 0.0).all()
    other = ops.HistoryIndex([0, 1], [0], "cpu")
    with pytest.raises(ValueError, match="HistoryIndex"):
        _run(tabs, w, users, lists, other, top, True)
    with pytest.raises(ValueError):
        ops.history_support(tabs[0], tabs[1], list(w), _t(users), _t(lists), hist, top, e_i, e_f)    # outputs too small
    with pytest.raises(TypeError):
        ops.history_support(tabs[0], tabs[1], list(w), _t(users).int(), _t(lists), hist, top, e_i, e_f)


@pytest.mark.parametrize("case", [hm.CASES[5], hm.CASES[11]], ids=IDS)
def test_a_pairs_bits_do_not_depend_on_its_surroundings(case):
    d, blocks, w, K, top, B, _ = case
    users, lists, ptr, items = hm.case_inputs(case)
    tabs, hist = _tables(d, blocks), _index(case)
    base = _run(tabs, w, users, lists, hist, top, True)
    again = _run(tabs, w, users, lists, hist, top, True)
    flipped = _run(tabs, w, users, lists[:, ::-1], hist, top, True)
    for a, b, c in zip(base, again, flipped):
        assert a.tobytes() == b.tobytes(), "the same call twice"
        assert np.ascontiguousarray(c[:, ::-1]).tobytes() == a.tobytes(), "the targets in reversed column order"
    for b, k in ((0, 0), (0, K - 1), (B - 1, K // 2)):                            # one target alone
        one = _run(tabs, w, users[b:b + 1], lists[b:b + 1, k:k + 1], hist, top, True)
        for a, c in zip(base, one):
            assert c[0, 0].tobytes() == a[b, k].tobytes(), ("K = 1", b, k)
    rng = np.random.default_rng(3)                                                # the same rows inside a larger B, other rows around
    big_users = rng.integers(-1, ptr.size, 3 * B + 7).astype(np.int64)
    big_lists = rng.integers(-1, hm.ITEMS + 1, (big_users.size, K)).astype(np.int32)
    at = np.sort(rng.permutation(big_users.size)[:B])
    big_users[at], big_lists[at] = users, lists
    big = _run(tabs, w, big_users, big_lists, hist, top, True)
    for a, c in zip(base, big):
        assert np.ascontiguousarray(c[at]).tobytes() == a.tobytes(), "inside a larger B"


def test_torch_op():
    from elimrec_amd import torch_ops
    case = hm.CASES[4]
    d, blocks, w, K, top, B, _ = case
    users, lists, ptr, items = hm.case_inputs(case)
    tabs = _tables(d, blocks)
    want = _run(tabs, w, users, lists, _index(case), top, True)
    got = torch_ops.load().history_support(tabs[0], tabs[1], list(w), _t(users), _t(lists), _t(ptr), _t(items), top, True)
    assert [tuple(x.shape) for x in got] == [(B, K, top), (B, K, top), (B, K), (B, K)]
    for a, b in zip(want, got):
        assert a.tobytes() == b.cpu().numpy().tobytes()
    with pytest.raises(RuntimeError):
        torch_ops.load().history_support(tabs[0], tabs[1], list(w), _t(users), _t(lists), _t(ptr[::-1].copy()), _t(items), top, True)


# ---- the model, the report, the switch
def _forward(name, extra=()):
    from helpers import build_model_from_fixture, load_golden
    g = load_golden(name)
    model, _ = build_model_from_fixture(g, DEV, extra_argv=extra)
    model.bpr_loss(_t(g["step1/users"]), _t(g["step1/pos"]), _t(g["step1/neg"]))
    return model


def _same(a, b):
    return a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_model_front():
    from helpers import build_model_from_fixture, load_golden
    from elimrec_amd import HistorySupport, ops
    from elimrec_amd.evaluator import CandidateScoringError
    fresh, _ = build_model_from_fixture(load_golden("ml3"), DEV)
    with pytest.raises(RuntimeError):
        fresh.explain_history([0, 1], top_k=3)
    model = _forward("ml3")
    U, I, d, nb = model.num_users, model.num_items, model.latent_dim, 1 + model.S
    train = model.dataset.get_user_train_dict()
    users = list(range(min(U, 24)))
    tl = [train.get(u, []) for u in users]
    ptr = np.cumsum([0] + [len(x) for x in tl]).astype(np.int64)
    flat = np.asarray([i for x in tl for i in x], dtype=np.int32)
    hist = ops.HistoryIndex(ptr, flat, DEV, n_items=I)
    K, top = min(5, I), 3
    rows = torch.arange(len(users), dtype=torch.int64, device=DEV)
    lists = model.predict_device(users, top_k=K, train_ptr=_t(ptr), train_items=_t(flat))[0]
    Y, sqn = model._ws["Y"], model._block_sqnorms(torch.device(DEV))
    for space in ("fused", "loss") + tuple(model._mods):
        w = model.hard_negative_weights(space)
        got = model.history_support_device(rows, lists, hist, top=top, space=space)
        want = (torch.empty(len(users), K, top, dtype=torch.int32, device=DEV), torch.empty(len(users), K, top, device=DEV),
                torch.empty(len(users), K, dtype=torch.int32, device=DEV), torch.empty(len(users), K, device=DEV))
        ops.history_support(Y[U:U + I, :nb * d], sqn[U:U + I], w, rows, lists, hist, top, *want)
        assert all(_same(a, b) for a, b in zip(got, want)), space
        # and the float64 model of the same slices
        res = hm.support_full(Y[U:U + I, :nb * d].cpu().numpy(), w, np.arange(len(users)), lists.cpu().numpy(), ptr, flat, top, True)
        t = hm.tol(d, w)
        assert np.array_equal(got[2].cpu().numpy(), res.cnt)
        clear = (res.idx >= 0) & (res.margin > t)
        assert (got[0].cpu().numpy()[clear] == res.idx[clear]).all() and clear.any()
        ok = res.idx >= 0
        assert np.abs(np.sort(got[1].cpu().numpy()[ok].astype(np.float64)) - np.sort(res.val[ok])).max() <= t
    # explain_history names explain()'s lists, and the default history is the train dict
    exclude = {u: train.get(u, []) for u in users}
    out = model.explain_history(users, top_k=K, top=top, exclude=exclude)
    assert isinstance(out, HistorySupport) and all(x.device.type == "cpu" for x in out)
    assert torch.equal(out.items, model.explain(users, top_k=K, exclude=exclude).items) and torch.equal(out.items, lists.cpu())
    got = model.history_support_device(rows, lists, hist, top=top)
    assert all(_same(a, b) for a, b in zip(out[1:], got))
    assert [tuple(x.shape) for x in out] == [(len(users), K), (len(users), K, top), (len(users), K, top), (len(users), K), (len(users), K)]
    listed = out.items.numpy() >= 0                                                   # the masked lists hold no history item
    assert (out.count.numpy()[listed] == np.array([[len(x)] * K for x in tl])[listed]).all() and listed.any()
    # ragged lists against an explicit, hypothetical history; a user absent from it has none
    mine = {0: [1, 2, 2, 0], 1: [3], 5: [0]}
    given = [[0, 1, 2], [3], []]
    out = model.explain_history([0, 1, 2], items=given, top=2, space=model._mods[0], history=mine)
    assert out.items.tolist() == [[0, 1, 2], [3, -1, -1], [-1, -1, -1]]
    w = model.hard_negative_weights(model._mods[0])
    res = hm.support_full(Y[U:U + I, :nb * d].cpu().numpy(), w, [0, 1, 2], out.items.numpy(), [0, 4, 5, 5], [1, 2, 2, 0, 3], 2, True)
    assert np.array_equal(out.count.numpy(), res.cnt) and out.count.tolist() == [[3, 3, 2], [0, 0, 0], [0, 0, 0]]
    assert np.array_equal(np.isnan(out.mean.numpy()), np.isnan(res.mean))
    clear = (res.idx >= 0) & (res.margin > hm.tol(d, w))
    assert (out.history.numpy()[clear] == res.idx[clear]).all()
    assert np.array_equal(out.history.numpy() < 0, res.idx < 0)
    ok = res.idx >= 0
    assert np.abs(out.scores.numpy()[ok] - res.val[ok]).max() <= hm.tol(d, w)
    assert out.history[0, 0].tolist().count(2) <= 2 and (out.history[1:] == -1).all() and torch.isneginf(out.scores[1:]).all()
    assert tuple(model.explain_history([], top_k=K).items.shape) == (0, K)
    model._eval_shard = object()
    try:
        with pytest.raises(CandidateScoringError):
            model.explain_history(users, top_k=K)
        with pytest.raises(CandidateScoringError):
            model.history_support_device(rows, lists, hist)
    finally:
        model._eval_shard = None


@pytest.mark.parametrize("view", [None, [2, 4]])
def test_history_report(view):
    from elimrec_amd import ops
    from elimrec_amd.evaluator import CandidateScoringError, HistoryReport
    model = _forward("ml3")
    train, test = model.dataset.get_user_train_dict(), model.dataset.get_user_test_dict()
    K, top = min(4, model.num_items), 2
    report = HistoryReport(model.dataset, train, test, K, top=top, group_view=view)
    report.block_users = (len(report.users) + 1) // 2                            # two user blocks
    tables = {}
    for effect in ("TE", "TIE"):
        model.predict_type = effect
        rows = report.history_rows(model)
        final, buf = report.evaluate(model, rows)
        columns = ops.history_columns(model._mods)
        nb, n, G = 1 + model.S, len(report.users), len(report.group_labels)
        assert report.columns == columns and tuple(rows.shape) == (n * K, len(columns)) and final.shape == (G, len(columns))
        assert (G > 1) == (view is not None)
        # the rows are the kernel's, space by space
        tl = [train.get(u, []) for u in report.users]
        ptr = np.cumsum([0] + [len(x) for x in tl]).astype(np.int64)
        flat = np.asarray([i for x in tl for i in x], dtype=np.int32)
        lists = model.predict_device(report.users, top_k=K, train_ptr=_t(ptr), train_items=_t(flat))[0]
        hist = ops.HistoryIndex(ptr, flat, DEV)
        at = torch.arange(n, dtype=torch.int64, device=DEV)
        h = rows.cpu().numpy()
        for s, space in enumerate(("fused",) + tuple(model._mods)):
            _, val, cnt, mean = model.history_support_device(at, lists, hist, top=top, space=space)
            assert h[:, s].tobytes() == val[:, :, 0].reshape(-1).cpu().numpy().tobytes()
            assert h[:, nb + s].tobytes() == mean.reshape(-1).cpu().numpy().tobytes()
            assert h[:, 2 * nb + s].tobytes() == (1.0 - val[:, :, 0]).reshape(-1).cpu().numpy().tobytes()
        assert h[:, 3 * nb].tolist() == cnt.reshape(-1).float().cpu().tolist()
        # the table: numpy means of those rows over the pairs with a history, overall and per group
        for g in range(G):
            pairs = (report._positions[g][:, None] * K + np.arange(K)[None, :]).reshape(-1)
            assert all(len(train.get(report.users[p], [])) > 0 for p in report._positions[g])
            want = h[pairs].astype(np.float64).mean(0)
            np.testing.assert_allclose(final[g], want, rtol=1e-6, atol=1e-7)
        assert np.isfinite(final).all()
        lines = buf.split("\n")
        assert len(lines) == 1 + G and lines[0].startswith("columns:") and all(c in lines[0] for c in columns)
        assert [ln[:12] for ln in lines[1:]] == [x[:12] for x in report.group_labels]
        assert report.evaluate(model)[1] == buf
        tables[effect] = (rows, final)
    shift, buf = report.shift(tables["TE"][0], tables["TIE"][0])
    assert report.shift_columns == tuple("d_" + c for c in report.columns) and all(c in buf for c in report.shift_columns)
    np.testing.assert_allclose(shift, tables["TIE"][1].astype(np.float64) - tables["TE"][1], rtol=0, atol=2e-6)
    d = (tables["TIE"][0] - tables["TE"][0]).cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(shift[0], d[(report._positions[0][:, None] * K + np.arange(K)[None, :]).reshape(-1)].mean(0), rtol=1e-6, atol=1e-7)
    with pytest.raises(ValueError):
        report.shift(tables["TE"][0], tables["TIE"][0][:-1])
    model._eval_shard = object()
    try:
        with pytest.raises(CandidateScoringError):
            report.evaluate(model)
    finally:
        model._eval_shard = None


def test_driver_switch(tmp_path):
    from test_lists_gpu import _driver
    from elimrec_amd import ops
    off, ev0, te0 = _driver(tmp_path / "a", ["--group_view=[10,30]", "--list_report=5"])
    assert not any("histor" in ln for ln in off)
    on, ev1, te1 = _driver(tmp_path / "b", ["--group_view=[10,30]", "--list_report=5", "--history_report=5", "--history_top=2"])
    added = [k for k, ln in enumerate(on) if ln.startswith("  [TE] support of the top-5 lists in the users' histories:\n")
             or ln.startswith("  [TIE] support of the top-5 lists in the users' histories:\n")
             or ln.startswith("  [TE->TIE] history support shift:\n")]
    assert len(added) == 3 and [ln for k, ln in enumerate(on) if k not in added] == off      # with the switch off: the log as it was
    te, tie, shift = added
    assert on[te - 1].startswith("  [TE] top-5 lists") and on[te + 1].startswith("  [TIE]\t")
    assert on[tie - 1].startswith("  [TIE] top-5 lists") and on[shift - 1].startswith("  [TE->TIE] list shift") and shift == len(on) - 1
    columns = ops.history_columns(("v", "a", "t"))
    for k in (te, tie):
        assert all(c in on[k] for c in columns) and on[k].count("\nall:") == 1
    assert all("d_" + c in on[shift] for c in columns)
    assert ev0.tobytes() == ev1.tobytes() and te0.tobytes() == te1.tobytes()
