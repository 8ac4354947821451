"""A plain torch / numpy model of the audience lists (per item the K users with the largest predict() score), on top of
tests/score_model.py. Nothing here calls elimrec_amd: it is the independent side.

columns(): the [U x Q] scores of the query items' columns in the dtype of Y. check_lists(): the list rules the GPU tests and the
float32 model's own top-K are held to. item_rows(): a numpy restatement of reports.audience_item_rows."""
import numpy as np
import torch

import score_model as sm


def columns(Y, U, items, d, S, head_mask, fusion, ptype, row_sum=None, I_total=None):
    """predict() of every user for the query items: [U x Q] in the dtype of Y (row_sum / I_total: score_model's TIE mean path)."""
    users = torch.arange(U)
    full = sm.score_model(Y, U, users, d, S, head_mask, fusion, ptype, I_total=I_total, row_sum=row_sum)
    return full[:, torch.as_tensor(items, dtype=torch.long)]


def rising_table(U, I, d, S, seed=0):
    """float32 [U + I, (1 + S) d] in which the score of items 0 .. I / 2 - 1 rises strictly with the user id under every predict type.
    Block 0: user u = t_u e with t_u evenly spaced over [-2, 2], item i = a_i e, a_i in [0.9, 1] for the first half of the catalogue
    and the same values negated for the second half -- so the dots of a listed item spread over [-2 a_i, 2 a_i], and the catalogue
    mean of sigmoid(dot) is 1 / 2 for every user (sigmoid(x) + sigmoid(-x) = 1): TIE's second term does not depend on the user.
    Head blocks: every user holds the same direction per head at a random positive length, so a head's cosine depends on the item
    alone and the fusions stay increasing in the dot."""
    g = torch.Generator().manual_seed(seed)
    Y = torch.randn(U + I, (1 + S) * d, generator=g, dtype=torch.float64) * 0.3
    e = sm.unit(torch.randn(d, generator=g, dtype=torch.float64))
    a = 0.9 + 0.1 * torch.arange(I // 2, dtype=torch.float64) / (I // 2 - 1)
    Y[:U, :d] = torch.linspace(-2.0, 2.0, U, dtype=torch.float64)[:, None] * e
    Y[U:U + I // 2, :d] = a[:, None] * e
    Y[U + I // 2:U + 2 * (I // 2), :d] = -a[:, None] * e
    for h in range(1, 1 + S):
        w = torch.randn(d, generator=g, dtype=torch.float64)
        Y[:U, h * d:(h + 1) * d] = (0.5 + torch.rand(U, generator=g, dtype=torch.float64))[:, None] * w
    return Y.float()


def rising_excl(U, Q):
    """Exclusion lists of the rising case: query 0 nobody, query 1 the 300 users it would list first, query 2 every second user,
    the others a few single users (one id twice)."""
    return ([[], list(range(U - 300, U)), list(range(0, U, 2))] + [[U - 1 - q, 5 * q, U - 1 - q] for q in range(3, Q)])[:Q]


def min_gap(s64, ok):
    """The smallest difference between the float64 scores of two eligible users of one column."""
    return min(float(np.diff(np.sort(s64[ok[:, q], q])).min()) for q in range(s64.shape[1]))


def eligible_mask(U, Q, excl):
    """bool [U x Q]: user u may be listed for query q (excl: one iterable of user ids per query, or None)."""
    ok = np.ones((U, Q), dtype=bool)
    if excl is not None:
        for q, ids in enumerate(excl):
            ids = np.asarray(list(ids), dtype=np.int64)
            ok[ids[(ids >= 0) & (ids < U)], q] = False
    return ok


def topk32(s32, ok, K):
    """The float32 model's own lists by (score descending, user id ascending): (idx int32 [Q x K], val float32 [Q x K])."""
    s32 = np.asarray(s32, dtype=np.float32)
    U, Q = s32.shape
    idx = np.full((Q, K), -1, dtype=np.int32)
    val = np.full((Q, K), -np.inf, dtype=np.float32)
    for q in range(Q):
        users = np.flatnonzero(ok[:, q])
        order = users[np.lexsort((users, -s32[users, q].astype(np.float64)))][:K]
        idx[q, :order.size] = order
        val[q, :order.size] = s32[order, q]
    return idx, val


def check_lists(idx, val, s64, s32, ok, K, fast, what=""):
    """Rules 1-4 for every (item, slot). s64 / s32 [U x Q]: the float64 / float32 model's scores; ok [U x Q]: eligibility.
    -> the largest |val - s64| seen, and the largest tolerance used (for the printed figures)."""
    s64 = np.asarray(s64, dtype=np.float64)
    s32 = np.asarray(s32)
    U, Q = s64.shape
    assert idx.shape == val.shape == (Q, K), (what, idx.shape, val.shape)
    worst = tol_max = 0.0
    for q in range(Q):
        users = np.flatnonzero(ok[:, q])
        tol, _ = sm.tolerance(torch.from_numpy(s64[users, q]), torch.from_numpy(s32[users, q].astype(np.float32)), fast)
        tol_max = max(tol_max, tol)
        n = min(K, users.size)
        ids, v = idx[q], val[q]
        # 1: distinct, eligible, in range; exactly n listed, fillers at the tail
        assert (ids[:n] >= 0).all() and (ids[:n] < U).all(), (what, q, ids)
        assert (ids[n:] == -1).all() and np.isneginf(v[n:]).all(), (what, q, ids, v)
        assert len(set(ids[:n].tolist())) == n and ok[ids[:n], q].all(), (what, q, ids)
        if n == 0:
            continue
        # 2: values
        err = np.abs(v[:n].astype(np.float64) - s64[ids[:n], q])
        assert not np.isnan(err).any() and err.max() <= tol, (what, q, float(err.max()), tol)
        worst = max(worst, float(err.max()))
        # 3: the right users
        t = np.sort(s64[users, q])[::-1][n - 1]
        assert (s64[ids[:n], q] >= t - 2 * tol).all(), (what, q, "listed below the K-th best")
        must = users[s64[users, q] > t + 2 * tol]
        assert np.isin(must, ids[:n]).all(), (what, q, "a clear winner is missing")
        # 4: order
        assert (v[:n - 1] >= v[1:n]).all(), (what, q, "values ascend")
        same = v[:n - 1] == v[1:n]
        assert (ids[:n - 1][same] < ids[1:n][same]).all(), (what, q, "ids among equal values")
    return worst, tol_max


def item_rows(lists, scores, test_ptr, test_users, user_train_len):
    """float64 [n x 4]: hit, first, act, score per item -- hit = |list & test users| / |test users| (NaN without test users), first =
    any test user listed, act / score = the mean training-history length / score of the listed users (NaN: nothing listed)."""
    lists = np.asarray(lists)
    n = lists.shape[0]
    out = np.full((n, 4), np.nan)
    for i in range(n):
        row = [int(u) for u in lists[i] if u >= 0]
        test = set(int(u) for u in test_users[int(test_ptr[i]):int(test_ptr[i + 1])])
        hits = sum(1 for u in row if u in test)
        if test:
            out[i, 0] = hits / len(test)
        out[i, 1] = float(hits > 0)
        if row:
            out[i, 2] = sum(float(user_train_len[u]) for u in row) / len(row)
            out[i, 3] = sum(float(s) for u, s in zip(lists[i], scores[i]) if u >= 0) / len(row)
    return out
