"""Float64 model of history support (csrc/history.hip), pure numpy, and the inputs the CPU and GPU tests share.

score(j, i) = sum over the blocks b with w_b != 0 of w_b * cos_b(j, i), cos_b = (T_b[j] . T_b[i]) / (max(|T_b[j]|, 1e-12) *
max(|T_b[i]|, 1e-12)) -- a zero row gives 0. A target (b, k) is listed when 0 <= lists[b, k] < rows and 0 <= users[b] < segments;
an entry of segment users[b] is listed when its id lies in [0, rows) and, with exclude_self, differs from the target; a repeated id
is an entry of its own. Per target the `top` listed entries with the largest score, the lower segment position first among equal
scores; cnt = the listed entries, mean = their mean score."""
import collections
import functools

import numpy as np

Support = collections.namedtuple("Support", ("idx", "val", "cnt", "mean", "margin", "pos", "flat"))


def unit_blocks(T, blocks):
    """[rows x blocks x d] float64, every block of every row scaled to unit length; a zero row stays zero."""
    X = np.asarray(T, dtype=np.float64)
    X = X.reshape(X.shape[0], blocks, -1)
    return X / np.maximum(np.sqrt((X * X).sum(2, keepdims=True)), 1e-12)


def scores(T, weights, users, lists, hist_ptr, hist_items, exclude_self):
    """Per row b a float64 array [K x H_b] (H_b = the length of segment users[b]; 0 for a user outside the index): the score of
    every entry against every target, -inf where the entry or the target is not listed."""
    w = np.asarray(weights, dtype=np.float64)
    Tn = unit_blocks(T, w.size)
    n = Tn.shape[0]
    users, lists = np.asarray(users, dtype=np.int64), np.asarray(lists, dtype=np.int64)
    ptr, items = np.asarray(hist_ptr, dtype=np.int64), np.asarray(hist_items, dtype=np.int64)
    Tw = Tn * np.where(w != 0, w, 0.0)[None, :, None]
    out = []
    for b in range(lists.shape[0]):
        u = users[b]
        if not 0 <= u < ptr.size - 1:
            out.append(np.full((lists.shape[1], 0), -np.inf))
            continue
        seg = items[ptr[u]:ptr[u + 1]]
        tgt = lists[b]
        ok_e, ok_t = (seg >= 0) & (seg < n), (tgt >= 0) & (tgt < n)
        A = Tw[np.where(ok_t, tgt, 0)].reshape(tgt.size, Tn.shape[1] * Tn.shape[2])
        H = Tn[np.where(ok_e, seg, 0)].reshape(seg.size, Tn.shape[1] * Tn.shape[2])
        s = A @ H.T
        listed = ok_t[:, None] & ok_e[None, :]
        if exclude_self:
            listed &= tgt[:, None] != seg[None, :]
        out.append(np.where(listed, s, -np.inf))
    return out


def brute_force(T, weights, users, lists, hist_ptr, hist_items, top, exclude_self):
    """The same outputs by plain loops over every (target, entry) pair: (idx, val, cnt, mean)."""
    w = [float(x) for x in weights]
    T = np.asarray(T, dtype=np.float64)
    n, d = T.shape[0], T.shape[1] // len(w)
    B, K = np.asarray(lists).shape
    idx, val = np.full((B, K, top), -1, dtype=np.int64), np.full((B, K, top), -np.inf)
    cnt, mean = np.zeros((B, K), dtype=np.int64), np.full((B, K), np.nan)
    for b in range(B):
        u = int(users[b])
        for k in range(K):
            i = int(lists[b][k])
            if not (0 <= i < n and 0 <= u < len(hist_ptr) - 1):
                continue
            found = []
            for p in range(int(hist_ptr[u]), int(hist_ptr[u + 1])):
                j = int(hist_items[p])
                if not 0 <= j < n or (exclude_self and j == i):
                    continue
                s = 0.0
                for blk, wb in enumerate(w):
                    if wb == 0.0:
                        continue
                    x, y = T[i, blk * d:(blk + 1) * d], T[j, blk * d:(blk + 1) * d]
                    s += wb * float(x @ y) / (max(np.sqrt(float(x @ x)), 1e-12) * max(np.sqrt(float(y @ y)), 1e-12))
                found.append((-s, p, j))
            cnt[b, k] = len(found)
            if found:
                mean[b, k] = sum(-f[0] for f in found) / len(found)
            for r, (ns, _, j) in enumerate(sorted(found)[:top]):
                idx[b, k, r], val[b, k, r] = j, -ns
    return idx, val, cnt, mean


def support_full(T, weights, users, lists, hist_ptr, hist_items, top, exclude_self):
    """Support(idx int64 [B x K x top] (-1 short), val float64 (-inf short), cnt int64 [B x K], mean float64 (NaN without a listed
    entry), margin float64 [B x K x top], pos int64 [B x K x top] the returned entries' positions in their segment (-1 short),
    flat bool [B x K]: every listed entry of the pair has the same float64 score -- the tie rule alone decides the pair).
    margin of a returned slot: the float64 gap between its score and the nearest score of a listed entry at another segment
    position that holds ANOTHER id (+inf without one) -- above or below it in the ranking, returned or not. Copies of one id score
    alike in any arithmetic and are ordered by position, so where that gap exceeds the tolerance of a comparison the slot's id is
    decided."""
    lists = np.asarray(lists, dtype=np.int64)
    items = np.asarray(hist_items, dtype=np.int64)
    ptr = np.asarray(hist_ptr, dtype=np.int64)
    B, K = lists.shape
    idx, pos = np.full((B, K, top), -1, dtype=np.int64), np.full((B, K, top), -1, dtype=np.int64)
    val, margin = np.full((B, K, top), -np.inf), np.full((B, K, top), np.inf)
    cnt, mean, flat = np.zeros((B, K), dtype=np.int64), np.full((B, K), np.nan), np.zeros((B, K), dtype=bool)
    for b, s in enumerate(scores(T, weights, users, lists, hist_ptr, hist_items, exclude_self)):
        H = s.shape[1]
        if not H:
            continue
        seg = items[ptr[users[b]]:ptr[users[b]] + H]
        listed = ~np.isneginf(s)
        cnt[b] = listed.sum(1)
        some = cnt[b] > 0
        mean[b, some] = np.where(listed, s, 0.0).sum(1)[some] / cnt[b, some]
        order = np.argsort(-s, axis=1, kind="stable")[:, :top]               # stable: the lower position among equal scores
        got = np.take_along_axis(s, order, 1)
        have = ~np.isneginf(got)
        r = order.shape[1]
        val[b, :, :r] = got
        pos[b, :, :r] = np.where(have, order, -1)
        idx[b, :, :r] = np.where(have, seg[order], -1)
        hi = np.where(listed, s, -np.inf).max(1)
        lo = np.where(listed, s, np.inf).min(1)
        flat[b] = some & (hi == lo)
        # the gap of every returned slot to the nearest listed score under another id
        other = listed[:, None, :] & (seg[None, None, :] != seg[order][:, :, None])
        gap = np.where(other, np.abs(s[:, None, :] - np.where(have, got, 0.0)[:, :, None]), np.inf).min(2)
        margin[b, :, :r] = np.where(have, gap, np.inf)
    return Support(idx, val, cnt, mean, margin, pos, flat)


def support(T, weights, users, lists, hist_ptr, hist_items, top, exclude_self):
    """(idx, val, cnt, mean, margin) of support_full."""
    return tuple(support_full(T, weights, users, lists, hist_ptr, hist_items, top, exclude_self)[:5])


def unclear_share(res, t):
    """The share of returned slots of a result whose id the tolerance t does not decide: margin <= t, outside the flat pairs."""
    returned = res.idx >= 0
    unclear = returned & (res.margin <= t) & ~res.flat[:, :, None]
    return float(unclear.sum()) / max(int(returned.sum()), 1)


# ---- the inputs the kernel tests run on (test_history_gpu.py on the device, test_history_cpu.py for the model's own unclear share)
ITEMS, SEED = 500, 11
# d, blocks, weights, K, top, B, with the 3 000-entry segment
CASES = (
    (4, 1, (1.0,), 1, 1, 1, False),
    (4, 1, (1.0,), 4, 3, 5, True),
    (20, 2, (0.0, 1.0), 2, 3, 5, False),
    (20, 2, (0.0, 1.0), 17, 16, 33, False),
    (64, 4, (1.0, 0.5, 0.0, 0.5), 16, 3, 33, False),
    (64, 4, (1.0, 0.5, 0.0, 0.5), 65, 16, 5, False),
    (64, 1, (1.0,), 64, 1, 5, False),
    (64, 1, (1.0,), 256, 3, 5, False),
    (64, 1, (1.0,), 17, 16, 33, False),
    (256, 4, (1.0, 0.5, 0.0, 0.5), 16, 3, 5, False),
    (256, 4, (1.0, 0.5, 0.0, 0.5), 65, 16, 1, False),
    (256, 2, (1.0, 0.0), 17, 1, 33, False),
    (256, 2, (1.0, 0.0), 256, 16, 1, False),
    (256, 2, (1.0, 0.0), 2, 3, 5, False),
)


def tol(d, w):
    """4 (d + 8) 2^-24 * sum |w_b|: the derived fp32 bound of a comparison of two scores (test_rerank_gpu.py's header)."""
    return 4.0 * (d + 8) * 2.0 ** -24 * float(np.abs(np.asarray(w, dtype=np.float64)).sum())


def unclear_cap(d):
    return 0.02 if d <= 64 else 0.10


@functools.lru_cache(maxsize=None)
def item_rows(d, blocks):
    """500 item rows of `blocks` blocks, fp32, as test_hardneg_gpu.py's _tables builds its item side (the same generator, its 300
    user rows drawn first): N(0, 1) + 1.5 x one of 8 centres, row 11 zero."""
    rng = np.random.default_rng(SEED + 1000 * d + blocks)
    X = None
    for rows in (300, ITEMS):
        centres = rng.standard_normal((8, blocks * d))
        X = (rng.standard_normal((rows, blocks * d)) + 1.5 * centres[rng.integers(0, 8, rows)]).astype(np.float32)
        X[11] = 0.0
    X.setflags(write=False)
    return X


def segments(top, rng, long_segment=False):
    """The histories of a case as CSR (ptr int64, items int32): lengths 0, 1, top - 1, top, top + 1, 63, 64, 65, 300, then a
    segment of 40 entries over six ids (item 11, the zero row, among them), one of 50 with ids of -1 and ITEMS sprinkled in, and --
    long_segment -- one of 3 000."""
    segs = [rng.integers(0, ITEMS, n) for n in (0, 1, top - 1, top, top + 1, 63, 64, 65, 300)]
    segs.append(np.array([11, 3, 77, 3, 408, 250])[rng.integers(0, 6, 40)])
    bad = rng.integers(0, ITEMS, 50)
    bad[rng.integers(0, 50, 8)] = -1
    bad[rng.integers(0, 50, 8)] = ITEMS
    bad[[0, 49]] = -1, ITEMS
    segs.append(bad)
    if long_segment:
        segs.append(rng.integers(0, ITEMS, 3000))
    ptr = np.zeros(len(segs) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in segs], out=ptr[1:])
    return ptr, np.concatenate(segs).astype(np.int32)


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """(users int64 [B], lists int32 [B x K], ptr, items) of a case. Rows walk the segments from the longest plain one (300, or the
    3 000) on; with B >= 5 row 1 has user -1 and row 4 the number of segments; every row has a target of -1 and one of ITEMS where K
    allows, row 0 targets the zero row, and every row with a history targets two of its own entries (the second one also a copy of the
    first where the list is long enough)."""
    d, blocks, w, K, top, B, long_segment = case
    rng = np.random.default_rng(SEED + 7 * d + 13 * K + 17 * top + B)
    ptr, items = segments(top, rng, long_segment)
    R = ptr.size - 1
    first = R - 1 if long_segment else 8
    order = [first, 9, 10] + [s for s in range(R) if s not in (first, 9, 10)]
    users = np.array([order[b % R] for b in range(B)], dtype=np.int64)
    if B >= 5:
        users[1], users[4] = -1, R
    lists = rng.integers(0, ITEMS, (B, K)).astype(np.int32)
    for b in range(B):
        u = users[b]
        seg = items[ptr[u]:ptr[u + 1]] if 0 <= u < R else items[:0]
        own = seg[(seg >= 0) & (seg < ITEMS)]
        at = rng.permutation(K)
        if own.size:
            lists[b, at[0]] = own[own.size // 2]
            if K > 1:
                lists[b, at[1]] = own[0]
            if K > 5:
                lists[b, at[5]] = own[own.size // 2]
        if K > 2:
            lists[b, at[2]] = -1
        if K > 3:
            lists[b, at[3]] = ITEMS
        if b == 0 and (K > 4 or not own.size):
            lists[b, at[min(4, K - 1)]] = 11
    for a in (users, lists, ptr, items):
        a.setflags(write=False)
    return users, lists, ptr, items


@functools.lru_cache(maxsize=None)
def case_model(case, exclude_self):
    """The float64 result of a case, computed once and shared (read-only)."""
    d, blocks, w, K, top, B, _ = case
    res = support_full(item_rows(d, blocks), w, *case_inputs(case), top, exclude_self)
    for a in res:
        a.setflags(write=False)
    return res
