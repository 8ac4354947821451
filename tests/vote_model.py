"""An exact host model of the neighbour votes (csrc/vote.hip, ops.neighbour_vote_topk) in pure numpy, following the definition
literally: a vote is a pair (history position p, slot s) with j = hist[p] in [0, n), i = idx[j, s] in [0, n) and val[j, s] finite; it
adds q = rint(float64(val) * 2^24) to an int64 sum S(u, i) and 1 to an int32 count c(u, i); listed are the items with c >= 1 that
are not left out; score = float32(float64(S) * 2^-24); order (score descending, id ascending); fillers -1 / -inf / 0. Also the
bookkeeping of the dense form's schedule and the report's columns."""
import collections

import numpy as np

FRAC_BITS = 24


def csr_of(lists):
    """(ptr int64, flat int64) of a list of id lists."""
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=ptr[1:])
    return ptr, np.asarray([i for x in lists for i in x], dtype=np.int64)


def fixed(val):
    """q of fp32 values (finite): int64."""
    return np.rint(np.asarray(val, dtype=np.float32).astype(np.float64) * 2.0 ** FRAC_BITS).astype(np.int64)


def score_of(S):
    return (np.asarray(S, dtype=np.int64).astype(np.float64) * 2.0 ** -FRAC_BITS).astype(np.float32)


def sums(nbr_idx, nbr_val, history):
    """(S int64 [n], c int64 [n]) of one history (a sequence of ids, any range)."""
    n, Kn = nbr_idx.shape
    S, c = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for j in history:
        j = int(j)
        if not 0 <= j < n:
            continue
        for s in range(Kn):
            i, v = int(nbr_idx[j, s]), nbr_val[j, s]
            if 0 <= i < n and np.isfinite(v):
                S[i] += int(fixed(v))
                c[i] += 1
    return S, c


def left_out(n, history, excluded, exclude_history):
    out = np.zeros(n, dtype=bool)
    for j in (list(history) if exclude_history else []) + list(excluded):
        if 0 <= int(j) < n:
            out[int(j)] = True
    return out


def topk(nbr_idx, nbr_val, hist, users, K, excl=None, exclude_history=True):
    """(idx int32, val float32, cnt int32) [B x K]: the model of ops.neighbour_vote_topk. hist / excl: lists of id lists, one per
    segment; users name segments of both."""
    nbr_idx, nbr_val = np.asarray(nbr_idx), np.asarray(nbr_val, dtype=np.float32)
    n = nbr_idx.shape[0]
    B = len(users)
    idx = np.full((B, K), -1, dtype=np.int32)
    val = np.full((B, K), -np.inf, dtype=np.float32)
    cnt = np.zeros((B, K), dtype=np.int32)
    for b, u in enumerate(users):
        S, c = sums(nbr_idx, nbr_val, hist[u])
        out = left_out(n, hist[u], excl[u] if excl is not None else [], exclude_history)
        ids = np.flatnonzero((c >= 1) & ~out)                                 # ascending ids
        s = score_of(S[ids])
        order = np.argsort(-s.astype(np.float64), kind="stable")[:K]         # stable: ascending id among equal scores
        m = order.size
        idx[b, :m], val[b, :m], cnt[b, :m] = ids[order], s[order], c[ids][order]
    return idx, val, cnt


def votes(Kn, hist, excl=None, exclude_history=True):
    """V of every segment: (history length) x Kn + (entries left out)."""
    return np.asarray([len(h) * Kn + (len(h) if exclude_history else 0) + (len(excl[u]) if excl is not None else 0)
                       for u, h in enumerate(hist)], dtype=np.int64)


def dense_groups(V_of_rows, lds, cap, max_groups, threads=256):
    """Which positions of `users` each workgroup of the dense form serves (vote_dense_kernel): position b is a dense row when lds is
    off or its V is past `cap` = VOTE_SLOTS / 2; G = min(dense rows, max_groups) workgroups run, workgroup w takes the dense
    positions b = w (mod G) in ascending order. Returns a list of G lists of (pass, position)."""
    V_of_rows = np.asarray(V_of_rows, dtype=np.int64)
    dense = ~((V_of_rows <= cap) & bool(lds))
    G = min(int(dense.sum()), int(max_groups))
    return [[(int(p // G) // threads, int(p)) for p in range(w, dense.size, G) if dense[p]] for w in range(G)]


Schedule = collections.namedtuple("Schedule", "cuts appended dropped longest ids")


def dense_schedule(nbr_idx, nbr_val, history, excluded, K, cap, positions=16, slots=32, exclude_history=True):
    """The bookkeeping of the dense form's pass 2 for one user: the history is walked `positions` entries at a time, `slots` slots
    of each entry's list per step; a touched item is claimed (with its whole sum and count) at the first step that meets it and --
    unless left out -- appended to the running list if and only if its key (score, then the lower id) exceeds the threshold read at
    the top of that step; after a step that leaves the list longer than cap - positions * slots the list is sorted and, holding at
    least K, cut to its K best, whose last key becomes the threshold. Which lane wins a claim inside a step changes none of these
    numbers: pass 1 is complete and the threshold is read once per step."""
    nbr_idx = np.asarray(nbr_idx)
    n, Kn = nbr_idx.shape
    S, c = sums(nbr_idx, nbr_val, history)
    out = left_out(n, history, excluded, exclude_history)
    score = score_of(S)
    limit = cap - positions * slots
    claimed, kept, thr = set(), [], None
    cuts = appended = dropped = longest = 0
    history = [int(j) for j in history]
    for p0 in range(0, len(history), positions):
        batch = [nbr_idx[j] if 0 <= j < n else nbr_idx[0][:0] for j in history[p0:p0 + positions]]
        s0 = 0
        while True:
            top = thr
            for held in batch:
                for i in held[s0:s0 + slots].tolist():
                    if not 0 <= i < n or c[i] == 0 or i in claimed:
                        continue
                    claimed.add(i)
                    if out[i]:
                        continue
                    key = (float(score[i]), -i)
                    if top is None or key > top:
                        kept.append(key)
                        appended += 1
                    else:
                        dropped += 1
            s0 += slots
            longest = max(longest, len(kept))
            if len(kept) > limit:
                cuts += 1
                kept.sort(reverse=True)
                if len(kept) >= K:
                    kept, thr = kept[:K], kept[K - 1]
            if not any(s0 < held.size for held in batch):
                break
    kept.sort(reverse=True)
    return Schedule(cuts, appended, dropped, longest, [-k[1] for k in kept[:K]])


# --------------------------------------------------------------------------- the report's columns
def metric_rows(lists, truth, metric_ids):
    """The metric curves of id lists as ops.rank_metrics computes them (csrc/eval.hip), float32 [users x len(metric_ids) * K],
    metric-major: 1 Precision, 2 Recall, 4 NDCG (the gains added one by one, each sum rounded to fp32) at every cutoff 1..K over the
    truth lists (distinct ids >= 0). A -1 filler is never in a truth list: a miss."""
    B, K = lists.shape
    w = 1.0 / np.log2(np.arange(K, dtype=np.float64) + 2.0)
    out = np.zeros((B, len(metric_ids), K), dtype=np.float32)
    for b in range(B):
        t = set(int(i) for i in truth[b])
        hit = [int(i) in t for i in lists[b]]
        for m, mid in enumerate(metric_ids):
            hits, dcg, idcg = 0, np.float32(0), np.float32(0)
            for i in range(K):
                hits += hit[i]
                if hit[i]:
                    dcg = np.float32(np.float64(dcg) + w[i])
                if i < len(t):
                    idcg = np.float32(np.float64(idcg) + w[i])
                if mid == 1:
                    out[b, m, i] = np.float32(1.0 * hits / (i + 1))
                elif mid == 2:
                    out[b, m, i] = np.float32(1.0 * hits / float(len(t)))
                elif mid == 4:
                    out[b, m, i] = dcg / idcg
                else:
                    raise ValueError(mid)
    return out.reshape(B, -1)


def list_columns(lists, own, item_counts):
    """The report's list columns per user, float32 [users x 3]: filled (the share of the K slots that hold an item), pop (the mean
    training interactions of the listed items, 0 for an empty list), overlap (the ids of the own list the baseline list also holds,
    over K)."""
    B, K = lists.shape
    counts = np.asarray(item_counts, dtype=np.float64)
    out = np.zeros((B, 3), dtype=np.float32)
    for b in range(B):
        ids = lists[b][lists[b] >= 0]
        mine = own[b][own[b] >= 0]
        out[b] = (ids.size / K, counts[ids].sum() / max(ids.size, 1), np.isin(mine, ids).sum() / K)
    return out
