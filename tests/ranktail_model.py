"""Plain numpy models of the evaluator's ranking tail (csrc/eval.hip: the top-K selections, topk_merge_kernel,
rank_metrics_kernel) and the case lists the CPU and GPU tests of that tail share. Nothing here calls elimrec_amd or oracle/: it is
the independent side.

metrics_model   the reference's five metric recurrences (metric.h:17-106), rounded where the C++ rounds
stable_topk     the first K of a stable sort by (score descending, id ascending): the rule of every selection with tie order "id"
merge_model     the same rule over candidate lists, -1 ids skipped, the tail -1 / -inf
selection_walk  what topk_tiles_kernel DECIDES for one row and one chunk (which ranking, tau, candidates, fall-back, accepted
                short). It only proves that the cases reach each branch; it is never a reference for results.
"""
import math

import numpy as np

TI = 16                  # items per scorer tile
TK_CAP = 1024            # candidates the selections rank in LDS
RM_KMAX = 256            # largest K of the tile-guided selection and of the metric kernel
SCORE_PILOT = 2048       # first chunk of the chunked (top-K only) form
SCORE_CHUNK = 16384      # items per scorer launch beyond it
MERGE_MAX = 20480        # candidates per row topk_merge accepts (160 KB of LDS)

F32 = np.float32


# ------------------------------------------------------------------------------------------------ metrics
def hit_flags(rank_row, truth):
    """hit[i] = rank_row[i] is one of the truth ids (a -1 id matches nothing: truth ids are >= 0)."""
    t = set(int(x) for x in truth)
    return [int(x) in t for x in rank_row]


def precision_curve(hit):
    out, hits = [], 0
    for i, h in enumerate(hit):
        hits += 1 if h else 0
        out.append(F32(1.0 * hits / (i + 1)))
    return out


def recall_curve(hit, nt):
    """hits / truth_len in double, then float; truth_len 0 gives 0 / 0 = NaN as the C++ does."""
    out, hits = [], 0
    with np.errstate(divide="ignore", invalid="ignore"):
        for h in hit:
            hits += 1 if h else 0
            out.append(F32(np.float64(1.0 * hits) / np.float64(nt)))
    return out


def ap_curve(hit):
    out, hits, sum_pre = [], 0, F32(0.0)
    for i, h in enumerate(hit):
        if h:
            hits += 1
            pre = F32(1.0 * hits / (i + 1))
            sum_pre = F32(sum_pre + pre)                 # float accumulator
        out.append(F32(0.0) if hits == 0 else F32(sum_pre / F32(hits)))
    return out


def ndcg_curve(hit, nt):
    """dcg / idcg: float accumulators, every term 1.0 / log2(i + 2) added in double; idcg grows while i < truth_len."""
    out, dcg, idcg = [], F32(0.0), F32(0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i, h in enumerate(hit):
            w = 1.0 / math.log2(float(i + 2))
            if h:
                dcg = F32(np.float64(dcg) + w)
            if i < nt:
                idcg = F32(np.float64(idcg) + w)
            out.append(F32(dcg / idcg))
    return out


def mrr_curve(hit):
    out, rr = [], F32(0.0)
    seen = False
    for i, h in enumerate(hit):
        if h and not seen:
            rr, seen = F32(1.0 / (i + 1)), True
        out.append(rr)
    return out


def curve(metric_id, hit, nt):
    if metric_id == 1:
        return precision_curve(hit)
    if metric_id == 2:
        return recall_curve(hit, nt)
    if metric_id == 3:
        return ap_curve(hit)
    if metric_id == 4:
        return ndcg_curve(hit, nt)
    assert metric_id == 5
    return mrr_curve(hit)


def metrics_model(rank, truth_ptr, truth_items, metric_ids, K):
    """float32 [B, len(metric_ids) * K]: row b = the curves @1..K of rank[b] against truth_items[truth_ptr[b]:truth_ptr[b + 1]],
    in the order of metric_ids (1 precision, 2 recall, 3 AP, 4 NDCG, 5 MRR). The divisor of recall and the iDCG limit are the
    LENGTH of the truth list."""
    rank = np.asarray(rank)
    B = rank.shape[0]
    assert rank.shape[1] == K
    out = np.zeros((B, len(metric_ids) * K), F32)
    for b in range(B):
        truth = truth_items[int(truth_ptr[b]):int(truth_ptr[b + 1])]
        hit = hit_flags(rank[b], truth)
        for m, mid in enumerate(metric_ids):
            out[b, m * K:(m + 1) * K] = curve(mid, hit, len(truth))
    return out


def metric_cases(K, seed=0):
    """The rank / truth lists of one K: (rank int32 [R, K], truth lists, names). Single hits at the ballot-word edges, no hit, all
    hits, hits at every 64th rank, truth lengths 1 / K - 1 / K / K + 1 / 300 on both sides of the iDCG limit, -1 ids in the tail
    of the list, an empty truth list. Ids are distinct within a list; truth lists are shuffled and hold no duplicate."""
    rng = np.random.default_rng(1000 + 7 * K + seed)
    pool = 4096
    lens = [1, K - 1, K, K + 1, 300]
    rank, truth, names = [], [], []

    def add(name, hits, nt, cut=None):
        ids = rng.permutation(pool)
        r = ids[:K].astype(np.int32)
        rest = ids[K:]
        t = [int(r[p]) for p in hits]
        nt = max(nt, len(t))
        t += [int(x) for x in rest[:nt - len(t)]]
        if cut is not None:
            r = r.copy()
            r[cut:] = -1
        rank.append(r)
        truth.append([t[i] for i in rng.permutation(len(t))])
        names.append(name)

    for n, p in enumerate(sorted({0, 62, 63, 64, 65, 127, 128, 191, 192, 255, K - 1})):
        if p < K:
            add("hit@%d" % p, [p], max(1, lens[n % len(lens)]))
    for nt in lens:
        add("hit@last/nt=%d" % nt, [K - 1], max(1, nt))
    add("none", [], K)
    add("none/nt=300", [], 300)
    add("all", list(range(K)), K)
    add("all/nt=K+1", list(range(K)), K + 1)
    add("all/nt=300", list(range(K)), 300)
    if K > 1:
        add("all-but-last/nt=K-1", list(range(K - 1)), K - 1)
    add("every64", list(range(0, K, 64)), 1)
    add("every64/nt=300", list(range(0, K, 64)), 300)
    add("before-every64", [p for p in range(63, K, 64)], K)
    add("random", [p for p in range(K) if rng.random() < 0.3], 300)
    add("random/nt=K+1", [p for p in range(K) if rng.random() < 0.5], K + 1)
    add("tail=-1", [p for p in range(K) if p % 3 == 0], K, cut=(K + 1) // 2)      # hits beyond the cut are truth ids not listed
    add("all=-1", [], 5, cut=0)
    add("empty-truth", [], 0)
    return np.stack(rank), truth, names


def csr(lists, dtype=np.int32):
    ptr = np.zeros(len(lists) + 1, np.int64)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    flat = np.asarray([i for x in lists for i in x], dtype=dtype)
    return ptr, flat


# ------------------------------------------------------------------------------------------------ selection and merge
def stable_topk(scores, K):
    """(ids int32 [..., K], values) of the first K of a stable sort by score descending: equal scores keep ascending ids."""
    scores = np.asarray(scores)
    order = np.argsort(-scores, axis=-1, kind="stable")[..., :K]
    return order.astype(np.int32), np.take_along_axis(scores, order, -1)


def merge_model(cand_val, cand_idx, K):
    """Per row the K best (score desc, id asc) of the candidates whose id is >= 0; -1 / -inf where the row runs out. The valid ids
    of a row are distinct (the lists come from disjoint item ranges)."""
    cand_val, cand_idx = np.asarray(cand_val, F32), np.asarray(cand_idx)
    B = cand_val.shape[0]
    oi = np.full((B, K), -1, np.int32)
    ov = np.full((B, K), -np.inf, F32)
    for b in range(B):
        keep = np.flatnonzero(cand_idx[b] >= 0)
        order = keep[np.lexsort((cand_idx[b][keep], -cand_val[b][keep]))][:K]
        oi[b, :len(order)] = cand_idx[b][order]
        ov[b, :len(order)] = cand_val[b][order]
    return oi, ov


def _rank_of_each(v):
    """rank[t] = how many entries come before v[t] by (value desc, index asc)."""
    order = np.argsort(-v, kind="stable")
    rank = np.empty(len(v), np.int64)
    rank[order] = np.arange(len(v))
    return rank


def selection_walk(tile_max, scores, masked, K, floor, n_listed=None):
    """topk_tiles_kernel's decisions for one row and one chunk. tile_max [n_tiles]: the tiles' maxima BEFORE masking; scores [I]
    the chunk's scores; masked bool [I]; floor: None = the whole-catalogue form, -inf = the first chunk of the running form,
    otherwise the running list's K-th score. n_listed: the length of the row's mask list where the kernel takes it for the number
    of masked items (the whole-catalogue form; a repeated id counts twice)."""
    tile_max, scores, masked = np.asarray(tile_max, F32), np.asarray(scores, F32), np.asarray(masked, bool)
    running = floor is not None
    floor_v = F32(floor) if running else F32(-np.inf)
    n_masked = int(masked.sum()) if n_listed is None else int(n_listed)
    gm = np.full(256, -np.inf, F32)
    for t in range(min(256, len(tile_max))):
        gm[t] = tile_max[t::256].max()                       # thread t folds tiles t, t + 256, ...
    want = K - 1 + n_masked
    coarse = want < 64
    groups = gm.reshape(64, 4).max(1) if coarse else gm
    at = np.flatnonzero(_rank_of_each(groups) == want)
    tau = F32(groups[at[0]]) if len(at) else F32(-np.inf)
    th = max(tau, floor_v)
    n_ct = n = 0
    if th != -np.inf:
        cand_tiles = np.flatnonzero(tile_max >= th)
        n_ct = len(cand_tiles)
        if n_ct > TK_CAP:
            n = TK_CAP + 1
        else:
            pos = (cand_tiles[:, None] * TI + np.arange(TI)[None, :]).reshape(-1)
            pos = pos[pos < len(scores)]
            n = int(((scores[pos] >= th) & ~masked[pos]).sum())
    short_ok = bool(running and floor_v > tau)
    fallback = bool(n > TK_CAP or (n < K and not short_ok) or th == -np.inf)
    return {"coarse": coarse, "n_masked": n_masked, "tau": tau, "th": th, "n_tiles": n_ct, "n_cand": n, "short_ok": short_ok,
            "fallback": fallback, "accepted_short": bool(not fallback and n < K), "over_cap": bool(n > TK_CAP)}


def chunk_bounds(I, chunked):
    """Item ranges of the scorer launches: the top-K-only form of K <= 256 starts with a pilot chunk."""
    if I <= SCORE_CHUNK:
        return [(0, I)]
    out, at = [], 0
    while at < I:
        step = SCORE_PILOT if (chunked and at == 0) else SCORE_CHUNK
        out.append((at, min(at + step, I)))
        at = out[-1][1]
    return out


# ------------------------------------------------------------------------------------------------ tables and mask lists
def continuous_table(U, I, d, S, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((U + I, (1 + S) * d)) * 0.3).astype(F32)


def nine_row_table(U, I, d, S, seed):
    """Nine distinct item rows repeated over the catalogue: every user sees at most nine score values (massive ties, far more
    than TK_CAP candidates at any threshold)."""
    Y = continuous_table(U, I, d, S, seed)
    Y[U:] = np.tile(Y[U:U + 9], ((I + 8) // 9, 1))[:I]
    return Y


def tie_block_table(U, I, d, S, K, seed):
    """About 2 K copies of one item row that every user scores above the ordinary items, and K / 2 distinct rows that every user
    scores higher still: the block of equal scores covers the ranks K / 2 .. 5 K / 2 of every user, across rank K. The copies
    are spread over the whole id range (every chunk, many tiles)."""
    rng = np.random.default_rng(seed)
    W = (1 + S) * d
    n_block, n_top = min(2 * K, I - K), K // 2
    Y = (rng.standard_normal((U + I, W)) * 0.05).astype(F32)
    c = rng.standard_normal(W).astype(F32)
    c /= np.linalg.norm(c[:d])
    Y[:U] += c                                               # every user leans the same way in every block
    ids = rng.permutation(I)
    Y[U + ids[:n_block]] = 3.0 * c
    for j, i in enumerate(ids[n_block:n_block + n_top]):
        Y[U + i] = (3.5 + 0.01 * j) * c
    return Y


MASK_KINDS = ["none", "top:K-1+m=62", "top:K-1+m=63", "top:K-1+m=64", "top:K+m=255", "top:K+m=256", "top:K+m=257", "duplicate",
              "all-but-4", "all-but-K-1", "all-but-K", "last-chunk-only", "first-chunk-only", "few-then-last"]


def mask_cases(raw, K):
    """Mask lists of the rows of raw [B, I] (unmasked scores of a first scoring call), one kind per row in turn:
    (lists, kinds, short) -- short = the rows left with fewer than K unmasked items, by construction.
      top:*            the row's own best m items, m such that K - 1 + n_masked is 62 / 63 / 64 (coarse | fine ranking) or
                       K + n_masked is 255 / 256 / 257 (the last threshold | none): the masked items own the group maxima
      duplicate        an id listed twice
      all-but-*        4, K - 1 and K items left
      last-chunk-only  only items of the last scorer launch left (its last 232 at most: fewer than K where K is larger)
      first-chunk-only only items of the pilot chunk left
      few-then-last    K / 2 items of the pilot chunk and K of the last launch: the running list is still short when it arrives"""
    B, I = raw.shape
    rng = np.random.default_rng(31 * K + I)
    last0 = chunk_bounds(I, False)[-1][0] if I > SCORE_CHUNK else (I * 3) // 4
    first1 = min(SCORE_PILOT, I // 2)
    lists, kinds, short = [], [], []
    for b in range(B):
        kind = MASK_KINDS[b % len(MASK_KINDS)]
        keep = None
        if kind.startswith("top:"):
            total = int(kind.split("=")[1])
            m = total - (K - 1) if "K-1+m" in kind else total - K
            if m <= 0 or m > I - K:
                kind, lst = "none", []
            else:
                lst = np.argsort(-raw[b], kind="stable")[:m].tolist()
                lst = [lst[i] for i in rng.permutation(m)]
        elif kind == "duplicate":
            lst = rng.choice(I, size=20, replace=False).tolist()
            lst.insert(7, lst[13])
        elif kind == "all-but-4":
            keep = rng.choice(I, size=4, replace=False)
        elif kind == "all-but-K-1":
            keep = rng.choice(I, size=K - 1, replace=False)
        elif kind == "all-but-K":
            keep = rng.choice(I, size=K, replace=False)
        elif kind == "last-chunk-only":
            keep = np.arange(max(last0, I - 232), I)
        elif kind == "first-chunk-only":
            keep = np.arange(first1)
        elif kind == "few-then-last":
            tail = np.arange(last0, I) if I - last0 >= K else np.arange(I - K, I)
            keep = np.concatenate([rng.choice(first1, size=K // 2, replace=False), rng.choice(tail, size=K, replace=False)])
        else:
            lst = []
        if keep is not None:
            gone = np.ones(I, bool)
            gone[keep] = False
            lst = np.flatnonzero(gone).tolist()
            if len(np.unique(keep)) < K:
                short.append(b)
        lists.append([int(x) for x in lst])
        kinds.append(kind)
    return lists, kinds, short


# ------------------------------------------------------------------------------------------------ the selection cases
SEL_U, SEL_B, SEL_S = 60, 37, 3
SEL_USERS = (np.arange(SEL_B) * 7) % SEL_U               # 37 distinct users, not in order
K_ONE_CHUNK = (63, 64, 65, 128, 255, 256, 257, 512, 513)
K_CHUNKED = (64, 256, 257)
# (recdim, catalogue, K values): recdim 64 = the 16-user scorers with tile maxima, 48 = the generic scorer without
SEL_SHAPES = [(64, 3000, K_ONE_CHUNK), (48, 3000, K_ONE_CHUNK + (1024,)), (64, 16400, K_CHUNKED), (64, 33000, K_CHUNKED)]
SEL_TABLES = ("continuous", "nine", "tieblock")


def selection_table(name, I, d, K):
    if name == "continuous":
        return continuous_table(SEL_U, I, d, SEL_S, 11)
    if name == "nine":
        return nine_row_table(SEL_U, I, d, SEL_S, 12)
    assert name == "tieblock"
    return tie_block_table(SEL_U, I, d, SEL_S, K, 13)
