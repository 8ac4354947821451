"""An exact host model of the co-interaction neighbours (csrc/cooccur.hip, ops.cooccur_topk) and of the report's columns.

The graph is the CSR q_ptr / q_nbr of the query side (row -> its neighbours on the other side). scipy.sparse forms A^T A from it with
repeated edges kept (duplicates are summed, so an edge listed twice has weight 2 and c is the product count); the three scores are
computed in float64 and rounded once to fp32; the order is a stable sort by (score descending, id ascending)."""
import collections

import numpy as np
import scipy.sparse as sp


def transpose_csr(ptr, nbr, n_other):
    """The other direction of the same edges: (o_ptr int64 [n_other + 1], o_nbr int64), rows in ascending order within a segment."""
    ptr, nbr = np.asarray(ptr, dtype=np.int64), np.asarray(nbr, dtype=np.int64)
    rows = np.repeat(np.arange(ptr.size - 1, dtype=np.int64), np.diff(ptr))
    order = np.argsort(nbr, kind="stable")
    o_ptr = np.zeros(n_other + 1, dtype=np.int64)
    np.cumsum(np.bincount(nbr, minlength=n_other), out=o_ptr[1:])
    return o_ptr, rows[order]


def csr_of(lists):
    """(ptr int64, flat int64) of a list of id lists."""
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=ptr[1:])
    flat = np.asarray([i for x in lists for i in x], dtype=np.int64)
    return ptr, flat


def incidence(q_ptr, q_nbr, n_other):
    """B [n_query x n_other] int64 with B[q, u] = the number of times the edge (q, u) is listed."""
    q_ptr, q_nbr = np.asarray(q_ptr, dtype=np.int64), np.asarray(q_nbr, dtype=np.int64)
    n = q_ptr.size - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(q_ptr))
    B = sp.coo_matrix((np.ones(q_nbr.size, dtype=np.int64), (rows, q_nbr)), shape=(n, n_other)).tocsr()
    B.sum_duplicates()
    return B


def walk(q_ptr, q_nbr, n_other):
    """W(q) of every row: the sum of deg(u) over the row's segment (int64)."""
    q_ptr, q_nbr = np.asarray(q_ptr, dtype=np.int64), np.asarray(q_nbr, dtype=np.int64)
    deg_o = np.bincount(q_nbr, minlength=n_other).astype(np.int64)
    along = np.concatenate([[0], np.cumsum(deg_o[q_nbr])])
    return along[q_ptr[1:]] - along[q_ptr[:-1]]


def scores(c, a, b, measure):
    """float32 scores from the three integers (arrays of one shape): float64 arithmetic, rounded once."""
    c, a, b = (np.asarray(x, dtype=np.float64) for x in (c, a, b))
    with np.errstate(divide="ignore", invalid="ignore"):
        if measure == "count":
            s = c
        elif measure == "cosine":
            s = c / np.sqrt(a * b)
        elif measure == "jaccard":
            s = c / (a + b - c)
        else:
            raise ValueError(measure)
    return s.astype(np.float32)


def topk(q_ptr, q_nbr, n_other, rows, K, measure):
    """(idx int32, val float32, cnt int32) [Q x K]: the model of ops.cooccur_topk."""
    q_ptr = np.asarray(q_ptr, dtype=np.int64)
    B = incidence(q_ptr, q_nbr, n_other)
    deg = np.diff(q_ptr)
    rows = np.asarray(rows, dtype=np.int64)
    idx = np.full((rows.size, K), -1, dtype=np.int32)
    val = np.full((rows.size, K), -np.inf, dtype=np.float32)
    cnt = np.zeros((rows.size, K), dtype=np.int32)
    C = (B[rows] @ B.T).tocsr() if rows.size else None
    for r, q in enumerate(rows):
        lo, hi = C.indptr[r], C.indptr[r + 1]
        j, c = C.indices[lo:hi].astype(np.int64), C.data[lo:hi].astype(np.int64)
        keep = (j != q) & (c >= 1)
        j, c = j[keep], c[keep]
        s = scores(c, np.full(j.size, deg[q]), deg[j], measure)
        first = np.argsort(j, kind="stable")
        j, c, s = j[first], c[first], s[first]
        order = np.argsort(-s.astype(np.float64), kind="stable")[:K]      # stable: ascending id among equal scores
        n = order.size
        idx[r, :n], val[r, :n], cnt[r, :n] = j[order], s[order], c[order]
    return idx, val, cnt


def dense_groups(walk_of_rows, lds, cap, max_groups, threads=256):
    """Which query positions each workgroup of the dense form serves (cooccur_dense_kernel): position p is a dense row when lds is
    off or its walk is past `cap` = COOCCUR_SLOTS / 2; G = min(dense rows, max_groups) workgroups run, workgroup b takes the dense
    positions p = b (mod G) in ascending order, `threads` of its residue's positions per pass of its outer loop. Returns a list of G
    lists of (pass, position)."""
    walk_of_rows = np.asarray(walk_of_rows, dtype=np.int64)
    dense = ~((walk_of_rows <= cap) & bool(lds))
    G = min(int(dense.sum()), int(max_groups))
    return [[(int(p // G) // threads, int(p)) for p in range(b, dense.size, G) if dense[p]] for b in range(G)]


Schedule = collections.namedtuple("Schedule", "cuts appended dropped longest ids")


def dense_schedule(graph, q, K, measure, cap, users=16, entries=64):
    """The bookkeeping of the dense form's pass 2 for query row q. graph: (q_ptr, q_nbr, o_ptr, o_nbr). The row's segment is walked
    `users` neighbours at a time, `entries` entries of each neighbour's list per step; a candidate is claimed (with its whole count
    c) at the first step that meets it, and appended to the running list if and only if its key (score, then the lower id) exceeds
    the threshold read at the top of that step; after a step that leaves the list longer than cap - users * entries the list is
    sorted and, holding at least K, cut to its K best, whose last key becomes the threshold. Returns Schedule(cuts, appended,
    dropped by the threshold, the longest list met, the final list's K best ids).
    Deterministic although the kernel is not: which lane wins a claim inside a step changes neither the candidate's count (pass 1
    is complete), nor its key, nor the threshold it meets (read once per step), so it changes none of these numbers."""
    q_ptr, q_nbr, o_ptr, o_nbr = (np.asarray(x, dtype=np.int64) for x in graph)
    deg = np.diff(q_ptr)
    seg = q_nbr[q_ptr[q]:q_ptr[q + 1]]
    lists = [o_nbr[o_ptr[u]:o_ptr[u + 1]] for u in seg]
    c = np.zeros(deg.size, dtype=np.int64)
    for held in lists:
        np.add.at(c, held, 1)
    score = scores(c, np.full(deg.size, deg[q]), deg, measure)
    limit = cap - users * entries
    claimed, kept, thr = {int(q)}, [], None
    cuts = appended = dropped = longest = 0
    for e0 in range(0, len(lists), users):
        f, batch = 0, lists[e0:e0 + users]
        while True:
            top = thr
            for held in batch:
                for j in held[f:f + entries].tolist():
                    if j in claimed:
                        continue
                    claimed.add(j)
                    key = (float(score[j]), -j)
                    if top is None or key > top:
                        kept.append(key)
                        appended += 1
                    else:
                        dropped += 1
            f += entries
            longest = max(longest, len(kept))
            if len(kept) > limit:
                cuts += 1
                kept.sort(reverse=True)
                if len(kept) >= K:
                    kept, thr = kept[:K], kept[K - 1]
            if not any(f < held.size for held in batch):
                break
    kept.sort(reverse=True)
    return Schedule(cuts, appended, dropped, longest, [-k[1] for k in kept[:K]])


def report_rows(co_idx, co_val, item_counts, space_lists):
    """The report's per-item columns in float64 [n x (3 + spaces)]: co_n, co_score (mean score of the listed), co_pop (their mean
    training interactions), co_overlap_<space> (the share of the listed co-neighbours the space's list also holds). co_val as fp32."""
    n = co_idx.shape[0]
    out = np.zeros((n, 3 + len(space_lists)), dtype=np.float64)
    for r in range(n):
        ids = co_idx[r][co_idx[r] >= 0]
        m = ids.size
        out[r, 0] = m
        if m == 0:
            out[r, 1:] = np.nan
            continue
        out[r, 1] = co_val[r, :m].astype(np.float64).sum() / m
        out[r, 2] = np.asarray(item_counts, dtype=np.float64)[ids].sum() / m
        for s, lists in enumerate(space_lists):
            out[r, 3 + s] = np.isin(ids, lists[r][lists[r] >= 0]).sum() / m
    return out
