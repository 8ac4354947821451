"""Float64 numpy model of the cosine top-K lists (csrc/knn.hip), of list_overlap and of the neighbour report's rows and means."""
import numpy as np


def tol(d):
    """Bound on |fp32 score - float64 score|: the worst case of an fp32 dot product of length d in any summation order is
    d u |a||b| (u = 2^-24); the roundings of two norms, their floors and the products add a few u; doubled for an approximate
    reciprocal square root with a Newton step. Derived, not measured."""
    return 2.0 * (d + 8) * 2.0 ** -24


def cos64(T, rows=None):
    """Scores of `rows` (default all) against every row of T: dot / (max(|q|, 1e-12) max(|c|, 1e-12)), float64."""
    T = np.asarray(T, dtype=np.float64)
    nrm = np.maximum(np.sqrt((T * T).sum(1)), 1e-12)
    q = np.arange(T.shape[0]) if rows is None else np.asarray(rows, dtype=np.int64)
    return (T[q] @ T.T) / (nrm[q][:, None] * nrm[None, :])


def cos64_loops(T):
    T = np.asarray(T, dtype=np.float64)
    n, d = T.shape
    out = np.zeros((n, n))
    for a in range(n):
        for b in range(n):
            dot = na = nb = 0.0
            for k in range(d):
                dot += T[a, k] * T[b, k]
                na += T[a, k] * T[a, k]
                nb += T[b, k] * T[b, k]
            out[a, b] = dot / (max(np.sqrt(na), 1e-12) * max(np.sqrt(nb), 1e-12))
    return out


def masked(scores, rows, exclude_self=True, excl=None):
    """Scores with the left-out entries at -inf: the query row itself, then the query's list of excl (one list per query)."""
    s = np.array(scores, dtype=np.float64, copy=True)
    for b, q in enumerate(rows):
        if exclude_self:
            s[b, int(q)] = -np.inf
        if excl is not None:
            for e in excl[b]:
                s[b, int(e)] = -np.inf
    return s


def topk64(scores, K):
    """Per row the K best by (score descending, id ascending); -inf entries are no candidates: ids -1 / values -inf behind."""
    scores = np.asarray(scores, dtype=np.float64)
    B, n = scores.shape
    ids = np.full((B, K), -1, dtype=np.int64)
    vals = np.full((B, K), -np.inf)
    for b in range(B):
        order = np.lexsort((np.arange(n), -scores[b]))
        order = order[scores[b, order] > -np.inf][:K]
        ids[b, :order.size] = order
        vals[b, :order.size] = scores[b, order]
    return ids, vals


def overlap(a, b):
    """Per row the number of ids >= 0 of a[r] that occur in b[r]."""
    return np.asarray([len(set(int(x) for x in ra if x >= 0) & set(int(x) for x in rb if x >= 0)) for ra, rb in zip(a, b)],
                      dtype=np.int32)


def csr(lists):
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=ptr[1:])
    return ptr, np.asarray([int(i) for x in lists for i in x], dtype=np.int32)


def rising_case(n, d, Q):
    """The case in which every candidate beats the running threshold: (T float32 [n x d], query rows [Q], exclusion lists). Rows
    0 .. n - 2 are unit vectors at evenly spaced angles from 150 down to 30 degrees to the LAST row, in a random plane of R^d, so the
    cosine to the last row rises strictly with the row id and adjacent scores differ by >= sin(30) * (120 degrees / (n - 2)) -- 2.5e-4
    at n = 4113, against tol(32) = 4.8e-6. A query whose own score (1) has to be the largest can only be the last row: all Q
    queries are that row, told apart by their exclusion lists -- none; the 300 best candidates; every second row; a few single ones."""
    ang = np.concatenate([np.linspace(5 * np.pi / 6, np.pi / 6, n - 1), [0.0]])
    basis, _ = np.linalg.qr(np.random.default_rng(0).standard_normal((d, d)))
    T = (np.cos(ang)[:, None] * basis[:, 0] + np.sin(ang)[:, None] * basis[:, 1]).astype(np.float32)
    excl = [[], list(range(n - 301, n - 1)), list(range(0, n, 2))] + [[n - 2 - b, 5 * b, n - 2 - b] for b in range(3, Q)]
    return T, np.full(Q, n - 1, dtype=np.int64), excl[:Q]


def min_gap(s):
    """The smallest difference between two scores of one row of s (masked float64 scores), -inf entries left out."""
    return min(float(np.diff(np.sort(r[r > -np.inf])).min()) for r in s if (r > -np.inf).sum() > 1)


def report_rows(ids, vals, counts, k):
    """The neighbour report's rows from the lists: ids / vals [1 + S x I x k] (fused first), counts [I] training interactions.
    Columns: overlap per head, mean score per space, mean count per space; float64 quotients rounded to float32 (what a row
    holds), NaN where a list is empty."""
    ids, vals = np.asarray(ids), np.asarray(vals, dtype=np.float64)
    S, I = ids.shape[0] - 1, ids.shape[1]
    listed = ids >= 0
    n = listed.sum(2).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        over = np.stack([np.where(n[0] > 0, overlap(ids[0], ids[1 + h]) / float(k), np.nan) for h in range(S)], 1) if S else np.zeros((I, 0))
        cos = (np.where(listed, vals, 0.0).sum(2) / n).T
        pop = (np.where(listed, np.asarray(counts, dtype=np.float64)[np.maximum(ids, 0)], 0.0).sum(2) / n).T
    return np.concatenate([over, cos, pop], 1).astype(np.float32)


def report_means(rows, positions):
    """Float64 means of the float32 rows per group of row positions."""
    return np.stack([rows[p].astype(np.float64).mean(0) for p in positions])


# ---- cross_topk (csrc/knn.hip with a query table of its own): the kernel's own expression in np.float32
def inv_norm32(sq, n):
    """cosine.h::inv_norm per row in np.float32: 1 / max(sqrt(sq), 1e-12f), both correctly rounded; sq = None: a vector of ones."""
    if sq is None:
        return np.ones(n, dtype=np.float32)
    with np.errstate(all="ignore"):
        return np.float32(1.0) / np.maximum(np.sqrt(np.asarray(sq, dtype=np.float32)), np.float32(1e-12))


def fma_chain_dot32(A, B):
    """[len(A) x len(B)] float32 dot products as the k-ordered fmaf chain the matrix instruction runs: acc <- fl32(a_k b_k + acc), the
    product unrounded (exact in float64). The float64 sum is exact for the operands this is used with (small integers, powers of two
    of one magnitude), so there is no double rounding. A product beyond float32 overflows only when the SUM is rounded: +inf plus a
    finite product of the other sign stays +inf, where separate float32 multiplies and adds would give inf - inf = NaN."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    acc = np.zeros((A.shape[0], B.shape[0]), dtype=np.float32)
    with np.errstate(all="ignore"):
        for k in range(A.shape[1]):
            acc = (A[:, k, None] * B[None, :, k] + acc.astype(np.float64)).astype(np.float32)
    return acc


def cross_scores32(Tq, sqq, T, sq, rows, chain=False):
    """float32 [len(rows) x n] scores (dot * invq) * invc in the kernel's order; rows: valid query ids. The dot product: a float64
    matrix product rounded once (exact when every partial sum is a float32, as for integer tables with |entry| <= 8 and d <= 256) or
    fma_chain_dot32 (chain=True)."""
    Tq, T = np.asarray(Tq, dtype=np.float32), np.asarray(T, dtype=np.float32)
    rows = np.asarray(rows, dtype=np.int64)
    dot = fma_chain_dot32(Tq[rows], T) if chain else (Tq[rows].astype(np.float64) @ T.astype(np.float64).T).astype(np.float32)
    with np.errstate(all="ignore"):
        return (dot * inv_norm32(sqq, Tq.shape[0])[rows][:, None]) * inv_norm32(sq, T.shape[0])[None, :]


def cross_lists32(Tq, sqq, T, sq, rows, K, excl=None, chain=False):
    """(ids int64, values float32) [Q x K] of cross_topk: a query id outside the query table gives a row of fillers, an exclusion id
    outside [0, n) excludes nothing, a score of -inf or NaN is no candidate (the kernel keeps what is > its threshold, -inf at
    first), +inf ranks first, ties by id."""
    rows = np.asarray(rows, dtype=np.int64)
    nq, n = np.asarray(Tq).shape[0], np.asarray(T).shape[0]
    ok = (rows >= 0) & (rows < nq)
    s = cross_scores32(Tq, sqq, T, sq, np.where(ok, rows, 0), chain).astype(np.float64) if nq else np.zeros((rows.size, n))
    s[np.isnan(s)] = -np.inf
    s[~ok] = -np.inf
    if excl is not None:
        for b, lst in enumerate(excl):
            hit = [int(e) for e in lst if 0 <= int(e) < n]
            s[b, hit] = -np.inf
    ids, vals = topk64(s, K)
    return ids, vals.astype(np.float32)
