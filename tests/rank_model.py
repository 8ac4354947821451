"""A numpy model of csrc/rank.hip's three kernels, written from their definitions; nothing here calls elimrec_amd.

ranks():     rank = #{ j in [0, I) : s_j > s_t  or  (s_j == s_t and j < t) }, -1 where s_t == -inf
pair_rows(): rank, rr = 1 / (rank + 1), pct = rank / (n_cand - 1) (0 when n_cand <= 1), hit@K = (rank < K); NaN row where rank < 0
user_rows(): auc = 1 - sum_t (rank_t - #valid targets ranked above t) / (T N_neg), mrr_full = 1 / (min rank + 1), first_rank;
             NaN when T == 0 or N_neg <= 0
The row functions return float64 computed with the kernels' operations in the kernels' order; .astype(np.float32) is the one
rounding the kernels make."""
import numpy as np


def csr(lists):
    """(ptr int64 [B + 1], flat int32) of a list of lists."""
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=ptr[1:])
    return ptr, np.asarray([i for x in lists for i in x], dtype=np.int32)


def ranks(block, ptr, items):
    """block [B x I] float32 (only its I columns), targets as CSR -> int32 [len(items)]."""
    block = np.asarray(block)
    B, I = block.shape
    out = np.empty(len(items), dtype=np.int32)
    ids = np.arange(I)
    for b in range(B):
        row = block[b]
        for p in range(int(ptr[b]), int(ptr[b + 1])):
            t = int(items[p])
            s = row[t]
            out[p] = -1 if s == -np.inf else int(((row > s) | ((row == s) & (ids < t))).sum())
    return out


def pair_rows(rank, n_cand, ks):
    rank = np.asarray(rank, dtype=np.int64)
    n_cand = np.asarray(n_cand, dtype=np.int64)
    out = np.full((rank.size, 3 + len(ks)), np.nan, dtype=np.float64)
    ok = rank >= 0
    r = rank[ok].astype(np.float64)
    nc = n_cand[ok]
    out[ok, 0] = r
    out[ok, 1] = 1.0 / (r + 1.0)
    out[ok, 2] = np.where(nc <= 1, 0.0, r / np.where(nc <= 1, 1.0, nc.astype(np.float64) - 1.0))
    for c, k in enumerate(ks):
        out[ok, 3 + c] = (rank[ok] < int(k)).astype(np.float64)
    return out


def user_rows(rank, ptr, n_cand):
    rank = np.asarray(rank, dtype=np.int64)
    B = len(ptr) - 1
    out = np.full((B, 3), np.nan, dtype=np.float64)
    for b in range(B):
        r = rank[int(ptr[b]):int(ptr[b + 1])]
        r = r[r >= 0]
        T = r.size
        n_neg = float(int(n_cand[b])) - float(T)
        if T == 0 or n_neg <= 0.0:
            continue
        total = sum(int(x) - int((r < x).sum()) for x in r)          # exact integers
        out[b, 0] = 1.0 - float(total) / (float(T) * n_neg)
        out[b, 1] = 1.0 / (float(r.min()) + 1.0)
        out[b, 2] = float(r.min())
    return out
