"""Float64 numpy model of the list kernels (csrc/lists.hip) -- the mean pairwise cosine of id lists, the exposure counters -- and of
the list report's rows, means, exposure summary and shift."""
import numpy as np


def _inv(sq):
    return 1.0 / np.maximum(np.sqrt(np.asarray(sq, dtype=np.float64)), 1e-12)


def pair_cosine64(T, sq32, lists, blocks):
    """out [B x blocks] float64: per list and column block of T [n x blocks * d] the mean over position pairs i < j with both
    entries in [0, n) of dot(T[a], T[b]) inv(sq[a]) inv(sq[b]), inv(x) = 1 / max(sqrt(x), 1e-12); sq32 [n x blocks]: the squared
    norms the kernel is given. NaN with fewer than two listed entries. Vectorised."""
    T = np.asarray(T, dtype=np.float64)
    n, d = T.shape[0], T.shape[1] // blocks
    inv = _inv(np.asarray(sq32).reshape(n, blocks))
    lists = np.asarray(lists, dtype=np.int64)
    out = np.full((lists.shape[0], blocks), np.nan)
    for b, row in enumerate(lists):
        ids = row[(row >= 0) & (row < n)]
        m = ids.size
        if m < 2:
            continue
        iu = np.triu_indices(m, 1)
        for h in range(blocks):
            R = T[ids, h * d:(h + 1) * d]
            G = (R @ R.T) * inv[ids, h][:, None] * inv[ids, h][None, :]
            out[b, h] = G[iu].sum() / (m * (m - 1) / 2.0)
    return out


def pair_cosine64_loops(T, sq32, lists, blocks):
    """pair_cosine64 as plain loops over lists, blocks and position pairs."""
    T = np.asarray(T, dtype=np.float64)
    n, d = T.shape[0], T.shape[1] // blocks
    sq = np.asarray(sq32, dtype=np.float64).reshape(n, blocks)
    out = np.full((len(lists), blocks), np.nan)
    for b in range(len(lists)):
        K = len(lists[b])
        for h in range(blocks):
            total, pairs = 0.0, 0
            for i in range(K):
                for j in range(i + 1, K):
                    a, c = int(lists[b][i]), int(lists[b][j])
                    if a < 0 or a >= n or c < 0 or c >= n:
                        continue
                    dot = 0.0
                    for k in range(d):
                        dot += T[a, h * d + k] * T[c, h * d + k]
                    total += dot / (max(np.sqrt(sq[a, h]), 1e-12) * max(np.sqrt(sq[c, h]), 1e-12))
                    pairs += 1
            if pairs:
                out[b, h] = total / pairs
    return out


def exposure(lists, n):
    """How often every id of [0, n) occurs in the lists (entries outside are skipped): int64 [n]."""
    x = np.asarray(lists, dtype=np.int64).reshape(-1)
    return np.bincount(x[(x >= 0) & (x < n)], minlength=n)[:n]


def rows(ils32, lists, item_counts):
    """The list report's user rows: the ils columns as given (float32), then pop = the mean training count of the listed items
    (float64 quotient rounded to float32, NaN for an empty list)."""
    lists = np.asarray(lists, dtype=np.int64)
    listed = lists >= 0
    with np.errstate(invalid="ignore", divide="ignore"):
        pop = np.where(listed, np.asarray(item_counts, dtype=np.float64)[np.maximum(lists, 0)], 0.0).sum(1) / listed.sum(1)
    return np.concatenate([np.asarray(ils32, dtype=np.float32), pop.astype(np.float32)[:, None]], 1)


def means(rows32, positions):
    """Float64 means of the float32 rows per group of row positions."""
    return np.stack([np.asarray(rows32)[p].astype(np.float64).mean(0) for p in positions])


def exposure_summary_loops(counts, positions):
    """evaluator.exposure_summary restated with explicit loops: per group items, coverage, gini (sorted-counts formula
    sum_i (2 i - n - 1) c_(i) / (n sum c)), entropy in bits, slot_share."""
    total = float(sum(float(c) for c in counts))
    out = []
    for at in positions:
        c = sorted(float(counts[int(i)]) for i in at)
        n, s = len(c), float(sum(c))
        covered = sum(1 for x in c if x > 0)
        gini = entropy = 0.0
        if n and s > 0:
            acc = 0.0
            for i, x in enumerate(c):
                acc += (2.0 * (i + 1) - n - 1.0) * x
            gini = acc / (n * s)
            for x in c:
                if x > 0:
                    entropy -= (x / s) * np.log2(x / s)
        out.append([float(n), covered / float(n) if n else 0.0, gini, entropy, s / total if total > 0 else 0.0])
    return np.asarray(out, dtype=np.float64).reshape(len(positions), 5)


def shift_rows(rows_a, lists_a, rows_b, lists_b):
    """The shift report's rows: overlap = |a & b| / K (fillers never match), then b - a per column in float32."""
    K = np.asarray(lists_a).shape[1]
    over = [len(set(int(x) for x in ra if x >= 0) & set(int(x) for x in rb if x >= 0)) / float(K) for ra, rb in zip(lists_a, lists_b)]
    return np.concatenate([np.asarray(over, dtype=np.float64).astype(np.float32)[:, None],
                           np.asarray(rows_b, dtype=np.float32) - np.asarray(rows_a, dtype=np.float32)], 1)
