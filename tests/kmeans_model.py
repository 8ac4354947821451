"""Float64 numpy model of spherical k-means (csrc/kmeans.hip, ops.spherical_kmeans): the assignment by largest cosine, the
centroid update as the normalised sum of the members' unit rows, Lloyd's loop, plain-loop forms of each, and the pure row functions'
inputs. The tolerance on a cosine is knn_model.tol(d)."""
import numpy as np

from knn_model import tol                                                   # noqa: F401  (2 (d + 8) 2^-24, derived there)


def _norms(T):
    T = np.asarray(T, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return (T * T).sum(1)


def _usable(sq):
    return np.isfinite(sq) & (sq > 0)


def assign64(T, Cen):
    """(assign int64 [n], cos float64 [n], margin float64 [n]): per row the centroid with the largest cosine
    dot / (max(|row|, 1e-12) max(|centroid|, 1e-12)), the lowest id among equals; margin = the best minus the second-best cosine
    over the usable centroids (inf with fewer than two). A row whose squared norm is 0 or not finite gets -1 / -inf (margin inf);
    a centroid whose squared norm is 0 or not finite is never chosen (no usable centroid: -1 / -inf)."""
    T, Cen = np.asarray(T, dtype=np.float64), np.asarray(Cen, dtype=np.float64)
    sq_t, sq_c = _norms(T), _norms(Cen)
    ok_t, ok_c = _usable(sq_t), _usable(sq_c)
    n = T.shape[0]
    assign = np.full(n, -1, dtype=np.int64)
    cos = np.full(n, -np.inf)
    margin = np.full(n, np.inf)
    if not ok_c.any() or not ok_t.any():
        return assign, cos, margin
    rows, cols = np.flatnonzero(ok_t), np.flatnonzero(ok_c)
    s = (T[rows] @ Cen[cols].T) / (np.maximum(np.sqrt(sq_t[rows]), 1e-12)[:, None] * np.maximum(np.sqrt(sq_c[cols]), 1e-12)[None, :])
    best = s.argmax(1)                                                     # (the first among equals: the lowest id)
    assign[rows] = cols[best]
    cos[rows] = s[np.arange(rows.size), best]
    if cols.size > 1:
        part = np.partition(s, cols.size - 2, axis=1)
        margin[rows] = part[:, -1] - part[:, -2]
    return assign, cos, margin


def assign64_loops(T, Cen):
    T, Cen = np.asarray(T, dtype=np.float64), np.asarray(Cen, dtype=np.float64)
    n, C = T.shape[0], Cen.shape[0]
    assign, cos, margin = np.full(n, -1, dtype=np.int64), np.full(n, -np.inf), np.full(n, np.inf)
    for r in range(n):
        sq = float(sum(x * x for x in T[r]))
        if not (np.isfinite(sq) and sq > 0):
            continue
        scores = []
        for c in range(C):
            sc = float(sum(x * x for x in Cen[c]))
            if not (np.isfinite(sc) and sc > 0):
                continue
            dot = float(sum(x * y for x, y in zip(T[r], Cen[c])))
            scores.append((dot / (max(np.sqrt(sq), 1e-12) * max(np.sqrt(sc), 1e-12)), c))
        if not scores:
            continue
        best = max(s for s, _ in scores)
        assign[r] = min(c for s, c in scores if s == best)
        cos[r] = best
        if len(scores) > 1:
            ordered = sorted((s for s, _ in scores), reverse=True)
            margin[r] = ordered[0] - ordered[1]
    return assign, cos, margin


def update64(T, assign, Cen, C):
    """(sums float64 [C x d], counts int64 [C], centroids float64 [C x d]): per cluster the sum of the unit rows of its members
    (assign[r] == c, the row's squared norm finite and not 0; entries outside [0, C) belong nowhere), the members, and
    sum / |sum| -- the previous centroid Cen[c] where the cluster has no member or its sum has norm 0."""
    T, Cen = np.asarray(T, dtype=np.float64), np.asarray(Cen, dtype=np.float64)
    assign = np.asarray(assign, dtype=np.int64)
    sq = _norms(T)
    member = _usable(sq) & (assign >= 0) & (assign < C)
    rows = np.flatnonzero(member)
    unit = T[rows] / np.maximum(np.sqrt(sq[rows]), 1e-12)[:, None]
    sums = np.zeros((C, T.shape[1]))
    np.add.at(sums, assign[rows], unit)
    counts = np.bincount(assign[rows], minlength=C).astype(np.int64)
    norm = np.sqrt((sums * sums).sum(1))
    cen = np.array(Cen, copy=True)
    moved = (counts > 0) & (norm > 0)
    cen[moved] = sums[moved] / norm[moved, None]
    return sums, counts, cen


def update64_loops(T, assign, Cen, C):
    T, Cen = np.asarray(T, dtype=np.float64), np.asarray(Cen, dtype=np.float64)
    d = T.shape[1]
    sums, counts, cen = np.zeros((C, d)), np.zeros(C, dtype=np.int64), np.array(Cen, copy=True)
    for r in range(T.shape[0]):
        c = int(assign[r])
        sq = float(sum(x * x for x in T[r]))
        if not 0 <= c < C or not (np.isfinite(sq) and sq > 0):
            continue
        for k in range(d):
            sums[c, k] += T[r, k] / max(np.sqrt(sq), 1e-12)
        counts[c] += 1
    for c in range(C):
        norm = np.sqrt(float(sum(x * x for x in sums[c])))
        if counts[c] > 0 and norm > 0:
            cen[c] = sums[c] / norm
    return sums, counts, cen


def default_init(T, C, seed):
    """The default first centroids of ops.spherical_kmeans: the first C of a seeded permutation of the rows with a usable norm, the
    norms as the device sees them (float32 sums of squares round the same way for these tests' purposes: a usable row stays usable)."""
    good = np.flatnonzero(_usable(_norms(T)))
    return good[np.random.default_rng(seed).permutation(good.size)[:C]]


def lloyd64(T, init, iters):
    """Lloyd's loop as ops.spherical_kmeans runs it: iteration i assigns against the centroids of iteration i - 1 (the init rows
    first), stops without an update when i > 1 and nothing changed, else updates. -> dict(assign, cos, centroids, counts, n_iter,
    converged, cohesion, trail): trail = per iteration (assign, cos, margin, cohesion)."""
    T = np.asarray(T, dtype=np.float64)
    init = np.asarray(init, dtype=np.int64)
    C = init.size
    cen = T[init].copy()
    prev, trail, converged, counts = None, [], False, np.zeros(C, dtype=np.int64)
    for it in range(iters):
        assign, cos, margin = assign64(T, cen)
        listed = assign >= 0
        trail.append((assign, cos, margin, float(cos[listed].mean()) if listed.any() else float("nan")))
        if it and np.array_equal(assign, prev):
            converged = True
            break
        _, counts, cen = update64(T, assign, cen, C)
        prev = assign
    assign, cos, _, cohesion = trail[-1]
    return dict(assign=assign, cos=cos, centroids=cen, counts=counts, n_iter=len(trail), converged=converged, cohesion=cohesion,
                trail=trail)


# ---- the cluster report's rows (reports.cluster_rows / cluster_user_rows restated with loops)
def cluster_rows_loops(assign, cos, item_counts, test_counts, exposure, C):
    """Per cluster: size, pop, cohesion, train_share, test_share, slot_share."""
    out = np.zeros((C, 6))
    tot_train, tot_test, tot_slots = float(np.sum(item_counts)), float(np.sum(test_counts)), float(np.sum(exposure))
    for c in range(C):
        members = [i for i in range(len(assign)) if assign[i] == c]
        out[c, 0] = len(members)
        out[c, 1] = np.mean([float(item_counts[i]) for i in members]) if members else np.nan
        out[c, 2] = np.mean([float(cos[i]) for i in members]) if members else np.nan
        out[c, 3] = sum(float(item_counts[i]) for i in members) / tot_train if tot_train else 0.0
        out[c, 4] = sum(float(test_counts[i]) for i in members) / tot_test if tot_test else 0.0
        out[c, 5] = sum(float(exposure[i]) for i in members) / tot_slots if tot_slots else 0.0
    return out
