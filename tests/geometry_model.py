"""A numpy model of csrc/geometry.hip and of the alignment: the unit rows are formed in float32 exactly as cosine.h's inv_norm does
(x * (1 / max(sqrt(sq), 1e-12)), every step rounded to float32), everything after them is float64."""
import numpy as np


def sqnorms(T):
    """Squared norms rounded once to fp32."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(T, dtype=np.float64) ** 2).sum(1).astype(np.float32)


def valid_entries(rows, sq, n_rows):
    """The list's valid entries in list order: an id in [0, n_rows) whose row's squared norm is > 0 and finite."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    sq = np.asarray(sq, dtype=np.float32).reshape(-1)
    inside = (rows >= 0) & (rows < n_rows)
    ok = np.zeros(rows.size, dtype=bool)
    with np.errstate(invalid="ignore"):
        ok[inside] = (sq[rows[inside]] > 0) & np.isfinite(sq[rows[inside]])
    return rows[ok]


def inv_norm(sq):
    """1 / max(sqrt(sq), 1e-12) in float32, step by step."""
    sq = np.asarray(sq, dtype=np.float32)
    return (np.float32(1) / np.maximum(np.sqrt(sq), np.float32(1e-12))).astype(np.float32)


def unit_rows(T, sq, ids):
    """float32 unit rows of the entries `ids`, as the kernels form them."""
    T = np.asarray(T, dtype=np.float32)
    return (T[ids] * inv_norm(np.asarray(sq, dtype=np.float32)[ids])[:, None]).astype(np.float32)


def live_cells(n, tile, chunk):
    """The (tile, chunk) cells uniformity_sum launches for a list of n positions, in launch order. By the definition, not by the
    kernel's closed form: the positions are cut into tiles of `tile` and chunks of `chunk`, the cells run tile-major, and tile i
    meets the chunks c >= i * tile // chunk -- its own chunk and every later one."""
    n_chunks = (n + chunk - 1) // chunk
    return [(i, c) for i in range((n + tile - 1) // tile) for c in range(i * tile // chunk, n_chunks)]


def cells_with_a_pair(n, tile, chunk):
    """The set of (tile of p, chunk of q) over all positions p < q < n, by brute force over the positions."""
    found = set()
    for p in range(n - 1):
        found.update((p // tile, int(c)) for c in np.unique(np.arange(p + 1, n) // chunk))
    return found


def uniformity_model(T, sq, rows, t, cells=None):
    """(S, pairs, n_valid, uniformity) in float64 over the valid entries of `rows`. With cells = (tile, chunk) and a list whose
    entries are all valid (position = rank among the valid ones), a fifth value: the float64 sum of every cell of
    live_cells(n, tile, chunk), in that order; a pair outside those cells is an error."""
    ids = valid_entries(rows, sq, np.asarray(T).shape[0])
    n = int(ids.size)
    pairs = n * (n - 1) // 2
    if cells is not None:
        tile, chunk = cells
        assert n == np.asarray(rows).size and 1024 % tile == 0
        per_cell = np.zeros(((n + tile - 1) // tile, (n + chunk - 1) // chunk))
    if n < 2:
        return (0.0, pairs, n, float("nan")) + (() if cells is None else ([0.0] * len(live_cells(n, tile, chunk)),))
    X = unit_rows(T, sq, ids).astype(np.float64)
    S = 0.0
    for a in range(0, n, 1024):                                      # row blocks: the strict upper triangle
        cos = X[a:a + 1024] @ X.T
        e = np.exp(2.0 * float(t) * (cos - 1.0))
        p = np.arange(a, min(a + 1024, n))[:, None]
        e = np.where(p < np.arange(n)[None, :], e, 0.0)
        S += float(e.sum())
        if cells is not None:
            by_chunk = np.add.reduceat(e, np.arange(0, n, chunk), axis=1)
            for i in range(a // tile, (min(a + 1024, n) + tile - 1) // tile):
                per_cell[i] = by_chunk[i * tile - a:(i + 1) * tile - a].sum(0)
    if cells is None:
        return S, pairs, n, float(np.log(S / pairs))
    live = live_cells(n, tile, chunk)
    mask = np.zeros(per_cell.shape, dtype=bool)
    mask[tuple(np.asarray(live).T)] = True
    assert not per_cell[~mask].any()
    return S, pairs, n, float(np.log(S / pairs)), [float(per_cell[i, c]) for i, c in live]


def gram_model(T, sq, rows):
    """(G [d x d], m [d], n_valid, A [d x d] = sum |x^_a x^_b|, a [d] = sum |x^_a|) in float64."""
    T = np.asarray(T)
    ids = valid_entries(rows, sq, T.shape[0])
    X = unit_rows(T, sq, ids).astype(np.float64)
    return X.T @ X, X.sum(0), int(ids.size), np.abs(X).T @ np.abs(X), np.abs(X).sum(0)


def alignment_model(TU, squ, TI, sqi, users, items):
    """2 - 2 cos of every pair in float64; a row without a norm gives cosine 0."""
    users, items = np.asarray(users, dtype=np.int64), np.asarray(items, dtype=np.int64)
    xu = np.asarray(TU, dtype=np.float64)[users] * inv_norm(np.asarray(squ, dtype=np.float32)[users]).astype(np.float64)[:, None]
    xi = np.asarray(TI, dtype=np.float64)[items] * inv_norm(np.asarray(sqi, dtype=np.float32)[items]).astype(np.float64)[:, None]
    return 2.0 - 2.0 * (xu * xi).sum(1)


def geometry_row_model(T, sq, rows, t):
    """(n, uniformity, erank, top1, rank99, centre) of a list of rows, the spectrum by its definition."""
    _, _, n, uni = uniformity_model(T, sq, rows, t)
    G, m, n_g, _, _ = gram_model(T, sq, rows)
    assert n_g == n
    nan = float("nan")
    if n < 1:
        return np.asarray([0.0, nan, nan, nan, nan, nan])
    mu = m / n
    centre = float(np.linalg.norm(mu))
    if n < 2:
        return np.asarray([float(n), uni, nan, nan, nan, centre])
    lam = np.clip(np.linalg.eigvalsh(G / n - np.outer(mu, mu)), 0.0, None)[::-1]
    lam[lam <= lam.size * np.finfo(np.float64).eps] = 0.0
    if lam.sum() <= 0:
        return np.asarray([float(n), uni, nan, nan, nan, centre])
    p = lam / lam.sum()
    nz = p[p > 0]
    rank99 = 1 + int(np.argmax(np.cumsum(p) >= 0.99 - 1e-12))
    return np.asarray([float(n), uni, float(np.exp(-(nz * np.log(nz)).sum())), float(p[0]), float(rank99), centre])
