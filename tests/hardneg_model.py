"""Float64 model of the hard-negative pick (csrc/hardneg.hip), pure numpy.

score(u, i) = sum over the blocks b with w_b != 0 of w_b * cos_b(u, i), cos_b = (U_b[u] . T_b[i]) / (max(|U_b[u]|, 1e-12) *
max(|T_b[i]|, 1e-12)) -- a zero row gives 0. A candidate is listed when its id lies in [0, item rows); the listed candidate with
the largest score wins, the lowest column among equal scores; a row with no listed candidate, or a user outside [0, user rows),
has no pick (-1)."""
import numpy as np


def block_cosines(U, T, blocks):
    """Unit rows per block: ([rows x blocks x d] for the users, the same for the items), float64; a zero row stays zero."""
    out = []
    for X in (U, T):
        X = np.asarray(X, dtype=np.float64)
        X = X.reshape(X.shape[0], blocks, -1)
        out.append(X / np.maximum(np.sqrt((X * X).sum(2, keepdims=True)), 1e-12))
    return out


def scores(U, T, weights, users, cands):
    """[n x M] float64 scores, -inf where the entry is not listed (or the row's user is outside the table)."""
    w = np.asarray(weights, dtype=np.float64)
    users, cands = np.asarray(users, dtype=np.int64), np.asarray(cands, dtype=np.int64)
    Un, Tn = block_cosines(U, T, w.size)
    n, M = cands.shape
    listed = (cands >= 0) & (cands < Tn.shape[0]) & ((users >= 0) & (users < Un.shape[0]))[:, None]
    out = np.full((n, M), -np.inf)
    if not listed.any():
        return out
    r, c = np.nonzero(listed)
    cos = np.einsum("pbd,pbd->pb", Un[users[r]], Tn[cands[r, c]])
    out[r, c] = (cos * w[None, :])[:, w != 0].sum(1)
    return out


def pick(score, cands):
    """(column int64 [n] -- the lowest column with the row's largest score, -1 where nothing is listed --, id int64 [n], the
    picked score [n] (-inf without a pick), margin [n]: the best score minus the best score among the listed candidates with
    ANOTHER id (+inf where there is none: the pick's id cannot be wrong))."""
    cands = np.asarray(cands, dtype=np.int64)
    n = score.shape[0]
    col = score.argmax(1)                                                   # numpy's argmax: the first of equal maxima
    best = score[np.arange(n), col]
    none = np.isneginf(best)
    ids = np.where(none, -1, cands[np.arange(n), col])
    other = np.where(cands == ids[:, None], -np.inf, score).max(1)
    margin = np.where(none, np.inf, np.where(none, 0.0, best) - other)
    return np.where(none, -1, col), ids, best, margin
