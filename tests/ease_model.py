"""Host models of csrc/ease.hip for the EASE tests: the block sweep in numpy float64, the dense EASE definition through
np.linalg.inv, the score and ranking rule of ease_topk, and a comparer of rankings up to a score tolerance."""
import numpy as np


def sweep_inverse(G, nb=64):
    """The symmetric block sweep of spd_inverse in float64: pad to a multiple of nb with an identity block; per pivot block k,
    D = A_kk, R = A_k,:, W = D^-1 R: A <- A - R^T W, A_k,: <- W, A_:,k <- W^T, A_kk <- -D^-1; after the last block A = -G^-1."""
    G = np.asarray(G, dtype=np.float64)
    n = G.shape[0]
    npad = -(-n // nb) * nb
    A = np.eye(npad)
    A[:n, :n] = G
    for k0 in range(0, npad, nb):
        k = slice(k0, k0 + nb)
        Dinv = np.linalg.inv(A[k, k])
        R = A[k, :].copy()
        W = Dinv @ R
        A -= R.T @ W
        A[k, :] = W
        A[:, k] = W.T
        A[k, k] = -Dinv
    return -A[:n, :n]


def inverse_bound(n, kappa):
    """The bound of the inverse tests, the form and constant of als_model.solve_bound: 64 n kappa 2^-53."""
    return 64.0 * n * kappa * 2.0 ** -53


def kappa(G):
    w = np.linalg.eigvalsh(np.asarray(G, dtype=np.float64))
    return float(w[-1] / w[0])


def gram(X, l2):
    X = np.asarray(X, dtype=np.float64)
    return X.T @ X + l2 * np.eye(X.shape[1])


def ease_P(X, l2):
    """P = (X^T X + l2 I)^-1 of the binary user x item matrix X."""
    return np.linalg.inv(gram(X, l2))


def scores(P, hist):
    """float32 [I]: s_j = -(sum_{i in hist, i != j} P[i, j]) / P[j, j], the sum in float64 in the list's order, one division,
    one rounding."""
    P = np.asarray(P, dtype=np.float64)
    I = P.shape[0]
    acc = np.zeros(I, dtype=np.float64)
    cols = np.arange(I)
    for i in hist:
        acc = acc + np.where(cols == i, 0.0, P[int(i), :])
    with np.errstate(all="ignore"):
        return (-acc / np.diagonal(P)).astype(np.float32)


def topk(P, hist, excl, K):
    """(ids int32 [K], vals float32 [K], all scores): the K best by (score descending, id ascending) among the items not in
    excl, fillers -1 / -inf behind them."""
    s = scores(P, hist)
    keep = np.ones(s.size, dtype=bool)
    keep[np.asarray(list(excl), dtype=np.int64)] = False
    cand = np.flatnonzero(keep & ~np.isnan(s))
    order = cand[np.lexsort((cand, -s[cand].astype(np.float64)))][:K]
    ids = np.full(K, -1, dtype=np.int32)
    vals = np.full(K, -np.inf, dtype=np.float32)
    ids[:order.size] = order
    vals[:order.size] = s[order]
    return ids, vals, s


def full_order(s, excl):
    """Every item not in excl and with a score, by (score descending, id ascending)."""
    keep = np.ones(s.size, dtype=bool)
    keep[np.asarray(list(excl), dtype=np.int64)] = False
    cand = np.flatnonzero(keep & ~np.isnan(s))
    return cand[np.lexsort((cand, -s[cand].astype(np.float64)))]


def rank_equal_up_to(got, order, ref_scores, tol):
    """Compare one list `got` [K] with the reference ranking `order` (full_order: all candidates) position by position; positions
    whose reference score lies within tol of a neighbour's in the reference ranking form runs that are compared as sets (a run
    that crosses position K: the list's part of it must come from the run, without repeats). -> (equal, positions of the list
    excused that way). Behind the candidates the list must hold -1."""
    got, order = np.asarray(got), np.asarray(order)
    K = got.size
    n = min(K, order.size)
    if not (got[n:] == -1).all():
        return False, 0
    s = np.asarray(ref_scores, dtype=np.float64)[order]
    excused, a = 0, 0
    while a < n:
        b = a + 1
        while b < order.size and abs(s[b] - s[b - 1]) <= tol:
            b += 1
        if b - a == 1:
            if got[a] != order[a]:
                return False, excused
        else:
            part = got[a:min(b, n)].tolist()
            excused += len(part)
            if len(set(part)) != len(part) or not set(part) <= set(order[a:b].tolist()) or (b <= n and set(part) != set(order[a:b].tolist())):
                return False, excused
        a = b
    return True, excused


# ---- the generated split of the end-to-end tests (test_ease_gpu; its seed is checked in test_ease_cpu)
E2E_U, E2E_I, E2E_L2, E2E_SEED, E2E_K = 150, 130, 5.0, 7, 20


def generated_split(U=E2E_U, I=E2E_I, seed=E2E_SEED):
    """The ml3 fixture's settings over a generated split: popularity-skewed interactions, 2 test items per user with >= 4 and a
    validation item per user with >= 8, one cold item (I // 3), a user without training items (user 0) and repeated (user, item) pairs in the training list."""
    from helpers import load_golden
    g = {k: v for k, v in load_golden("ml3").items() if "/" not in k}
    rng = np.random.default_rng(seed)
    pop = 1.0 / np.arange(1, I + 1) ** 0.7
    pop[I // 3] = 0.0
    pop /= pop.sum()
    split = {"train": {}, "valid": {}, "test": {}}
    for u in range(1, U):
        items = rng.choice(I, size=int(rng.integers(2, 25)), replace=False, p=pop)
        if items.size >= 4:
            split["test"][u], items = items[:2].tolist(), items[2:]
        if items.size >= 6:
            split["valid"][u], items = items[:1].tolist(), items[1:]
        split["train"][u] = items.tolist() + items[:1].tolist() * (u % 3 == 0)      # a repeated pair
    for name, d in split.items():
        users = np.asarray(sorted(d), dtype=np.int64)
        g["%s_dict_users" % name] = users
        g["%s_dict_ptr" % name] = np.concatenate([[0], np.cumsum([len(d[u]) for u in users])]).astype(np.int64)
        g["%s_dict_items" % name] = np.asarray([i for u in users for i in d[u]], dtype=np.int64)
    pairs = sorted({(u, i) for u, v in split["train"].items() for i in v})
    g["train_u"], g["train_i"] = (np.asarray(x, dtype=np.int64) for x in zip(*pairs))
    g["num_users"], g["num_items"] = np.int64(U), np.int64(I)
    for m in ("v", "a", "t"):
        g[m + "_feat"] = rng.standard_normal((I, g[m + "_feat"].shape[1])).astype(np.float32)
    return g, split


def reference(split, U=E2E_U, I=E2E_I, l2=E2E_L2):
    """The dense numpy EASE of the split: (P, kappa of G, per-user histories in the train dict's order)."""
    X = np.zeros((U, I))
    for u, v in split["train"].items():
        X[u, v] = 1.0
    return ease_P(X, l2), kappa(gram(X, l2))


def compare(lists, users, split, P, kap, K=E2E_K, I=E2E_I):
    """Position by position up to tol = 64 I kappa 2^-53 max|s| -> the share of list slots excused."""
    excused = 0
    for b, u in enumerate(users):
        h = split["train"].get(int(u), [])
        s = scores(P, h)
        tol = 64.0 * I * kap * 2.0 ** -53 * float(np.abs(s).max())
        ok, n = rank_equal_up_to(lists[b], full_order(s, h), s, tol)
        assert ok, (u, lists[b], full_order(s, h)[:K])
        excused += n
    return excused / float(len(users) * K)
