"""The inputs of the calibrated re-ranking tests, shared by the host test (which checks that the float64 model's steps are clear on
them) and the device test (which runs the kernel on them): per shape (N, K, C) 200 pools of distinct random ids over a 2000-item
catalogue with descending uniform fp32 scores, a random class per item and Dirichlet-like targets with some exact zeros."""
import functools

import numpy as np

import calibrate_model as cm

SHAPES = ((1, 1, 1), (17, 5, 3), (37, 37, 2), (64, 10, 4), (65, 10, 4), (100, 10, 5), (256, 50, 16), (256, 256, 16))   # N, K, C
LAMBDAS = (0.0, 0.3, 0.7, 1.0)
ITEMS, LISTS, SEED = 2000, 200, 11
SMOOTH = 0.01
# A bound, not a measurement: an objective is lam * rel - (1 - lam) * KL with KL a sum of at most C = 16 terms p log(p / q~); each
# term takes a division, a log (within an ulp in either library) and a product, the objective C + 3 further float64 operations, all
# on values of magnitude below 8 (KL <= log(1 / smooth) = log 100 < 8): an error of order 16 * 8 * 2^-52 ~ 3e-14 on either side.
TOL = 1e-12


@functools.lru_cache(maxsize=None)
def case(N, K, C):
    """-> (ids int32 [B x N], vals float32 [B x N], class_of int32 [ITEMS], targets float32 [B x C])."""
    rng = np.random.default_rng(SEED + 1000 * N + 10 * K + C)
    ids = np.stack([rng.permutation(ITEMS)[:N] for _ in range(LISTS)]).astype(np.int32)
    vals = -np.sort(-rng.uniform(size=(LISTS, N)).astype(np.float32), axis=1)
    class_of = rng.integers(0, C, ITEMS).astype(np.int32)
    g = rng.gamma(0.7, size=(LISTS, C))
    if C > 1:
        g[rng.uniform(size=(LISTS, C)) < 0.25] = 0.0                            # exact zeros: classes the user never touched
    g[g.sum(1) == 0, 0] = 1.0
    targets = (g / g.sum(1, keepdims=True)).astype(np.float32)
    for a in (ids, vals, class_of, targets):
        a.setflags(write=False)
    return ids, vals, class_of, targets


@functools.lru_cache(maxsize=None)
def pools(N, K, C):
    ids, vals, class_of, targets = case(N, K, C)
    return cm.Pools64(ids, vals, class_of, targets, SMOOTH)


@functools.lru_cache(maxsize=None)
def greedy(N, K, C, lam):
    """The float64 greedy lists of one shape at one lambda: (picks, objs, margins), computed once and shared."""
    out = pools(N, K, C).greedy(K, lam)
    for a in out:
        a.setflags(write=False)
    return out
