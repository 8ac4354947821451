"""Float64 numpy model of the greedy maximal-marginal-relevance re-ranking (csrc/rerank.hip).

A pool is N (id, score) positions over a table T [n x d] with squared norms sq [n]. A position is listed when its id lies in
[0, n) and its score is finite. Over the listed positions rel_i = (s_i - s_min) / (s_max - s_min) (0 when s_max == s_min) and
step t picks, among the listed positions not picked yet, the largest
    obj_t(i) = lam * rel_i - (1 - lam) * pen_t(i),  pen_0 = 0,  pen_t(i) = max over the picks j so far of cos(i, j),
    cos(i, j) = dot(T[i], T[j]) inv(sq_i) inv(sq_j),  inv(x) = 1 / max(sqrt(x), 1e-12)
the lowest position among equal objectives, until K picks are made or no listed position is left."""
import numpy as np


def listed(ids, vals, n):
    ids, vals = np.asarray(ids, dtype=np.int64), np.asarray(vals, dtype=np.float64)
    return (ids >= 0) & (ids < n) & np.isfinite(vals)


def relevance(vals, mask):
    """rel [N] float64 (0 at unlisted positions)."""
    vals = np.asarray(vals, dtype=np.float64)
    rel = np.zeros(vals.shape[0])
    if mask.any():
        lo, hi = vals[mask].min(), vals[mask].max()
        if hi > lo:
            rel[mask] = (vals[mask] - lo) / (hi - lo)
    return rel


class Pools64(object):
    """B pools at once: ids / vals [B x N] over T [n x d], sq [n] (the squared norms the kernel is given). The listed mask, the
    relevance and the [B x N x N] cosines are formed once and shared by greedy() and replay() at any lambda."""

    def __init__(self, T, sq, ids, vals):
        ids = np.atleast_2d(np.asarray(ids, dtype=np.int64))
        vals = np.atleast_2d(np.asarray(vals, dtype=np.float64))
        n = np.asarray(T).shape[0]
        self.B, self.N = ids.shape
        self.mask = np.stack([listed(i, v, n) for i, v in zip(ids, vals)])
        self.rel = np.stack([relevance(v, m) for v, m in zip(vals, self.mask)])
        safe = np.where(self.mask, ids, 0)
        R = np.asarray(T, dtype=np.float64)[safe]                                   # [B x N x d]
        inv = np.where(self.mask, 1.0 / np.maximum(np.sqrt(np.asarray(sq, dtype=np.float64)[safe]), 1e-12), 0.0)
        R = R * self.mask[:, :, None]
        self.G = np.matmul(R, R.transpose(0, 2, 1)) * inv[:, :, None] * inv[:, None, :]
        self._ar = np.arange(self.B)

    def _obj(self, alive, pen, lam):
        return np.where(alive, lam * self.rel - (1.0 - lam) * pen, -np.inf)

    def greedy(self, K, lam):
        """-> (picks int64 [B x K], objs, margins float64 [B x K]): the picked positions in order (-1 once no listed position is
        left), each pick's objective (-inf at fillers) and its margin to the step's runner-up (inf when it was the only candidate,
        and at fillers)."""
        ar = self._ar
        alive, pen = self.mask.copy(), np.zeros((self.B, self.N))
        picks = np.full((self.B, K), -1, dtype=np.int64)
        objs, margins = np.full((self.B, K), -np.inf), np.full((self.B, K), np.inf)
        for t in range(K):
            obj = self._obj(alive, pen, lam)
            p = obj.argmax(axis=1)                                   # (the first of equal maxima: the lowest position)
            has = alive.any(axis=1)
            top = obj[ar, p]
            obj[ar, p] = -np.inf
            picks[has, t], objs[has, t] = p[has], top[has]
            margins[has, t] = top[has] - obj[has].max(axis=1)
            alive[ar[has], p[has]] = False
            col = self.G[ar, :, p]
            pen = col if t == 0 else np.maximum(pen, col)
        return picks, objs, margins

    def replay(self, picks, lam):
        """The objectives along given pick sequences [B x K] (a row ends at its first position < 0) -> (objs, bests float64
        [B x K], ok bool [B x K]): per step the objective of the given pick and the step's maximum (NaN behind a row's end), and
        whether the pick was listed and not picked before (True behind a row's end). A row's replay ends at its first bad pick."""
        picks = np.asarray(picks, dtype=np.int64)
        ar, K = self._ar, picks.shape[1]
        alive, pen = self.mask.copy(), np.zeros((self.B, self.N))
        objs, bests = np.full((self.B, K), np.nan), np.full((self.B, K), np.nan)
        ok = np.ones((self.B, K), dtype=bool)
        active = np.ones(self.B, dtype=bool)
        for t in range(K):
            p = picks[:, t]
            active = active & (p >= 0)
            pc = np.clip(p, 0, self.N - 1)
            good = active & (p < self.N) & alive[ar, pc]
            ok[:, t] = good | ~active
            obj = self._obj(alive, pen, lam)
            objs[good, t] = obj[ar, pc][good]
            bests[active, t] = obj.max(axis=1)[active]
            active = good
            alive[ar[good], pc[good]] = False
            col = self.G[ar, :, pc]
            pen = col if t == 0 else np.maximum(pen, col)
        return objs, bests, ok


def greedy(T, sq, ids, vals, K, lam):
    """One pool -> (picks, objs, margins) as lists, cut at the pool's last pick."""
    picks, objs, margins = Pools64(T, sq, ids, vals).greedy(K, lam)
    m = int((picks[0] >= 0).sum())
    return picks[0, :m].tolist(), objs[0, :m].tolist(), margins[0, :m].tolist()


def greedy_loops(T, sq, ids, vals, K, lam):
    """greedy()'s picks as plain loops."""
    n = len(T)
    N = len(ids)
    ok = [0 <= int(ids[i]) < n and np.isfinite(float(vals[i])) for i in range(N)]
    lst = [float(vals[i]) for i in range(N) if ok[i]]
    lo, hi = (min(lst), max(lst)) if lst else (0.0, 0.0)
    rel = [(float(vals[i]) - lo) / (hi - lo) if ok[i] and hi > lo else 0.0 for i in range(N)]

    def cos(i, j):
        a, b = int(ids[i]), int(ids[j])
        dot = 0.0
        for k in range(len(T[a])):
            dot += float(T[a][k]) * float(T[b][k])
        return dot / (max(np.sqrt(float(sq[a])), 1e-12) * max(np.sqrt(float(sq[b])), 1e-12))

    picks = []
    for _ in range(K):
        best, bo = -1, -np.inf
        for i in range(N):
            if not ok[i] or i in picks:
                continue
            pen = max(cos(i, j) for j in picks) if picks else 0.0
            o = lam * rel[i] - (1.0 - lam) * pen
            if best < 0 or o > bo:
                best, bo = i, o
        if best < 0:
            break
        picks.append(best)
    return picks
