"""Float64 numpy model of the greedy calibrated re-ranking and of the class shares (csrc/calibrate.hip).

A pool is N (id, score) positions over a catalogue with a class per item, class_of [n], and a target p [C] (an entry that is
negative or not finite counts as 0). A position is listed when its id lies in [0, n), its score is finite and its class lies in
[0, C). Over the listed positions rel_i = (s_i - s_min) / (s_max - s_min) (0 when s_max == s_min) and step t picks, among the
listed positions not picked yet, the largest
    obj_t(i) = lam * rel_i - (1 - lam) * KL_t(class_i),
    KL_t(c') = sum over c ascending with p_c > 0 of p_c * log(p_c / q~_c),  q~_c = (1 - smooth) q_c + smooth p_c,
    q_c = (n_c(t) + [c == c']) / (t + 1),   n_c(t) = the picks so far in class c,
the lowest position among equal objectives, until K picks are made or no listed position is left.

Margins. Two candidates with the same lam * rel_i whose classes are the same -- or both have no target share, so that neither
enters any q~_c that is summed -- have the same objective in ANY arithmetic that forms KL_t once per class: such a tie is settled
by the position rule, exactly, and is no unclear step. A pick's margin is therefore taken to the best candidate that is not tied
to it in this way."""
import numpy as np


def targets(p):
    """p as the kernel reads it: float64, 0 where negative or not finite."""
    p = np.asarray(p, dtype=np.float64)
    return np.where(np.isfinite(p) & (p > 0), p, 0.0)


def listed(ids, vals, class_of, C):
    ids, vals = np.asarray(ids, dtype=np.int64), np.asarray(vals, dtype=np.float64)
    class_of = np.asarray(class_of, dtype=np.int64)
    ok = (ids >= 0) & (ids < class_of.shape[0]) & np.isfinite(vals)
    cls = np.where(ok, class_of[np.where(ok, ids, 0)], -1) if class_of.shape[0] else np.full(ids.shape, -1, dtype=np.int64)
    return ok & (cls >= 0) & (cls < C)


def relevance(vals, mask):
    """rel [N] float64 (0 at unlisted positions)."""
    vals = np.asarray(vals, dtype=np.float64)
    rel = np.zeros(vals.shape[0])
    if mask.any():
        lo, hi = vals[mask].min(), vals[mask].max()
        if hi > lo:
            rel[mask] = (vals[mask] - lo) / (hi - lo)
    return rel


def c_kl(p, q, smooth=0.01):
    """C_KL(p, q~) = sum over c ascending with p_c > 0 of p_c log(p_c / ((1 - smooth) q_c + smooth p_c)); p [.. x C] as targets()
    returns it, q [.. x C] float64 -> [..] float64. The terms are added one class at a time, in ascending order."""
    p, q = np.broadcast_arrays(np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64))
    out = np.zeros(p.shape[:-1])
    for c in range(p.shape[-1]):
        pc, on = p[..., c], p[..., c] > 0
        safe = np.where(on, pc, 1.0)
        term = safe * np.log(safe / ((1.0 - smooth) * q[..., c] + smooth * safe))
        out = np.where(on, out + term, out)
    return out


def class_counts(lists, class_of, C):
    """int64 [B x C]: per row of lists (rows of ids, any fillers) the entries of every class; an id outside the catalogue or with
    a class outside [0, C) is skipped, a repeated id counts each time."""
    class_of = np.asarray(class_of, dtype=np.int64)
    out = np.zeros((len(lists), C), dtype=np.int64)
    for b, row in enumerate(lists):
        for i in np.asarray(row, dtype=np.int64).reshape(-1):
            if 0 <= i < class_of.shape[0] and 0 <= class_of[i] < C:
                out[b, class_of[i]] += 1
    return out


def class_shares(lists, class_of, C):
    """float32 [B x C]: float32(count) / float32(listed), one fp32 division; zeros for a row without a listed entry."""
    cnt = class_counts(lists, class_of, C)
    tot = cnt.sum(1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = cnt.astype(np.float32) / tot.astype(np.float32)
    return np.where(tot > 0, out, np.float32(0)).astype(np.float32)


def list_kl(lists, class_of, C, p, smooth=0.01):
    """float64 [B]: C_KL of every row's class shares (float64 count / listed; 0 when nothing is listed) against its target row."""
    cnt = class_counts(lists, class_of, C)
    tot = cnt.sum(1, keepdims=True)
    q = np.where(tot > 0, cnt / np.maximum(tot, 1).astype(np.float64), 0.0)
    return c_kl(targets(p), q, smooth)


class Pools64(object):
    """B pools at once: ids / vals [B x N], class_of [n], targets p [B x C]. The listed mask, the relevance and the classes are
    formed once and shared by greedy() and replay() at any lambda."""

    def __init__(self, ids, vals, class_of, p, smooth=0.01):
        ids = np.atleast_2d(np.asarray(ids, dtype=np.int64))
        vals = np.atleast_2d(np.asarray(vals, dtype=np.float64))
        self.p = targets(np.atleast_2d(p))
        self.B, self.N = ids.shape
        self.C = self.p.shape[1]
        self.smooth = float(smooth)
        class_of = np.asarray(class_of, dtype=np.int64)
        self.mask = np.stack([listed(i, v, class_of, self.C) for i, v in zip(ids, vals)])
        self.rel = np.stack([relevance(v, m) for v, m in zip(vals, self.mask)])
        self.cls = np.where(self.mask, class_of[np.where(self.mask, ids, 0)], 0) if class_of.shape[0] else np.zeros_like(ids)
        # classes without a target share are one class as far as the objective goes (see the module's note on margins)
        self.key = np.where(np.take_along_axis(self.p, self.cls, 1) > 0, self.cls, -1)
        self._ar = np.arange(self.B)

    def _kl(self, counts, t):
        """[B x C]: KL_t(c') for every class c' a candidate may have."""
        out = np.empty((self.B, self.C))
        for c in range(self.C):
            add = np.zeros(self.C)
            add[c] = 1.0
            out[:, c] = c_kl(self.p, (counts + add) / float(t + 1), self.smooth)
        return out

    def _obj(self, alive, counts, t, lam):
        kl = np.take_along_axis(self._kl(counts, t), self.cls, 1)
        return np.where(alive, lam * self.rel - (1.0 - lam) * kl, -np.inf)

    def greedy(self, K, lam):
        """-> (picks int64 [B x K], objs, margins float64 [B x K]): the picked positions in order (-1 once no listed position is
        left), each pick's objective (-inf at fillers) and its margin to the best candidate not tied to it by construction (inf
        when there is none, and at fillers)."""
        ar = self._ar
        alive, counts = self.mask.copy(), np.zeros((self.B, self.C))
        picks = np.full((self.B, K), -1, dtype=np.int64)
        objs, margins = np.full((self.B, K), -np.inf), np.full((self.B, K), np.inf)
        lrel = lam * self.rel
        for t in range(K):
            obj = self._obj(alive, counts, t, lam)
            p = obj.argmax(axis=1)                                   # (the first of equal maxima: the lowest position)
            has = alive.any(axis=1)
            top = obj[ar, p]
            tied = (self.key == self.key[ar, p][:, None]) & (lrel == lrel[ar, p][:, None])
            rest = np.where(tied, -np.inf, obj).max(axis=1)
            picks[has, t], objs[has, t] = p[has], top[has]
            margins[has, t] = top[has] - rest[has]
            alive[ar[has], p[has]] = False
            counts[ar[has], self.cls[ar, p][has]] += 1.0
        return picks, objs, margins

    def replay(self, picks, lam):
        """The objectives along given pick sequences [B x K] (a row ends at its first position < 0) -> (objs, bests float64
        [B x K], ok bool [B x K]): per step the objective of the given pick and the step's maximum (NaN behind a row's end), and
        whether the pick was listed and not picked before (True behind a row's end). A row's replay ends at its first bad pick."""
        picks = np.asarray(picks, dtype=np.int64)
        ar, K = self._ar, picks.shape[1]
        alive, counts = self.mask.copy(), np.zeros((self.B, self.C))
        objs, bests = np.full((self.B, K), np.nan), np.full((self.B, K), np.nan)
        ok = np.ones((self.B, K), dtype=bool)
        active = np.ones(self.B, dtype=bool)
        for t in range(K):
            p = picks[:, t]
            active = active & (p >= 0)
            pc = np.clip(p, 0, self.N - 1)
            good = active & (p < self.N) & alive[ar, pc]
            ok[:, t] = good | ~active
            obj = self._obj(alive, counts, t, lam)
            objs[good, t] = obj[ar, pc][good]
            bests[active, t] = obj.max(axis=1)[active]
            active = good
            alive[ar[good], pc[good]] = False
            counts[ar[good], self.cls[ar, pc][good]] += 1.0
        return objs, bests, ok


def greedy(ids, vals, class_of, p, K, lam, smooth=0.01):
    """One pool -> (picks, objs, margins) as lists, cut at the pool's last pick."""
    picks, objs, margins = Pools64(ids, vals, class_of, p, smooth).greedy(K, lam)
    m = int((picks[0] >= 0).sum())
    return picks[0, :m].tolist(), objs[0, :m].tolist(), margins[0, :m].tolist()


def greedy_loops(ids, vals, class_of, p, K, lam, smooth=0.01):
    """greedy()'s picks as plain loops."""
    n, N, C = len(class_of), len(ids), len(p)
    p = [float(x) if np.isfinite(float(x)) and float(x) > 0 else 0.0 for x in p]
    ok = [0 <= int(ids[i]) < n and bool(np.isfinite(float(vals[i]))) and 0 <= int(class_of[int(ids[i])]) < C for i in range(N)]
    lst = [float(vals[i]) for i in range(N) if ok[i]]
    lo, hi = (min(lst), max(lst)) if lst else (0.0, 0.0)
    rel = [(float(vals[i]) - lo) / (hi - lo) if ok[i] and hi > lo else 0.0 for i in range(N)]
    counts, picks = [0] * C, []
    for t in range(K):
        best, bo = -1, -np.inf
        for i in range(N):
            if not ok[i] or i in picks:
                continue
            ci, kl = int(class_of[int(ids[i])]), 0.0
            for c in range(C):
                if p[c] > 0:
                    q = (counts[c] + (1 if c == ci else 0)) / float(t + 1)
                    kl += p[c] * np.log(p[c] / ((1.0 - smooth) * q + smooth * p[c]))
            o = lam * rel[i] - (1.0 - lam) * kl
            if best < 0 or o > bo:
                best, bo = i, o
        if best < 0:
            break
        picks.append(best)
        counts[int(class_of[int(ids[best])])] += 1
    return picks
