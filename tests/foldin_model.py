"""Host models of the new-user fold-in (float64 numpy).

segment_row_sum: the definition of ops.segment_row_sum (csrc/foldin.hip) and the error bound float64 accumulation with one rounding
gives it. weights: the off-diagonal adjacency values for the five adjacency types, written from create_adj_mat's definitions, not
from reports.fold_in_weights. fold_in_rows: EliMRec.fold_in_users restated in float64 -- weights, sum, id term, user fusion Linear
and heads -- with the magnitudes the projections' bound needs. user_rows / table: the report's pure functions."""
import numpy as np


def csr(lists, dtype=np.int64):
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=ptr[1:])
    flat = np.concatenate([np.asarray(x, dtype=dtype) for x in lists]) if ptr[-1] else np.zeros(0, dtype=dtype)
    return ptr, flat.astype(dtype)


def segment_row_sum(table, ptr, rows, weights, row_offset=0):
    """(want, bound, magnitude), float64 [Q x C] each: out[q] = sum_j w_j table[row_offset + rows_j] in float64 and the bound
    |got - want| <= 2^-23 |want| + n 2^-50 sum_j |w_j x_j| of a float64 accumulation in any order followed by one rounding; magnitude = sum_j |w_j x_j|."""
    t = np.asarray(table, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    Q = len(ptr) - 1
    want = np.zeros((Q, t.shape[1]))
    mag = np.zeros((Q, t.shape[1]))
    for q in range(Q):
        for j in range(int(ptr[q]), int(ptr[q + 1])):
            x = t[row_offset + int(rows[j])]
            want[q] += w[j] * x
            mag[q] += np.abs(w[j] * x)
    n = np.diff(np.asarray(ptr, dtype=np.int64)).astype(np.float64)[:, None]
    return want, 2.0 ** -23 * np.abs(want) + n * 2.0 ** -50 * mag, mag


def weights(adj_type, ptr, items, item_degree):
    """float64 off-diagonal adjacency values of the edges (new user q, item i): n = the history's length, deg = the item's
    training degree (a cold item: 1, the new edge is its first)."""
    out = np.zeros(len(items))
    for q in range(len(ptr) - 1):
        lo, hi = int(ptr[q]), int(ptr[q + 1])
        n = float(hi - lo)
        for j in range(lo, hi):
            if adj_type == "plain":
                out[j] = 1.0
            elif adj_type == "norm":
                out[j] = 1.0 / (n + 1.0)
            elif adj_type == "pre":
                out[j] = 1.0 / np.sqrt(n * max(float(item_degree[int(items[j])]), 1.0))
            else:                                                        # gcmc, mean
                out[j] = 1.0 / n
    return out


def isolated_row_scale(adj_type, L):
    return 1.0 / (L + 1) if adj_type in ("plain", "gcmc", "pre") else 1.0


def fold_in_rows(out_items, ptr, items, w, id_rows, kappa, W, mods, d, mm_fusion_mode="concat"):
    """(rows float64 [Q x (1 + S) d], their bound, OutNew float64 [Q x C], its bound): the fold-in in float64 from the float32 inputs, and the bound of the float32 path --
    Out within 3 2^-24 of its magnitudes (the sum's rounding, the id product, their add) plus the sum's own bound, then each Linear
    within tau(K) of its magnitudes plus Out's error carried through |W| (the bound of tests/test_coldstart_gpu.py)."""
    from fp64_tools import TINY, tau
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    a = np.abs
    M = 1 + len(mods)
    s, s_bound, mag = segment_row_sum(out_items, ptr, items, w)
    x0 = np.tile(kappa * f64(id_rows), (1, M))
    out = x0 + s
    out_abs = a(x0) + mag
    out_err = 3.0 * 2.0 ** -24 * out_abs + s_bound
    wu, bu = f64(W["embedding_user_after_GCN.weight"]), f64(W["embedding_user_after_GCN.bias"])
    if mm_fusion_mode != "concat":
        wu = np.tile(wu / M, (1, M))
    rows = [out @ wu.T + bu]
    bound = [tau(M * d) * (out_abs @ a(wu).T + a(bu)) + out_err @ a(wu).T]
    for h, m in enumerate(mods):
        ws, bs = f64(W["s_dense_%s.weight" % m]), f64(W["s_dense_%s.bias" % m])
        blk = slice((h + 1) * d, (h + 2) * d)
        rows.append(out[:, blk] @ ws.T + bs)
        bound.append(tau(d) * (out_abs[:, blk] @ a(ws).T + a(bs)) + out_err[:, blk] @ a(ws).T)
    return np.concatenate(rows, 1), np.concatenate(bound, 1) * (1 + 1e-3) + TINY, out, out_err + TINY


def metrics_at(lists, truth, ks):
    """Recall@k of id lists against truth sets, float64 [n x len(ks)] (the one metric the report tests replay on the host)."""
    out = np.zeros((len(lists), len(ks)))
    for r, (row, t) in enumerate(zip(lists, truth)):
        t = set(int(i) for i in t)
        for c, k in enumerate(ks):
            out[r, c] = len(t & set(int(i) for i in row[:k] if i >= 0)) / float(len(t)) if t else 0.0
    return out


def user_rows(metrics, own_lists, lists, k, own_rows, rows):
    """Per-user rows [n x (Cs + 2)]: metrics, overlap = |own[:k] & list[:k]| / k, cos of the fused rows (0 for a zero row)."""
    n = len(lists)
    overlap = np.asarray([len(set(own_lists[r][:k].tolist()) & set(lists[r][:k].tolist())) / float(k) for r in range(n)])
    a, b = np.asarray(own_rows, dtype=np.float64), np.asarray(rows, dtype=np.float64)
    den = np.sqrt((a * a).sum(1) * (b * b).sum(1))
    cos = np.where(den > 0, (a * b).sum(1) / np.where(den > 0, den, 1.0), 0.0)
    return np.concatenate((np.asarray(metrics, dtype=np.float64).reshape(n, -1), overlap[:, None], cos[:, None]), axis=1)


def table(rows, positions):
    return np.asarray([[float(len(p))] + rows[np.asarray(p, dtype=np.int64)].mean(0).tolist() for p in positions])
