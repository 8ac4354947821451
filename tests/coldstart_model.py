"""Host models of the cold-start paths.

rank_values: the exact integer model of ops.rank_values (csrc/coldstart.hip) -- per value v of row b the number of columns j != skip
with scores[b, j] >= v, -1 where v is not finite -- once by sort + searchsorted (what the kernel does) and once by brute force.
fold_in_rows: the float64 model of EliMRec.fold_in_items -- kappa, the feature projections, the item fusion Linear and the heads."""
import numpy as np


def csr(lists, dtype=np.float32):
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=ptr[1:])
    flat = np.concatenate([np.asarray(x, dtype=dtype) for x in lists]) if ptr[-1] else np.zeros(0, dtype=dtype)
    return ptr, flat.astype(dtype)


def rank_values_brute(scores, ptr, vals, skip=None):
    """The definition, one comparison at a time (IEEE: -0.0 == 0.0, -inf >= a finite v is false, NaN compares false)."""
    scores = np.asarray(scores, dtype=np.float32)
    out = np.zeros(len(vals), dtype=np.int32)
    for b in range(scores.shape[0]):
        for p in range(int(ptr[b]), int(ptr[b + 1])):
            v = np.float32(vals[p])
            if not np.isfinite(v):
                out[p] = -1
                continue
            n = 0
            for j in range(scores.shape[1]):
                if skip is not None and j == int(skip[p]):
                    continue
                n += 1 if scores[b, j] >= v else 0
            out[p] = n
    return out


def rank_values(scores, ptr, vals, skip=None):
    """The same counts from a sorted row: #{s >= v} = I - searchsorted(sorted row, v, 'left'); the skipped column taken off."""
    scores = np.asarray(scores, dtype=np.float32)
    vals = np.asarray(vals, dtype=np.float32)
    out = np.zeros(len(vals), dtype=np.int32)
    I = scores.shape[1]
    for b in range(scores.shape[0]):
        lo, hi = int(ptr[b]), int(ptr[b + 1])
        if hi <= lo:
            continue
        row = np.sort(scores[b])
        v = vals[lo:hi]
        fin = np.isfinite(v)
        n = (I - np.searchsorted(row, np.where(fin, v, 0), side="left")).astype(np.int64)
        if skip is not None:
            s = np.asarray(skip[lo:hi], dtype=np.int64)
            own = np.where(s >= 0, scores[b, np.clip(s, 0, I - 1)], -np.inf)
            n -= ((s >= 0) & (own >= np.where(fin, v, 0))).astype(np.int64)
        out[lo:hi] = np.where(fin, n, -1)
    return out


def among(vals_block):
    """[B x Q] scores of the new items -> per (b, q) the number of other new items that beat q by (score descending, q ascending)."""
    v = np.asarray(vals_block)
    order = np.argsort(-v.astype(np.float64), axis=1, kind="stable")
    place = np.empty_like(order)
    np.put_along_axis(place, order, np.broadcast_to(np.arange(v.shape[1]), v.shape).copy(), axis=1)
    return place.astype(np.int32)


def isolated_row_scale(adj_type, L):
    """kappa in exact arithmetic: 1 / (L + 1) without a diagonal, 1 with one."""
    return 1.0 / (L + 1) if adj_type in ("plain", "gcmc", "pre") else 1.0


def fold_in_rows(feats, id_rows, W, mods, d, kappa, mm_fusion_mode="concat"):
    """float64 rows [Q x (1 + S) d] of items without an edge. feats: dict letter -> [Q x D_m]; W: dict of the model's parameter
    arrays by state_dict name; kappa as a float (pass the float32 kappa to model the kernels' constant)."""
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    blocks = [kappa * f64(id_rows)]
    for m in mods:
        blocks.append(kappa * (f64(feats[m]) @ f64(W[m + "_dense.weight"]).T + f64(W[m + "_dense.bias"])))
    wi, bi = f64(W["embedding_item_after_GCN.weight"]), f64(W["embedding_item_after_GCN.bias"])
    if mm_fusion_mode == "concat":
        fused = np.concatenate(blocks, axis=1) @ wi.T + bi
    else:
        fused = (sum(blocks) / len(blocks)) @ wi.T + bi
    heads = [blocks[1 + h] @ f64(W["s_dense_%s.weight" % m]).T + f64(W["s_dense_%s.bias" % m]) for h, m in enumerate(mods)]
    return np.concatenate([fused] + heads, axis=1)
