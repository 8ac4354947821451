"""An exact host model of the weighted two-step walk (csrc/walk.hip, ops.walk_topk, ops.rp3_weights) and the dense float64 RP3beta it
is held against.

The graph is the CSR q_ptr / q_nbr of the query side (row -> its neighbours on the other side), repeated edges kept. S(q, j) is the
int64 sum over the walks q -> u -> j of mid_weight[u] -- integer sparse products, so exact --, a row is listed when it has at least
one walk (its S may be 0), val = float32((float64(S) * 2^-40) * row_scale[q] * col_scale[j]), three float64 multiplies left to
right and one rounding; the order is (fp32 value descending, id ascending)."""
import numpy as np

import cooccur_model as cm

FRAC_BITS = 40


def rp3_weights(deg_query, deg_other, alpha, beta):
    """(mid_weight int64 [n_other], row_scale, col_scale float64 [n_query]) as ops.rp3_weights forms them."""
    def power(deg, p):
        deg = np.asarray(deg, dtype=np.int64)
        return np.where(deg > 0, np.power(np.maximum(deg.astype(np.float64), 1.0), -float(p)), 0.0)
    return np.rint(power(deg_other, alpha) * 2.0 ** FRAC_BITS).astype(np.int64), power(deg_query, alpha), power(deg_query, beta)


def sums(q_ptr, q_nbr, n_other, rows, mid_weight, back=None):
    """(C, S): CSR [Q x n_query] int64 of the walk counts and of the weighted sums of the given rows. S is stored wherever C is: a
    weight of 0 keeps its place (the products are formed with weight + 1 and the counts taken off again). back: the second step's
    CSR (o_ptr, o_nbr) where it is not the transpose of the first (edges one direction has lost)."""
    B = cm.incidence(q_ptr, q_nbr, n_other)
    Bt = B.T.tocsr() if back is None else cm.incidence(back[0], back[1], B.shape[0])
    w = np.asarray(mid_weight, dtype=np.int64)
    assert w.shape == (n_other,) and (w >= 0).all()
    rows = np.asarray(rows, dtype=np.int64)
    C = (B[rows] @ Bt).tocsr()
    S1 = (B[rows].multiply((w + 1)[None, :]).tocsr() @ Bt).tocsr()
    C.sort_indices()
    S1.sort_indices()
    assert np.array_equal(C.indptr, S1.indptr) and np.array_equal(C.indices, S1.indices)
    S = S1.copy()
    S.data = S1.data - C.data
    return C, S


def values(S, row_scale_q, col_scale_j):
    return (((np.asarray(S, dtype=np.int64).astype(np.float64) * 2.0 ** -FRAC_BITS) * np.float64(row_scale_q))
            * np.asarray(col_scale_j, dtype=np.float64)).astype(np.float32)


def topk(q_ptr, q_nbr, n_other, rows, K, mid_weight, row_scale, col_scale, back=None):
    """(idx int32, val float32) [Q x K]: the model of ops.walk_topk."""
    rows = np.asarray(rows, dtype=np.int64)
    idx = np.full((rows.size, K), -1, dtype=np.int32)
    val = np.full((rows.size, K), -np.inf, dtype=np.float32)
    if not rows.size:
        return idx, val
    C, S = sums(q_ptr, q_nbr, n_other, rows, mid_weight, back)
    row_scale, col_scale = np.asarray(row_scale, dtype=np.float64), np.asarray(col_scale, dtype=np.float64)
    for r, q in enumerate(rows):
        lo, hi = C.indptr[r], C.indptr[r + 1]
        j, c, s = C.indices[lo:hi].astype(np.int64), C.data[lo:hi], S.data[lo:hi]
        keep = (j != q) & (c >= 1)
        j, s = j[keep], s[keep]
        v = values(s, row_scale[q], col_scale[j])
        order = np.lexsort((j, -v.astype(np.float64)))[:K]
        idx[r, :order.size], val[r, :order.size] = j[order], v[order]
    return idx, val


def vote_scale(val, vote_bits=24):
    """(e, val * 2^e float32, zero_votes): the power of two that puts the largest finite value of a block of lists into [0.5, 1) (0
    without a positive one, at most 126), the block scaled by it -- exact in fp32 --, and the share of its finite entries whose
    fixed-point vote rint(float64(val) * 2^24) is 0 (EliMRec.neighbour_lists, source "rp3")."""
    val = np.asarray(val, dtype=np.float32)
    finite = np.isfinite(val)
    top = float(val[finite].max()) if finite.any() else 0.0
    e = min(126, -int(np.frexp(top)[1])) if top > 0.0 else 0
    scaled = np.ldexp(val, e).astype(np.float32)
    lost = (np.rint(scaled[finite].astype(np.float64) * 2.0 ** vote_bits) == 0).sum()
    return e, scaled, (float(lost) / int(finite.sum()) if finite.any() else 0.0)


def rp3_dense(q_ptr, q_nbr, n_other, alpha, beta):
    """The dense float64 RP3beta of a graph WITHOUT repeated edges, as the papers write it: W = normalize(A, l1)^alpha @
    normalize(A^T, l1)^alpha, every column j divided by deg(j)^beta; [n_query x n_query], the diagonal included."""
    A = cm.incidence(q_ptr, q_nbr, n_other).toarray().astype(np.float64)
    assert A.max() <= 1.0

    def normalized(M):                                       # (M / its row sums)^alpha on the edges, 0 elsewhere -- also for alpha = 0
        d = np.maximum(M.sum(axis=1, keepdims=True), 1.0)
        return np.where(M > 0, np.power(np.where(M > 0, M / d, 1.0), alpha), 0.0)

    W = normalized(A) @ normalized(A.T)
    deg = A.sum(axis=1)
    pen = np.where(deg > 0, np.power(np.maximum(deg, 1.0), -beta), 0.0)
    return W * pen[None, :]
