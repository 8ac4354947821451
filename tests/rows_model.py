"""Float64 model of the layer means at listed rows (csrc/rows_args.h: rows_piece, run by slab_rows_kernel and by
head_rows_fwd16_kernel) and of the wide form (csrc/wide.hip: wide_from_master, wide_rows, wide_grad), the graph their tests share
and a numpy float32 restatement of rows_piece in the kernel's own order. Nothing here calls a project kernel.

rows_piece at row r of a table of d columns, L + 1 layers:
    out0[r]   = 1/(L+1) (X^0[r] + X^1[r] + ... + X^L[r])
    narrow[r] = 1/(L+1) sum of X^k[r] over the even k (r < U: a user row) or the odd k (an item row)
X^0 .. X^(L-1) are given fp32 tables; X^L is a given table, or A X^(L-1) evaluated on the spot: one fma chain over the row's
neighbours in CSR order for a row of at most T entries, the row's entry of the compact long-row table otherwise.

The criterion is fp64_tools.assert_close with a bound per row: K = the row's own length + L + 2 where hop L is evaluated (the
row's chain, the L additions of the running sum, the scale), L + 2 where X^L is given, and scale = the same expression over
magnitudes (|A||X^(L-1)| for the evaluated layer). wide_rows adds two halves per layer: K = 2 (L + 1) + 1.
"""
import functools
import types

import numpy as np
import scipy.sparse as sp
import torch

import slab_model as sm
from propagate_model import _from_lengths, _t, row_lengths

UNSPLIT_LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)     # on and next to the 16-wide groups of the inline hop


# ----------------------------------------------------------------------------------------------------------- the ladder
def upper_lengths(T, G):
    """The shortest and the longest row slab_model's ladder names in each upper tier (wave, workgroup, segmented; the 9 G T row
    that only lengthens the segment combine left out: the rows evaluation reads one table entry per long row whatever its length)."""
    named = np.asarray([n for n in sm.ladder_named_lengths(T, G) if n > T and n != sm.big_row(T, G)])
    tier = sm.tier_of(named, T, G)
    out = []
    for k in (sm.WAVE, sm.WORKGROUP, sm.SEGMENTED):
        assert (tier == k).any(), "no named row in tier %s (T %d, G %d)" % (sm.TIER_NAMES[k], T, G)
        out += [int(named[tier == k].min()), int(named[tier == k].max())]
    return out


@functools.lru_cache(maxsize=None)
def rows_ladder(T, G, U_frac=0.4, seed=0):
    """(m, U, named): a square CSR matrix (float32 weights in +-[0.1, 1.1], sorted distinct columns), the side boundary U and
    {(side, length): row}. On each side ("user": rows < U, "item": the others) the unsplit rows hold the lengths 0, 1, 2, 15, 16,
    17, 31, 32, 33, 47, 48, 49, 63, 64 that do not exceed T, once each by construction, and there are two rows of every upper
    tier of a tiered plan (threshold T, G lane groups). Rows U - 1 and U are not empty, row 0 and the last row are; the row
    count is odd."""
    side = [n for n in UNSPLIT_LENGTHS if n <= T] + upper_lengths(T, G)
    N = max(side) + 38
    N += 1 - N % 2
    n_user = min(max(int(round(U_frac * N)), len(side) + 2), N - len(side) - 2)
    fill = [1, 0, 2, 1, 3, 1, 0, 1, 5, 1, 0, 2, 7, 1, 0, 4]
    f = lambda k, at: [min(fill[(i + at) % len(fill)], T) for i in range(k)]
    users = side + f(n_user - len(side) - 1, 0) + [3]                          # row U - 1: three entries
    items = [5] + side + f(N - n_user - len(side) - 2, 5) + [0]                # row U: five entries; the last row: none
    lens = users + items
    assert len(lens) == N and lens[0] == 0 and lens[n_user - 1] > 0 and lens[n_user] > 0
    m = _from_lengths(lens, N, seed + 64 * T + G + 3)
    named = {("user", n): r for r, n in enumerate(side)}
    named.update({("item", n): n_user + 1 + r for r, n in enumerate(side)})
    return m, n_user, named


def listed_rows(m, U, named, n_random, seed, sort=False):
    """The named rows, rows U - 1 and U and n_random others, shuffled (or sorted): int64 node ids, each once."""
    rs = np.random.RandomState(seed)
    must = sorted(set(named.values()) | {U - 1, U})
    rest = np.setdiff1d(np.arange(m.shape[0]), must)
    rows = np.concatenate([must, rs.choice(rest, size=min(n_random, len(rest)), replace=False)]).astype(np.int64)
    return np.sort(rows) if sort else rs.permutation(rows)


# ----------------------------------------------------------------------------------------------------------- float64
def _f64(x):
    return np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float64)


def rows_ref(m, X, XL, rows, U):
    """(out0, scale0, narrow, scale_n, K) of the listed rows as float64 tensors ([R x d]; K [R x 1]). X: the L tables X^0 ..
    X^(L-1) ([N x d]); XL: the table X^L taken as an input, or None: A X^(L-1) in float64."""
    L = len(X)
    rows = np.asarray(rows, dtype=np.int64)
    lay = [_f64(x)[rows] for x in X]
    mag = [np.abs(v) for v in lay]
    if XL is None:
        A = sp.csr_matrix(m, dtype=np.float64)[rows]
        xlm1 = _f64(X[L - 1])
        lay.append(A @ xlm1)
        mag.append(abs(A) @ np.abs(xlm1))
        K = row_lengths(m)[rows].astype(np.float64) + L + 2.0
    else:
        lay.append(_f64(XL)[rows])
        mag.append(np.abs(lay[-1]))
        K = np.full(len(rows), L + 2.0)
    inv = 1.0 / (L + 1.0)
    user = (rows < U)[:, None]
    part = lambda v, p: sum(v[k] for k in range(p, L + 1, 2)) if p <= L else np.zeros_like(v[0])
    out0, s0 = sum(lay) * inv, sum(mag) * inv
    nar = np.where(user, part(lay, 0), part(lay, 1)) * inv
    sn = np.where(user, part(mag, 0), part(mag, 1)) * inv
    return _t(out0), _t(s0), _t(nar), _t(sn), _t(K).unsqueeze(1)


# ----------------------------------------------------------------------------------------------------------- float32
def _fma(a, b, c):
    """fmaf on float32 arrays: the product of two floats is exact in float64, the sum is rounded once more to float32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def rows_fp32(m, X, XL, rows, U, T=None, long_tab=None):
    """rows_piece in numpy float32, in the kernel's order: hop L as ONE fmaf chain over the row's neighbours in CSR order from
    zero, sum = ((X^0 + X^1) + X^2) + ... + X^L, narrow likewise over its layers, each times the float 1 / (L + 1).
    T, long_tab: rows longer than T take row long_index[r] of long_tab ([n_long x d] float32, the rows above T in row order)
    instead of the chain. Returns (out0, narrow) as float32 arrays [R x d]."""
    L = len(X)
    rows = np.asarray(rows, dtype=np.int64)
    X = [np.asarray(x, dtype=np.float32) for x in X]
    if XL is not None:
        xl = np.asarray(XL, dtype=np.float32)[rows]
    else:
        m = sp.csr_matrix(m)
        lens = row_lengths(m)
        chain = np.ones(len(rows), dtype=bool)
        xl = np.zeros((len(rows), X[0].shape[1]), dtype=np.float32)
        if T is not None:
            long_index = np.cumsum(lens > T) - 1
            chain = lens[rows] <= T
            xl[~chain] = np.asarray(long_tab, dtype=np.float32)[long_index[rows[~chain]]]
        beg, n = m.indptr[rows].astype(np.int64), np.where(chain, lens[rows], 0)
        for j in range(int(n.max()) if len(n) else 0):
            on = np.nonzero(n > j)[0]
            e = beg[on] + j
            xl[on] = _fma(m.data[e].astype(np.float32)[:, None], X[L - 1][m.indices[e]], xl[on])
    lay = [x[rows] for x in X] + [xl]
    user = rows < U
    s = lay[0] + lay[1]
    nar = np.where(user[:, None], lay[0], lay[1])
    for k in range(2, L + 1):
        s = s + lay[k]
        take = user if k % 2 == 0 else ~user
        nar = np.where(take[:, None], nar + lay[k], nar)
    inv = np.float32(1.0) / np.float32(L + 1)
    return (s * inv).astype(np.float32), (nar * inv).astype(np.float32)


def long_table_fp32(m, XLm1, T):
    """The rows above T of A X^(L-1), each correctly rounded to float32: a stand-in for the hop's compact long-row table."""
    m = sp.csr_matrix(m, dtype=np.float64)
    return (m[np.nonzero(row_lengths(m) > T)[0]] @ np.asarray(XLm1, dtype=np.float64)).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------- the wide form
def wide_from_master(master, U):
    """wide_from_master, exactly: [N x 2 d] float32 = [E | 0] on user rows, [0 | E] on item rows (a select)."""
    E = np.asarray(master, dtype=np.float32)
    user = (np.arange(E.shape[0]) < U)[:, None]
    z = np.zeros_like(E)
    return np.concatenate([np.where(user, E, z), np.where(user, z, E)], axis=1)


def wide_grad(wide, U, scale):
    """wide_grad, exactly: [N x d] float32 = float(scale) * (the left half on user rows, the right half on item rows)."""
    W = np.asarray(wide, dtype=np.float32)
    d = W.shape[1] // 2
    user = (np.arange(W.shape[0]) < U)[:, None]
    return (np.where(user, W[:, :d], W[:, d:]) * np.float32(scale)).astype(np.float32)


def wide_rows(layers, rows):
    """wide_rows in float64: (out0, scale0, narrow, scale_n, K) of the listed rows, out0 = 1/(L+1) sum_k (left_k + right_k),
    narrow = 1/(L+1) sum_k left_k; a negative id is padding: its slot is NaN here (not written there). K = 2 (L + 1) + 1."""
    L = len(layers) - 1
    rows = np.asarray(rows, dtype=np.int64)
    d = np.asarray(layers[0]).shape[1] // 2
    real = rows >= 0
    lay = [_f64(x)[np.where(real, rows, 0)] for x in layers]
    inv = 1.0 / (L + 1.0)
    pad = lambda v: _t(np.where(real[:, None], v, np.nan))
    out0 = sum(v[:, :d] + v[:, d:] for v in lay) * inv
    s0 = sum(np.abs(v[:, :d]) + np.abs(v[:, d:]) for v in lay) * inv
    nar = sum(v[:, :d] for v in lay) * inv
    sn = sum(np.abs(v[:, :d]) for v in lay) * inv
    return pad(out0), pad(s0), pad(nar), pad(sn), 2.0 * (L + 1) + 1.0


wide_ref = types.SimpleNamespace(from_master=wide_from_master, grad=wide_grad, rows=wide_rows)
