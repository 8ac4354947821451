"""Float64 model of the dense forward projection (linear_fwd_kernel of csrc/gemm.hip behind elimrec_linear_fwd and
elimrec_linear_fwd_batched), the cases with their poison, the checker and the restated launch decision. Nothing here calls a
project kernel; everything is host torch, so the unmarked self-tests (tests/test_linear_model_cpu.py) run on the very inputs the
GPU tests (tests/test_linear_fwd_gpu.py) use.

Contract (include/elimrec_hip.h, elimrec_linear_desc): for output row m in [max(range[0], 0), min(range[1], M)), or [0, M) without
a range,
    s = row_index ? row_index[m] : m
    C[m, n] = act( sum_k A[s, k] W[n, k] + (rowscale ? rowscale[s] : 1) * bias[n] + (add ? add[s, n] : 0) )
and nothing else is written. Reference: that formula in float64 torch on the CPU. Criterion: fp64_tools.assert_close, element by
element, with K_eff = K + 2 (the K products, the bias term, the add term) and scale = |A||W|^T + |rowscale||bias| + |add|: the
existing tau bound, no new constant. relu is 1-Lipschitz, so the reference under relu is max(ref, 0) and the same bound applies; in
addition, wherever ref < -bound the fp32 pre-activation is certainly negative and the output must be +0.0 bit for bit.

A case (`case()`) is a dict of host tensors. Its poison: the output buffer starts as NaN and everything the contract does not name
must still hold the same NaN bits afterwards (rows outside the range, the columns of the buffer beside the [off, off + N) window,
every row of an M == 0 or empty-range problem); whatever a call must not read holds NaN (columns >= K inside lda / ldw, rows of A /
rowscale / add that no in-range row_index entry names, columns beside the window of `add` inside ldadd). row_index entries outside
the row range are valid row numbers: they name a dedicated all-NaN last row of A, so a wrong read shows as NaN and never as a
fault. No case holds an out-of-bounds index or pointer.

`fwd_form` restates the host's launch decision (elimrec_linear_fwd_batched) ONLY to choose shapes and to assert that the intended
branch is reached; it is never a reference. One workgroup per 64 x 64 tile; tiles_m from the largest descriptor M (not from the
range), tiles_n from the largest N; the register pipeline is 8 K-chunks deep when the launch has at most 768 workgroups and 1 deep
above that; a workgroup's software pipeline has G = ceil(K / 16) stages.

Unreachable through the current host code, and so not tested: the persistent multi-tile walk of the kernel (wg_budget = 1 << 30
gives every tile its own workgroup, my_tiles is always 1) and the <128, 1> and <64, 4> instantiations (tile_rows is 64 and the
depth is 8 or 1).
"""
import torch

from fp64_tools import NAN, TINY, assert_close, same_bits, tau

TILE, KCHUNK, DEEP_WGS = 64, 16, 768


# ----------------------------------------------------------------------------------------------------------- launch form
def fwd_form(problems):
    """problems: (M, N, K) per problem of one launch -> dict(tiles_m, tiles_n, wgs, depth, G). depth is None when nothing is
    launched (every M == 0)."""
    n = len(problems)
    max_m = max(p[0] for p in problems)
    tiles_m = -(-max_m // TILE)
    tiles_n = max(-(-p[1] // TILE) for p in problems)
    wgs = tiles_m * tiles_n * n
    depth = None if max_m == 0 else (8 if wgs <= DEEP_WGS else 1)
    return dict(tiles_m=tiles_m, tiles_n=tiles_n, wgs=wgs, depth=depth, G=[-(-p[2] // KCHUNK) for p in problems])


def form_of(cases):
    return fwd_form([(c["M"], c["N"], c["K"]) for c in cases])


# ----------------------------------------------------------------------------------------------------------- cases
def clamp_range(rng, M):
    """The rows [lo, hi) a problem of M rows produces under `rng` (None: all)."""
    if rng is None:
        return 0, M
    lo, hi = max(int(rng[0]), 0), min(int(rng[1]), M)
    return (lo, hi) if hi > lo else (0, 0)


def case(M, N, K, bias=True, rowscale=False, add=False, index=None, rng=None, act=0, lda_pad=0, ldw_pad=0, c_off=0, c_pad=0,
         add_off=3, add_pad=2, seed=0):
    """One problem with its poison. index: None | 'perm' (a permutation into a taller A) | 'hot' (70 % of the entries name one
    row) | 'tall' (M larger than A's row count); rng: None | (begin, end) as given to the kernel (unclamped); act: 0 | 1."""
    g = torch.Generator().manual_seed(100003 * seed + 1009 * M + 31 * N + K)
    lo, hi = clamp_range(rng, M)
    rows = torch.arange(lo, hi)
    if index is None:
        ra, idx = max(M, 1), None
        named = rows
    else:
        ra = {"perm": M + 9, "hot": M + 1, "tall": max(M // 8, 4) + 1}[index]      # the last row is the NaN row
        if index == "perm":
            idx = torch.randperm(ra - 1, generator=g)[:M]
        else:
            idx = torch.randint(0, ra - 1, (M,), generator=g)
            if index == "hot":
                idx[torch.rand(M, generator=g) < 0.7] = 3
        inside = torch.zeros(M, dtype=torch.bool)
        inside[rows] = True
        idx[~inside] = ra - 1
        idx = idx.int()
        named = idx[rows].long().unique()
    A = torch.full((ra, K + lda_pad), NAN)
    A[named, :K] = torch.randn(len(named), K, generator=g)
    W = torch.full((max(N, 1), K + ldw_pad), NAN)
    W[:, :K] = torch.randn(max(N, 1), K, generator=g)
    c = dict(M=M, N=N, K=K, act=act, rng=rng, rows=rows, named=named, idx=idx, A=A, W=W, c_off=c_off, add_off=add_off,
             bias=torch.randn(N, generator=g) if bias else None, rowscale=None, add=None,
             C0=torch.full((max(M, 1), c_off + N + c_pad), NAN))
    if rowscale:
        rs = torch.full((ra,), NAN)
        rs[named] = torch.randn(len(named), generator=g)                  # mixed signs
        if len(named):
            rs[named[len(named) // 2]] = 0.0                              # one exact zero
        c["rowscale"] = rs
    if add:
        ad = torch.full((ra, add_off + N + add_pad), NAN)                 # a column window of a wider table
        ad[named, add_off:add_off + N] = torch.randn(len(named), N, generator=g)
        c["add"] = ad
    return c


def first_rows(c, M):
    """The same problem cut to its first M rows (no row_index, no range): shares W / bias and the first M rows of A."""
    assert c["idx"] is None and c["rng"] is None and c["rowscale"] is None and c["add"] is None and 0 < M <= c["M"]
    rows = torch.arange(M)
    return dict(c, M=M, rows=rows, named=rows, A=c["A"][:M].clone(), C0=c["C0"][:M].clone())


def source_rows(c):
    """The row of A / rowscale / add each produced row reads."""
    return c["rows"] if c["idx"] is None else c["idx"][c["rows"]].long()


def operands(c):
    """(A rows, W, bias, rowscale, add) of the produced rows, float32, the windows only."""
    s, N, K = source_rows(c), c["N"], c["K"]
    return (c["A"][s, :K], c["W"][:N, :K], c["bias"], None if c["rowscale"] is None else c["rowscale"][s],
            None if c["add"] is None else c["add"][s, c["add_off"]:c["add_off"] + N])


def reference(c):
    """(pre, ref, scale) over the produced rows in float64: the pre-activation, the output, the magnitude the bound multiplies."""
    a, w, b, rs, ad = [None if t is None else t.double() for t in operands(c)]
    pre, scale = a @ w.T, a.abs() @ w.abs().T
    if b is not None:
        r = torch.ones(a.shape[0], dtype=torch.float64) if rs is None else rs
        pre, scale = pre + r[:, None] * b[None, :], scale + r.abs()[:, None] * b.abs()[None, :]
    if ad is not None:
        pre, scale = pre + ad, scale + ad.abs()
    return pre, (pre.clamp_min(0.0) if c["act"] == 1 else pre), scale


def bound(c, scale):
    return tau(c["K"] + 2.0) * scale + TINY


def written(c):
    """Boolean mask over the output buffer: the elements the contract names."""
    m = torch.zeros(c["C0"].shape, dtype=torch.bool)
    m[c["rows"], c["c_off"]:c["c_off"] + c["N"]] = True
    return m


def window(c, buf):
    return buf[c["rows"], c["c_off"]:c["c_off"] + c["N"]]


def check(c, buf, what, elsewhere=None, ref=None):
    """The output buffer `buf` (host, after the call) against the contract. elsewhere: mask of elements another problem of the
    same launch writes into this buffer (they are that problem's to check). Returns the worst err / tol."""
    assert buf.shape == c["C0"].shape and buf.dtype == torch.float32, what
    pre, want, scale = reference(c) if ref is None else ref
    got = window(c, buf)
    tol = bound(c, scale)
    assert_close(got, want, scale, c["K"] + 2.0, what)
    if c["act"] == 1:
        dead = pre < -tol
        bits = got.contiguous().view(torch.int32)
        assert bool((bits[dead] == 0).all()), "%s: %d elements under relu with ref < -bound are not +0.0" % (
            what, int((bits[dead] != 0).sum()))
    keep = ~written(c)
    if elsewhere is not None:
        keep &= ~elsewhere
    assert same_bits(buf[keep], c["C0"][keep]), "%s: %d elements outside the contract were written" % (
        what, int((buf[keep].view(torch.int32) != c["C0"][keep].view(torch.int32)).sum()))
    return float(((got.double() - want).abs() / tol).max()) if got.numel() else 0.0


def place(c, values):
    """An output buffer as a correct call would leave it if the produced rows held `values` ([rows x N], any float dtype)."""
    buf = c["C0"].clone()
    buf[c["rows"], c["c_off"]:c["c_off"] + c["N"]] = values.float()
    return buf


# ----------------------------------------------------------------------------------------------------------- the shapes
MS = [1, 31, 32, 33, 63, 64, 65, 127, 129, 200]
NS = [1, 5, 31, 32, 33, 63, 64, 65, 96, 130]
KS = [4, 12, 16, 20, 112, 128, 132, 144, 260, 272, 2048]
KS_G = [1, 1, 1, 2, 7, 8, 9, 9, 17, 17, 128]
EXTREMES = [(1, 1, 4), (65, 65, 20), (129, 130, 2048)]


def plain_triples():
    """The covering list of section A: three passes over the M list with the N and K lists rotated, plus the extremes."""
    out = []
    for r in range(3):
        for i in range(10):
            out.append((MS[i], NS[(i + 3 * r) % 10], KS[(i + 10 * r) % 11]))
    return out + [t for t in EXTREMES if t not in out]


def plain_layout(j):
    """Strides and offsets of plain case j: lda = K + {0, 4, 24}, ldw = K + {0, 8}, the output a view buf[:, off:off + N] with
    off in {0, 3, 8} and ldc = N + off + {0, 5}."""
    return dict(lda_pad=[0, 4, 24][j % 3], ldw_pad=[0, 8][j % 2], c_off=[0, 3, 8][(j // 2) % 3], c_pad=[0, 5][(j // 3) % 2])


def plain_case(j, bias, act):
    M, N, K = plain_triples()[j]
    return case(M, N, K, bias=bias, act=act, seed=j, **plain_layout(j))


# section B: M = 200 so that the ranges of the issue cut tile rows 0..3 in every way; N = 70 and K = 36 cross one tile edge each
FM, FN, FK = 200, 70, 36
RANGES = [(0, 200), (17, 200), (64, 128), (70, 71), (150, 1000), (-5, 10), (40, 40), (50, 20)]
INDEX_FORMS = ["perm", "hot", "tall"]


_ALL4 = dict(rowscale=True, add=True, index="perm")
FIELD_CASES = dict([
    ("rowscale", dict(rowscale=True)), ("rowscale, no bias", dict(rowscale=True, bias=False)), ("add", dict(add=True)),
    ("index perm", dict(index="perm")), ("index hot", dict(index="hot")), ("index tall", dict(index="tall"))]
    + [("range %d %d" % r, dict(rng=r)) for r in RANGES]
    # _fold_problems of model.py: the gathered form (all four fields), and the compact form (no row_index, range given)
    + [("all four", dict(_ALL4, rng=(0, 137))), ("all four, relu", dict(_ALL4, rng=(0, 137), act=1)),
       ("all four, inner range, relu", dict(_ALL4, rng=(17, 150), act=1)), ("all four, hot", dict(_ALL4, index="hot", rng=(0, 137))),
       ("compact", dict(rowscale=True, add=True, rng=(0, 137))), ("compact, relu", dict(rowscale=True, add=True, rng=(0, 137), act=1))])


def field_case(name):
    kw = dict(lda_pad=4, c_off=3, c_pad=5)
    kw.update(FIELD_CASES[name])
    return case(FM, FN, FK, seed=1000 + list(FIELD_CASES).index(name), **kw)


# section C: problems of different shapes in one launch
def batch_cases(n):
    """n = 2, 3, 5, 8 problems, a different (M, N, K) each, the fields mixed across them; from 5 on, one M == 0 problem, one
    empty range and N = 130 beside N = 5."""
    pool = [dict(M=130, N=130, K=20, bias=True, rowscale=True, add=True, index="perm", rng=(3, 120), act=1),
            dict(M=33, N=5, K=132, bias=True, act=0, c_off=3, c_pad=5),
            dict(M=200, N=65, K=16, bias=False, add=True, rng=(64, 129), act=1, lda_pad=4),
            dict(M=0, N=33, K=12, bias=True),
            dict(M=90, N=64, K=144, bias=True, rowscale=True, rng=(40, 40), ldw_pad=8),
            dict(M=65, N=96, K=4, bias=True, index="hot", act=0, c_off=8),
            dict(M=1, N=1, K=260, bias=False, act=1),
            dict(M=129, N=31, K=112, bias=True, rowscale=True, index="tall", rng=(-5, 100), act=0, lda_pad=24)]
    return [case(seed=2000 + 10 * n + i, **kw) for i, kw in enumerate(pool[:n])]


def split_cases(n_lo, n=150, N=70, K=36):
    """The fused-head pattern of model.py (_fwd_head): two problems write the disjoint row ranges (0, n_lo) and (n_lo, n) of the
    SAME output window with different weights and biases. The second case's C0 is the first's."""
    a = case(n, N, K, rng=(0, n_lo), c_off=3, c_pad=5, seed=3000 + n_lo)
    b = case(n, N, K, rng=(n_lo, n), c_off=3, c_pad=5, seed=3500 + n_lo)
    return a, b


# the depth threshold: (cases of the 768-workgroup launch, cases of the launch just above it), sharing rows and inputs
def threshold_single():
    big = case(49153, 64, 20, seed=4000)
    return [first_rows(big, 49152)], [big]


def threshold_batch():
    rest = [case(M, N, K, seed=4100 + i, **kw) for i, (M, N, K, kw) in enumerate([
        (2048, 130, 132, dict(act=1)), (700, 5, 20, dict(bias=False)), (64, 64, 16, dict(c_off=3)), (1, 130, 4, {}),
        (1000, 33, 144, dict(lda_pad=4)), (2047, 96, 12, dict(act=1, bias=False)), (129, 1, 272, {})])]
    big = case(2049, 130, 132, seed=4200)
    return [first_rows(big, 2048)] + rest, [big] + rest


WIDE_M, WIDE_N, WIDE_KS = 64 * 60, 64 * 13, [16, 144, 2048]        # 780 workgroups: depth 1 at G = 1, 9, 128


# section E: one MLP layer
MLP_SHAPES = [(10, 6, 37), (24, 16, 130), (100, 64, 37), (10, 64, 130), (100, 6, 130), (24, 6, 37)]
MLP_SEED = 0


def mlp_case(n_in, n_out, rows, seed=MLP_SEED):
    g = torch.Generator().manual_seed(7919 * seed + 101 * n_in + 11 * n_out + rows)
    return dict(x=torch.randn(rows, n_in, generator=g), w=torch.randn(n_out, n_in, generator=g) / n_in ** 0.5,
                b=torch.randn(n_out, generator=g), gy=torch.randn(rows, n_out, generator=g))


def mlp_reference(m, relu):
    """Float64 autograd of y = act(x W^T + b) under the upstream gradient gy: dict of (value, scale, K) per output. Scales: the
    forward's as above (K + 2); dX: |g||W| with K = n_out + 2; dW, db: the contraction bound tau(rows) |g|^T |x| (g = gy under the
    relu mask)."""
    x, w, b = [m[k].double().requires_grad_(True) for k in ("x", "w", "b")]
    pre = x @ w.T + b
    y = pre.clamp_min(0.0) if relu else pre
    y.backward(m["gy"].double())
    g = m["gy"].double() * ((pre > 0).double() if relu else 1.0)
    xa, wa = m["x"].double().abs(), m["w"].double().abs()
    rows, n_out = m["x"].shape[0], m["w"].shape[0]
    fs = xa @ wa.T + m["b"].double().abs()
    return dict(pre=pre.detach(), y=(y.detach(), fs, m["x"].shape[1] + 2.0), dx=(x.grad, g.abs() @ wa, n_out + 2.0),
                dw=(w.grad, g.abs().T @ xa, float(rows)), db=(b.grad, g.abs().sum(0), float(rows)))
