"""The staging of the weight-gradient partial products (csrc/bwd_w.h: bwd_w_partial_body), bit for bit.

A workgroup owns a chunk of rows and a PAIR of adjacent 64 x 64 output tiles; the chunk's A rows are staged once for both. What the
staging must not change is the arithmetic, which bwd_w.h documents and `model` below restates in NumPy:
  * a chunk is `chunk_rows` consecutive rows of the range (bwd_w_dims); inside a chunk every output element is one accumulator that
    takes the rows in row order, each as one fused multiply-add in float32 (v_mfma_f32_32x32x2_f32 walks its two k in order);
    rows behind the range enter as zeros (they add +0 and change nothing);
  * the reduce gives lane q of an element's four the chunks q, q + 4, ... in that order, then (q0 + q1) + (q2 + q3);
  * the column sum is a plain float32 sum of A's rows in row order per chunk, reduced the same way.
The fused multiply-add is formed exactly: the product of two float32 is exact in float64, the float64 sum is corrected to
round-to-odd with the error term of TwoSum, and rounding that to float32 is then the single rounding of an fma.

Shapes (the smallest at which the staging can go wrong): R = 1, 31, 32, 33, 65 rows (one row; one short of a 32-row stage; exactly
one; one over; three stages with a ragged last one, which at chunk_rows = 64 is also a second chunk of ONE row = chunk_rows + 1);
outputs of one, two and four tiles in either direction (64 x 64, 128 x 64, 256 x 64, 64 x 128, 64 x 256: the last two are the pair
and the two pairs of one chunk); duplicate row indices; and a range that ends before the rows do, so that the last stage of the
first chunk is ragged or the whole last chunk is padding (its workgroups run over no row and the reduce must not read them).
"""
import numpy as np
import pytest
import torch

from fp64_tools import same_bits
import slab_model as sm

DEV = "cuda:0"
gpu = pytest.mark.gpu
TN, TRB = 64, 32
SHAPES = [(64, 64), (128, 64), (256, 64), (64, 128), (64, 256)]
ROWS = [1, 31, 32, 33, 65]


def dims(R, n1, n2):
    """chunk_rows of bwd_w_dims."""
    t1, t2 = -(-n1 // TN), -(-n2 // TN)
    want = -(-(R * t1 * t2) // 480)
    want = -(-want // TRB) * TRB
    return min(max(want, 64), 512)


def fma32(a, b, c):
    """round32(a * b + c) of float32 arrays, one rounding."""
    p = a.astype(np.float64) * b.astype(np.float64)            # exact
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)                              # TwoSum: p + c = s + e exactly
    bits = s.view(np.int64)
    fix = (e != 0) & ((bits & 1) == 0)
    toward = np.where(e > 0, np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, toward), s)              # round to odd
    return s.astype(np.float32)


def lane_order_sum(parts):
    """parts: [chunks, ...] float32 -> the reduce's (q0 + q1) + (q2 + q3)."""
    lanes = []
    for q in range(4):
        s = np.zeros(parts.shape[1:], np.float32)
        for c in range(q, parts.shape[0], 4):
            s = s + parts[c]
        lanes.append(s)
    return (lanes[0] + lanes[1]) + (lanes[2] + lanes[3])


def model(A, B, rows_b, lo, hi, R):
    """out, colsum of the contraction over rows lo..hi-1 of A (B's row rows_b[r]) as the kernels add them."""
    n1, n2 = A.shape[1], B.shape[1]
    cr = dims(R, n1, n2)
    chunks = max(-(-(hi - lo) // cr), 0)
    parts = np.zeros((chunks, n1, n2), np.float32)
    cparts = np.zeros((chunks, n1), np.float32)
    for c in range(chunks):
        for r in range(lo + c * cr, min(lo + (c + 1) * cr, hi)):
            parts[c] = fma32(A[r][:, None], B[rows_b[r]][None, :], parts[c])
            cparts[c] = cparts[c] + A[r]
    return lane_order_sum(parts), lane_order_sum(cparts)


def run(A, B, idx, rng, R, n1, n2):
    from elimrec_amd import ops
    out = torch.full((n1, n2), float("nan"), device=DEV)
    cs = torch.full((n1,), float("nan"), device=DEV)
    ws = torch.full((ops.linear_bwd_w_workspace(R, n1, n2),), 0xFF, dtype=torch.uint8, device=DEV)
    ops.linear_bwd_w(A, B, out, ws, row_index=idx, rng=rng, colsum=cs, rows=R)
    return out, cs


def check(R, n1, n2, index=None, rng=None, seed=0):
    g = np.random.RandomState(1000 * seed + 31 * R + n1 + 3 * n2)
    nb = R if index is None else 40
    A = g.standard_normal((R, n1)).astype(np.float32)
    B = g.standard_normal((nb, n2)).astype(np.float32)
    rows_b = np.arange(R) if index is None else g.randint(0, nb, R)
    if index == "hot":
        rows_b[g.rand(R) < 0.7] = 3                            # a popular item, listed many times
    lo, hi = (0, R) if rng is None else rng
    want, cwant = model(A, B, rows_b, lo, hi, R)
    Ad, Bd = torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)
    idx = None if index is None else torch.from_numpy(rows_b.astype(np.int32)).to(DEV)
    rg = None if rng is None else torch.tensor([lo, hi], dtype=torch.int32, device=DEV)
    out, cs = run(Ad, Bd, idx, rg, R, n1, n2)
    what = "R %d, %d x %d, index %s, range %s" % (R, n1, n2, index, rng)
    bad = int((out.cpu().numpy().view(np.int32) != want.view(np.int32)).sum())
    cbad = int((cs.cpu().numpy().view(np.int32) != cwant.view(np.int32)).sum())
    print("%s: %d of %d outputs, %d of %d column sums differ from the model" % (what, bad, n1 * n2, cbad, n1))
    assert bad == 0 and cbad == 0, what
    for _ in range(9):                                         # ten launches, identical bytes
        o2, c2 = run(Ad, Bd, idx, rg, R, n1, n2)
        assert same_bits(o2, out) and same_bits(c2, cs), what + ": a later launch differs"


@gpu
@pytest.mark.parametrize("n1,n2", SHAPES)
def test_contraction_is_the_documented_sum_bit_for_bit(n1, n2):
    for R in ROWS:
        assert dims(R, n1, n2) == 64                           # so R = 65 is chunk_rows + 1: a second chunk of one row
        check(R, n1, n2)


@gpu
@pytest.mark.parametrize("n1,n2", SHAPES)
def test_duplicate_rows_and_padding_stages(n1, n2):
    check(65, n1, n2, index="hot", seed=1)
    check(33, n1, n2, index="hot", seed=2)
    check(96, n1, n2, rng=(0, 40), seed=3)                     # the chunk's second stage is ragged, the second chunk all padding
    check(96, n1, n2, rng=(0, 64), seed=4)                     # two full stages; the second chunk's workgroups see no row
    check(96, n1, n2, index="hot", rng=(5, 70), seed=5)        # a range that starts inside the rows: one row in the second chunk


def _hop_case():
    from elimrec_amd import slab
    d, w, T = 64, 32, 64
    ns = d // w
    gs = slab.choose_groups(ns)
    G = 64 // ((ns // gs) * (w // 4))
    m, _ = sm.tier_ladder(T, G)
    n = m.shape[0]
    plan = slab.SellPlan(m, DEV, threshold=T, side_split=n // 3, tiered=True, ipw=G)
    x = slab.SlabTable(n, ns, w, DEV).from_rows(torch.randn(n, d, generator=torch.Generator().manual_seed(5)).to(DEV))
    return plan, x, gs, n


@gpu
def test_partial_products_riding_the_masked_hop_change_no_bit():
    """elimrec_slab_hop_bwd_w with the partial products (phase 0) on a tier ladder: the slabs are the stand-alone launch's bytes, the
    hop's table the plain masked hop's; ten launches, the same bytes."""
    from elimrec_amd import ops, slab
    plan, x, gs, n = _hop_case()
    g = torch.Generator().manual_seed(9)
    R = 700                                                    # 11 chunks: more than the reduce's four lanes, a ragged last one
    shapes = [(64, 256), (64, 128), (64, 64), (128, 64)]
    idx = torch.randint(0, 300, (R,), generator=g).int().to(DEV)
    rng = torch.tensor([3, R - 2], dtype=torch.int32, device=DEV)
    A = [torch.randn(R, n1, generator=g).to(DEV) for n1, _ in shapes]
    B = [torch.randn(300 if k % 2 else R, n2, generator=g).to(DEV) for k, (_, n2) in enumerate(shapes)]
    wt = torch.randn(R, generator=g).to(DEV)
    nbytes = ops.linear_bwd_w_batched_workspace([(R, n1, n2) for n1, n2 in shapes])

    def problems():
        outs = [torch.full(s, float("nan"), device=DEV) for s in shapes]
        css = [torch.full((s[0],), float("nan"), device=DEV) for s in shapes]
        pr = []
        for k in range(len(shapes)):
            p = dict(A=A[k], B=B[k], out=outs[k], colsum=css[k], rng=rng, rows=R)
            if k % 2:
                p["row_index"] = idx
            if k == 0:
                p["colsum_weight"] = wt
            pr.append(p)
        return pr, outs, css

    mask = torch.rand(n, generator=g) < 0.3
    bm = torch.from_numpy(sm.bitmap_words(mask.numpy())).to(DEV)
    y0 = x.like()
    y0.data.fill_(float("nan"))
    slab.hop(plan, x, y0, gs=gs, src_mask=bm)
    pr, outs0, css0 = problems()
    ws0 = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    h = ops.linear_bwd_w_batched(pr, ws0, defer_reduce=True)
    ops.linear_bwd_w_reduce(h)
    for _ in range(10):
        pr, outs, css = problems()
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
        h = ops.linear_bwd_w_batched(pr, ws, defer_all=True)
        y = x.like()
        y.data.fill_(float("nan"))
        slab.hop(plan, x, y, gs=gs, src_mask=bm, bwd_w=h, bwd_w_phase=0)
        assert torch.equal(ws, ws0), "the slabs differ from the stand-alone launch's"
        assert same_bits(y.data, y0.data), "the hop's table differs from the plain masked hop's"
        ops.linear_bwd_w_reduce(h)
        for k in range(len(shapes)):
            assert same_bits(outs[k], outs0[k]) and same_bits(css[k], css0[k]), shapes[k]
