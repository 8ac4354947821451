"""The part of the training step that WRITES the parameters, against plain float64 math, element by element: the weight-gradient
contraction (csrc/gemm.hip, csrc/bwd_w.h: elimrec_linear_bwd_w, _batched, _batched_merge, _reduce and both phases riding in
elimrec_slab_hop_bwd_w) and the optimizer in all its forms (elimrec_adam_step, elimrec_adam_step_out, elimrec_adam_multi, the Adam
epilogue of elimrec_slab_hop_adam with its tail jobs and loss-sum workgroup, elimrec_slab_sweep_hop_adam).

Conventions (those of tests/test_head_kernels_gpu.py): the references are float64 torch / numpy / scipy written here from the
contract in include/elimrec_hip.h and never call a project kernel; every output starts as NaN and everything the contract does not
name must still be NaN afterwards, bit for bit; every input must be unchanged, bit for bit; whatever a call must not read (rows of A
outside `range`, rows of B that row_index never names, columns behind n1 / n2 inside lda / ldb) holds NaN; a second launch gives the
same bits; comparisons are element-wise.

A. Contraction. out[i, j] = sum_r A[r, i] B[row(r), j], colsum[i] = sum_r w[row(r)] A[r, i]; bound tau(K) |A|^T |B| (tau of
   fp64_tools, K = rows actually summed), under `accumulate` plus 2^-23 (|previous| + |sum|). The shapes follow the branches of
   bwd_w_dims / bwd_w_partial_body / reduce_slabs_body; `bw_dims` below restates the host's decomposition ONLY to choose shapes and to
   assert that the intended branch is reached. One layout pin goes beyond the contract: bwd_w.h states that the waves of an empty
   half tile (wave_on) "do not multiply zeros or write them" -- the slab columns of those waves must keep the workspace's previous
   content (test_bw_idle_waves_leave_their_slab_columns_alone).
   Unreachable by the gate conditions: n1 / n2 / lda / ldb that are not multiples of 4 and a 9th problem are refused (asserted);
   colsum_weight exists in the batched descriptor only, so the weighted cases go through the batched call.

B. Adam on given gradients. Reference in float64 on the fp32 inputs, hyper-parameters = the float32 values widened:
       g' = g + wd p;  m' = m + (1 - b1)(g' - m);  v' = b2 v + (1 - b2) g'^2;  p' = p - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps)
   First-order forward bound, u = 2^-24, G = |g| + wd |p| (>= |g'|):
     * g' is one fma or a product and a sum: |dg'| <= 2 u G (absolute: g and wd p may cancel).
     * m': the lerp cancels, so absolute: dg' enters with (1 - b1); the subtraction, the product and the sum round once each on
       quantities <= |m| + G:  |dm'| <= CM u (|m| + G), CM = 4  (the count is 1 + 5 (1 - b1) <= 1.5 at b1 = 0.9).
     * v': both terms are non-negative, so relative: b2 v rounds once, g'^2 and its scaling twice, the sum once: <= 3 u v'; plus what
       dg' does to g'^2:  |dv'| <= CV u v' + 2 (1 - b2) |g'| 2 u G, CV = 4.
     * den = sqrt(v') r + eps with r = fl32(1 / sqrt(bc2)): sqrt halves dv' / v' and rounds, r is rounded, the product and the sum
       round: d den / den <= dv' / (2 v') + 4 u. The update U = s m' / den, s = fl32(lr / bc1): s, the division and the product round
       once each:  |dU| <= CU u |U| + s |dm'| / den + |U| dv' / (2 v'), CU = 8 (the count is 7).
     * p' = p - U rounds once:  |dp'| <= u |p'| + |dU|.
   The constants are held by the unmarked self-tests on the very inputs the GPU tests use: float32 torch arithmetic of the formula,
   with and without fused multiply-adds, is inside the bound on every element, and each of six mutants (wd dropped, bc2 inside the
   root at the wrong power, eps added before the division by sqrt(bc2), step off by one, m and v swapped, one element's update
   skipped) is outside on at least one.

C. Adam as the last hop's epilogue, in independent steps so that no tolerance absorbs a gradient error amplified by the optimizer:
   grad_out = the bits of slab.hop and inside 4e-6 (|A| |x| + |add|) + 1e-6 of float64; p / m / v = the bits of adam_step_out fed
   that gradient and inside B's bound; the same p / m / v bits without grad_out.
   Unreachable: the window sweep takes slabs of 16 or 32 floats only (sweep_launch refuses others), so the (8, 8) geometry has no
   swept form.
"""
import numpy as np
import pytest
import torch

from fp64_tools import NAN, TINY, all_nan, assert_close, same_bits, tau, within
from test_shard_gpu import _bipartite, _bitmap, _random_graph

DEV = "cuda:0"
gpu = pytest.mark.gpu
U24 = 2.0 ** -24
WORST = {}          # family -> worst err / tol seen in this session (printed by the last test)


def _note(family, err, tol):
    ok = tol > 0
    r = float((err[ok] / tol[ok]).max()) if bool(ok.any()) else 0.0
    WORST[family] = max(WORST.get(family, 0.0), r)


# ============================================================================= A. weight-gradient contraction
TN, TRB = 64, 32


def bw_dims(R, n1, n2):
    """chunk_rows, chunks, t1, t2 as bwd_w_dims cuts a problem (to choose shapes and to assert the branch; not a reference)."""
    t1, t2 = -(-n1 // TN), -(-n2 // TN)
    want = -(-(R * t1 * t2) // 480)
    want = -(-want // TRB) * TRB
    cr = min(max(want, 64), 512)
    return cr, max(-(-R // cr), 1), t1, t2


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def bw_case(R, n1, n2, pad=(0, 0, 0), index=None, rng=None, colsum=None, accumulate=False, b_rows=None, seed=0):
    """One contraction with its poison. index: None | 'perm' | 'hot'; rng: None | (lo, hi); colsum: None | 'plain' | 'weighted'."""
    g = torch.Generator().manual_seed(1000 * seed + R + 7 * n1 + 13 * n2)
    lo, hi = (0, R) if rng is None else rng
    rows = torch.arange(lo, hi) if hi > lo else torch.zeros(0, dtype=torch.int64)
    nb = max(R, 1) if index is None else max(b_rows or 0, R, 8)
    A = torch.full((max(R, 1), n1 + pad[0]), NAN)
    A[rows, :n1] = torch.randn(len(rows), n1, generator=g)
    idx = None
    if index == "perm":
        idx = torch.randperm(nb, generator=g)[:R].int()
    elif index == "hot":
        idx = torch.randint(0, nb, (R,), generator=g).int()
        idx[torch.rand(R, generator=g) < 0.7] = 3                        # one hot row
    named = rows if idx is None else idx[rows].long().unique()
    B = torch.full((nb, n2 + pad[1]), NAN)
    B[named, :n2] = torch.randn(len(named), n2, generator=g)
    c = dict(R=R, n1=n1, n2=n2, rows=rows, A=A.to(DEV), B=B.to(DEV), idx=None if idx is None else idx.to(DEV), colsum=colsum,
             accumulate=accumulate, rng=None if rng is None else torch.tensor([lo, hi], dtype=torch.int32, device=DEV))
    out = torch.full((n1, n2 + pad[2]), NAN)
    if accumulate:
        out[:, :n2] = torch.randn(n1, n2, generator=g)
    c["out0"] = out.to(DEV)
    if colsum:
        c["cs0"] = (torch.randn(n1, generator=g) if accumulate else torch.full((n1,), NAN)).to(DEV)
    if colsum == "weighted":
        w = torch.full((nb,), NAN)
        w[named] = torch.randn(len(named), generator=g)                   # mixed signs
        if len(named):
            w[named[0]] = 0.0                                             # a zero weight
        c["w"] = w.to(DEV)
    return c


def bw_problem(c):
    """Fresh outputs + the problem dict of ops.linear_bwd_w_batched."""
    c["out"] = c["out0"].clone()
    p = dict(A=c["A"][:, :c["n1"]], B=c["B"][:, :c["n2"]], out=c["out"][:, :c["n2"]], rows=c["R"], accumulate=c["accumulate"])
    if c["idx"] is not None:
        p["row_index"] = c["idx"]
    if c["rng"] is not None:
        p["rng"] = c["rng"]
    if c["colsum"]:
        c["cs"] = c["cs0"].clone()
        p["colsum"] = c["cs"]
    if c["colsum"] == "weighted":
        p["colsum_weight"] = c["w"]
    return p


def bw_check(c, what):
    """The outputs of one problem against float64, its padding and its inputs against what they were."""
    n1, n2, rows = c["n1"], c["n2"], c["rows"].to(DEV)
    K = float(len(rows))
    br = rows if c["idx"] is None else c["idx"][rows].long()
    A64, B64 = c["A"][rows, :n1].double(), c["B"][br, :n2].double()
    ref, sc = (A64.T @ B64).cpu(), (A64.abs().T @ B64.abs()).cpu()
    prev = c["out0"][:, :n2].double().cpu()
    if c["accumulate"]:
        sc = sc + 2.0 ** -23 * (prev.abs() + ref.abs()) / tau(K)
        ref = ref + prev
    got = c["out"][:, :n2]
    assert_close(got, ref, sc, K, what + " out")
    _note("contraction", (got.double().cpu() - ref).abs(), tau(K) * sc + TINY)
    if K == 0:
        assert same_bits(got, c["out0"][:, :n2]) if c["accumulate"] else bool((got == 0).all()), what + ": empty range"
    assert same_bits(c["out"][:, n2:], c["out0"][:, n2:]), what + ": columns behind n2 written"
    if c["colsum"]:
        wv = c["w"][br].double()[:, None] if c["colsum"] == "weighted" else torch.ones(len(rows), 1, dtype=torch.float64, device=DEV)
        cref, csc = (wv * A64).sum(0).cpu(), (wv.abs() * A64.abs()).sum(0).cpu()
        if c["accumulate"]:
            cprev = c["cs0"].double().cpu()
            csc = csc + 2.0 ** -23 * (cprev.abs() + cref.abs()) / tau(K)
            cref = cref + cprev
        assert_close(c["cs"], cref, csc, K, what + " colsum")
        _note("colsum", (c["cs"].double().cpu() - cref).abs(), tau(K) * csc + TINY)
        if K == 0:
            assert same_bits(c["cs"], c["cs0"]) if c["accumulate"] else bool((c["cs"] == 0).all()), what + ": empty range colsum"


def bw_workspace(cases, fill=0xFF):
    from elimrec_amd import ops
    n = ops.linear_bwd_w_batched_workspace([(c["R"], c["n1"], c["n2"]) for c in cases])
    return torch.full((n,), fill, dtype=torch.uint8, device=DEV)           # 0xFF bytes: NaN slabs


def bw_run(cases, what, single=False, wsp=None):
    """The plain call (single: elimrec_linear_bwd_w) on NaN outputs and a NaN workspace, checked; twice, same bits."""
    from elimrec_amd import ops
    keep = [(c["A"].clone(), c["B"].clone()) for c in cases]
    wsp = bw_workspace(cases) if wsp is None else wsp
    outs = []
    for rep in range(2):
        pr = [bw_problem(c) for c in cases]
        if single:
            p = pr[0]
            ops.linear_bwd_w(p["A"], p["B"], p["out"], wsp, row_index=p.get("row_index"), rng=p.get("rng"), colsum=p.get("colsum"),
                             accumulate=p["accumulate"], rows=p["rows"])
        else:
            ops.linear_bwd_w_batched(pr, wsp)
        outs.append([(c["out"].clone(), c["cs"].clone() if c["colsum"] else None) for c in cases])
    for k, c in enumerate(cases):
        bw_check(c, "%s[%d]" % (what, k))
        assert same_bits(c["A"], keep[k][0]) and same_bits(c["B"], keep[k][1]), what + ": an input changed"
        assert same_bits(outs[0][k][0], outs[1][k][0]), what + ": second launch differs"
        if c["colsum"]:
            assert same_bits(outs[0][k][1], outs[1][k][1]), what + ": second launch differs (colsum)"
    return wsp


# ----------------------------------------------------------------------------- the criterion has teeth (no GPU)
def test_bw_dims_reach_the_intended_branches():
    """The shapes the GPU cases rely on land where they are meant to: chunk_rows at both clamps and between, every chunk count."""
    assert bw_dims(64, 64, 64)[:2] == (64, 1) and bw_dims(65, 64, 64)[:2] == (64, 2) and bw_dims(0, 64, 64)[:2] == (64, 1)
    assert [bw_dims(R, 64, 64)[1] for R in _CHUNK_ROWS] == [1, 2, 3, 4, 5, 13, 16, 17, 20]
    assert all(bw_dims(R, n1, n2)[:2] == (cr, chunks) for R, n1, n2, cr, chunks in _CLAMPS)


def test_contraction_bound_rejects_a_dropped_chunk_and_an_unweighted_row():
    """The fp32 product torch computes on the CPU passes; one 64-row chunk left out, or one row's weight taken as 1, does not."""
    g = torch.Generator().manual_seed(5)
    R = 1000
    A, B, w = torch.randn(R, 64, generator=g), torch.randn(R, 68, generator=g), torch.randn(R, generator=g)
    A64, B64 = A.double(), B.double()
    ref, sc = A64.T @ B64, A64.abs().T @ B64.abs()
    assert within(A.T @ B, ref, sc, float(R)).all()
    assert not within(ref - A64[64:128].T @ B64[64:128], ref, sc, float(R)).all()
    cref, csc = (w.double()[:, None] * A64).sum(0), (w.double().abs()[:, None] * A64.abs()).sum(0)
    assert within((w[:, None] * A).sum(0), cref, csc, float(R)).all()
    assert not within(cref + (1 - w.double()[7]) * A64[7], cref, csc, float(R)).all()


# ----------------------------------------------------------------------------- A on the GPU
_CHUNK_ROWS = [64, 65, 150, 256, 257, 827, 1024, 1025, 1279]


@gpu
@pytest.mark.parametrize("R", [0, 1, 31, 32, 33] + _CHUNK_ROWS)
def test_bw_row_counts_and_chunk_counts(R):
    """n1 = n2 = 64 (chunk_rows at its 64 clamp): 0 .. 33 rows, exactly one chunk, one more, and every chunk count at the reduce's
    unroll edge (the c + 12 < chunks loop runs 0, 1 times; every residue mod 4), through the single and the batched call."""
    assert bw_dims(R, 64, 64)[0] == 64
    bw_run([bw_case(R, 64, 64, colsum="plain")], "R=%d" % R, single=True)
    bw_run([bw_case(R, 64, 64, pad=(4, 8, 12), index="perm", colsum="weighted", seed=1)], "R=%d batched" % R)


_CLAMPS = [(20000, 64, 256, 192, 105), (70000, 64, 256, 512, 137), (4100, 128, 128, 64, 65), (9000, 192, 2048, 512, 18),
           (128, 192, 8192, 128, 1), (129, 192, 8192, 128, 2), (512, 192, 10240, 512, 1), (513, 192, 10240, 512, 2)]


@gpu
@pytest.mark.parametrize("R,n1,n2,cr,chunks", _CLAMPS)
def test_bw_chunk_rows_at_the_clamps_and_between(R, n1, n2, cr, chunks):
    """chunk_rows strictly between the clamps, at 512 (the large count: the unrolled loop runs >= 2 times) and at 64; exactly
    chunk_rows and chunk_rows + 1 rows above the 64 clamp (chunk_rows follows R, so these need some 400 output tiles)."""
    assert bw_dims(R, n1, n2)[:2] == (cr, chunks)
    bw_run([bw_case(R, n1, n2, colsum="plain", pad=(0, 4, 0))], "R=%d" % R, single=True)


@gpu
@pytest.mark.parametrize("n1,n2,pad", [(4, 4, (0, 0, 0)), (4, 2048, (4, 0, 4)), (60, 32, (4, 4, 4)), (64, 36, (0, 4, 0)), (68, 68, (4, 4, 4)),
                                         (128, 128, (0, 0, 0)), (192, 4, (4, 0, 0)), (192, 2048, (0, 0, 0)), (64, 256, (8, 8, 8)),
                                         (68, 32, (0, 0, 0)), (128, 64, (0, 4, 0))])
def test_bw_widths(n1, n2, pad):
    """Every n1 of {4, 60, 64, 68, 128, 192} and n2 of {4, 32, 36, 64, 68, 128, 256, 2048} at least once and the corners together,
    lda / ldb / ldo padded and not; n2 = 32 / 4: the waves of the empty half tile are idle; one vector past a 64 tile."""
    for R, kw in ((200, dict(colsum="plain")), (700, dict(index="hot", colsum="weighted", rng=(37, 655), accumulate=True))):
        bw_run([bw_case(R, n1, n2, pad=pad, **kw)], "%dx%d R=%d" % (n1, n2, R))


@gpu
@pytest.mark.parametrize("n1,n2", [(64, 32), (64, 4), (64, 68), (128, 96), (64, 36)])
def test_bw_idle_waves_leave_their_slab_columns_alone(n1, n2):
    """The layout pin of the module docstring: in every slab of the workspace the 32-column halves that hold no output column keep
    the bytes the workspace held, the others are written for EVERY chunk the host counted (also beyond the device range)."""
    R = 300
    c = bw_case(R, n1, n2, rng=(10, 100), colsum="plain")
    wsp = bw_run([c], "idle", single=True)
    cr, chunks, t1, t2 = bw_dims(R, n1, n2)
    slabs = wsp[:chunks * t1 * TN * t2 * TN * 4].view(torch.float32).view(chunks, t1 * TN, t2 * TN)
    live = (torch.arange(t2 * TN, device=DEV) // 32) * 32 < n2
    assert bool((~live).any()) == (0 < n2 % 64 <= 32) and (cr, chunks) == (64, 5)
    assert all_nan(slabs[:, :, ~live]) and not bool(torch.isnan(slabs[:, :, live]).any())
    assert bool((slabs[2:, :, live] == 0).all())                        # chunks behind the device range hold exact zeros


@gpu
def test_bw_device_ranges():
    """range = [0, R), empty (lo == hi, lo > hi), a few rows of a large R (device chunks << host chunks), hi = R, bounds that are not
    multiples of 32, with row_index; the empty ones on a workspace an earlier, larger problem has just filled: exact zeros (the
    previous content under accumulate), not NaN, not stale slab content."""
    R = 5000
    big = bw_case(R, 64, 128, colsum="plain")
    wsp = bw_run([big], "fill")
    assert not bool(torch.isnan(wsp[:bw_dims(R, 64, 128)[1] * 64 * 128 * 4].view(torch.float32)).any())
    for rng in ((0, R), (777, 777), (900, 100), (R, R), (4321, 4330), (4989, R), (33, 4967), (0, 1)):
        for acc in (False, True):
            for index in (None, "hot"):
                c = bw_case(R, 64, 128, rng=rng, colsum="weighted" if index else "plain", accumulate=acc, index=index, seed=3)
                bw_run([c], "range %s acc=%s %s" % (rng, acc, index), wsp=wsp)


@gpu
@pytest.mark.parametrize("index", [None, "perm", "hot"])
@pytest.mark.parametrize("colsum", [None, "plain", "weighted"])
def test_bw_row_index_and_colsum_forms(index, colsum):
    """row_index absent / a permutation / one hot row x colsum absent / present / weighted (mixed signs, a zero weight, the weight
    read through row_index), with and without accumulate and a range, B taller than R."""
    for acc, rng in ((False, None), (True, None), (False, (65, 1900)), (True, (1, 64))):
        bw_run([bw_case(2000, 64, 68, pad=(4, 4, 4), index=index, colsum=colsum, accumulate=acc, rng=rng, b_rows=2600, seed=2)],
               "index=%s colsum=%s acc=%s rng=%s" % (index, colsum, acc, rng))


def _batch(n):
    """n problems of unequal shapes: the largest output LAST (max_out sizes the reduce grid), an empty range in the middle."""
    shapes = [(300, 64, 64), (1000, 4, 36), (2500, 68, 32), (40, 128, 64), (700, 64, 68), (0, 60, 4), (1279, 64, 128), (900, 192, 256)]
    pick = {1: [7], 2: [0, 7], 3: [0, 2, 7], 8: list(range(8))}[n]
    cases = []
    for k, i in enumerate(pick):
        R, n1, n2 = shapes[i]
        cases.append(bw_case(R, n1, n2, pad=(4 * (k % 2), 4 * (k % 3 == 0), 4 * (k % 2)), index=[None, "perm", "hot"][k % 3],
                             colsum=[None, "plain", "weighted"][(k + 1) % 3], accumulate=k % 4 == 1,
                             rng=(R // 2, R // 2) if (n >= 3 and k == n // 2) else (None if k % 2 else (R // 7, R - R // 9)), seed=10 + k))
    return cases


@gpu
@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_bw_batches(n):
    cases = _batch(n)
    assert cases[-1]["n1"] * cases[-1]["n2"] == max(c["n1"] * c["n2"] for c in cases)
    bw_run(cases, "batch of %d" % n)


@gpu
def test_bw_refusals_write_nothing():
    """A 9th problem, and widths / leading dimensions that are not multiples of 4: an error, and no output element written."""
    from elimrec_amd import ops
    cases = _batch(8) + [bw_case(100, 64, 64, seed=99)]
    pr = [bw_problem(c) for c in cases]
    wsp = torch.full((1 << 24,), 0xFF, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError):
        ops.linear_bwd_w_batched(pr, wsp)
    torch.cuda.synchronize()
    assert all(same_bits(c["out"], c["out0"]) for c in cases)
    c = bw_case(100, 64, 64)
    off = torch.randn(100 * 64 + 4, device=DEV)[1:1 + 6400].view(100, 64)
    for bad in (lambda p: p.update(out=c["out"][:, :62]), lambda p: p.update(out=c["out"][:62]),
                lambda p: p.update(A=torch.randn(100, 66, device=DEV)[:, :64]), lambda p: p.update(B=torch.randn(100, 70, device=DEV)[:, :64]),
                lambda p: p.update(A=off)):
        p = bw_problem(c)
        bad(p)
        with pytest.raises(RuntimeError):
            ops.linear_bwd_w_batched([p], wsp)
    torch.cuda.synchronize()
    assert same_bits(c["out"], c["out0"])


def _hop_setup(n, seed, d=64, w=32):
    from elimrec_amd import slab
    m = _random_graph(n, seed, hot=3, hot_deg=min(700, n // 2))
    ns = d // w
    gs = slab.choose_groups(ns)
    plan = slab.SellPlan(m, DEV, threshold=64, side_split=n // 3, tiered=True, ipw=64 // ((ns // gs) * (w // 4)))
    g = torch.Generator().manual_seed(seed)
    x = slab.SlabTable(n, ns, w, DEV).from_rows(torch.randn(n, d, generator=g).to(DEV))
    return plan, x, gs


@gpu
@pytest.mark.parametrize("shape", ["one-workgroup", "more-workgroups-than-tiles", "three-problems"])
def test_bw_every_way_to_run_the_two_phases_gives_the_plain_calls_bits(shape):
    """defer_reduce + linear_bwd_w_reduce; defer_reduce + hop(phase 1); defer_all + hops carrying phase 0 then phase 1 (masked and
    unmasked hop; the hop's own output = the hop without passengers); merge= (M = 0, 1, 3; padded keys; srcA / srcB / mask = those of
    slab.merge_rows): all give the bits of the plain batched call, which is itself checked against float64."""
    from elimrec_amd import ops, slab
    if shape == "one-workgroup":
        cases, n = [bw_case(50, 64, 64, colsum="plain", rng=(3, 47))], 3000
    elif shape == "more-workgroups-than-tiles":
        cases, n = [bw_case(20000, 64, 256, colsum="weighted", index="hot", b_rows=20000)], 300
    else:
        cases, n = _batch(3), 3000
    blocks = sum(np.prod(bw_dims(c["R"], c["n1"], c["n2"])[1:]) for c in cases)
    plan, x, gs = _hop_setup(n, 11)
    assert (blocks == 1) if shape == "one-workgroup" else (blocks > plan.n_tiles) == (shape == "more-workgroups-than-tiles")
    bw_run(cases, shape)
    ref = [(c["out"].clone(), c["cs"].clone() if c["colsum"] else None) for c in cases]

    def equal(what):
        for c, (o, cs) in zip(cases, ref):
            assert same_bits(c["out"], o) and (cs is None or same_bits(c["cs"], cs)), (shape, what)

    for masked in (True, False):
        bm = _bitmap(torch.rand(n, device=DEV) < 0.2) if masked else None
        y0, y1, z0, z1 = x.like(), x.like(), x.like(), x.like()
        slab.hop(plan, x, y0, gs=gs, src_mask=bm)
        slab.hop(plan, y0, y1, gs=gs)
        h = ops.linear_bwd_w_batched([bw_problem(c) for c in cases], bw_workspace(cases), defer_all=True)
        z0.data.fill_(NAN)
        z1.data.fill_(NAN)
        slab.hop(plan, x, z0, gs=gs, src_mask=bm, bwd_w=h, bwd_w_phase=0)
        slab.hop(plan, z0, z1, gs=gs, bwd_w=h, bwd_w_phase=1)
        assert same_bits(z0.data, y0.data) and same_bits(z1.data, y1.data)
        equal("defer_all masked=%s" % masked)
        h = ops.linear_bwd_w_batched([bw_problem(c) for c in cases], bw_workspace(cases), defer_reduce=True)
        z0.data.fill_(NAN)
        slab.hop(plan, x, z0, gs=gs, src_mask=bm, bwd_w=h, bwd_w_phase=1)
        assert same_bits(z0.data, y0.data)
        equal("defer_reduce + hop masked=%s" % masked)
    h = ops.linear_bwd_w_batched([bw_problem(c) for c in cases], bw_workspace(cases), defer_reduce=True)
    ops.linear_bwd_w_reduce(h)
    equal("defer_reduce + reduce")
    U, I, d, w = n // 3, n - n // 3, 64, 32
    for M in (0, 1, 3):
        keys = torch.sort(torch.randperm(n)[:n // 5])[0].int().to(DEV)
        keys = torch.cat([keys, torch.full((-len(keys) % 64 + 64,), -(1 << 30), dtype=torch.int32, device=DEV)])
        rows = torch.randn(len(keys), (M if M else 2) * d, device=DEV)
        sa, sb, ta, tb = (slab.SlabTable(n, d // w, w, DEV) for _ in range(4))
        for t in (sa, sb, ta, tb):
            t.data.zero_()
        mk1 = torch.full(((n + 31) // 32 + 2,), -1, dtype=torch.int32, device=DEV)
        mk2 = mk1.clone()
        slab.merge_rows(rows, keys, 1, U, I, sa, sb, mk1, M=M)
        ops.linear_bwd_w_batched([bw_problem(c) for c in cases], bw_workspace(cases),
                                 merge=dict(rows=rows, keys=keys, world=1, U=U, I=I, srcA=ta, srcB=tb, mask=mk2, M=M))
        assert same_bits(sa.data, ta.data) and same_bits(sb.data, tb.data) and torch.equal(mk1, mk2)
        equal("merge M=%d" % M)


# ============================================================================= B. Adam on given gradients
LR, B1, B2, EPS, WD = 1e-3, 0.9, 0.999, 1e-8, 1e-4       # conf/: lr, weight_decay; torch.optim.Adam's defaults
CM, CV, CU = 4.0, 4.0, 8.0
CONFIGS = [(st, step, wd) for st, step in (("zero", 1), ("step1", 2), ("long", 10), ("long", 1000), ("long", 100000)) for wd in (0.0, WD)]
f32 = lambda x: float(np.float32(x))


def adam_inputs(n, seed, state):
    """p ~ N(0, 0.1); g of magnitude 1e-12 .. 1e2 with exact zeros; moments all-zero / as after step 1 / as after ~1000 steps;
    element 1: g = m = v = 0 (denominator = eps), elements 2, 3: g' cancels m (with and without weight decay). float32 CPU."""
    g_ = torch.Generator().manual_seed(seed)
    mag = lambda: 10.0 ** (torch.rand(n, generator=g_) * 14 - 12) * (torch.randint(0, 2, (n,), generator=g_) * 2 - 1)
    p = torch.randn(n, generator=g_) * 0.1
    g = mag()
    g[torch.rand(n, generator=g_) < 0.1] = 0.0
    if state == "zero":
        m, v = torch.zeros(n), torch.zeros(n)
    elif state == "step1":
        g0 = mag()
        m, v = f32(1 - f32(B1)) * g0, f32(1 - f32(B2)) * g0 * g0
    else:
        s = mag().abs()
        m, v = s * torch.randn(n, generator=g_) * 0.3, s * s * (0.2 + 1.8 * torch.rand(n, generator=g_))
    if n > 4:
        g[1] = m[1] = v[1] = 0.0
        if state != "zero":
            m[2] = g[2]
            m[3] = g[3] + f32(WD) * p[3]
    return p.float(), g.float(), m.float(), v.float()


def adam_ref(p, g, m, v, step, wd, variant=None, skip=None):
    """float64 torch.optim.Adam with coupled L2 as include/elimrec_hip.h states it, and the bound of the module docstring.
    variant: one of the mutants of the self-test. Returns (p', m', v'), (tol_p, tol_m, tol_v)."""
    p, g, m, v = (t.double() for t in (p, g, m, v))
    lr, b1, b2, eps, wd = f32(LR), f32(B1), f32(B2), f32(EPS), f32(wd)
    if variant == "swap":
        m, v = v, m
    t = step + 1 if variant == "step+1" else step
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    gp = g + (0.0 if variant == "no-wd" else wd) * p
    m1 = m + (1 - b1) * (gp - m)
    v1 = b2 * v + (1 - b2) * gp * gp
    if variant == "bc2-power":
        den = torch.sqrt(v1 / (bc2 * bc2)) + eps
    elif variant == "eps-first":
        den = (torch.sqrt(v1) + eps) / np.sqrt(bc2)
    else:
        den = torch.sqrt(v1) / np.sqrt(bc2) + eps
    s = lr / bc1
    upd = s * m1 / den
    p1 = p - upd
    if skip is not None:
        p1[skip], m1[skip], v1[skip] = p[skip], m[skip], v[skip]
    G = g.abs() + wd * p.abs()
    tol_m = CM * U24 * (m.abs() + G)
    tol_v = CV * U24 * v1 + 4 * (1 - b2) * gp.abs() * U24 * G
    rel_v = torch.where(v1 > 0, tol_v / (2 * v1.clamp_min(1e-300)), torch.zeros_like(v1))
    tol_p = U24 * p1.abs() + CU * U24 * upd.abs() + s * tol_m / den + upd.abs() * rel_v
    return (p1, m1, v1), (tol_p + TINY, tol_m + TINY, tol_v + TINY)


def adam_f32(p, g, m, v, step, wd, fma):
    """The formula in float32 torch arithmetic on the CPU, with or without fused multiply-adds (an fma = the exact product and
    sum in float64 -- the product of two floats is exact there -- rounded to float32)."""
    F = torch.float32
    b1, b2 = f32(B1), f32(B2)
    s, r = f32(f32(LR) / (1.0 - b1 ** step)), f32(1.0 / np.sqrt(1.0 - b2 ** step))
    c1, c2, wd, eps = f32(1 - b1), f32(1 - b2), f32(wd), f32(EPS)
    fm = (lambda a, b, c: (a.double() * b.double() + c.double()).to(F)) if fma else (lambda a, b, c: a * b + c)
    t = lambda x: torch.full_like(p, float(x))
    gp = fm(t(wd), p, g)
    m1 = fm(t(c1), gp - m, m) if fma else m + c1 * (gp - m)
    v1 = fm(t(c2), gp * gp, b2 * v)
    den = fm(torch.sqrt(v1), t(r), t(eps))
    p1 = fm(t(-s), m1 / den, p) if fma else p - s * (m1 / den)
    return p1, m1, v1


def adam_inside(got, ref, tol):
    return [torch.isfinite(a.double()) & ((a.double() - b).abs() <= t) for a, b, t in zip(got, ref, tol)]


def adam_assert(got, inputs, step, wd, what, family="adam"):
    """got = (p', m', v') float32 (any device) against float64 Adam of `inputs` (float32, any device)."""
    got = [t.detach().cpu() for t in got]
    ref, tol = adam_ref(*[t.detach().cpu() for t in inputs], step, wd)
    for name, a, b, t in zip("pmv", got, ref, tol):
        ok = torch.isfinite(a) & ((a.double() - b).abs() <= t)
        _note("%s %s'" % (family, name), (a.double() - b).abs(), t)
        assert bool(ok.all()), "%s: %d of %d elements of %s' outside the bound, first %s" % (what, int((~ok).sum()), ok.numel(), name,
                                                                                           (~ok).nonzero()[:4].flatten().tolist())


ADAM_NS = [1, 255, 256, 257, 4096 * 256 - 1, 4096 * 256 + 1]


def _adam_configs(n):
    return CONFIGS if n <= 257 else [CONFIGS[3], CONFIGS[6]] if n % 2 else [CONFIGS[1], CONFIGS[8]]


@pytest.mark.parametrize("n", ADAM_NS)
def test_adam_bound_holds_fp32_arithmetic_and_rejects_the_mutants(n):
    """On the inputs the GPU tests use: float32 arithmetic with and without fma stays inside the bound on every element; over the
    configurations of this n every mutant leaves it on at least one element (n = 1 has one element: only the skipped update)."""
    caught = {k: False for k in ("no-wd", "bc2-power", "eps-first", "step+1", "swap", "skip")}
    for ci, (state, step, wd) in enumerate(_adam_configs(n)):
        x = adam_inputs(n, 100 * n + ci, state)
        ref, tol = adam_ref(*x, step, wd)
        for fma in (False, True):
            ok = adam_inside(adam_f32(*x, step, wd, fma), ref, tol)
            assert all(bool(o.all()) for o in ok), (state, step, wd, fma, [int((~o).sum()) for o in ok])
        k = int((ref[0] - x[0].double()).abs().argmax())
        for name in caught:
            if name == "no-wd" and wd == 0:
                continue
            mut = adam_ref(*x, step, wd, variant=name, skip=k if name == "skip" else None)[0]
            if name == "skip" and bool((ref[0][k] == x[0][k].double())):
                continue
            caught[name] |= not all(bool(o.all()) for o in adam_inside([t.float() for t in mut], ref, tol))
    want = ["skip"] if n == 1 else list(caught)
    assert all(caught[k] for k in want), caught


# ----------------------------------------------------------------------------- B on the GPU
GUARD = 64


def _guarded(t):
    """A device copy of a float32 CPU tensor inside NaN guards: (whole buffer, the view)."""
    buf = _nan(t.numel() + 2 * GUARD)
    buf[GUARD:GUARD + t.numel()] = t.to(DEV)
    return buf, buf[GUARD:GUARD + t.numel()]


def _guards_ok(buf):
    return all_nan(buf[:GUARD]) and all_nan(buf[-GUARD:])


@gpu
@pytest.mark.parametrize("n", ADAM_NS)
def test_adam_step_forms(n):
    """elimrec_adam_step, elimrec_adam_step_out aliased and with two buffers: inside the bound of float64 Adam, the same bits from
    all three, guards and inputs untouched, the grid-stride wrap beyond 4096 workgroups included."""
    from elimrec_amd import ops, slab
    for ci, (state, step, wd) in enumerate(_adam_configs(n)):
        x = adam_inputs(n, 100 * n + ci, state)
        hyper = (LR, B1, B2, EPS, wd, step)
        res = []
        for form in ("step", "out-aliased", "out-two", "out-two"):
            (bp, p), (bg, g), (bm, m), (bv, v) = (_guarded(t) for t in x)
            bo, po = _guarded(torch.full((n,), NAN))
            if form == "step":
                ops.adam_step(p, g, m, v, *hyper)
            elif form == "out-aliased":
                slab.adam_step_out(p, p, g, m, v, *hyper)
            else:
                slab.adam_step_out(p, po, g, m, v, *hyper)
                assert same_bits(p, x[0].to(DEV)), "p_in changed"
                p = po
            assert same_bits(g, x[1].to(DEV)) and all(_guards_ok(b) for b in (bp, bg, bm, bv, bo)), (form, n)
            assert form.startswith("out-two") or all_nan(po)
            res.append((p.clone(), m.clone(), v.clone()))
        adam_assert(res[0], x, step, wd, "adam_step n=%d %s" % (n, (state, step, wd)))
        for r in res[1:]:
            assert all(same_bits(a, b) for a, b in zip(r, res[0])), (n, state, step, wd)


def _jobs(spec, wd, seed):
    """spec: list of (n, kind, step), kind in 'update' | 'copy' | 'snapshot' | 'two' (update into a second buffer). The jobs' spans lie
    back to back in one buffer per role, four NaN floats between neighbours. Returns (AdamJob list, state for _jobs_check)."""
    from elimrec_amd import _lib
    total = sum(n + 4 for n, _, _ in spec) + 4
    bufs = {k: _nan(total) for k in ("p", "g", "m", "v", "out", "copy")}
    jobs, info, off = [], [], 4
    for k, (n, kind, step) in enumerate(spec):
        x = adam_inputs(n, seed + k, CONFIGS[2 * (k % 5)][0])
        sl = slice(off, off + n)
        for name, t in zip("pgmv", x):
            bufs[name][sl] = t.to(DEV)
        ptr = lambda name: bufs[name].data_ptr() + 4 * off
        upd, copy = kind != "copy", kind in ("copy", "snapshot")
        jobs.append(_lib.AdamJob(ptr("p"), (ptr("out") if kind == "two" else ptr("p")) if upd else None, ptr("g") if upd else None,
                                 ptr("m") if upd else None, ptr("v") if upd else None, ptr("copy") if copy else None, n, step if upd else 0))
        info.append((sl, kind, step, x))
        off += n + 4
    return jobs, dict(bufs=bufs, before={k: v.clone() for k, v in bufs.items()}, info=info, wd=wd)


def _jobs_check(st, what, family):
    """Every job against float64 Adam and against elimrec_adam_step_out's bits on the same inputs; everything outside the spans the
    jobs write (the guards, the other roles of copy-only jobs, jobs of length 0) as it was."""
    from elimrec_amd import slab
    want = {k: v.clone() for k, v in st["before"].items()}
    for sl, kind, step, x in st["info"]:
        if sl.stop == sl.start:
            continue
        if kind in ("copy", "snapshot"):
            want["copy"][sl] = x[0].to(DEV)
        if kind == "copy":
            continue
        p, g, m, v = (t.to(DEV).clone() for t in x)
        po = torch.empty_like(p)
        slab.adam_step_out(p, po, g, m, v, LR, B1, B2, EPS, st["wd"], step)
        want["out" if kind == "two" else "p"][sl], want["m"][sl], want["v"][sl] = po, m, v
        got = (st["bufs"]["out" if kind == "two" else "p"][sl], st["bufs"]["m"][sl], st["bufs"]["v"][sl])
        adam_assert(got, x, step, st["wd"], "%s job at %d (%s, step %d)" % (what, sl.start, kind, step), family)
    for k in want:
        assert same_bits(st["bufs"][k], want[k]), "%s: buffer '%s' differs from adam_step_out / was written outside a job" % (what, k)


JOB_SETS = {1: [(1, "update", 3)],
            3: [(257, "update", 1), (0, "update", 5), (256, "copy", 0)],
            8: [(1, "update", 1), (256, "snapshot", 2), (257, "two", 10), (0, "snapshot", 7), (1048577 + 3, "update", 1000),
                (300, "copy", 0), (255, "snapshot", 100000), (5, "two", 2)]}


@gpu
@pytest.mark.parametrize("n_jobs", [1, 3, 8])
@pytest.mark.parametrize("wd", [0.0, WD])
def test_adam_multi(n_jobs, wd):
    """elimrec_adam_multi: lengths 1 / 256 / 257 / 0 (skipped) / 1 048 580 (the grid-stride wrap inside a job), a copy-only job, jobs
    that snapshot their PRE-update parameters while updating in place, jobs writing a second buffer, a step per job."""
    from elimrec_amd import _lib, ops
    jobs, st = _jobs(JOB_SETS[n_jobs], wd, 7000 + n_jobs)
    arr = (_lib.AdamJob * len(jobs))(*jobs)
    _lib.check(_lib.load().elimrec_adam_multi(arr, len(jobs), LR, B1, B2, EPS, wd, ops._stream()), "adam_multi")
    _jobs_check(st, "adam_multi(%d)" % n_jobs, "adam_multi")


# ============================================================================= C. Adam as the last hop's epilogue
GEOMETRIES = [(64, 32), (32, 32), (16, 16), (8, 8), (128, 32), (256, 32)]
LOSS_NS = [0, 1, 1023, 1024, 1025, 5000]


def _tier_graph(ipw, seed):
    """_random_graph with rows of length 0, 1, T, T + 1, T1, T1 + 1, T2, T2 + 1 and T2 + 3000 (ticketed segments)."""
    T, T1, T2 = 64, (64 if ipw <= 8 else 32) * ipw, 256 * ipw
    n = T2 + 3000 + 1500
    lens = [0, 1, T, T + 1, T1, T1 + 1, T2, T2 + 1, T2 + 3000, 0, T1 - 7, T2 - 9]
    row_len = {11 + 97 * k: L for k, L in enumerate(lens)}
    m = _random_graph(n, seed, hot=4, hot_deg=300, row_len=row_len)
    deg = np.diff(m.indptr)
    assert all(deg[r] == L for r, L in row_len.items())
    return m, row_len, (T, T1, T2)


def _table(n, ns, w, t):
    """Slab-major flat device tensor [ns x n x w] -> row-major float64 CPU [n x ns*w]."""
    return t.view(ns, n, w).permute(1, 0, 2).reshape(n, ns * w).double().cpu()


@gpu
@pytest.mark.parametrize("variant", ["plain", "add", "masked-add"])
@pytest.mark.parametrize("d,w", GEOMETRIES)
def test_hop_adam_on_a_plan_of_every_tier(d, w, variant):
    from elimrec_amd import _lib, ops, slab
    ns = d // w
    gs = slab.choose_groups(ns)
    ipw = 64 // ((ns // gs) * (w // 4))
    gi, vi = GEOMETRIES.index((d, w)), ["plain", "add", "masked-add"].index(variant)
    m, row_len, (T, T1, T2) = _tier_graph(ipw, 40 + ipw)
    n = m.shape[0]
    plan = slab.SellPlan(m, DEV, threshold=T, side_split=n // 3, tiered=True, ipw=ipw)
    deg = np.diff(m.indptr)
    assert plan.n_w1 > 0 and plan.n_w4 > 0 and plan.n_seg > 0 and (deg == 0).sum() > 0 and plan.n_w1 == ((deg > T) & (deg <= T1)).sum() \
        and plan.n_w4 == ((deg > T1) & (deg <= T2)).sum() and plan.n_long - plan.n_w1 - plan.n_w4 == (deg > T2).sum() == 2
    gen = torch.Generator().manual_seed(d + w + vi)
    X = torch.randn(n, d, generator=gen)
    S = torch.randn(n, d, generator=gen)
    x = slab.SlabTable(n, ns, w, DEV).from_rows(X.to(DEV))
    add = slab.SlabTable(n, ns, w, DEV).from_rows(S.to(DEV)) if variant != "plain" else None
    flags = None
    if variant == "masked-add":
        flags = torch.rand(n, generator=gen) < 0.4
        empty, seg = [r for r, L in row_len.items() if L == 0], [r for r, L in row_len.items() if L > T2]
        flags[empty[0]], flags[empty[1]], flags[seg[0]], flags[seg[1]] = True, False, True, False
    bm = None if flags is None else _bitmap(flags.to(DEV))
    scale = [1.0, 0.25, 1.0 / 3][vi]
    pingpong = variant != "plain"
    state, step, wd = CONFIGS[(2 * gi + vi) % len(CONFIGS)]
    xin = adam_inputs(n * d, 31 * d + vi, state)
    # 1. the gradient: slab.hop's bits, float64's value
    y = x.like()
    y.data.fill_(NAN)
    slab.hop(plan, x, y, gs=gs, add=add, add_mask=bm, scale=scale)
    m64, X64 = m.astype(np.float64), X.double().numpy()
    Sm = np.zeros_like(X64) if add is None else S.double().numpy() * (1.0 if flags is None else flags.numpy()[:, None])
    want = torch.from_numpy((m64 @ X64 + Sm) * np.float64(np.float32(scale)))
    tol = 4e-6 * torch.from_numpy(abs(m64) @ np.abs(X64) + np.abs(Sm)) + 1e-6
    # the optimizer spans riding along, and the loss rows
    spec = {"plain": [], "add": JOB_SETS[1], "masked-add": JOB_SETS[8]}[variant]
    n_loss = LOSS_NS[(2 * gi + vi - 1) % 6] if variant != "plain" else None
    loss_buf = torch.randn(5008, generator=gen).to(DEV)
    runs = []
    for keep_grad in (True, False, False):
        p_in, mm, vv = (t.to(DEV).clone() for t in (xin[0], xin[2], xin[3]))
        p_out = _nan(n * d) if pingpong else p_in
        G = x.like()
        G.data.fill_(NAN)
        jobs, st = _jobs(spec, wd, 9000 + gi) if spec else ([], None)
        loss_out, loss_ref = _nan(3), _nan(3)
        loss = None if n_loss is None else (loss_buf[4:4 + n_loss], loss_out[1:2])
        part = plan.partials(ns, w)
        if n_loss == 0:         # (an empty tensor has no address: zero loss rows behind a real pointer go through the C entry)
            arr = (_lib.AdamJob * len(jobs))(*jobs) if jobs else None
            dp = lambda t: None if t is None else t.data_ptr()
            _lib.check(_lib.load().elimrec_slab_hop_adam(
                plan.ref(), ns, w, gs, x.data.data_ptr(), dp(G.data if keep_grad else None), dp(None if add is None else add.data), dp(bm),
                scale, part.data_ptr(), part.numel() * 4, p_in.data_ptr(), p_out.data_ptr(), mm.data_ptr(), vv.data_ptr(), LR, B1, B2, EPS,
                wd, step, arr, len(jobs), loss_buf.data_ptr() + 16, 0, loss_out.data_ptr() + 4, ops._stream()), "slab_hop_adam")
        else:
            slab.hop_adam(plan, x, G if keep_grad else None, gs, add, bm, scale, p_in, p_out, mm, vv, LR, B1, B2, EPS, wd, step,
                          tail_jobs=jobs, loss_sum=loss)
        if keep_grad:
            assert same_bits(G.data, y.data), "grad_out differs from slab.hop"
            got = _table(n, ns, w, G.data)
            err = (got - want).abs()
            _note("hop gradient", err, tol)
            assert bool((torch.isfinite(got) & (err <= tol)).all()), "grad_out outside 4e-6 (|A||x| + |add|) + 1e-6: %d elements" % int((err > tol).sum())
        else:
            assert all_nan(G.data)
        if pingpong:
            assert same_bits(p_in, xin[0].to(DEV)), "p_in changed"
        if st is not None:
            _jobs_check(st, "hop_adam tail", "hop_adam tail jobs")
        if loss is not None:
            _lib.check(_lib.load().elimrec_sum(loss_buf.data_ptr() + 16, n_loss, loss_ref.data_ptr() + 4, ops._stream()), "sum")
            assert same_bits(loss_out, loss_ref), "loss sum n=%d" % n_loss
        # the ticket counters behind the partial rows are back at zero
        t0 = -(-max(plan.n_seg, 1) * ns * w * 4 // 256) * 256 // 4
        assert bool((part[t0:t0 + 8 * max(plan.n_long, 1)].view(torch.int32) == 0).all()), "tickets not reset"
        runs.append((p_out.clone(), mm.clone(), vv.clone()))
    # 2. p / m / v: adam_step_out's bits on that gradient, float64 Adam's value
    p2, m2, v2 = (t.to(DEV).clone() for t in (xin[0], xin[2], xin[3]))
    po2 = torch.empty_like(p2)
    slab.adam_step_out(p2, po2, y.data, m2, v2, LR, B1, B2, EPS, wd, step)
    for r in runs:
        bad = [int((a.view(torch.int32) != b.view(torch.int32)).view(ns, n, w).any(2).any(0).sum()) for a, b in zip(r, (po2, m2, v2))]
        assert bad == [0, 0, 0], "rows of p / m / v that differ from adam_step_out: %s" % bad
    adam_assert(runs[0], (xin[0], y.data, xin[2], xin[3]), step, wd, "hop_adam %s" % ((d, w, variant),), "hop_adam")
    assert same_bits(x.data, slab.SlabTable(n, ns, w, DEV).from_rows(X.to(DEV)).data)


@gpu
@pytest.mark.parametrize("d,w,U,I,window", [(256, 32, 40000, 3000, 256), (64, 32, 700, 9000, 512), (16, 16, 3001, 6000, 700)])
def test_sweep_hop_adam_updates_every_row_exactly_once(d, w, U, I, window, monkeypatch):
    """SweepPlan.hop_adam for the user rows + the tile launch for the item rows: U not a multiple of the block rows, a window that
    does not divide the item range, more than one pass (U = 40 000 at 8 slabs of 32 floats: one row part, 32 blocks of <= 1247 rows
    per pass; at 16-float pieces 40 000 rows are ONE pass of 256 blocks of <= 2495 rows). From all-distinct m, every element of m
    changes exactly as ONE update predicts (adam_step_out's bits on the hop's gradient): no row updated twice or not at all."""
    from elimrec_amd import slab
    monkeypatch.setenv("ELIMREC_SWEEP_WINDOW", str(window))
    n, ns = U + I, d // w
    m = _bipartite(U, I, d + w)
    gs = slab.choose_groups(ns)
    ipw = 64 // ((ns // gs) * (w // 4))
    plan = slab.SellPlan(m, DEV, threshold=64, side_split=U, tiered=True, ipw=ipw)
    plan.sweep = slab.SweepPlan(plan, m, U, DEV, threshold=64, ipw=ipw)
    geo = plan.sweep.geometry(ns, w)
    blk = np.diff(geo["block_ptr"].cpu().numpy())
    assert I % window != 0 and blk.min() != blk.max() and (geo["passes"] > 1) == (U == 40000) and (np.diff(m.indptr[:U + 1]) == 0).any()
    gen = torch.Generator().manual_seed(U)
    X, S = torch.randn(n, d, generator=gen), torch.randn(n, d, generator=gen)
    x = slab.SlabTable(n, ns, w, DEV).from_rows(X.to(DEV))
    add = slab.SlabTable(n, ns, w, DEV).from_rows(S.to(DEV))
    flags = torch.rand(n, generator=gen) < 0.3
    bm, scale = _bitmap(flags.to(DEV)), 0.25
    state, step, wd = CONFIGS[7]
    xin = list(adam_inputs(n * d, U + d, state))
    xin[2] = 100.0 + torch.arange(n * d, dtype=torch.float32) / 1024          # all distinct, far from any g'
    assert len(torch.unique(xin[2])) == n * d
    y = x.like()
    y.data.fill_(NAN)
    slab.hop(plan, x, y, gs=gs, add=add, add_mask=bm, scale=scale)
    m64, X64 = m.astype(np.float64), X.double().numpy()
    Sm = S.double().numpy() * flags.numpy()[:, None]
    want = torch.from_numpy((m64 @ X64 + Sm) * scale)
    tol = 4e-6 * torch.from_numpy(abs(m64) @ np.abs(X64) + np.abs(Sm)) + 1e-6
    p2, m2, v2 = (t.to(DEV).clone() for t in (xin[0], xin[2], xin[3]))
    po2 = torch.empty_like(p2)
    slab.adam_step_out(p2, po2, y.data, m2, v2, LR, B1, B2, EPS, wd, step)
    assert bool((m2 != xin[2].to(DEV)).all())
    for keep_grad in (True, False):
        p_in, mm, vv = (t.to(DEV).clone() for t in (xin[0], xin[2], xin[3]))
        p_out, G = _nan(n * d), x.like()
        G.data.fill_(NAN)
        slab.hop_adam(plan, x, G if keep_grad else None, gs, add, bm, scale, p_in, p_out, mm, vv, LR, B1, B2, EPS, wd, step)
        if keep_grad:
            assert same_bits(G.data, y.data)
            got = _table(n, ns, w, G.data)
            _note("sweep gradient", (got - want).abs(), tol)
            assert bool((torch.isfinite(got) & ((got - want).abs() <= tol)).all())
        else:
            assert all_nan(G.data)
        changed = (mm != xin[2].to(DEV)).view(ns, n, w)
        assert bool(changed.all()), "%d rows not updated" % int((~changed).any(2).any(0).sum())
        assert same_bits(mm, m2) and same_bits(vv, v2) and same_bits(p_out, po2) and same_bits(p_in, xin[0].to(DEV))
    adam_assert((p_out, mm, vv), (xin[0], y.data, xin[2], xin[3]), step, wd, "sweep hop_adam", "sweep hop_adam")


@gpu
def test_zz_report_the_worst_ratios():
    """Prints the worst err / tol per family of this session (pytest -s shows it; the figures of the commit message)."""
    print("\nworst err / tol: " + ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))
    assert all(v <= 1.0 for v in WORST.values())
