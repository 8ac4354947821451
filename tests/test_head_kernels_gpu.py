"""The training step's head kernels against plain float64 math at their edge shapes: the fused head forward (csrc/head.hip:
head_fwd16_kernel, head_rows_fwd16_kernel), the head input gradient (csrc/bpr.hip: head_bwd_input_kernel,
head_bwd_input_mfma_kernel, head_bwd_input16_kernel) and the BPR loss head over compact rows (bpr_head_kernel,
bpr_head_sum_kernel). The references below never call a project kernel; every output buffer starts as NaN, so a row or
column a call must not write is seen to stay untouched. The tolerance self-tests at the top run without a GPU."""
import types

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from fp64_tools import NAN, all_nan, assert_close, same_bits, tau, within

DEV = "cuda:0"
F = torch.nn.functional
HD = 64                  # the fused head's recdim


# ----------------------------------------------------------------------------- float64 references
def ref_head_fwd(act, n_lo, out0, narrow, c, S, Wm, bm, Wf, bf, Ws, bs):
    """The fused head at active rows r < len(act), node n = act[r], side user when r < n_lo:
        Out_m = S_m[n] W_m^T + c[n] b_m + narrow[r]     (the m_dense projections through the graph, models/EliMRec.py:243-252,
                                                          in the folded form: S_m, c are the propagated constants)
        Out   = [out0[r] | Out_1 .. Out_M]               (mm_fusion "concat", :221-225)
        Y_0   = Out Wf_side^T + bf_side                  (embedding_{user,item}_after_GCN, :262-270)
        Y_m   = Out_m Ws_m^T + bs_m                      (s_dense_m, :146-151)
    Arguments are float64 CPU tensors (None: no bias). Returns Out, Y, their magnitudes and the reduction lengths per column."""
    n = len(act)
    user = torch.arange(n) < n_lo
    cr = c[act][:, None]
    blocks, sblocks, kout = [out0], [out0.abs()], [torch.zeros(HD, dtype=torch.float64)]
    for m in range(len(S)):
        s = S[m][act]
        o = s @ Wm[m].T + narrow
        so = s.abs() @ Wm[m].abs().T + narrow.abs()
        if bm[m] is not None:
            o, so = o + cr * bm[m], so + cr.abs() * bm[m].abs()
        blocks.append(o)
        sblocks.append(so)
        kout.append(torch.full((HD,), S[m].shape[1] + 3.0, dtype=torch.float64))
    Out, sOut = torch.cat(blocks, 1), torch.cat(sblocks, 1)
    side = [(Wf[0], bf[0]), (Wf[1], bf[1])]
    ys = []
    for W, b in side:
        y, sy = Out @ W.T, sOut @ W.abs().T           # |Out| <= sOut: the first stage's error carried through the second
        if b is not None:
            y, sy = y + b, sy + b.abs()
        ys.append((y, sy))
    Y0 = torch.where(user[:, None], ys[0][0], ys[1][0])
    sY0 = torch.where(user[:, None], ys[0][1], ys[1][1])
    yb, syb = [Y0], [sY0]
    ky = [torch.full((HD,), Out.shape[1] + max(t.shape[1] for t in S) + 4.0, dtype=torch.float64)]
    for m in range(len(S)):
        o, so = blocks[1 + m], sblocks[1 + m]
        y, sy = o @ Ws[m].T, so @ Ws[m].abs().T
        if bs[m] is not None:
            y, sy = y + bs[m], sy + bs[m].abs()
        yb.append(y)
        syb.append(sy)
        ky.append(torch.full((HD,), HD + S[m].shape[1] + 4.0, dtype=torch.float64))
    return dict(Out=Out, sOut=sOut, KOut=torch.cat(kout)[None, :], Y=torch.cat(yb, 1), sY=torch.cat(syb, 1),
                KY=torch.cat(ky)[None, :])


def ref_head_bwd(dY, dYabs, nodes, U, d, C, mblock, Wu, Wi, Wh, gscale, Kin=0):
    """The head's input gradient at the active rows (the backward of ref_head_fwd's second stage, models/EliMRec.py:262-270
    and :146-151 under autograd, main.py:99-100):
        dOut[r] = gscale * (dY_0[r] W_side(r) + sum_h place(mblock[h], dY_h[r] Ws_h))
    side(r) = user when nodes[r] < U. dYabs: a bound on |dY| (the segment sums' magnitudes); Kin: the reduction length that
    formed dY (per row). float64 CPU tensors; returns dOut, its magnitude and the reduction length per element."""
    user = (nodes < U)[:, None]
    y0, a0 = dY[:, :d], dYabs[:, :d]
    out = torch.where(user, y0 @ Wu, y0 @ Wi)
    sc = torch.where(user, a0 @ Wu.abs(), a0 @ Wi.abs())
    kb = torch.full((C // d,), float(d))
    for h, mb in enumerate(mblock):
        blk, src = slice(mb * d, (mb + 1) * d), slice((1 + h) * d, (2 + h) * d)
        out[:, blk] += dY[:, src] @ Wh[h]
        sc[:, blk] += dYabs[:, src] @ Wh[h].abs()
        kb[mb] += d
    K = kb.repeat_interleave(d)[None, :] + (Kin if torch.is_tensor(Kin) else torch.tensor(float(Kin)))
    return gscale * out, abs(gscale) * sc, K


def ref_bpr_rows(Y, slot_rows, d, w):
    """The cosine-BPR loss of models/EliMRec.py:291-297 and :129-142 (fusion block + alpha-weighted single-modal blocks), read
    through slot_rows (slot 3b+j of triplet b is row slot_rows[3b+j] of Y), by float64 autograd: per-triplet loss rows
    sum_k w_k softplus(<a,n> - <a,p>)_k / B and the gradient of the batch loss with respect to each slot's row. Also returns
    the magnitudes the element-wise bound scales with."""
    B = len(slot_rows) // 3
    G = Y.double()[slot_rows].clone().requires_grad_(True)
    rows = G.view(B, 3, -1)
    loss_rows = torch.zeros(B, dtype=torch.float64)
    sl = torch.zeros(B, dtype=torch.float64)
    sg = torch.zeros(B, 3, Y.shape[1], dtype=torch.float64)
    for k, wk in enumerate(w):
        blk = rows[:, :, k * d:(k + 1) * d]
        a, p, n = (F.normalize(blk[:, j], dim=1) for j in range(3))
        x = (a * n).sum(1) - (a * p).sum(1)
        loss_rows = loss_rows + wk * F.softplus(x) / B
        with torch.no_grad():
            norms = blk.norm(dim=2).clamp_min(1e-12)
            ah, ph, nh = a.abs(), p.abs(), n.abs()
            g = abs(wk) * torch.sigmoid(x)[:, None] / B
            xx = x.abs()[:, None] + 1
            sl += abs(wk) * (2 + F.softplus(x)) / B
            sg[:, 0, k * d:(k + 1) * d] = g * (nh + ph + ah * xx) / norms[:, 0:1]
            sg[:, 1, k * d:(k + 1) * d] = g * (ah + ph * 2) / norms[:, 1:2]
            sg[:, 2, k * d:(k + 1) * d] = g * (ah + nh * 2) / norms[:, 2:3]
    loss_rows.sum().backward()
    return loss_rows.detach(), G.grad.view(3 * B, -1), sl, sg.view(3 * B, -1)


# ----------------------------------------------------------------------------- the criterion has teeth (no GPU)
@pytest.mark.parametrize("K", [64, 1024])
def test_tolerance_rejects_one_dropped_term_swapped_rows_and_bf16_operands(K):
    """On random operands the exact fp32 product torch computes on the CPU passes the bound; dropping one k term, swapping two
    output rows or rounding the operands through bf16 does not."""
    g = torch.Generator().manual_seed(K)
    A, B = torch.randn(48, K, generator=g), torch.randn(K, 40, generator=g)
    Ad, Bd = A.double(), B.double()
    ref, sc = Ad @ Bd, Ad.abs() @ Bd.abs()
    assert within(A @ B, ref, sc, K).all()
    assert not within(ref - Ad[:, K // 3:K // 3 + 1] @ Bd[K // 3:K // 3 + 1], ref, sc, K).all()
    perm = list(range(48))
    perm[5], perm[6] = 6, 5
    assert not within(ref[perm], ref, sc, K).all()
    assert not within(A.bfloat16().double() @ B.bfloat16().double(), ref, sc, K).all()


def _cpu_head_case(seed=0, dims=(60, 8), n=40, n_lo=23):
    g = torch.Generator().manual_seed(seed)
    N = 90
    C = (1 + len(dims)) * HD
    S = [torch.randn(N, D, generator=g) for D in dims]
    t = dict(act=torch.randperm(N, generator=g)[:n], n_lo=n_lo, out0=torch.randn(n, HD, generator=g),
             narrow=torch.randn(n, HD, generator=g), c=torch.randn(N, generator=g), S=S,
             Wm=[torch.randn(HD, D, generator=g) / D ** 0.5 for D in dims], bm=[torch.randn(HD, generator=g) for _ in dims],
             Wf=[torch.randn(HD, C, generator=g) / C ** 0.5 for _ in range(2)], bf=[torch.randn(HD, generator=g) for _ in range(2)],
             Ws=[torch.randn(HD, HD, generator=g) / 8 for _ in dims], bs=[torch.randn(HD, generator=g) for _ in dims])
    return t


def _dbl(t):
    out = {}
    for k, v in t.items():
        if torch.is_tensor(v):
            out[k] = v if v.dtype == torch.int64 else v.double()
        elif isinstance(v, list):
            out[k] = [None if x is None else x.double() for x in v]
        else:
            out[k] = v
    return out


def test_tolerance_on_the_head_forward_rejects_wrong_side_and_missing_bias():
    """The same criterion on the head forward's reference: the fp32 forward torch computes on the CPU passes; W_user applied
    to one item row, or one bias left out, is rejected."""
    t = _cpu_head_case()
    r = ref_head_fwd(**_dbl(t))
    # fp32 on the CPU, the same formula
    n, n_lo = len(t["act"]), t["n_lo"]
    out = [t["out0"]] + [t["S"][m][t["act"]] @ t["Wm"][m].T + t["c"][t["act"]][:, None] * t["bm"][m] + t["narrow"]
                         for m in range(len(t["S"]))]
    Out = torch.cat(out, 1)
    user = (torch.arange(n) < n_lo)[:, None]
    Y0 = torch.where(user, Out @ t["Wf"][0].T + t["bf"][0], Out @ t["Wf"][1].T + t["bf"][1])
    Y = torch.cat([Y0] + [out[1 + m] @ t["Ws"][m].T + t["bs"][m] for m in range(len(t["S"]))], 1)
    assert within(Out, r["Out"], r["sOut"], r["KOut"]).all() and within(Y, r["Y"], r["sY"], r["KY"]).all()
    wrong = Y.clone()
    wrong[n_lo + 3, :HD] = Out[n_lo + 3] @ t["Wf"][0].T + t["bf"][0]       # W_user on an item row
    assert not within(wrong, r["Y"], r["sY"], r["KY"]).all()
    nob = dict(t)
    nob["bm"] = [None] + t["bm"][1:]
    r2 = ref_head_fwd(**_dbl(nob))
    assert not within(Out, r2["Out"], r2["sOut"], r2["KOut"]).all()
    nob = dict(t)
    nob["bs"] = t["bs"][:1] + [None]
    r3 = ref_head_fwd(**_dbl(nob))
    assert not within(Y, r3["Y"], r3["sY"], r3["KY"]).all()


# ----------------------------------------------------------------------------- 1. fused head forward
def _node_ids(g, U, N, n_lo, n_hi):
    """n_lo user ids in [0, U) and n_hi item ids in [U, N), sorted, the top id of each side included."""
    us = torch.randperm(U - 1, generator=g)[:max(n_lo - 1, 0)].sort()[0].tolist() + ([U - 1] if n_lo else [])
    it = (U + torch.randperm(N - U - 1, generator=g)[:max(n_hi - 1, 0)]).sort()[0].tolist() + ([N - 1] if n_hi else [])
    return us + it


def _fwd_case(dims, R, n_act, n_lo, bias="all", seed=0, N=300, pad=4):
    g = torch.Generator().manual_seed(seed)
    U = N // 2
    C = (1 + len(dims)) * HD
    nodes = _node_ids(g, U, N, n_lo, n_act - n_lo)
    act = torch.tensor(nodes + [0] * (R - n_act), dtype=torch.int32)           # valid ids in the unused tail too
    full = [torch.randn(N, D + pad, generator=g) for D in dims]                # row stride D + pad: ldS > D
    S = [f[:, :D] for f, D in zip(full, dims)]
    t = dict(act=act, seg=torch.tensor([n_act, n_lo, 0, 0, 0, 0, 0, 0], dtype=torch.int32),
             out0=torch.randn(R, HD, generator=g), narrow=torch.randn(R, HD, generator=g), c=torch.randn(N, generator=g),
             full=full, S=S, Wm=[torch.randn(HD, D, generator=g) / D ** 0.5 for D in dims],
             bm=[torch.randn(HD, generator=g) for _ in dims], Wf=[torch.randn(HD, C, generator=g) / C ** 0.5 for _ in range(2)],
             bf=[torch.randn(HD, generator=g) for _ in range(2)], Ws=[torch.randn(HD, HD, generator=g) / 8 for _ in dims],
             bs=[torch.randn(HD, generator=g) for _ in dims], n_act=n_act, n_lo=n_lo, R=R, C=C, dims=list(dims))
    t["out0"][n_act:] = NAN
    t["narrow"][n_act:] = NAN
    if bias == "none":
        t["bm"], t["bf"], t["bs"] = [None] * len(dims), [None, None], [None] * len(dims)
    elif bias == "mixed":
        t["bm"] = [None] + t["bm"][1:]
        t["bf"] = [t["bf"][0], None]
        t["bs"] = t["bs"][:-1] + [None]
    return t


def _ref_of(t, S=None, c=None):
    a = t["act"][:t["n_act"]].long()
    S = t["S"] if S is None else S
    c = t["c"] if c is None else c
    d = lambda x: None if x is None else x.double()
    return ref_head_fwd(a, t["n_lo"], t["out0"][:t["n_act"]].double(), t["narrow"][:t["n_act"]].double(), c.double(),
                        [s.double() for s in S], [w.double() for w in t["Wm"]], [d(b) for b in t["bm"]],
                        [w.double() for w in t["Wf"]], [d(b) for b in t["bf"]], [w.double() for w in t["Ws"]], [d(b) for b in t["bs"]])


def _to_dev(t):
    o = {}
    for k, v in t.items():
        if torch.is_tensor(v):
            o[k] = v.to(DEV)
        elif isinstance(v, list) and v and (v[0] is None or torch.is_tensor(v[0])):
            o[k] = [None if x is None else x.to(DEV) for x in v]
        else:
            o[k] = v
    # the strided S views: views of the padded tables on the device
    o["S"] = [f[:, :D] for f, D in zip(o["full"], t["dims"])]
    return o


def _bufs(R, C):
    """OutAct / YAct as [R x C] views of [R x (C + 4)] NaN buffers: the 4 columns past C must stay NaN."""
    ob, yb = torch.full((R, C + 4), NAN, device=DEV), torch.full((R, C + 4), NAN, device=DEV)
    return ob, yb


def _fwd_call(o, pack, ob, yb, phase, form="plain", peers=None, src16=None):
    from elimrec_amd import ops
    C = o["C"]
    args = (o["Wm"], o["bm"], o["Wf"][0], o["bf"][0], o["Wf"][1], o["bf"][1], o["Ws"], o["bs"], pack, ob[:, :C], yb[:, :C], HD)
    if form == "src16":
        fs, S_out, c_out = src16
        return ops.head_fwd_fused_src16(fs, S_out, c_out, o["act"], o["seg"], o["out0"], o["narrow"], *args, phase=phase)
    return ops.head_fwd_fused(o["act"], o["seg"], o["out0"], o["narrow"], o["c"], o["S"], *args, phase=phase,
                              peers=peers if phase in (0, 2, 4) else None)


def _run_fwd(o, phases, **kw):
    """One pass of the head over fresh NaN buffers; between the launches of a split head, what the earlier ones may and may
    not have written is checked."""
    from elimrec_amd import ops
    R, C, n = o["R"], o["C"], o["n_act"]
    pack = torch.full((ops.head_pack_floats(o["dims"]),), NAN, device=DEV)
    ob, yb = _bufs(R, C)
    mid = None
    for ph in phases:
        assert _fwd_call(o, pack, ob, yb, ph, **kw)
        torch.cuda.synchronize()
        if ph == 1:
            assert not torch.isnan(pack).any() and all_nan(ob) and all_nan(yb)       # pack only
        if ph == 3:
            assert all_nan(yb) and all_nan(ob[:, :HD]) and all_nan(ob[n:]) and all_nan(ob[:, C:])
            mid = ob[:n, HD:C].clone()                  # the feature blocks without the shared part
    return ob, yb, pack, mid


def _check_fwd(t, ob, yb, mid=None, ref=None):
    n, C = t["n_act"], t["C"]
    r = _ref_of(t) if ref is None else ref
    assert same_bits(ob[:n, :HD].cpu(), t["out0"][:n])                         # block 0: a copy
    assert_close(ob[:n, :C], r["Out"], r["sOut"], r["KOut"], "OutAct")
    assert_close(yb[:n, :C], r["Y"], r["sY"], r["KY"], "YAct")
    assert all_nan(ob[n:]) and all_nan(yb[n:]) and all_nan(ob[:, C:]) and all_nan(yb[:, C:])
    if mid is not None:
        nar = t["narrow"][:n].double().repeat(1, len(t["dims"]))
        assert_close(mid, r["Out"][:, HD:] - nar, r["sOut"][:, HD:], r["KOut"][:, HD:], "OutAct after phase 3")


FWD_CASES = [
    # dims, R, n_act, n_lo, bias, phases
    ((4,), 20, 17, 16, "all", (0,)),                      # K/4 = 1; n_lo % 16 = 0, an item side of 1
    ((8, 60), 40, 33, 1, "none", (1, 2)),                 # n_lo % 16 = 1; K/4 = 2, 15
    ((64, 68, 124), 48, 47, 15, "all", (1, 3, 4)),        # n_lo % 16 = 15; K/4 = 16, 17, 31 (prefetch + tails)
    ((132,), 16, 16, 16, "mixed", (0,)),                  # every row a user (item side 0); K/4 = 33
    ((256, 4), 17, 17, 0, "all", (1, 3, 4)),              # every row an item
    ((1024,), 40, 1, 1, "all", (0,)),                     # one active row, R > n_act; K/4 = 256, C/4 = 32
    ((60, 256, 8), 80, 65, 48, "mixed", (1, 2)),          # three tables; an item side of 17
    ((124, 132), 64, 31, 31, "none", (1, 3, 4)),          # users only, R = 2 n_act
    ((2324,), 24, 20, 9, "all", (0,)),                    # the widest table one table allows at phase 0 (see below)
]


@pytest.mark.gpu
@pytest.mark.parametrize("dims,R,n_act,n_lo,bias,phases", FWD_CASES)
def test_fused_head_forward_vs_fp64(dims, R, n_act, n_lo, bias, phases):
    """elimrec_head_fwd_fused, head_fwd16_kernel: OutAct and YAct at every active row element by element against ref_head_fwd,
    nothing written past n_act or past C, phase 3's feature blocks, and the same bits from a second pass."""
    t = _fwd_case(dims, R, n_act, n_lo, bias, seed=len(dims) * 100 + n_act)
    o = _to_dev(t)
    ob, yb, pack, mid = _run_fwd(o, phases)
    _check_fwd(t, ob, yb, mid)
    ob2, yb2, pack2, _ = _run_fwd(o, phases)
    assert same_bits(ob[:n_act], ob2[:n_act]) and same_bits(yb[:n_act], yb2[:n_act]) and same_bits(pack, pack2)


@pytest.mark.gpu
def test_fused_head_forward_refuses_one_step_past_the_lds_limit():
    """Phase 0 stages the narrow tile, the feature tiles and the Out tile: 16 (64 + 4) + 16 (D + 4) + 16 (C + 4) floats <=
    158 KiB, i.e. D <= 2324 for one table (FWD_CASES runs it). D = 2328 returns False and writes nothing, the pack included."""
    from elimrec_amd import ops
    assert 4 * (16 * 68 + 16 * (2324 + 4) + 16 * (128 + 4)) <= 158 * 1024 < 4 * (16 * 68 + 16 * (2328 + 4) + 16 * (128 + 4))
    t = _fwd_case((2328,), 16, 5, 2, seed=1)
    o = _to_dev(t)
    pack = torch.full((ops.head_pack_floats([2328]),), NAN, device=DEV)
    ob, yb = _bufs(16, o["C"])
    assert _fwd_call(o, pack, ob, yb, 0) is False
    torch.cuda.synchronize()
    assert all_nan(pack) and all_nan(ob) and all_nan(yb)


def _src16_table(t, dtype, seed):
    """The 16-bit rows the head reads in place (lookup.FeatureShard's layout, lookup.py:76-79): [S_1 | .. | S_n | c_hi c_lo |
    pad], row length a multiple of 8 elements. Values span the fp16 range: near its top and subnormal."""
    g = torch.Generator().manual_seed(seed)
    tdt = torch.float16 if dtype == "f16" else torch.bfloat16
    N, dims = t["c"].shape[0], t["dims"]
    sum_d = sum(dims)
    row_elems = ((sum_d + 2) * 2 + 15) // 16 * 16 // 2
    tab = torch.zeros(N, row_elems, dtype=tdt)
    off = 0
    for m, D in enumerate(dims):
        v = torch.randn(N, D, generator=g)
        big = torch.rand(N, D, generator=g) < 0.05
        tiny = torch.rand(N, D, generator=g) < 0.05
        v[big] = torch.sign(v[big]) * (6.0e4 + 5.0e3 * torch.rand(int(big.sum()), generator=g))
        v[tiny] = v[tiny] * 3e-7                                       # fp16 subnormals (below 6.1e-5)
        tab[:, off:off + D] = v.to(tdt)
        off += D
    c = torch.randn(N, generator=g) * 3
    hi = c.to(tdt)
    tab[:, off] = hi
    tab[:, off + 1] = (c - hi.float()).to(tdt)
    S_w = [tab[:, o:o + D].float() for o, D in zip(np.cumsum([0] + dims[:-1]).tolist(), dims)]
    c_w = tab[:, off].float() + tab[:, off + 1].float()                 # c = fp32(hi) + fp32(lo), one fp32 addition
    fs = types.SimpleNamespace(dims=list(dims), sum_d=sum_d, table=tab.to(DEV), row_elems=row_elems,
                               code=1 if dtype == "f16" else 2)
    return fs, S_w, c_w


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,dims,R,n_act,n_lo,phases", [
    ("f16", (8, 60), 40, 33, 17, (0,)),
    ("bf16", (64, 124, 4), 48, 45, 30, (1, 3, 4)),
    ("f16", (132,), 20, 16, 0, (1, 3, 4)),
    ("bf16", (4,), 24, 1, 1, (0,)),
])
def test_fused_head_forward_on_16bit_constants(dtype, dims, R, n_act, n_lo, phases):
    """elimrec_head_fwd_fused (16-bit source form): S_out / c_out are the exactly widened rows of the active nodes (c = fp32(hi) + fp32(lo)),
    OutAct / YAct meet the fp64 reference of the widened values, and have the bits of the plain head on the widened tables."""
    from elimrec_amd import ops
    t = _fwd_case(dims, R, n_act, n_lo, "all", seed=7 + n_act)
    fs, S_w, c_w = _src16_table(t, dtype, seed=n_act)
    o = _to_dev(t)
    sd = sum(dims)
    sbuf = torch.full((R, sd + 4), NAN, device=DEV)
    cbuf = torch.full((R + 3,), NAN, device=DEV)
    pack = torch.full((ops.head_pack_floats(list(dims)),), NAN, device=DEV)
    ob, yb = _bufs(R, o["C"])
    for ph in phases:
        src = (fs, sbuf[:, :sd], cbuf) if ph != 4 else (fs, None, None)
        assert _fwd_call(o, pack, ob, yb, ph, form="src16", src16=src)
    torch.cuda.synchronize()
    a = t["act"][:n_act].long()
    assert same_bits(sbuf[:n_act, :sd].cpu(), torch.cat(S_w, 1)[a]) and same_bits(cbuf[:n_act].cpu(), c_w[a])
    assert all_nan(sbuf[n_act:]) and all_nan(sbuf[:, sd:]) and all_nan(cbuf[n_act:])
    _check_fwd(t, ob, yb, ref=_ref_of(t, S=S_w, c=c_w))
    # the plain head on the widened fp32 tables: the same bits
    o2 = dict(o)
    o2["S"], o2["c"] = [s.to(DEV) for s in S_w], c_w.to(DEV)
    ob2, yb2, _, _ = _run_fwd(o2, phases)
    assert same_bits(ob[:n_act], ob2[:n_act]) and same_bits(yb[:n_act], yb2[:n_act])


@pytest.mark.gpu
@pytest.mark.parametrize("W", [1, 2, 4, 8])
def test_fused_head_forward_reading_the_peers_pieces(W):
    """elimrec_head_fwd_fused (peers form) on a received [W x R x (out0 dl | narrow dl)] buffer: the fp64 reference, and the bits of
    ops.peer_cols_to_rows followed by the plain head (phases 0 and 1, 3, 4)."""
    from elimrec_amd import ops
    t = _fwd_case((60, 128), 40, 37, 21, "all", seed=W)
    o = _to_dev(t)
    dl = HD // W
    recv = torch.empty(W, 40, 2 * dl, device=DEV)
    for q in range(W):
        recv[q, :, :dl] = o["out0"][:, q * dl:(q + 1) * dl]
        recv[q, :, dl:] = o["narrow"][:, q * dl:(q + 1) * dl]
    r = _ref_of(t)
    for phases in ((0,), (1, 3, 4)):
        ob, yb, _, mid = _run_fwd(o, phases, peers=recv)
        _check_fwd(t, ob, yb, mid, ref=r)
        pair = torch.full((40, 2, HD), NAN, device=DEV)
        ops.peer_cols_to_rows(recv, pair[:, 0, :], pair[:, 1, :])
        assert same_bits(pair[:37, 0].cpu(), t["out0"][:37]) and same_bits(pair[:37, 1].cpu(), t["narrow"][:37])
        o2 = dict(o)
        o2["out0"], o2["narrow"] = pair[:, 0, :], pair[:, 1, :]
        ob2, yb2, _, _ = _run_fwd(o2, phases)
        assert same_bits(ob[:37], ob2[:37]) and same_bits(yb[:37], yb2[:37])


def _random_graph(n, U, seed):
    """A bipartite-looking ragged graph: empty rows, short rows and a few rows far above the long-row threshold."""
    rng = np.random.RandomState(seed)
    deg = rng.poisson(5, n)
    deg[rng.rand(n) < 0.05] = 0
    deg[rng.choice(n, 4, replace=False)] = 200 + rng.randint(0, 60, 4)
    rows = np.repeat(np.arange(n), deg)
    cols = np.where(rows < U, rng.randint(U, n, len(rows)), rng.randint(0, U, len(rows)))
    m = sp.csr_matrix((rng.rand(len(rows)).astype(np.float32) + 0.1, (rows, cols)), shape=(n, n))
    m.sum_duplicates()
    m.sort_indices()
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("n_act,n_lo", [(45, 17), (16, 0)])
def test_fused_head_forward_with_the_rows_inline(n_act, n_lo):
    """elimrec_head_fwd_fused (rows form), head_rows_fwd16_kernel: out0 = the layer means (L + 1 layers, the last A x_{L-1} evaluated
    inline: SELL rows from the tables, long rows from the seg_only launch's table) and narrow = the side's alternating layers
    (users: layers 0, 2, ..; items: 1, 3, ..) / (L + 1), against an fp64 A @ x; then the head over them."""
    from elimrec_amd import ops, slab
    n, U, L, w = 600, 250, 3, 32
    ns = HD // w
    m = _random_graph(n, U, seed=n_act)
    plan = slab.SellPlan(m, DEV, threshold=32, side_split=U)
    g = torch.Generator().manual_seed(n_act)
    X = [torch.randn(n, HD, generator=g) for _ in range(L)]
    layers = [x.view(n, ns, w).permute(1, 0, 2).contiguous().view(-1).to(DEV) for x in X]      # slab-major [ns][n][w]
    long_tab = torch.empty(ns * max(plan.n_long, 1) * w, device=DEV)
    slab.hop(plan, slab.SlabTable(n, ns, w, DEV, data=layers[-1]), long_tab, seg_only=True)
    t = _fwd_case((24, 68), 48, n_act, n_lo, "all", seed=3, N=n)
    t["act"][:n_act] = torch.tensor(_node_ids(g, U, n, n_lo, n_act - n_lo), dtype=torch.int32)
    A = torch.from_numpy(m.astype(np.float64).toarray())
    Xd = [x.double() for x in X]
    XL = A @ Xd[-1]
    sXL = A.abs() @ Xd[-1].abs()
    lay, slay = Xd + [XL], [x.abs() for x in Xd] + [sXL]
    a = t["act"][:n_act].long()
    inv = 1.0 / (L + 1)
    mean = sum(x[a] for x in lay) * inv
    smean = sum(x[a] for x in slay) * inv
    user = (a < U)[:, None]
    nar = torch.where(user, sum(lay[k][a] for k in range(0, L + 1, 2)), sum(lay[k][a] for k in range(1, L + 1, 2))) * inv
    snar = torch.where(user, sum(slay[k][a] for k in range(0, L + 1, 2)), sum(slay[k][a] for k in range(1, L + 1, 2))) * inv
    Kr = float(np.diff(m.indptr).max() + L + 2)
    o = _to_dev(t)
    R, C = 48, o["C"]
    pack = torch.full((ops.head_pack_floats(o["dims"]),), NAN, device=DEV)
    nbuf = torch.full((R, HD + 4), NAN, device=DEV)
    outs = []
    for _ in range(2):
        ob, yb = _bufs(R, C)
        nbuf.fill_(NAN)
        assert _fwd_call(o, pack, ob, yb, 1) and _fwd_call(o, pack, ob, yb, 3)
        rows = dict(plan=plan, ns=ns, w=w, L=L, U=U, layers=layers + [None], long_tab=long_tab, narrow=nbuf[:, :HD])
        assert ops.head_fwd_fused_rows(rows, o["act"], o["seg"], o["c"], o["S"], o["Wm"], o["bm"], o["Wf"][0], o["bf"][0],
                                       o["Wf"][1], o["bf"][1], o["Ws"], o["bs"], pack, ob[:, :C], yb[:, :C], HD)
        torch.cuda.synchronize()
        outs.append((ob, yb, nbuf.clone()))
    ob, yb, nb = outs[0]
    assert_close(ob[:n_act, :HD], mean, smean, Kr, "layer means")
    assert_close(nb[:n_act, :HD], nar, snar, Kr, "narrow")
    assert all_nan(nb[n_act:]) and all_nan(nb[:, HD:])
    # the head over the rows it made: its reference takes the kernel's own (checked) out0 / narrow as inputs
    t2 = dict(t)
    t2["out0"], t2["narrow"] = ob[:, :HD].cpu().clone(), nb[:, :HD].cpu().clone()
    _check_fwd(t2, ob, yb)
    for x, y in zip(outs[0], outs[1]):
        assert same_bits(x[:n_act], y[:n_act])


_LADDER_ROWS = {}


def _ladder_rows_case(w):
    """The rows ladder (tests/rows_model.py) at T = 64 on the tiered plan of a 64-column table in slabs of w floats (two slab
    groups, as the engine's choose_groups gives them), with eight random layer tables: built once per session."""
    import rows_model as rm
    from elimrec_amd import slab
    if w not in _LADDER_ROWS:
        T, ns = 64, HD // w
        gs = min(2, ns)
        G = 64 // ((ns // gs) * (w // 4))
        m, U, named = rm.rows_ladder(T, G)
        N = m.shape[0]
        plan = slab.SellPlan(m, DEV, threshold=T, side_split=U, tiered=True, ipw=G)
        assert plan.tiered and min(plan.n_w1, plan.n_w4, plan.n_seg) > 0
        g = torch.Generator().manual_seed(w)
        X = [torch.randn(N, HD, generator=g) for _ in range(4)]
        xs = [slab.SlabTable(N, ns, w, DEV).from_rows(x.to(DEV)) for x in X]
        long_tabs = {}
        for L in (1, 2, 3, 4):
            long_tabs[L] = torch.full((ns * plan.n_long * w,), NAN, device=DEV)
            slab.hop(plan, xs[L - 1], long_tabs[L], gs=gs, seg_only=True)
        _LADDER_ROWS[w] = types.SimpleNamespace(m=m, U=U, N=N, named=named, plan=plan, ns=ns, w=w, X=X, xs=xs, long_tabs=long_tabs)
    return _LADDER_ROWS[w]


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 2, 3, 4])
@pytest.mark.parametrize("w", [8, 16, 32, 64])
def test_fused_head_rows_form_on_the_ladder_at_every_boundary_offset(w, L):
    """elimrec_head_fwd_fused (rows form) on the tiered T = 64 plan: the batch holds every named row of the rows ladder on both
    sides (the 16-wide groups' remainders, all three upper tiers out of the compact table), the user / item boundary of the sorted
    active list sits at every offset 0..16 of a 16-row tile, the row count is no multiple of 16. OutAct (every block), YAct and the
    narrow buffer are bit for bit those of slab.rows into the same buffers followed by the plain phase-4 head (the engine with
    ELIMREC_ROWS_IN_HEAD=0); the out0 block and the narrow buffer lie inside the float64 bound of rows_model.rows_ref; rows past
    the active count are untouched. A geometry the entry point refuses must write nothing."""
    import rows_model as rm
    from elimrec_amd import ops, slab
    c = _ladder_rows_case(w)
    R = 96
    layers = [t.data for t in c.xs[:L]] + [None]
    users = sorted(r for (s, _), r in c.named.items() if s == "user")
    items = sorted(r for (s, _), r in c.named.items() if s == "item")
    rs = np.random.RandomState(16 * w + L)
    rest_u = np.setdiff1d(np.arange(c.U), users + [c.U - 1])
    rest_i = np.setdiff1d(np.arange(c.U, c.N), items + [c.U])
    for off in range(17):
        n_lo = 32 + off
        n_hi = 24 if (off + 23) % 16 == 0 else 23
        n_act = n_lo + n_hi
        assert n_act % 16 != 0 and n_act <= R
        a_u = np.sort(np.concatenate([users, [c.U - 1], rs.choice(rest_u, n_lo - len(users) - 1, replace=False)]))
        a_i = np.sort(np.concatenate([items, [c.U], rs.choice(rest_i, n_hi - len(items) - 1, replace=False)]))
        nodes = np.concatenate([a_u, a_i]).astype(np.int64)
        t = _fwd_case((24, 68), R, n_act, n_lo, "all", seed=3, N=c.N)
        t["act"][:n_act] = torch.from_numpy(nodes).int()
        o = _to_dev(t)
        C = o["C"]
        what = "w %d L %d boundary offset %d" % (w, L, off)
        pack = torch.full((ops.head_pack_floats(o["dims"]),), NAN, device=DEV)
        cnt = torch.tensor([n_act], dtype=torch.int32, device=DEV)
        res = {}
        for form in ("launches", "fused"):
            ob, yb = _bufs(R, C)
            nbuf = torch.full((R, HD + 4), NAN, device=DEV)
            assert _fwd_call(o, pack, ob, yb, 1) and _fwd_call(o, pack, ob, yb, 3)
            if form == "launches":
                slab.rows(c.plan, c.ns, w, L, c.U, layers, c.long_tabs[L], o["act"].view(1, R), cnt, R, 1, ob[:, :HD], nbuf[:, :HD], False)
                o2 = dict(o)
                o2["out0"], o2["narrow"] = ob[:, :HD], nbuf[:, :HD]
                assert _fwd_call(o2, pack, ob, yb, 4)
            else:
                rows = dict(plan=c.plan, ns=c.ns, w=w, L=L, U=c.U, layers=layers, long_tab=c.long_tabs[L], narrow=nbuf[:, :HD])
                try:
                    ok = ops.head_fwd_fused_rows(rows, o["act"], o["seg"], o["c"], o["S"], o["Wm"], o["bm"], o["Wf"][0], o["bf"][0],
                                                 o["Wf"][1], o["bf"][1], o["Ws"], o["bs"], pack, ob[:, :C], yb[:, :C], HD)
                except RuntimeError:
                    ok = False
                torch.cuda.synchronize()
                if not ok:              # refused: nothing beyond what phase 3 left
                    assert all_nan(yb) and all_nan(nbuf) and all_nan(ob[:, :HD]), what + ": refused, but something was written"
                    pytest.fail(what + ": refused (the entry point takes every ns x w = 64 with w / 4 a power of two)")
            torch.cuda.synchronize()
            res[form] = (ob, yb, nbuf)
        for name, x, y in zip(("OutAct", "YAct", "narrow"), res["launches"], res["fused"]):
            assert same_bits(x, y), "%s: %s differs from slab.rows + the phase-4 head" % (what, name)
        ob, yb, nbuf = res["fused"]
        assert all_nan(ob[n_act:]) and all_nan(yb[n_act:]) and all_nan(nbuf[n_act:]) and all_nan(nbuf[:, HD:]) and all_nan(ob[:, C:])
        assert not bool(torch.isnan(ob[:n_act, :C]).any()) and not bool(torch.isnan(yb[:n_act, :C]).any())
        o64, s0, n64, sn, K = rm.rows_ref(c.m, c.X[:L], None, nodes, c.U)
        assert_close(ob[:n_act, :HD], o64, s0, K, what + ": layer means")
        assert_close(nbuf[:n_act, :HD], n64, sn, K, what + ": narrow")


@pytest.mark.gpu
def test_fused_head_gate_never_sends_a_shape_the_kernel_refuses():
    """ColumnShardEngine._fused_head_ok's LDS estimate (still the removed 32-row head's layout) against the 16-row kernel: every
    width set the gate accepts runs at phase 0. The gate is conservative only: it turns away shapes the kernel would take
    (Kwai's one 2048-wide table), never the other way."""
    from elimrec_amd import ops
    from elimrec_amd.shard import ColumnShardEngine
    width_sets = [(128, 128, 128), (2048,), (2048, 128, 100),      # Tiktok, Kwai, MovieLens
                  (24, 16, 128), (48,), (40, 24, 20), (16, 12, 24),  # the fixtures' tables
                  (4,), (1024,), (1024, 1024), (512, 512, 512), (2324,), (2328,), (640, 640, 640), (1200, 4, 4)]
    seen = {}
    for dims in width_sets:
        mods = ["v", "a", "t"][:len(dims)]
        model = types.SimpleNamespace(latent_dim=HD, S=len(dims), C=(1 + len(dims)) * HD, mm_fusion_mode="concat", _mods=mods,
                                      _device=lambda: DEV)
        for k, D in zip(mods, dims):
            setattr(model, k + "_feat", torch.empty(1, D))
        stub = types.SimpleNamespace(model=model, _fused=None)
        gate = ColumnShardEngine._fused_head_ok(stub)
        t = _fwd_case(dims, 16, 3, 1, seed=2, N=40)
        o = _to_dev(t)
        pack = torch.full((ops.head_pack_floats(list(dims)),), NAN, device=DEV)
        ob, yb = _bufs(16, o["C"])
        ok = _fwd_call(o, pack, ob, yb, 0)
        torch.cuda.synchronize()
        if ok:
            _check_fwd(t, ob, yb)
        else:
            assert all_nan(ob) and all_nan(yb)
        assert ok or not gate, dims
        seen[dims] = (gate, ok)
    assert seen[(128, 128, 128)] == (True, True) and seen[(2048,)] == (False, True) and seen[(2048, 128, 100)] == (False, False)


# ----------------------------------------------------------------------------- 2. head input gradient
def _bwd_weights(g, d, S, fusion):
    C = (1 + S) * d
    if fusion == "mean":         # EliMRec._fusion_weights: the [d x d] Linear over the mean of the M blocks as a [d x C] map
        M = C // d
        wu, wi = (torch.randn(d, d, generator=g) / M).repeat(1, M), (torch.randn(d, d, generator=g) / M).repeat(1, M)
    else:
        wu, wi = torch.randn(d, C, generator=g), torch.randn(d, C, generator=g)
    return C, wu.contiguous(), wi.contiguous(), [torch.randn(d, d, generator=g) for _ in range(S)]


BWD_CASES = [
    # d, S, mblock, n_act, n_users, n_max, fusion, out (G0 / compact / both), scatter_cols (None: C)   -> kernel
    (4, 0, [], 1, 1, 16, "concat", "G0", None),                  # scalar
    (16, 2, [2, 1], 17, 5, 40, "mean", "both", 40),              # scalar, scatter_cols < C
    (48, 4, [4, 1, 3, 2], 15, 0, 15, "concat", "compact", None),  # scalar, items only
    (192, 3, [1, 2, 3], 16, 16, 20, "concat", "both", 500),      # scalar: over the MFMA kernel's 96 KB of LDS
    (32, 1, [1], 17, 9, 64, "concat", "both", 20),               # MFMA
    (64, 3, [3, 1, 2], 16, 16, 16, "mean", "compact", None),     # MFMA, users only
    (96, 4, [2, 4, 1, 3], 70, 33, 96, "concat", "G0", None),     # MFMA, boundary at offset 1 of a 32-row tile
    (128, 0, [], 40, 31, 64, "concat", "both", 100),             # MFMA, S = 0, offset 31
]


def _bwd_direct(d, S, mblock, n_act, n_users, n_max, fusion, out, scatter_cols, seed):
    from elimrec_amd import ops
    g = torch.Generator().manual_seed(seed)
    U, N = 200, 420
    C, wu, wi, wh = _bwd_weights(g, d, S, fusion)
    sc = C if scatter_cols is None else scatter_cols
    nodes = torch.tensor(_node_ids(g, U, N, n_users, n_act - n_users), dtype=torch.int64)
    act = torch.zeros(n_max, dtype=torch.int32)
    act[:n_act] = nodes.int()
    dY = torch.randn(n_max, (1 + S) * d, generator=g)
    dY[n_act:] = NAN
    gscale = 0.75
    dOut, sOut, K = ref_head_bwd(dY[:n_act].double(), dY[:n_act].double().abs(), nodes, U, d, C, mblock, wu.double(),
                                 wi.double(), [w.double() for w in wh], gscale)
    dev = lambda x: x.to(DEV)
    res = []
    for _ in range(2):
        G0 = torch.full((N, C + 4), NAN, device=DEV) if out in ("G0", "both") else None
        comp = torch.full((n_max, C), NAN, device=DEV) if out in ("compact", "both") else None
        ops.head_bwd_input(dev(dY), dev(act), dev(torch.tensor([n_act, n_users, 0, 0, 0, 0, 0, 0], dtype=torch.int32)), U, d, C,
                           mblock, dev(wu), dev(wi), [dev(w) for w in wh], gscale, G0,
                           scatter_cols=(sc if G0 is not None else None), compact=comp)
        torch.cuda.synchronize()
        res.append((G0, comp))
    G0, comp = res[0]
    if comp is not None:
        assert_close(comp[:n_act], dOut, sOut, K, "compact dOut")
        assert all_nan(comp[n_act:])
        assert same_bits(comp[:n_act], res[1][1][:n_act])
    if G0 is not None:
        w = min(sc, C)
        assert_close(G0[nodes.to(DEV), :w], dOut[:, :w], sOut[:, :w], K[:, :w], "G0 scatter")
        written = torch.zeros(N, C + 4, dtype=torch.bool)
        written[nodes, :w] = True
        assert all_nan(G0.cpu()[~written])
        assert same_bits(G0[nodes.to(DEV), :w], res[1][0][nodes.to(DEV), :w])


@pytest.mark.gpu
@pytest.mark.parametrize("d,S,mblock,n_act,n_users,n_max,fusion,out,scatter_cols", BWD_CASES)
def test_head_bwd_input_vs_fp64(d, S, mblock, n_act, n_users, n_max, fusion, out, scatter_cols):
    """elimrec_head_bwd_input (head_bwd_input_kernel when d % 32 != 0 or 32 ((1+S) d + 1) floats pass 96 KB, else
    head_bwd_input_mfma_kernel) against ref_head_bwd: the compact rows and / or the G0 scatter at act[r], columns <
    scatter_cols; nothing else written; the same bits twice."""
    _bwd_direct(d, S, mblock, n_act, n_users, n_max, fusion, out, scatter_cols, seed=d + S + n_act)


@pytest.mark.gpu
def test_head_bwd_input_at_every_tile_offset_of_the_user_item_boundary():
    """The tile that straddles the user/item boundary takes both weight matrices and picks per row: the boundary at every
    offset 0..15 of a 16-row tile (scalar kernel, d = 16) and at 0, 1 and 31 of a 32-row tile (MFMA kernel, d = 32)."""
    for off in range(16):
        _bwd_direct(16, 1, [1], 40, 16 + off, 48, "concat", "compact", None, seed=off)
    for off in (0, 1, 31):
        _bwd_direct(32, 2, [2, 1], 70, 32 + off, 72, "concat", "compact", None, seed=100 + off)


def _seg_case(d, S, n_users, n_items, extra, hot, seed, U=300, I=500):
    """A key list whose distinct keys are n_users users and n_items items (every active row listed once, then `extra` repeats
    at random and `hot` more slots of one item), shuffled; its fp64 segment sums."""
    g = torch.Generator().manual_seed(seed)
    nodes = torch.tensor(_node_ids(g, U, U + I, n_users, n_items), dtype=torch.int64)
    keys = [nodes]
    if extra:
        keys.append(nodes[torch.randint(0, len(nodes), (extra,), generator=g)])
    if hot:
        keys.append(torch.full((hot,), int(nodes[-1]), dtype=torch.int64))
    keys = torch.cat(keys)
    keys = keys[torch.randperm(len(keys), generator=g)]
    rows = torch.randn(len(keys), (1 + S) * d, generator=g)
    uniq = torch.unique(keys)
    inv = torch.searchsorted(uniq, keys)
    red = torch.zeros(len(uniq), rows.shape[1], dtype=torch.float64).index_add_(0, inv, rows.double())
    ared = torch.zeros_like(red).index_add_(0, inv, rows.double().abs())
    cnt = torch.bincount(inv, minlength=len(uniq)).double()
    return dict(keys=keys, rows=rows, uniq=uniq, red=red, ared=ared, cnt=cnt, U=U, I=I, g=g)


def _pack_for(g, S, C):
    """The packed weights ops.head_fwd_fused leaves behind (phase 1: pack only), and the backward region's offset."""
    from elimrec_amd import ops
    dims = [8] * S
    Wf = [torch.randn(HD, C, generator=g).to(DEV) for _ in range(2)]
    Ws = [torch.randn(HD, HD, generator=g).to(DEV) for _ in range(S)]
    z = lambda *s: torch.zeros(*s, device=DEV)
    pack = torch.full((ops.head_pack_floats(dims),), NAN, device=DEV)
    assert ops.head_fwd_fused(torch.zeros(16, dtype=torch.int32, device=DEV), torch.zeros(8, dtype=torch.int32, device=DEV),
                              z(16, HD), z(16, HD), z(4), [z(4, 8) for _ in range(S)], [z(HD, 8) for _ in range(S)], [None] * S,
                              Wf[0], None, Wf[1], None, Ws, [None] * S, pack, z(16, C), z(16, C), HD, phase=1)
    return Wf, Ws, pack[ops.head_pack_bwd_offset(dims):]


def _seg_run(c, d, S, mblock, form="plain", fusion="concat", world=1, w=16):
    """ops.segment_apply_head_bwd over segment_plan's plan of c["keys"], checked against the fp64 segment sums + ref_head_bwd.
    form: plain (unpacked: MFMA with the reduce fused, or segment_apply + the scalar kernel), packed, sources, split."""
    from elimrec_amd import ops
    g = c["g"]
    U, I, n = c["U"], c["I"], len(c["keys"])
    Cy = (1 + S) * d
    if form == "plain":
        C, wu, wi, wh = _bwd_weights(g, d, S, fusion)
        wu, wi, wh = wu.to(DEV), wi.to(DEV), [x.to(DEV) for x in wh]
        pack_bwd = None
    else:
        C = Cy
        (wu, wi), wh, pack_bwd = _pack_for(g, S, C)
    keys = c["keys"].int().to(DEV)
    ws = torch.empty(ops.segment_plan_workspace(n), dtype=torch.uint8, device=DEV)
    act = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    seg = torch.zeros(8, dtype=torch.int32, device=DEV)
    ops.segment_plan(keys, U, U + I, act, seg, torch.empty(n, dtype=torch.int32, device=DEV), ws)
    na = int(seg[0])
    assert na == len(c["uniq"]) and same_bits(act[:na].cpu().long(), c["uniq"])
    scale = 0.37
    dY, adY = c["red"] * scale, c["ared"] * scale
    dOut, sOut, K = ref_head_bwd(dY, adY, c["uniq"], U, d, C, mblock, wu.double().cpu(), wi.double().cpu(),
                                 [x.double().cpu() for x in wh], 1.0, Kin=c["cnt"][:, None])
    rows_d = c["rows"].to(DEV)
    sc_t = torch.full((1,), scale, device=DEV)
    res = []
    for _ in range(2):
        red = torch.full((n, Cy), NAN, device=DEV)
        comp = torch.full((n, C), NAN, device=DEV)
        sources, extra = None, None
        if form == "sources":
            N = U + I
            extra = (torch.full((d // w * N * w,), NAN, device=DEV), torch.full((d // w * N * w,), NAN, device=DEV))
            from elimrec_amd import slab
            sources = (slab.SlabTable(N, d // w, w, DEV, data=extra[0]), slab.SlabTable(N, d // w, w, DEV, data=extra[1]))
        elif form == "split":
            extra = torch.full((world, n + 5, 2 * (d // world)), NAN, device=DEV)
            sources = ("split", extra, world)
        ops.segment_apply_head_bwd(rows_d, act, seg, red, ws, U, d, C, mblock, wu, wi, wh, comp, scale=sc_t, pack_bwd=pack_bwd,
                                   sources=sources)
        torch.cuda.synchronize()
        res.append((red, comp, extra))
    red, comp, extra = res[0]
    assert_close(red[:na], dY, adY, c["cnt"][:, None], "segment sums dY")
    assert_close(comp[:na], dOut, sOut, K, "dOut rows")
    assert all_nan(red[na:]) and all_nan(comp[na:])
    assert same_bits(red[:na], res[1][0][:na]) and same_bits(comp[:na], res[1][1][:na])
    if form in ("sources", "split"):
        # H = the C / d column blocks added in block order (fp32, the kernel's own order: the same bits as the compact blocks),
        # G = block 0; fp64: H within the blocks' bounds
        blocks = comp[:na].view(na, C // d, d)
        H = blocks[:, 0].clone()
        for b in range(1, C // d):
            H = H + blocks[:, b]
        G = blocks[:, 0]
        Hr = dOut.view(na, C // d, d).sum(1)
        sH = sOut.view(na, C // d, d).sum(1)
        assert_close(H, Hr, sH, K.max() + C // d, "H")
        if form == "sources":
            N = U + I
            ta, tb = (x.view(d // w, N, w).permute(1, 0, 2).reshape(N, d) for x in extra)
            nodes = act[:na].long()
            user = (nodes < U)[:, None]
            assert same_bits(ta[nodes], torch.where(user, H, G)) and same_bits(tb[nodes], torch.where(user, G, H))
            mask = torch.ones(N, dtype=torch.bool, device=DEV)
            mask[nodes] = False
            assert all_nan(ta[mask]) and all_nan(tb[mask])
        else:
            dl = d // world
            for q in range(world):
                assert same_bits(extra[q, :na, :dl], H[:, q * dl:(q + 1) * dl])
                assert same_bits(extra[q, :na, dl:], G[:, q * dl:(q + 1) * dl])
            assert all_nan(extra[:, na:])
        for x, y in zip(extra if isinstance(extra, tuple) else (extra,), res[1][2] if isinstance(extra, tuple) else (res[1][2],)):
            assert same_bits(torch.nan_to_num(x, nan=7.0), torch.nan_to_num(y, nan=7.0))


@pytest.mark.gpu
@pytest.mark.parametrize("d,S,mblock,n_users,n_items,extra,hot,fusion", [
    (32, 2, [1, 2], 21, 30, 40, 0, "concat"),        # MFMA kernel, segment reduce fused (first members + the serial loop)
    (128, 1, [1], 40, 9, 20, 700, "mean"),           # MFMA kernel, one hot segment of 701 members
    (48, 2, [2, 1], 17, 16, 30, 0, "concat"),        # segment_apply + the scalar kernel
    (96, 0, [], 1, 0, 3, 0, "concat"),               # one active row, S = 0
])
def test_segment_apply_head_bwd_unpacked_vs_fp64(d, S, mblock, n_users, n_items, extra, hot, fusion):
    """ops.segment_apply_head_bwd without the packed operands: dY = scale * the segment sums, dOut = ref_head_bwd of them."""
    c = _seg_case(d, S, n_users, n_items, extra, hot, seed=d * 7 + S)
    _seg_run(c, d, S, mblock, "plain", fusion)


@pytest.mark.gpu
@pytest.mark.parametrize("S,mblock,n_users,n_items,extra,hot", [
    (3, [1, 2, 3], 32, 16, 30, 700),     # every tile on one side: the fast path only; the hot segment walks the 16-, 4- and 1-wide loops
    (1, [1], 1, 14, 6, 0),               # one 15-row tile, straddling at offset 1: the in-kernel fallback only
    (2, [2, 1], 16, 1, 0, 0),            # n_act 17: a full user tile and one item row
    (2, [1, 2], 5, 10, 4, 0),            # n_act 15
    (1, [1], 0, 1, 0, 0),                # n_act 1
])
def test_segment_apply_head_bwd_packed_vs_fp64(S, mblock, n_users, n_items, extra, hot):
    """head_bwd_input16_kernel (recdim 64, the pack of ops.head_fwd_fused at head_pack_bwd_offset): the fast path
    (PACKED && !mixed && C <= 256) for tiles on one side, the in-kernel fallback for the straddling tile."""
    c = _seg_case(HD, S, n_users, n_items, extra, hot, seed=S * 31 + n_users)
    _seg_run(c, HD, S, mblock, "packed")


@pytest.mark.gpu
def test_segment_apply_head_bwd_packed_at_every_tile_offset():
    """The packed 16-row kernel with the user/item boundary at every offset 0..15 of a tile (S = 1..3 in turn)."""
    for off in range(16):
        S = 1 + off % 3
        c = _seg_case(HD, S, 16 + off, 20, 10, 0, seed=off)
        _seg_run(c, HD, S, list(range(1, S + 1)), "packed")


@pytest.mark.gpu
@pytest.mark.parametrize("form,S,w_or_world,n_users,n_items,hot", [
    ("sources", 3, 16, 21, 40, 0),
    ("sources", 1, 64, 16, 16, 50),
    ("sources", 2, 4, 7, 9, 0),
    ("split", 2, 1, 19, 20, 0),
    ("split", 3, 2, 16, 33, 30),
    ("split", 1, 4, 3, 12, 0),
])
def test_segment_apply_head_bwd_adjoint_sources_vs_fp64(form, S, w_or_world, n_users, n_items, hot):
    """The 16-row head backward filling the adjoint sources itself: H (the sum of the C/64 column blocks) into A for user rows
    and B for item rows, G (block 0) the other way, in [64/w x N x w] slab tables (_sources); or [H | G] cut into `world`
    column slices (_split). Every other row of the tables stays NaN."""
    c = _seg_case(HD, S, n_users, n_items, 25, hot, seed=S * 5 + w_or_world)
    if form == "sources":
        _seg_run(c, HD, S, list(range(1, S + 1)), "sources", w=w_or_world)
    else:
        _seg_run(c, HD, S, list(range(1, S + 1)), "split", world=w_or_world)


# ----------------------------------------------------------------------------- 3. BPR loss head over compact rows
BPR_CASES = [
    # d, weights, B
    (4, [1.0], 1),
    (8, [1.0, 0.5], 3),
    (12, [1.0, 0.0, 0.25], 4),           # d / 4 = 3: a group of 4 lanes with one idle
    (20, [1.0, 0.5, 0.5, 0.5], 5),       # d / 4 = 5
    (64, [1.0, 0.5, 0.0, 0.25], 1023),
    (96, [1.0, 0.3], 1024),              # d / 4 = 24
    (256, [1.0, 0.0, 0.7], 1025),
    (260, [1.0, 0.5], 6145),             # d / 4 = 65: a whole wave per block, two column rounds
]


def _bpr_case(d, w, B, seed):
    g = torch.Generator().manual_seed(seed)
    nb = len(w)
    R = min(3 * B, 64) + 5
    Y = torch.randn(R, nb * d + 4, generator=g)           # ldy > nb * d
    Y[2] = 0.0                                            # a zero row: the eps branch
    slot = torch.randint(0, R, (3 * B,), generator=g, dtype=torch.int32)
    slot[:min(3 * B, 4)] = 2
    if B > 3:
        slot[6:9] = slot[3:6]                             # a repeated triplet
    return Y, slot


@pytest.mark.gpu
@pytest.mark.parametrize("d,w,B", BPR_CASES)
def test_bpr_head_rows_vs_fp64_autograd(d, w, B):
    """ops.bpr_head_rows / _sum / _sum_pub (bpr_head_kernel, bpr_head_sum_kernel) against ref_bpr_rows: the loss rows and the
    gradient rows element by element, zero-weight blocks exact zeros, no row past 3B written; the summed loss has the bits of
    elimrec_sum over the loss rows, the ticket is back at 0, the published (sequence, value) pair advances by one per launch."""
    from elimrec_amd import ops
    Y, slot = _bpr_case(d, w, B, seed=d + B)
    nb = len(w)
    lr, gr, sl, sg = ref_bpr_rows(Y[:, :nb * d], slot.long(), d, w)
    Kb = 4 * d + 32
    Yd, sd = Y.to(DEV), slot.to(DEV)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    pub = ops.LossPublisher(8)
    results = []
    for form in ("rows", "sum", "sum", "pub", "pub"):
        loss_rows = torch.full((B + 3,), NAN, device=DEV)
        grad_rows = torch.full((3 * B + 2, nb * d), NAN, device=DEV)
        loss = torch.full((1,), NAN, device=DEV)
        if form == "rows":
            ops.bpr_head_rows(Yd[:, :nb * d + 4], sd, d, w, loss_rows, grad_rows)
        elif form == "sum":
            ops.bpr_head_rows_sum(Yd, sd, d, w, loss_rows, grad_rows, loss, ticket)
        else:
            seq0 = pub.issued()
            ops.bpr_head_rows_sum_pub(Yd, sd, d, w, loss_rows, grad_rows, loss, ticket, pub.handle)
            assert pub.issued() == seq0 + 1
            got = pub.wait(seq0 + 1, timeout_s=30.0)
        torch.cuda.synchronize()
        assert_close(loss_rows[:B], lr, sl, Kb, "loss rows")
        assert_close(grad_rows[:3 * B], gr, sg, Kb, "gradient rows")
        for k, wk in enumerate(w):
            if wk == 0.0:
                assert bool((grad_rows[:3 * B, k * d:(k + 1) * d] == 0).all())
        assert all_nan(loss_rows[B:]) and all_nan(grad_rows[3 * B:])
        if form != "rows":
            ref_sum = torch.empty((), device=DEV)
            ops.fixed_order_sum(loss_rows[:B], ref_sum)
            assert same_bits(loss[0], ref_sum) and int(ticket[0]) == 0
            assert within(loss.cpu(), lr.sum()[None], sl.sum()[None], Kb + B).all()
            if form == "pub":
                assert got == float(loss[0])
        results.append((loss_rows[:B].clone(), grad_rows[:3 * B].clone(), loss.clone()))
    for r in results[1:]:
        assert same_bits(r[0], results[0][0]) and same_bits(r[1], results[0][1])
    assert same_bits(results[1][2], results[2][2]) and same_bits(results[3][2], results[4][2])
    assert same_bits(results[1][2], results[3][2])
