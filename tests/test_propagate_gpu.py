"""The row-major propagation kernels (csrc/spmm.hip, embed_grad of csrc/optim.hip) against the float64 model of
tests/propagate_model.py, element by element, on the ladder graphs: every row length at which the code branches (0, 7/8/9, a
multiple of the lane-group width +- 1, the threshold and threshold + 1, a last segment of one entry, >= 8 segments per lane group)
occurs by construction. Calls go through elimrec_amd.ops only. Every output starts as NaN and what the contract leaves unwritten
must still be NaN afterwards; every input region that must not be read holds NaN.

The bound is fp64_tools.assert_close with the K of propagate_model (a row's own length + 3 for one hop, L (longest row + 2) + 2
for L hops); copies compare bit for bit. Two-stage checks where an op forms its own inputs: propagate_bipartite_bwd's gE_u is held
to the Horner adjoint of the H it was given (H itself: blocksum_rows, K = M), propagate_folded_bwd's grad to the Horner adjoint of
the SrcA / SrcB it left (their H part: K = M against dOutR, their G part: bits), so no K grows.

HalfArgs::row_list is set by no entry point and cannot be reached through the ABI: not tested.
"""
import numpy as np
import pytest
import torch

import propagate_model as pm
from fp64_tools import NAN, TINY, all_nan, assert_close, same_bits, tau

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORST = {}          # family -> worst err / tol seen in this session (printed by the last test)
T32 = pm.LADDER_T


def _ops():
    from elimrec_amd import ops
    return ops


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def _rand(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _close(family, got, ref, scale, K, what):
    g = got.detach().double().cpu()
    tol = tau(K) * scale + TINY
    if isinstance(tol, torch.Tensor) and tol.shape != g.shape:
        tol = tol.expand_as(g)
    fin = torch.isfinite(g) & torch.isfinite(ref)
    if bool(fin.any()):
        WORST[family] = max(WORST.get(family, 0.0), float(((g - ref).abs()[fin] / tol[fin]).max()))
    assert_close(got, ref, scale, K, what)


def _csr(m, C, T):
    ops = _ops()
    return ops.Csr.from_scipy(m, DEV, C=C, threshold=T) if T else ops.Csr.from_scipy(m, DEV)


_GRAPHS = {}


def _graph(name):
    if not _GRAPHS:
        _GRAPHS.update(square=pm.ladder_square("long"), rect=pm.ladder_rect("empty"),
                       alllong=pm.ladder_all_long(37, pm.SQUARE_N), bip=pm.ladder_bipartite())
    return _GRAPHS[name]


def _seg(count, n_users):
    return torch.tensor([count, n_users, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=DEV)


def _active(N, U, n_max, count, seed):
    """active_rows [n_max] (sorted, the mandatory rows first in line for any count >= 6, zeros past count) and its count."""
    rs = np.random.RandomState(seed)
    must = np.array([0, 31, 32, U - 1, U, N - 1])
    rest = np.setdiff1d(np.arange(N), must)
    act = np.sort(np.concatenate([must, rs.choice(rest, size=max(count - len(must), 0), replace=False)]))[:count]
    rows = np.zeros(n_max, dtype=np.int32)
    rows[:count] = act
    return rows, int(count)


# ============================================================================= half hop via block_spmm
WIDTHS = [4, 8, 12, 16, 32, 48, 64, 128, 256, 260, 512]
CONFIGS = [("square", T32), ("square", 4), ("square", None), ("rect", T32), ("rect", 4), ("rect", None), ("alllong", T32)]
FORMS = ("plain", "epilogue", "window")


def _hop_launch(csr, m, W, form, X, add):
    """One block_spmm in the given form: (Xout table, acc table or None, column offset of the window)."""
    ops = _ops()
    n, nc = m.shape
    pad, c0 = (8, 4) if form == "window" else (0, 0)
    ld = W + pad
    xin, xout = _nan(nc, ld), _nan(n, ld)
    xin[:, c0:c0 + W] = X
    if form == "plain":
        ops.block_spmm(csr, xin[:, c0:c0 + W], Xout=xout[:, c0:c0 + W])
        return xout, None, c0
    a1, acc = _nan(n, ld), _nan(n, ld)
    a1[:, c0:c0 + W] = add
    ops.block_spmm(csr, xin[:, c0:c0 + W], Xout=xout[:, c0:c0 + W], add1=a1[:, c0:c0 + W], acc_out=acc[:, c0:c0 + W], scale=0.25)
    return xout, acc, c0


def _hop_inputs(name, W):
    m = _graph(name)
    X, add = _rand(W, m.shape[1], W), _rand(W + 1, m.shape[0], W)
    return m, X.to(DEV), add.to(DEV), pm.block_spmm(m, X, add1=add, scale=0.25)


@pytest.mark.parametrize("W", WIDTHS)
def test_half_hop_is_inside_the_bound_on_every_row_length(W):
    kept = {}
    for name in ("square", "rect", "alllong"):
        m, X, add, ((r, rs), (acc, accs)) = _hop_inputs(name, W)
        K = pm.hop_K(m)
        for T in [t for g, t in CONFIGS if g == name]:
            csr = _csr(m, W, T)
            if T:
                assert csr._split.n_long > 0 and (name != "alllong" or csr._split.n_row_items == 0)
            for form in FORMS:
                what = "%s T=%s W=%d %s" % (name, T, W, form)
                xout, ao, c0 = _hop_launch(csr, m, W, form, X, add)
                _close("half hop", xout[:, c0:c0 + W], r, rs, K, what + " Xout")
                if ao is not None:
                    _close("half hop", ao[:, c0:c0 + W], acc, accs, K, what + " acc_out")
                for t in (xout, ao):
                    if t is not None and form == "window":          # columns outside the window are not written
                        assert all_nan(t[:, :c0]) and all_nan(t[:, c0 + W:]), what
                xout2, ao2, _ = _hop_launch(csr, m, W, form, X, add)
                assert same_bits(xout, xout2) and (ao is None or same_bits(ao, ao2)), what + ": second launch differs"
                kept[(name, T, form)] = (xout, ao)
        lens = torch.from_numpy(pm.row_lengths(m))
        for T in [t for g, t in CONFIGS if g == name and t]:       # the same fma chain with and without a plan
            rows = (lens <= T).nonzero().flatten().to(DEV)
            for form in FORMS if (name, None, "plain") in kept else ():
                for a, b in zip(kept[(name, T, form)], kept[(name, None, form)]):
                    assert a is None or same_bits(a[rows], b[rows]), "%s T=%d W=%d %s: unsplit rows differ from the plan-less launch" % (name, T, W, form)


@pytest.mark.parametrize("W", WIDTHS)
def test_split_rows_combined_in_the_launch_equal_the_fixup_launch(W):
    from elimrec_amd import _lib
    lib = _lib.load()
    for name, T in [c for c in CONFIGS if c[1]]:
        m, X, add, _ = _hop_inputs(name, W)
        csr = _csr(m, W, T)
        assert csr._split.n_long > 0
        for form in FORMS:
            runs = []
            try:
                for setting in (0, 1):
                    lib.elimrec_set_ticket_fixup(setting)
                    runs += [_hop_launch(csr, m, W, form, X, add)[:2] for _ in range(2)]
            finally:
                lib.elimrec_set_ticket_fixup(1)
            for xo, ao in runs[1:]:
                assert same_bits(xo, runs[0][0]) and (ao is None or same_bits(ao, runs[0][1])), (name, T, W, form)
            assert int(csr._split_tensors[5].abs().sum()) == 0, "ticket counters not back to zero"


# ============================================================================= spmm_hop / propagate
@pytest.mark.parametrize("T", [T32, 4])
@pytest.mark.parametrize("C", [4, 64, 260, 512])
def test_spmm_hop_forms_and_propagate(C, T):
    ops = _ops()
    m = _graph("square")
    n = m.shape[0]
    csr = _csr(m, C, T)
    X, acc_in = _rand(C, n, C), _rand(C + 1, n, C)
    Xd, Ad = X.to(DEV), acc_in.to(DEV)
    K = pm.hop_K(m)
    (r, rs), _ = pm.spmm_hop(m, X)
    _, (acc, accs) = pm.spmm_hop(m, X, acc_in=acc_in, scale=1.0 / 3.0)
    xo = _nan(n, C)
    ops.spmm_hop(csr, Xd, Xout=xo)
    _close("spmm_hop", xo, r, rs, K, "spmm_hop Xout only")
    ao = _nan(n, C)
    ops.spmm_hop(csr, Xd, acc_in=Ad, acc_out=ao, scale=1.0 / 3.0)
    _close("spmm_hop", ao, acc, accs, K, "spmm_hop acc_out only")
    xo2, ao2 = _nan(n, C), _nan(n, C)
    ops.spmm_hop(csr, Xd, Xout=xo2, acc_in=Ad, acc_out=ao2, scale=1.0 / 3.0)
    assert same_bits(xo2, xo) and same_bits(ao2, ao)
    assert same_bits(Xd.cpu(), X) and same_bits(Ad.cpu(), acc_in)
    for L in range(5):
        t0, t1, out = _nan(n, C), _nan(n, C), _nan(n, C)
        ops.propagate(csr, Xd, L, t0, t1, out)
        ref, scale = pm.propagate(m, X, L)
        _close("propagate", out, ref, scale, pm.chain_K(L, m), "propagate C=%d T=%d L=%d" % (C, T, L))
        assert same_bits(Xd.cpu(), X), "X0 changed"
        assert (L >= 2 or all_nan(t0)) and (L >= 3 or all_nan(t1))
        if L == 0:
            assert same_bits(out, Xd)
        out2 = _nan(n, C)
        ops.propagate(csr, Xd, L, t0, t1, out2)
        assert same_bits(out, out2)


# ============================================================================= propagate_bipartite and its adjoint
@pytest.mark.parametrize("L", [1, 2, 3, 4])
@pytest.mark.parametrize("d,M", [(4, 1), (8, 3), (16, 4), (32, 2), (64, 4), (128, 2)])
def test_bipartite_propagation_and_adjoint(d, M, L):
    ops = _ops()
    P, Q, _ = _graph("bip")
    U, I = P.shape[0], Q.shape[0]
    N, C = U + I, d * M
    Eu, XI = _rand(d + L, U, d), _rand(d + L + 1, I, C)
    Pd, Qd = _csr(P, C, T32), _csr(Q, C, T32)
    ws = torch.empty(ops.bipartite_workspace(U, I, d, M), dtype=torch.uint8, device=DEV)
    Eud, XId = Eu.to(DEV), XI.to(DEV)
    out, nar = _nan(N, C), _nan(N, d)
    ops.propagate_bipartite(Pd, Qd, U, I, d, M, L, Eud, XId, out, ws, narrow_out=nar)
    (ref, scale), (nref, nscale) = pm.propagate_bipartite(P, Q, U, I, d, M, L, Eu, XI)
    K = pm.chain_K(L, P, Q)
    _close("bipartite fwd", out, ref, scale, K, "bipartite Out")
    _close("bipartite fwd", nar, nref, nscale, K, "bipartite narrow_out")
    assert same_bits(Eud.cpu(), Eu) and same_bits(XId.cpu(), XI)
    out2 = _nan(N, C)
    ops.propagate_bipartite(Pd, Qd, U, I, d, M, L, Eud, XId, out2, ws)        # without narrow_out: the same Out
    assert same_bits(out, out2)
    # ---- adjoint: G is NaN off the active rows
    PTm, QTm = P.T.tocsr(), Q.T.tocsr()
    PT, QT = _csr(PTm, C, T32), _csr(QTm, C, T32)
    n_max = 100
    for count in (46, 0, n_max):
        rows, count = _active(N, U, n_max, count, seed=count + L)
        G = torch.full((N, C), NAN)
        G[torch.from_numpy(rows[:count].astype(np.int64))] = _rand(count + d, count, C)
        rows_d, seg = torch.from_numpy(rows).to(DEV), _seg(count, int((rows[:count] < U).sum()))
        Gd, H = G.to(DEV), _nan(N, d)
        ops.blocksum_rows(Gd, rows_d, seg, d, M, H)
        href, hscale = pm.blocksum_rows(G, rows, count, d, M, N)
        keep = torch.from_numpy(pm.bits_of(rows[:count], N))
        assert all_nan(H[~keep.to(DEV)])
        if count:
            _close("blocksum_rows", H[keep.to(DEV)], href[keep], hscale[keep], float(M), "blocksum_rows (node rows)")
        gXI, gEu = _nan(I, C), _nan(U, d)
        ops.propagate_bipartite_bwd(PT, QT, U, I, d, M, L, Gd, H, rows_d, seg, gXI, gEu, ws)
        (xref, xscale), (eref, escale) = pm.propagate_bipartite_bwd(PTm, QTm, U, I, d, M, L, G, H.cpu(), rows, count)
        Kb = pm.chain_K(L, PTm, QTm)
        _close("bipartite bwd", gXI, xref, xscale, Kb, "gXI count=%d" % count)
        _close("bipartite bwd", gEu, eref, escale, Kb, "gE_u count=%d" % count)
        if count == 0:
            assert not bool(gXI.any()) and not bool(gEu.any())


# ============================================================================= propagate_folded and its adjoint
@pytest.mark.parametrize("L", [1, 2, 3, 4])
@pytest.mark.parametrize("d", [4, 16, 32, 64, 128])
def test_folded_propagation_and_adjoint(d, L):
    ops = _ops()
    P, Q, A = _graph("bip")
    U, I = P.shape[0], Q.shape[0]
    N = U + I
    ATm = A.T.tocsr()
    Ad, ATd = _csr(A, d, T32), _csr(ATm, d, T32)
    ws = torch.empty(ops.folded_workspace(N, d), dtype=torch.uint8, device=DEV)
    X0 = _rand(d + L, N, d)
    X0d = X0.to(DEV)
    table, nar = _nan(N, 3 * d), _nan(N, d)
    ops.propagate_folded(Ad, U, I, d, L, X0d, table[:, :d], nar, ws)
    (oref, oscale), (nref, nscale) = pm.propagate_folded(A, U, I, d, L, X0)
    K = pm.chain_K(L, A)
    _close("folded fwd", table[:, :d], oref, oscale, K, "folded Out0")
    _close("folded fwd", nar, nref, nscale, K, "folded Narrow")
    assert all_nan(table[:, d:]), "column blocks 1 and 2 of the Out table were written"
    assert same_bits(X0d.cpu(), X0), "X0 changed"
    b_out0, b_nar = tau(K) * oscale + TINY, tau(K) * nscale + TINY
    out0_64, nar_64 = table[:, :d].double().cpu(), nar.double().cpu()
    Kb = pm.chain_K(L, ATm)
    n_max = 100
    for M in (1, 3, 4):
        rows, count = _active(N, U, n_max, 46, seed=M + L)
        dOutR = torch.full((n_max, d * M), NAN)
        dOutR[:count] = _rand(M + d, count, d * M)
        rows_d, seg = torch.from_numpy(rows).to(DEV), _seg(count, int((rows[:count] < U).sum()))
        srcA, srcB, grad = _nan(N, d), _nan(N, d), _nan(N, d)
        ops.propagate_folded_bwd(ATd, U, I, d, M, L, dOutR.to(DEV), rows_d, seg, srcA, srcB, grad, ws)
        # the source tables: H (K = M) and G (bits) on the active rows, nothing elsewhere
        G, H, Hs, keep = pm.folded_sources(dOutR, rows, count, U, N, d, M)
        keep_t = torch.from_numpy(keep)
        user = (torch.arange(N) < U).unsqueeze(1)
        a, b = srcA.cpu(), srcB.cpu()
        assert all_nan(a[~keep_t]) and all_nan(b[~keep_t]), "source rows outside the active set were written"
        h_got, g_got = torch.where(user, a, b)[keep_t], torch.where(user, b, a)[keep_t]
        _close("folded sources", h_got, torch.from_numpy(H)[keep_t], torch.from_numpy(Hs)[keep_t], float(M), "H of SrcA / SrcB")
        assert same_bits(g_got, torch.from_numpy(G)[keep_t].float()), "G of SrcA / SrcB"
        gref, gscale = pm.propagate_folded_bwd(ATm, U, I, d, M, L, None, rows, count, srcA=a, srcB=b)
        _close("folded bwd", grad, gref, gscale, Kb, "folded grad M=%d" % M)
        # prefilled form: the same tables and their bitmap
        mask = torch.from_numpy(pm.bitmap_words(keep)).to(DEV)
        grad2 = _nan(N, d)
        ops.propagate_folded_bwd(ATd, U, I, d, M, L, None, None, None, srcA, srcB, grad2, ws, active_mask=mask)
        assert same_bits(grad2, grad), "prefilled form differs"
        assert same_bits(srcA.cpu(), a) and same_bits(srcB.cpu(), b)
        # adjoint identity against the forward: <grad, X0> = <H, Nar> + <G, Out0 - Nar>, dot products in float64 from the fp32
        # outputs, tolerance = the two sides' element bounds times the other factor's magnitude
        Hz = torch.zeros(N, d, dtype=torch.float64)
        Gz = torch.zeros(N, d, dtype=torch.float64)
        Hz[keep_t], Gz[keep_t] = h_got.double(), g_got.double()
        lhs = float((grad.double().cpu() * X0.double()).sum())
        rhs = float((Hz * nar_64).sum() + (Gz * (out0_64 - nar_64)).sum())
        tol = float(((tau(Kb) * gscale + TINY) * X0.double().abs()).sum() + (b_nar * Hz.abs()).sum() + ((b_out0 + b_nar) * Gz.abs()).sum())
        WORST["adjoint identity"] = max(WORST.get("adjoint identity", 0.0), abs(lhs - rhs) / tol)
        assert abs(lhs - rhs) <= tol, ("adjoint identity", d, L, M, lhs, rhs, tol)


# ============================================================================= small kernels
@pytest.mark.parametrize("d,M", [(4, 1), (12, 3), (64, 4), (260, 2)])
def test_assemble_x0_embed_grad_and_blocksum(d, M):
    ops = _ops()
    U, I = 37, 70
    N = U + I
    ue, ie = _rand(d, U, d), _rand(d + 1, I, d)
    X0 = _nan(N, d * M)
    ops.assemble_x0(ue.to(DEV), ie.to(DEV), X0, M)
    want, _ = pm.assemble_x0(ue, ie, M)
    assert same_bits(X0.cpu(), want.float())                      # the item rows' other blocks: still NaN
    G = _rand(d + 2, N, d * M)
    gu, gi = _nan(U, d), _nan(I, d)
    ops.embed_grad(G.to(DEV), U, I, d, M, gu, gi)
    (uref, uscale), (iref, _) = pm.embed_grad(G, U, I, d, M)
    assert same_bits(gi.cpu(), iref.float())
    _close("embed_grad", gu, uref, uscale, float(M), "embed_grad users")
    seq = G[:U, :d].clone()                                        # the block order the kernel adds in: bit for bit
    for k in range(1, M):
        seq = seq + G[:U, k * d:(k + 1) * d]
    assert same_bits(gu.cpu(), seq)
    # blocksum_rows, both layouts, count < n_max
    n_max, count = 29, 23
    rows, count = _active(N, U, n_max, count, seed=d)
    rows_d, seg = torch.from_numpy(rows).to(DEV), _seg(count, int((rows[:count] < U).sum()))
    keep = torch.from_numpy(pm.bits_of(rows[:count], N))
    Gn = torch.full((N, d * M), NAN)
    Gn[keep] = _rand(d + 3, count, d * M)
    Gs = torch.full((n_max, d * M), NAN)
    Gs[:count] = _rand(d + 4, count, d * M)
    for slot_major, Gin in ((False, Gn), (True, Gs)):
        H = _nan(N, d)
        ops.blocksum_rows(Gin.to(DEV), rows_d, seg, d, M, H, slot_major=slot_major)
        href, hscale = pm.blocksum_rows(Gin, rows, count, d, M, N, slot_major=slot_major)
        assert all_nan(H.cpu()[~keep]), "rows outside the first `count` active rows were written"
        _close("blocksum_rows", H.cpu()[keep], href[keep], hscale[keep], float(M), "blocksum_rows slot_major=%s" % slot_major)


@pytest.mark.parametrize("count", [0, 5, 21])
@pytest.mark.parametrize("d,M", [(32, 1), (32, 4), (64, 1), (64, 4)])
@pytest.mark.parametrize("world", [1, 2, 4, 8])
def test_source_rows_split(world, d, M, count):
    ops = _ops()
    n_max = 21
    dOutR = torch.full((n_max, d * M), NAN)
    dOutR[:count] = _rand(world + d + M, count, d * M)
    out = _nan(world, n_max, 2 * d // world)
    ops.source_rows_split(dOutR.to(DEV), torch.tensor([count], dtype=torch.int32, device=DEV), d, M, world, out)
    ref, scale = pm.source_rows_split(dOutR, count, d, M, world)
    got = out.cpu()
    assert all_nan(got[:, count:]), "rows >= count were written"
    dl = d // world
    if count:
        _close("source_rows_split", got[:, :count, :dl], ref[:, :count, :dl], scale[:, :count, :dl], float(M), "H slices")
        assert same_bits(got[:, :count, dl:].contiguous(), ref[:, :count, dl:].float().contiguous()), "G slices"


@pytest.mark.parametrize("n,w,lds,ldd", [(5, 4, 4, 4), (37, 12, 20, 16), (300, 64, 64, 72), (70000, 64, 72, 80)])
def test_copy_cols_on_strided_windows(n, w, lds, ldd):
    """70000 x 64 is above 4096 x 256 float4: the grid-stride loop runs."""
    ops = _ops()
    src, dst = _nan(n, lds), _nan(n, ldd)
    s0, d0 = lds - w, (ldd - w) // 8 * 4
    vals = _rand(n % 97 + w, n, w)
    src[:, s0:s0 + w] = vals.to(DEV)
    ops.copy_cols(src[:, s0:s0 + w], dst[:, d0:d0 + w])
    assert same_bits(dst[:, d0:d0 + w].contiguous().cpu(), pm.copy_cols(vals)[0].float())
    assert all_nan(dst[:, :d0]) and all_nan(dst[:, d0 + w:])


def test_zz_report_the_worst_ratios():
    """Prints the worst err / tol per kernel family of this session (pytest -s shows it; the figures of the commit message)."""
    print("\nworst err / tol: " + ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))
    assert all(v <= 1.0 for v in WORST.values())
