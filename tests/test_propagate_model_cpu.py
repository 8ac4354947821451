"""The float64 model and the bound of tests/propagate_model.py, checked without a GPU and without a project kernel:

1. self-consistency on the golden fixtures (ml3: symmetric 'pre' adjacency, gcmc: Q != P^T): the bipartite and folded models equal
   the plain 1/(L+1) sum_k A^k X0 of the assembled table to 1e-12, their backward models the transpose product;
2. the bound holds for fp32 arithmetic: a hop emulated in numpy float32 in the two orders the kernels use (one fma chain in column
   order; threshold-sized segment partials combined in the combine_split_row order) stays inside tau(K) for L = 1..4 on the ladder
   graph -- measured against the float64 model, never against a kernel; the worst error / bound is printed;
3. the bound rejects mutants: each listed defect, applied to the float64 model, moves some element by more than 100 x its bound.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import propagate_model as pm
from fp64_tools import TINY, tau, within
from helpers import load_golden

F32, F64 = np.float32, np.float64


def _same(a, b, what):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    assert a.shape == b.shape, what
    assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max()), (what, float(np.abs(a - b).max()))


def _plain(Ad, X, L):
    """1/(L+1) sum_k A^k X with a dense float64 matrix."""
    acc, x = X.copy(), X
    for _ in range(L):
        x = Ad @ x
        acc = acc + x
    return acc / (L + 1.0)


# ============================================================================= 1. self-consistency on the golden fixtures
@pytest.mark.parametrize("L", [1, 2, 3, 4])
@pytest.mark.parametrize("name", ["ml3", "gcmc"])
def test_models_equal_the_plain_product_on_the_fixtures(name, L):
    from elimrec_amd.model import create_adj_mat
    g = load_golden(name)
    U, I = int(g["num_users"]), int(g["num_items"])
    N = U + I
    A = create_adj_mat(g["train_u"], g["train_i"], U, I, str(g["adj_type"])).tocsr()
    assert abs(A[:U, :U]).sum() == 0 and abs(A[U:, U:]).sum() == 0           # no diagonal blocks
    P, Q = A[:U, U:].tocsr(), A[U:, :U].tocsr()
    Ad = A.toarray().astype(F64)
    Eu, Ei = g["init/embedding_user.weight"].astype(F64), g["init/embedding_item.weight"].astype(F64)
    d, M = Eu.shape[1], 3
    rs = np.random.RandomState(L)
    XI = np.concatenate([Ei, rs.randn(I, d * (M - 1))], 1)
    X0 = np.concatenate([np.tile(Eu, (1, M)), XI])
    want = _plain(Ad, X0, L)
    (out, _), (nar, _) = pm.propagate_bipartite(P, Q, U, I, d, M, L, Eu, XI)
    _same(out, want, "bipartite Out")
    _same(nar, _plain(Ad, np.concatenate([Eu, np.zeros((I, d))]), L), "bipartite narrow_out")
    _same(pm.propagate(A, X0, L)[0], want, "propagate")
    X0f = np.concatenate([Eu, Ei])
    (out0, _), (nar_f, _) = pm.propagate_folded(A, U, I, d, L, X0f)
    _same(out0, want[:, :d], "folded Out0")
    _same(nar_f, nar, "folded Narrow")
    # ---- backward: sparse G, NaN off the active rows
    act = np.sort(rs.choice(N, size=23, replace=False))
    act[0], act[-1] = 0, N - 1
    act = np.unique(np.concatenate([act, [U - 1, U]]))
    G = np.full((N, d * M), np.nan)
    G[act] = rs.randn(len(act), d * M)
    Gz = np.nan_to_num(G, nan=0.0)
    Hz = Gz.reshape(N, M, d).sum(1)
    full = _plain(Ad.T, Gz, L)
    (gXI, _), (gEu, _) = pm.propagate_bipartite_bwd(P.T.tocsr(), Q.T.tocsr(), U, I, d, M, L, G,
                                                    np.where(np.isnan(G[:, :d]), np.nan, Hz), act, len(act))
    _same(gXI, full[U:], "bipartite gXI")
    _same(gEu, full[:U].reshape(U, M, d).sum(1), "bipartite gE_u")
    n_max = len(act) + 5
    dOutR = np.full((n_max, d * M), np.nan)
    dOutR[:len(act)] = G[act]
    rows = np.concatenate([act, np.zeros(5, np.int64)])
    grad, _ = pm.propagate_folded_bwd(A.T.tocsr(), U, I, d, M, L, dOutR, rows, len(act))
    _same(grad, np.concatenate([_plain(Ad.T, Hz, L)[:U], _plain(Ad.T, Gz[:, :d], L)[U:]]), "folded grad")
    # the adjoint identity the GPU test uses: <grad, X0> = <H, Nar> + <G, Out0 - Nar>
    lhs = float((grad.numpy() * X0f).sum())
    rhs = float((Hz * nar_f.numpy()).sum() + (Gz[:, :d] * (out0.numpy() - nar_f.numpy())).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))


def test_the_ladder_graphs_are_what_the_tests_assume():
    T = pm.LADDER_T
    for m in (pm.ladder_square("long"), pm.ladder_square("empty"), pm.ladder_rect()):
        lens = pm.row_lengths(m)
        assert list(lens[:2 * T + 3]) == list(range(2 * T + 3))
        assert {8 * T, 8 * T + 1, 16 * T + 5, pm.LONG_AT_T4} <= set(lens.tolist()) and pm.LONG_AT_T4 >= 115 * 4
        assert m.shape[0] % 4 != 0                                     # no multiple of 4 * (64 / LPR), LPR = 4 .. 64
        assert np.all(np.abs(m.data) >= 0.1) and np.all(np.abs(m.data) <= 1.1) and (m.data < 0).any() and (m.data > 0).any()
        for r in range(m.shape[0]):
            c = m.indices[m.indptr[r]:m.indptr[r + 1]]
            assert np.all(np.diff(c) > 0)
            assert len(c) < 2 or (c[0] == 0 and c[-1] == m.shape[1] - 1)
    assert pm.row_lengths(pm.ladder_square("long"))[-1] == 16 * T + 5 and pm.row_lengths(pm.ladder_square("empty"))[-1] == 0
    assert pm.ladder_rect().shape[0] != pm.ladder_rect().shape[1]
    P, Q, A = pm.ladder_bipartite()
    U = P.shape[0]
    lens = pm.row_lengths(A)
    assert U % 32 != 0 and lens[U - 1] > 0 and lens[U] > 0 and lens[0] == 0 and lens[-1] == 0 and A.shape[0] % 4 != 0
    assert abs(Q - P.T).sum() > 0
    for Tn in (T, 4):
        assert pm.row_lengths(pm.ladder_all_long(37, 300, T=Tn)).min() > Tn
    # >= 8 segments per lane group at threshold 4, LPR 4
    assert -(-(-(-pm.LONG_AT_T4 // 4)) // 16) >= 8


# ============================================================================= 2. the bound holds for fp32 arithmetic
def _fma_items(col, val, beg, end, X):
    """acc = fma(val[j], X[col[j]], acc) for j in [beg, end) in order, from zero, for many items at once. The product of two
    float32 is exact in float64, so each step is one rounding (up to a rare double rounding), as an fma."""
    acc = np.zeros((len(beg), X.shape[1]), F32)
    if len(beg) == 0:
        return acc
    for j in range(int((end - beg).max())):
        live = np.nonzero(beg + j < end)[0]
        idx = beg[live] + j
        acc[live] = (acc[live].astype(F64) + val[idx].astype(F64)[:, None] * X[col[idx]].astype(F64)).astype(F32)
    return acc


def _hop_f32(A, X, threshold=None, rpw=16):
    """One hop in float32. threshold None: every row one chain. Otherwise rows longer than it are cut into segments of that many
    entries, each summed as a chain, and the partial rows are added as combine_split_row adds them: `rpw` lane groups take
    contiguous runs of ceil(n_seg / rpw) segments each in order, the group sums are added in group order."""
    ptr, col, val = A.indptr.astype(np.int64), A.indices, A.data.astype(F32)
    lens = np.diff(ptr)
    if threshold is None:
        return _fma_items(col, val, ptr[:-1], ptr[1:], X)
    short = np.nonzero(lens <= threshold)[0]
    out = np.zeros((A.shape[0], X.shape[1]), F32)
    out[short] = _fma_items(col, val, ptr[short], ptr[short + 1], X)
    for r in np.nonzero(lens > threshold)[0]:
        beg = np.arange(ptr[r], ptr[r + 1], threshold)
        part = _fma_items(col, val, beg, np.minimum(beg + threshold, ptr[r + 1]), X)
        per = -(-len(beg) // rpw)
        tot = None
        for q in range(rpw):
            acc = np.zeros(X.shape[1], F32)
            for s in range(min(q * per, len(beg)), min(q * per + per, len(beg))):
                acc = acc + part[s]
            tot = acc if tot is None else tot + acc
        out[r] = tot
    return out


def _propagate_f32(A, X0, L, threshold, rpw):
    """ops.propagate's arithmetic: hop k folds X^k into the running sum, the last hop applies 1/(L+1)."""
    x, out = X0, X0
    for k in range(1, L + 1):
        x = _hop_f32(A, x, threshold, rpw)
        out = (out + x) * (F32(1.0) / F32(L + 1) if k == L else F32(1.0))
    return out


@pytest.mark.parametrize("order", ["chain", "segments T=32", "segments T=4", "segments T=4 one group"])
def test_fp32_arithmetic_stays_inside_the_bound(order):
    A = pm.ladder_square("long")
    threshold, rpw = {"chain": (None, 1), "segments T=32": (32, 16), "segments T=4": (4, 16), "segments T=4 one group": (4, 1)}[order]
    X0 = np.random.RandomState(7).randn(A.shape[1], 8).astype(F32)
    # one hop, a bound per row
    r = _hop_f32(A, X0, threshold, rpw)
    (ref, scale), _ = pm.hop(A, X0)
    tol = tau(pm.hop_K(A)) * scale + TINY
    worst = {"hop": float(((torch.from_numpy(r).double() - ref).abs() / tol).max())}
    assert bool(within(torch.from_numpy(r), ref, scale, pm.hop_K(A)).all())
    assert r.dtype == F32
    for L in (1, 2, 3, 4):
        got = _propagate_f32(A, X0, L, threshold, rpw)
        assert got.dtype == F32
        ref, scale = pm.propagate(A, X0, L)
        K = pm.chain_K(L, A)
        worst["L=%d" % L] = float(((torch.from_numpy(got).double() - ref).abs() / (tau(K) * scale + TINY)).max())
        assert bool(within(torch.from_numpy(got), ref, scale, K).all()), (order, L, worst)
    print("\nfp32 emulation, %s: worst error / bound " % order + ", ".join("%s %.2e" % kv for kv in sorted(worst.items())))
    assert max(worst.values()) < 1.0


# ============================================================================= 3. the bound rejects mutants
def _rejected(mut, ref, scale, K):
    """Some element moved by more than 100 x its bound, and `within` fails there."""
    mut = mut if isinstance(mut, torch.Tensor) else torch.from_numpy(np.asarray(mut, F64))
    far = (mut - ref).abs() > 100.0 * (tau(K) * scale + TINY)
    ok = within(mut, ref, scale, K)
    return bool(far.any()) and not bool(ok[far].any())


def _without(A, r, j0, j1):
    """A without entries [j0, j1) of row r."""
    A = A.tolil(copy=True)
    cols = A.rows[r][j0:j1]
    for c in cols:
        A[r, c] = 0
    A = A.tocsr()
    A.eliminate_zeros()
    return A


def _ladder_case(W=8):
    A = pm.ladder_square("long")
    X = np.random.RandomState(11).randn(A.shape[1], W)
    return A, X


def test_mutant_last_neighbour_of_a_short_row_dropped():
    A, X = _ladder_case()
    (ref, scale), _ = pm.hop(A, X)
    for r in (1, 9, 32):
        assert pm.row_lengths(A)[r] == r
        (mut, _), _ = pm.hop(_without(A, r, r - 1, r), X)
        assert _rejected(mut, ref, scale, pm.hop_K(A))


def test_mutant_neighbour_dropped_at_a_segment_boundary_and_segment_skipped():
    A, X = _ladder_case()
    T = pm.LADDER_T
    (ref, scale), _ = pm.hop(A, X)
    K = pm.hop_K(A)
    # rows cut at T (T+1: a last segment of one entry; 2T+1, 2T+2) and at 4 (9 = 4 + 4 + 1): a neighbour on either side of a cut
    for r, j in ((T + 1, T), (T + 1, T - 1), (2 * T + 1, T), (2 * T + 1, 2 * T), (2 * T + 2, 2 * T - 1), (9, 4), (9, 8)):
        assert pm.row_lengths(A)[r] == r
        (mut, _), _ = pm.hop(_without(A, r, j, j + 1), X)
        assert _rejected(mut, ref, scale, K), (r, j)
    # a whole segment missing from the combine: the middle one, the one-entry tail, and one of the 17 of the 16T+5 row
    long_row = 2 * T + 3 + 2
    assert pm.row_lengths(A)[long_row] == 16 * T + 5
    for r, j0, j1 in ((2 * T + 1, T, 2 * T), (2 * T + 1, 2 * T, 2 * T + 1), (long_row, T, 2 * T), (long_row, 16 * T, 16 * T + 5)):
        (mut, _), _ = pm.hop(_without(A, r, j0, j1), X)
        assert _rejected(mut, ref, scale, K), (r, j0, j1)


def test_mutant_add1_read_on_a_row_whose_mask_bit_is_clear():
    A, X = _ladder_case()
    n = A.shape[0]
    add1 = np.random.RandomState(12).randn(n, X.shape[1])
    mask = np.arange(n) % 3 != 1
    _, (ref, scale) = pm.hop(A, X, add1=add1, add1_mask=mask, scale=0.25)
    for r in (1, 31, 34, n - 2):                                       # bits clear, next to word boundaries too
        assert not mask[r]
        m2 = mask.copy()
        m2[r] = True
        _, (mut, _) = pm.hop(A, X, add1=add1, add1_mask=m2, scale=0.25)
        assert _rejected(mut, ref, scale, pm.hop_K(A))


def test_mutant_source_row_outside_the_bitmap_read():
    A, X = _ladder_case()
    src = np.arange(A.shape[1]) % 5 == 0
    src[0], src[-1] = True, False                                      # column 0 is in every row of >= 2 entries, the last is too
    _, (ref, scale) = pm.hop(A, X, src_mask=src, scale=1.0)
    for c in (A.shape[1] - 1, 31, 33):
        assert not src[c]
        s2 = src.copy()
        s2[c] = True
        _, (mut, _) = pm.hop(A, X, src_mask=s2, scale=1.0)
        assert _rejected(mut, ref, scale, pm.hop_K(A))
    Xn = X.copy()
    Xn[~src] = np.nan                                                  # and the model itself never reads them
    _, (again, _) = pm.hop(A, Xn, src_mask=src)
    assert torch.equal(again, ref)


def test_mutant_addn_broadcast_with_the_wrong_block_period():
    A, X = _ladder_case(W=32)
    addN = np.random.RandomState(13).randn(A.shape[0], 16)
    _, (ref, scale) = pm.hop(A, X, addN=addN)
    _, (mut, _) = pm.hop(A, X, addN=addN[:, :8])                       # period 8 instead of 16
    assert _rejected(mut, ref, scale, pm.hop_K(A))


# The L-hop mutants run on the signed ladder for L <= 3 and on its magnitudes (|A|, |x0|) for every L: with weights of both signs
# and rows of hundreds of entries |A|^4 |x0| is hundreds of times |A^4 x0|, so at L = 4 no defect of the size of the value itself
# reaches 100 x the bound there; without cancellation scale = |value| and the bound is the relative tau(K).
CHAIN_CASES = [(L, signed) for L in (1, 2, 3, 4) for signed in (True, False) if signed is False or L <= 3]


def _folded_case(L, signed, d=8, M=3):
    P, Q, A = pm.ladder_bipartite()
    U, I = P.shape[0], Q.shape[0]
    rs = np.random.RandomState(20 + L)
    X0 = rs.randn(U + I, d)
    if not signed:
        P, Q, A, X0 = abs(P), abs(Q), abs(A), np.abs(X0)
    act = np.unique(np.concatenate([[0, 31, 32, U - 1, U, U + I - 1], rs.choice(U + I, 40, replace=False)]))
    dOutR = rs.randn(len(act), d * M) if signed else rs.rand(len(act), d * M)
    return P, Q, A, U, I, d, M, X0, act, dOutR


@pytest.mark.parametrize("L,signed", CHAIN_CASES)
def test_mutant_source_tables_swapped(L, signed):
    P, Q, A, U, I, d, M, X0, act, dOutR = _folded_case(L, signed)
    AT = A.T.tocsr()
    K = pm.chain_K(L, AT)
    ref, scale = pm.propagate_folded_bwd(AT, U, I, d, M, L, dOutR, act, len(act))
    G, H, _, _ = pm.folded_sources(dOutR, act, len(act), U, U + I, d, M)
    srcA, srcB = np.concatenate([H[:U], G[U:]]), np.concatenate([G[:U], H[U:]])
    same = pm.horner_adjoint(sp.csr_matrix(AT, dtype=F64), srcA, srcB, L)
    assert np.abs(same - ref.numpy()).max() <= 1e-12 * np.abs(same).max()
    mut = pm.horner_adjoint(sp.csr_matrix(AT, dtype=F64), srcB, srcA, L)          # parity
    assert _rejected(mut, ref, scale, K)


@pytest.mark.parametrize("L,signed", CHAIN_CASES)
def test_mutants_of_the_shared_part(L, signed):
    P, Q, A, U, I, d, M, X0, act, dOutR = _folded_case(L, signed)
    K = pm.chain_K(L, A)
    _, (ref, scale) = pm.propagate_folded(A, U, I, d, L, X0)
    xs = pm.chain(sp.csr_matrix(A, dtype=F64), X0, L)
    assert np.abs(pm.narrow_of_chain(xs, U, L) - ref.numpy()).max() <= 1e-12
    for shifted in (U - 1, U + 1):                                     # the acc2 row range off by one at row U
        assert _rejected(pm.narrow_of_chain(xs, shifted, L), ref, scale, K), shifted
    for side in (slice(0, U), slice(U, U + I)):                        # 1/(L+1) of the last visit of a side missing
        mut = ref.clone()
        mut[side] *= (L + 1.0)
        assert _rejected(mut, ref, scale, K)


@pytest.mark.parametrize("L,signed", [(3, True), (3, False), (4, False)])
def test_mutant_ping_pong_buffer_of_hop_k_minus_2_read(L, signed):
    A, X = _ladder_case()
    if not signed:
        A, X = abs(A), np.abs(X)
    ref, scale = pm.propagate(A, X, L)
    A64 = sp.csr_matrix(A, dtype=F64)
    for k in range(3, L + 1):
        xs = [X]
        for j in range(1, L + 1):
            xs.append(A64 @ (xs[j - 2] if j == k else xs[j - 1]))
        assert _rejected(sum(xs) / (L + 1.0), ref, scale, pm.chain_K(L, A)), k
