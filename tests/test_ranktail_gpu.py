"""The evaluator's ranking tail beyond 64 ranks (csrc/eval.hip): rank_metrics_kernel at every ballot-word edge up to K = 256, the
top-K selections through score_topk at every K / mask count / catalogue size where they change form, the reference's tie order
on both sides of its switch at K = 256, and topk_merge_kernel up to its LDS limit. The references are the numpy models of
tests/ranktail_model.py (checked on the CPU by tests/test_ranktail_cpu.py) and the oracle's port. Needs a real MI355X."""
import numpy as np
import pytest
import torch

import ranktail_model as rm
from helpers import reference_lists, tie_free

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL_IDS = [1, 2, 3, 4, 5]


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


# ------------------------------------------------------------------------------------------------ a. rank_metrics_kernel
@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256])
def test_rank_metrics_at_every_ballot_word_edge(K):
    """rank_metrics_kernel against the metric model (cross-checked here with the oracle's port): K on both sides of every 64-rank
    ballot word, B = 1 / 3 / 4 / 5 / 9 and all rows (four rows share a workgroup), the id lists [1..5], [4], [5, 1] and eight ids
    with repeats; single hits at ranks 0, 62, 63, 64, 65, 127, 128, 191, 192, 255 and K - 1, no hit, all hits, hits at every
    64th rank, truth lengths 1 / K - 1 / K / K + 1 / 300, -1 ids in the tail of the list. Precision, recall, AP and MRR are IEEE
    divisions and additions: bit for bit. NDCG goes through the device's double log2: |diff| < 1e-7, the entries that are not
    bit-identical counted and printed.

    The row without truth items: a caller CAN pass one (evaluate(test_users=...) with a user absent from the test split, or an
    empty list in it: lists_csr gives an empty segment). The kernel then gives what the reference's metric.h gives -- recall and
    NDCG 0 / 0 = NaN, precision, AP and MRR 0 -- which is asserted here against the port (same NaN pattern)."""
    from elimrec_amd import ops
    from oracle import eval_oracle as ev
    rank, truth, names = rm.metric_cases(K)
    R = len(names)
    tp, ti = rm.csr(truth)
    want = rm.metrics_model(rank, tp, ti, ALL_IDS, K).reshape(R, 5, K)
    assert same_bits(ev.metrics_from_rank(rank, tp, ti, ALL_IDS, K).reshape(R, 5, K), want)
    n_ndcg = n_off = 0
    windows = [(0, R)] + [((7 * B) % (R - B), B) for B in (1, 3, 4, 5, 9)]
    for ids in (ALL_IDS, [4], [5, 1], [3, 3, 1, 4, 2, 4, 5, 2]):
        for at, B in windows:
            ptr, items = rm.csr(truth[at:at + B])
            if items.size == 0:
                items = np.zeros(1, np.int32)
            out = torch.full((B, len(ids) * K), -7.0, device=DEV)
            ops.rank_metrics(_t(rank[at:at + B]), _t(ptr), _t(items), ids, out)
            got = out.cpu().numpy().reshape(B, len(ids), K)
            for m, mid in enumerate(ids):
                ref = want[at:at + B, mid - 1]
                if mid != 4:
                    assert same_bits(got[:, m], ref), (K, ids, at, B, mid)
                    continue
                nan = np.isnan(ref)
                assert np.array_equal(np.isnan(got[:, m]), nan), (K, ids, at, B)
                diff = np.abs(got[:, m][~nan] - ref[~nan])
                off = int((got[:, m][~nan].view(np.uint32) != ref[~nan].view(np.uint32)).sum())
                n_ndcg += diff.size
                n_off += off
                print("K=%d ids=%s rows %d..%d: NDCG max |diff| %.3g, %d of %d not bit-identical" % (K, ids, at, at + B, diff.max() if diff.size else 0.0, off, diff.size))
                assert diff.size == 0 or diff.max() < 1e-7, (K, ids, at, B, diff.max())
    print("K=%d: NDCG entries not bit-identical: %d of %d" % (K, n_off, n_ndcg))


def test_rank_metrics_refuses_k_outside_1_to_256():
    from elimrec_amd import ops
    tp, ti = rm.csr([[1, 2], [3]])
    for K in (257, 0):
        out = torch.full((2, 5 * max(K, 1)), float("nan"), device=DEV)
        rank = torch.zeros(2, K, dtype=torch.int32, device=DEV)
        with pytest.raises(RuntimeError, match="rank_metrics"):
            ops.rank_metrics(rank, _t(tp), _t(ti), ALL_IDS, out)
        assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------------ b. selection
U, B, S = rm.SEL_U, rm.SEL_B, rm.SEL_S


class _Scorer(object):
    """score_topk on one table at one (recdim, catalogue) shape, rubi / TIE."""

    def __init__(self, Y, I, d):
        self.Y, self.I, self.d = _t(Y), I, d
        self.users = _t(rm.SEL_USERS.astype(np.int64))

    def __call__(self, K=0, scores=None, lists=False, mask=None, tie_order="id"):
        from elimrec_amd import ops
        ws = torch.empty(ops.score_workspace(B, U, self.I, S, max(K, 1), topk_only=scores is None, d=self.d), dtype=torch.uint8, device=DEV)
        idx = torch.full((B, K), -5, dtype=torch.int32, device=DEV) if lists else None
        val = torch.full((B, K), float("nan"), device=DEV) if lists else None
        ptr, items = mask if mask is not None else (None, None)
        ops.score_topk(self.Y, U, self.I, self.users, self.d, S, 0b111, "rubi", "TIE", ws, scores=scores, K=K if lists else 0,
                       topk_idx=idx, topk_val=val, train_ptr=ptr, train_items=items, tie_order=tie_order)
        return (idx.cpu().numpy(), val.cpu().numpy()) if lists else None


def _masked_case(scorer, raw, K):
    """The mask lists of one K on the device, and the masked score matrix the same call shape returns."""
    I = scorer.I
    lists, kinds, short = rm.mask_cases(raw, K)
    ptr, items = rm.csr(lists)
    mask = (_t(ptr), _t(items))
    ref = torch.empty(B, I, device=DEV)
    scorer(scores=ref, mask=mask)
    sc = ref.cpu().numpy()
    gone = np.zeros((B, I), bool)
    for b, x in enumerate(lists):
        gone[b, x] = True
    assert np.array_equal(sc == -np.inf, gone) and np.array_equal(sc[~gone], raw[~gone])
    return lists, kinds, short, mask, ref, sc, gone


def _check_lists(idx, val, sc, gone, short, K, what):
    want_i, want_v = rm.stable_topk(sc, K)
    for b in range(B):
        if b not in short:
            assert np.array_equal(idx[b], want_i[b]), (what, b, np.flatnonzero(idx[b] != want_i[b])[:5])
            assert np.array_equal(val[b], want_v[b]), (what, b)
            continue
        n = int((~gone[b]).sum())
        assert n < K
        assert np.array_equal(idx[b, :n], want_i[b, :n]) and np.array_equal(val[b, :n], want_v[b, :n]), (what, b, "prefix")
        assert (val[b, n:] == -np.inf).all(), (what, b, "tail values")
        tail = idx[b, n:]
        assert ((tail == -1) | ((tail >= 0) & gone[b][np.maximum(tail, 0)])).all(), (what, b, "tail ids", tail[:8])


@pytest.mark.parametrize("d,I,Ks", rm.SEL_SHAPES, ids=["d64-I3000", "d48-I3000", "d64-I16400", "d64-I33000"])
def test_selection_equals_the_stable_sort_at_every_form_switch(d, I, Ks):
    """score_topk's lists against the stable sort (score desc, id asc) of the masked score matrix the same call shape returns,
    ids and values exact, for every row with at least K unmasked items; 37 of 60 users, three heads.
    K = 63 .. 513 (and 1024 at recdim 48) at one chunk, 64 / 256 / 257 at two and three chunks: across 64 coarse | 256 fine groups,
    across the last threshold (K + n_masked = 255 / 256 / 257: the K-round sweep), across K = 256 (tile-guided | private matrix
    with topk_select_kernel), across 2 K = 1024 (topk_kernel alone) and, on the nine-row table, across TK_CAP candidates.
    recdim 48 = the generic scorer without tile maxima. Lists alone (the chunked running form beyond 16 384 items) and lists
    together with the caller's matrix. Tables: continuous, nine distinct item rows, 2 K equal scores across rank K. Mask lists
    per row (ranktail_model.mask_cases): none, the row's own top m (the masked items own the group maxima), a repeated id, all
    but 4 / K - 1 / K, only the last launch's items, only the pilot chunk's, a few then the last launch's.
    Rows with fewer than K unmasked items: the finite prefix is the model's, every tail value is -inf and every tail id is -1 or
    one of the row's masked ids (the sweep lists masked ids, the running form leaves -1), never an unmasked id."""
    from elimrec_amd import ops
    ops.score_range_violations(reset=True)
    for table in rm.SEL_TABLES:
        scorer = raw = None
        for K in Ks:
            if scorer is None or table == "tieblock":
                scorer = _Scorer(rm.selection_table(table, I, d, K), I, d)
                raw_d = torch.empty(B, I, device=DEV)
                scorer(scores=raw_d)
                raw = raw_d.cpu().numpy()
            lists, kinds, short, mask, ref, sc, gone = _masked_case(scorer, raw, K)
            idx, val = scorer(K=K, lists=True, mask=mask)
            _check_lists(idx, val, sc, gone, short, K, (table, K, "lists"))
            both = torch.empty(B, I, device=DEV)
            idx, val = scorer(K=K, scores=both, lists=True, mask=mask)
            assert torch.equal(both, ref), (table, K)
            _check_lists(idx, val, sc, gone, short, K, (table, K, "lists+matrix"))
    assert ops.score_range_violations(reset=True) == 0


@pytest.mark.parametrize("I", [3000, 16400, 33000])
def test_reference_tie_order_on_both_sides_of_k_256(I):
    """tie_order = "reference" inside the scoring call at K = 255 / 256 (tile-guided; beyond one chunk the heap is carried from
    launch to launch and its top published as the store threshold) and K = 257 / 1024 (ref_order_kernel<false> over the masked
    private matrix): the lists and their scores equal the oracle's std::partial_sort_copy of the masked matrix the same call
    shape returns, every row, short ones included. The tie rule is exercised on every row of the nine-row table (K + 1 > 9
    values among nine: pigeonhole), which sets the minimum asserted."""
    from elimrec_amd import ops
    ops.score_range_violations(reset=True)
    d, Ks = 64, (255, 256, 257, 1024)
    n_tied = 0
    for table in rm.SEL_TABLES:
        scorer = raw = None
        for K in Ks:
            if scorer is None or table == "tieblock":
                scorer = _Scorer(rm.selection_table(table, I, d, K), I, d)
                raw_d = torch.empty(B, I, device=DEV)
                scorer(scores=raw_d)
                raw = raw_d.cpu().numpy()
            lists, kinds, short, mask, ref, sc, gone = _masked_case(scorer, raw, K)
            want = reference_lists(sc, K)
            n_tied += int((~tie_free(sc, K)).sum())
            idx, val = scorer(K=K, lists=True, mask=mask, tie_order="reference")
            bad = np.flatnonzero((idx != want).any(1))
            assert bad.size == 0, (table, K, bad, [kinds[b] for b in bad])
            assert np.array_equal(val, np.take_along_axis(sc, want.astype(np.int64), 1)), (table, K)
    assert n_tied >= B * len(Ks)
    assert ops.score_range_violations(reset=True) == 0


# ------------------------------------------------------------------------------------------------ c. topk_merge_kernel
def _merge_rows(n, K, seed):
    """Five rows of n candidates: plain; -1 ids at the front and scattered; whole lists of -1 and fewer than K valid ids; eight
    score levels with the equal scores' ids spread over the lists; all scores equal. Valid ids are distinct within a row."""
    rng = np.random.default_rng(seed)
    val = rng.random((5, n)).astype(np.float32)
    idx = np.stack([rng.permutation(4 * n)[:n] for _ in range(5)]).astype(np.int32)
    idx[1, :n // 3] = -1
    idx[1, rng.random(n) < 0.2] = -1
    keep = rng.permutation(n)[:max(0, min(K - 1, n) // 2)]
    row = np.full(n, -1, np.int32)
    row[keep] = idx[2, keep]
    idx[2] = row
    val[3] = rng.integers(0, 8, size=n).astype(np.float32) / 8
    val[4] = 0.25
    return val, idx


@pytest.mark.parametrize("K", [1, 10, 256, 300])
def test_topk_merge_up_to_its_lds_limit(K):
    """ops.topk_merge against merge_model, ids and values exact: n_cand = K, 2 K, 8 K, 8192 and 8193 (the two sides of the 64 KB
    default of dynamic LDS) and 20 480 (the limit exactly); -1 ids, short rows (tail -1 / -inf), ties resolved by ascending id
    across lists, with and without out_val. One candidate more is refused and the outputs stay as they were."""
    from elimrec_amd import ops
    for n in sorted({K, 2 * K, 8 * K, 8192, 8193, rm.MERGE_MAX}):
        val, idx = _merge_rows(n, K, 100 * K + n % 97)
        want_i, want_v = rm.merge_model(val, idx, K)
        assert (want_i[2] == -1).sum() >= 1 and (want_i[0] >= 0).all()
        vd, id_ = _t(val), _t(idx)
        oi = torch.full((5, K), -5, dtype=torch.int32, device=DEV)
        ov = torch.full((5, K), float("nan"), device=DEV)
        ops.topk_merge(vd, id_, K, oi, ov)
        assert np.array_equal(oi.cpu().numpy(), want_i), (K, n, np.flatnonzero((oi.cpu().numpy() != want_i).any(1)))
        assert np.array_equal(ov.cpu().numpy(), want_v), (K, n)
        oi2 = torch.full((5, K), -5, dtype=torch.int32, device=DEV)
        ops.topk_merge(vd, id_, K, oi2)
        assert np.array_equal(oi2.cpu().numpy(), want_i), (K, n, "no out_val")
    n = rm.MERGE_MAX + 1
    oi = torch.full((5, K), -5, dtype=torch.int32, device=DEV)
    ov = torch.full((5, K), float("nan"), device=DEV)
    with pytest.raises(RuntimeError, match="exceed the LDS budget"):
        ops.topk_merge(torch.zeros(5, n, device=DEV), torch.zeros(5, n, dtype=torch.int32, device=DEV), K, oi, ov)
    assert bool((oi == -5).all()) and bool(torch.isnan(ov).all())
