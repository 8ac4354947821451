"""The models of the ranking tail (tests/ranktail_model.py) and the case lists of tests/test_ranktail_gpu.py, checked without a
GPU: the metric model against the oracle's port (and the reference's compiled code where it was built), the cases' sensitivity to
the errors a ballot-word kernel can make, and the proof that the selection cases reach every branch of topk_tiles_kernel."""
import numpy as np
import pytest
import torch

import ranktail_model as rm
import score_model as sm
from helpers import ROOT  # noqa: F401  (puts the repository root on sys.path)

METRIC_KS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)
ALL_IDS = [1, 2, 3, 4, 5]


def same_bits(a, b):
    """Equal NaN pattern and equal bits everywhere else."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


@pytest.fixture(scope="module")
def metric_refs():
    out = {}
    for K in METRIC_KS:
        rank, truth, names = rm.metric_cases(K)
        tp, ti = rm.csr(truth)
        out[K] = (rank, truth, names, tp, ti, rm.metrics_model(rank, tp, ti, ALL_IDS, K))
    return out


def test_metric_model_equals_the_oracle_port_bit_for_bit(metric_refs):
    """Two independent statements of metric.h:17-106 -- the C port and the numpy loops -- on every row of the GPU test: the same
    bits for all five metrics (NDCG too: both run the host's log2), the same NaN pattern on the row without truth items."""
    from oracle import eval_oracle as ev
    for K, (rank, truth, names, tp, ti, want) in metric_refs.items():
        got = ev.metrics_from_rank(rank, tp, ti, ALL_IDS, K)
        for r, name in enumerate(names):
            assert same_bits(got[r], want[r]), (K, name)
        empty = names.index("empty-truth")
        row = want[empty].reshape(5, K)
        assert np.isnan(row[1]).all() and np.isnan(row[3]).all() and not np.isnan(row[[0, 2, 4]]).any() and not row[[0, 2, 4]].any()


def test_metric_model_equals_the_references_compiled_code(metric_refs):
    """Where oracle/_ref was built: score rows whose stable order is tie-free and IS the case's list, ranked and scored by the
    reference's own evaluate.h / metric.h."""
    from oracle import eval_oracle as ev
    if ev.ref_lib() is None:
        pytest.skip("oracle/_ref/libref_eval.so was not built")
    for K, (rank, truth, names, tp, ti, want) in metric_refs.items():
        rows = [r for r in range(len(names)) if (rank[r] >= 0).all()]
        sc = np.zeros((len(rows), 4096), np.float32)
        for k, r in enumerate(rows):
            rest = np.setdiff1d(np.arange(4096), rank[r])
            sc[k, rest] = np.linspace(0.1, 0.4, len(rest), dtype=np.float32)
            sc[k, rank[r]] = np.linspace(0.9, 0.5, K, dtype=np.float32)
        tp2, ti2 = rm.csr([truth[r] for r in rows])
        res, topk = ev.evaluate_matrix(sc, tp2, ti2, ALL_IDS, K, use_ref=True)
        assert np.array_equal(topk, rank[rows]), K
        assert same_bits(res, want[rows]), K


def test_metric_cases_tell_the_model_from_its_mutants(metric_refs):
    """Each of the errors a kernel with one 64-bit ballot per 64 ranks can make changes the model's output on the case list:
    hits at ranks >= 64 lost, the hit at a rank 64 c lost, the iDCG limit min(i + 1, truth_len) taken as i + 1, recall divided
    by K."""
    for K, (rank, truth, names, tp, ti, want) in metric_refs.items():
        if K > 64:
            cut = rank.copy()
            cut[:, 64:] = -1
            assert not same_bits(rm.metrics_model(cut, tp, ti, ALL_IDS, K), want), K
            for m in range(5):         # every metric sees it
                assert not same_bits(rm.metrics_model(cut, tp, ti, [m + 1], K), want[:, m * K:(m + 1) * K].reshape(len(names), K)), (K, m)
            edge = rank.copy()
            edge[:, 64::64] = -1
            assert not same_bits(rm.metrics_model(edge, tp, ti, ALL_IDS, K), want), K
        if K > 1:
            nd = np.stack([rm.ndcg_curve(rm.hit_flags(rank[r], truth[r]), K) for r in range(len(names))])
            assert not same_bits(nd, want[:, 3 * K:4 * K]), K
            rc = np.stack([rm.recall_curve(rm.hit_flags(rank[r], truth[r]), K) for r in range(len(names))])
            assert not same_bits(rc, want[:, K:2 * K]), K


def test_truth_csr_builder_drops_duplicates():
    """rank_metrics_kernel divides by the LENGTH of the truth list where the reference counts distinct ids (unordered_set): the
    evaluator and the reports build it with lists_csr(unique=True), which must leave each id once, in ascending order -- a
    duplicate in the test split then counts once in recall and in the iDCG limit, as in the reference. A user absent from the
    table gets an empty list (the row whose recall / NDCG are NaN)."""
    from elimrec_amd.reports import lists_csr
    table = {3: [7, 2, 7, 9, 2], 5: [4], 8: []}
    ptr, items = lists_csr([5, 3, 11, 8], table, "cpu", unique=True)
    assert ptr.tolist() == [0, 1, 4, 4, 4] and items.tolist() == [4, 2, 7, 9]
    assert ptr.dtype == torch.int64 and items.dtype == torch.int32
    ptr, items = lists_csr([3], table, "cpu", unique=False)          # the train mask keeps the list as it is
    assert ptr.tolist() == [0, 5] and items.tolist() == [7, 2, 7, 9, 2]
    # what the duplicate would cost: recall over the list's length is not recall over the distinct ids
    rank = np.array([[7, 1, 2, 0]], np.int32)
    dup = rm.metrics_model(rank, [0, 5], [7, 2, 7, 9, 2], [2], 4)
    uniq = rm.metrics_model(rank, [0, 3], [2, 7, 9], [2], 4)
    assert dup[0, 3] == np.float32(2 / 5) and uniq[0, 3] == np.float32(2 / 3)


# ------------------------------------------------------------------------------------------------ selection
def _scores(Y, d):
    """The float64 model of predict() (rubi / TIE) on the table, rounded to float32: the scores the device's differ from by 1e-7."""
    Yt = torch.from_numpy(Y).double()
    users = torch.from_numpy(rm.SEL_USERS)
    return sm.score_model(Yt, rm.SEL_U, users, d, rm.SEL_S, 0b111, "rubi", "TIE").float().numpy()


def _tile_max(row):
    pad = (-len(row)) % rm.TI
    return np.concatenate([row, np.full(pad, -np.inf, np.float32)]).reshape(-1, rm.TI).max(1)


def test_selection_cases_reach_every_branch_of_the_tile_guided_selection():
    """selection_walk over the rows of the GPU test's tile-guided shapes (recdim 64, K <= 256): the whole-catalogue form at
    I = 3000 and with the caller's matrix, the running form chunk by chunk at 16 400 and 33 000 (floor = the exact K-th best of
    the chunks before). Among them: both rankings, K + n_masked on the three sides of the last threshold, more candidates than
    the LDS pool, rows that bring fewer than K candidates, a running chunk accepted short, a running chunk that finds the list
    still shorter than K. And the rows with fewer than K unmasked items are exactly the ones the builder names."""
    seen = {"coarse": 0, "fine": 0, 255: 0, 256: 0, 257: 0, "over_cap": 0, "few_own": 0, "accepted_short": 0, "list_short": 0,
            "fallback": 0, "straddle": 0}
    for d, I, Ks in rm.SEL_SHAPES:
        for table in rm.SEL_TABLES:
            raw = None
            for K in Ks:
                if raw is None or table == "tieblock":
                    raw = _scores(rm.selection_table(table, I, d, K), d)
                lists, kinds, short = rm.mask_cases(raw, K)
                left = [I - len(set(x)) for x in lists]
                assert [b for b in range(rm.SEL_B) if left[b] < K] == short, (d, I, K, table)
                assert short, (d, I, K)
                if table == "tieblock":
                    top = -np.sort(-raw, axis=1)
                    n_str = int((top[:, K - 1] == top[:, K]).sum())
                    assert n_str >= rm.SEL_B - 2, (d, I, K, n_str)       # the block of equal scores lies across rank K
                    seen["straddle"] += n_str
                if d != 64 or K > rm.RM_KMAX:
                    continue
                for b in range(rm.SEL_B):
                    masked = np.zeros(I, bool)
                    masked[lists[b]] = True
                    tmx = _tile_max(raw[b])
                    walks = [rm.selection_walk(tmx, raw[b], masked, K, None, n_listed=len(lists[b]))]
                    seen[K + len(lists[b])] = seen.get(K + len(lists[b]), 0) + 1
                    if I > rm.SCORE_CHUNK:
                        live = np.where(masked, -np.inf, raw[b]).astype(np.float32)
                        for ch, (a, e) in enumerate(rm.chunk_bounds(I, True)):
                            have = int((~masked[:a]).sum())
                            floor = -np.inf if ch == 0 or have < K else -np.sort(-live[:a])[K - 1]
                            w = rm.selection_walk(tmx[a // rm.TI:(e + rm.TI - 1) // rm.TI], raw[b, a:e], masked[a:e], K, floor)
                            walks.append(w)
                            seen["accepted_short"] += w["accepted_short"]
                            seen["list_short"] += ch > 0 and have < K
                    for w in walks:
                        seen["coarse" if w["coarse"] else "fine"] += 1
                        seen["over_cap"] += w["over_cap"]
                        seen["few_own"] += w["n_cand"] < K
                        seen["fallback"] += w["fallback"]
    for what in ("coarse", "fine", 255, 256, 257, "over_cap", "few_own", "accepted_short", "list_short", "fallback", "straddle"):
        assert seen[what] > 0, (what, seen)


def test_merge_model_and_stable_topk_agree():
    """Top-K of a union = top-K of the parts' top-Ks under one total order: stable_topk over a row equals merge_model over the
    stable_topk lists of its pieces (ties across the pieces included), and merge_model skips -1 ids and pads short rows."""
    rng = np.random.default_rng(4)
    for I, K, parts in ((500, 10, 4), (3000, 256, 3), (900, 300, 3), (64, 1, 8)):
        sc = rng.integers(0, 40, size=(5, I)).astype(np.float32) / 64              # forty values: ties everywhere
        want_i, want_v = rm.stable_topk(sc, K)
        cv, ci = [], []
        for p in range(parts):
            a, e = p * I // parts, (p + 1) * I // parts
            k = min(K, e - a)
            pi, pv = rm.stable_topk(sc[:, a:e], k)
            cv.append(np.pad(pv, ((0, 0), (0, K - k)), constant_values=-np.inf))
            ci.append(np.pad(pi + a, ((0, 0), (0, K - k)), constant_values=-1))
        got_i, got_v = rm.merge_model(np.concatenate(cv, 1), np.concatenate(ci, 1), K)
        if I >= K:
            assert np.array_equal(got_i, want_i) and np.array_equal(got_v, want_v), (I, K)
    oi, ov = rm.merge_model([[0.5, 0.9, 0.5, 0.1]], [[7, -1, 3, -1]], 3)
    assert oi.tolist() == [[3, 7, -1]] and ov.tolist() == [[0.5, 0.5, -np.inf]]
