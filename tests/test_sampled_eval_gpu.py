"""Candidate scoring and sampled-negative evaluation on the device (csrc/eval.hip score_cand_kernel, csrc/sampler.hip
sample_negatives_kernel) against the full-catalogue scorer, the reference's recorded predict() and the reference's compiled
ranking code (oracle/_ref), re-enacting cpp/uni_evaluator.py:132-140."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import ROOT, build_model_from_fixture, csr_dict, load_golden, sub

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(params=["exact", "fast"])
def eval_math(request):
    from elimrec_amd import _lib
    lib = _lib.load()
    before = int(lib.elimrec_score_get_math())
    lib.elimrec_score_set_math(0 if request.param == "exact" else 1)
    yield request.param
    lib.elimrec_score_set_math(before)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _load_cache(model, g):
    ws = model._workspace(8)
    c = sub(g, "cache")
    U, d = model.num_users, model.latent_dim
    Y = ws["Y"]
    Y[:U, :d] = _t(c["all_users"])
    Y[U:, :d] = _t(c["all_items"])
    for h, m in enumerate(model._mods):
        Y[:U, (h + 1) * d:(h + 2) * d] = _t(c["pre_fusion_user_" + m])
        Y[U:, (h + 1) * d:(h + 2) * d] = _t(c["pre_fusion_item_" + m])
    model._publish_cache(Y)


def _check_rows(got, full, lists, ref=None):
    width = max(len(c) for c in lists)
    assert got.shape == (len(lists), width)
    for b, c in enumerate(lists):
        n = len(c)
        if n:
            assert np.abs(got[b, :n] - full[b, c]).max() <= 5e-7
            if ref is not None:
                assert np.abs(got[b, :n] - ref[b, c]).max() < 1e-5
        assert np.all(got[b, n:] == -np.inf)


def test_candidate_scores_equal_the_full_scorer(fixture_name, eval_math):
    """Every predict type x fusion mode of the fixture, both math modes: candidate (u, i) within 5e-7 of predict_device's score
    at (u, i), within 1e-5 of the reference's recorded predict(); -inf beyond each row; empty rows and repeated ids allowed."""
    g = load_golden(fixture_name)
    model, _ = build_model_from_fixture(g, DEV)
    _load_cache(model, g)
    users = g["eval_users"].tolist()
    I = model.num_items
    rng = np.random.default_rng(1)
    lens = [0 if b % 7 == 3 else int(rng.integers(1, 2 * I)) for b in range(len(users))]
    lists = [rng.integers(0, I, size=n).tolist() for n in lens]
    for key, want in sub(g, "predict").items():
        model.fusion_mode, model.predict_type = key.split("/")
        full = torch.empty(len(users), I, device=DEV)
        model.predict_device(users, scores=full)
        got = model.predict_candidates(users, lists)
        assert got.device.type == "cpu" and got.dtype == torch.float32
        _check_rows(got.numpy(), full.cpu().numpy(), lists, want)


@pytest.mark.parametrize("d", [36, 64, 128, 200])
def test_candidate_scorer_forms_over_recdims_and_heads(d):
    """The register forms (recdim <= 64, <= 128) and the generic one, S = 0 .. 3, every predict type and fusion: the candidate
    rows equal the full scorer's rows at their ids (5e-7)."""
    from elimrec_amd import ops
    U, I, B = 40, 300, 24
    g = torch.Generator().manual_seed(d)
    for S in range(4):
        Y = (torch.randn(U + I, (1 + S) * d, generator=g) * 0.2).to(DEV)
        sqn = torch.empty(U + I, 1 + S, device=DEV)
        ops.row_sqnorms(Y, d, 1 + S, sqn)
        users = torch.arange(3, 3 + B, device=DEV, dtype=torch.int64)
        rng = np.random.default_rng(d + S)
        lists = [rng.integers(0, I, size=int(n)).tolist() for n in rng.integers(0, 70, size=B)]
        lists[5] = []
        ptr = np.cumsum([0] + [len(c) for c in lists]).astype(np.int64)
        flat = np.asarray([i for c in lists for i in c], dtype=np.int32)
        width = int(max(len(c) for c in lists))
        for ptype in ("normal", "TE", "TIE"):
            for fmode in (("rubi",) if ptype == "normal" or S == 0 else ("rubi", "hm", "sum")):
                ws = torch.empty(ops.score_workspace(B, U, I, S, 1, d=d), dtype=torch.uint8, device=DEV)
                full = torch.empty(B, I, device=DEV)
                ops.score_topk(Y, U, I, users, d, S, 0b111, fmode, ptype, ws, scores=full, sqnorm=sqn)
                row_sum = None
                if ptype == "TIE":
                    row_sum = torch.empty(B, device=DEV)
                    ops.score_topk_shard(Y, U, I, users, d, S, 0b111, fmode, ptype, ws, 1, row_sum, I, 0, sqnorm=sqn)
                out = torch.full((B, width + 3), 7.0, device=DEV)[:, :width]
                ops.score_candidates(Y, U, I, users, d, S, 0b111, fmode, ptype, _t(ptr), _t(flat), out, sqnorm=sqn,
                                     row_sum=row_sum, I_total=I)
                _check_rows(out.cpu().numpy(), full.cpu().numpy(), lists)


def _sampled_setup(fixture, n_neg, dup=True, seed=7):
    g = load_golden(fixture)
    model, _ = build_model_from_fixture(g, DEV)
    _load_cache(model, g)
    U, I = model.num_users, model.num_items
    if dup:                       # groups of duplicated item rows: equal scores inside and across the top-K
        Y = model._ws["Y"]
        rng = np.random.default_rng(5)
        for base in rng.choice(I, size=12, replace=False):
            for c in rng.choice(I, size=3, replace=False):
                Y[U + int(c)] = Y[U + int(base)]
        model._publish_cache(Y)
    train, test, valid = csr_dict(g, "train"), csr_dict(g, "test"), csr_dict(g, "valid")
    rng = np.random.default_rng(seed)
    neg = {}
    for u in range(U):
        seen = set(train.get(u, [])) | set(test.get(u, [])) | set(valid.get(u, []))
        neg[u] = sorted(rng.choice(sorted(set(range(I)) - seen), size=n_neg, replace=False).tolist())
    return g, model, train, test, neg


def _ref_rank(model, users, test, neg, mids, K):
    from oracle import eval_oracle as ev
    lists = [list(test[u]) + neg[u] for u in users]
    sc = model.predict_candidates(users, lists).numpy()
    tp, ti = ev.truth_to_csr([list(range(len(test[u]))) for u in users])
    rows, topk = ev.evaluate_matrix(sc.copy(), tp, ti, mids, K, use_ref=True)
    return sc, np.asarray(rows, np.float32).reshape(len(users), -1), topk


def test_sampled_ranking_is_the_references_on_the_devices_scores():
    """Lists and metric rows bit for bit the reference's compiled evaluate.h applied to the device's own padded candidate scores,
    with ties inside and across K (duplicated item rows), at K = neg + 1; K = neg + 2 raises."""
    from oracle import eval_oracle as ev
    from elimrec_amd import ProxyEvaluator, ops
    from elimrec_amd.evaluator import CandidateScoringError
    if ev.ref_lib() is None:
        pytest.skip("oracle/_ref/libref_eval.so was not built (needs the reference sources at build time)")
    n_neg = 20
    g, model, train, test, neg = _sampled_setup("ml3", n_neg)
    users = sorted(test)
    model.fusion_mode, model.predict_type = "rubi", "TIE"
    mids = [1, 2, 3, 4, 5]
    tied_rows = 0
    for K in (10, n_neg + 1):
        evalr = ProxyEvaluator(None, train, test, neg, metric=["Precision", "Recall", "MAP", "NDCG", "MRR"], top_k=[K]).evaluator
        sc, ref_rows, ref_topk = _ref_rank(model, users, test, neg, mids, K)
        rows = evalr.metric_rows(model, users).cpu().numpy()
        assert np.array_equal(rows, ref_rows)
        idx = torch.empty(len(users), K, dtype=torch.int32, device=DEV)
        ops.topk_reference_order(_t(sc), K, idx)
        assert np.array_equal(idx.cpu().numpy(), ref_topk)
        s = np.sort(sc, axis=1)[:, ::-1][:, :K + 1]
        tied_rows += int((s[:, 1:] == s[:, :-1]).any(1).sum())
    assert tied_rows >= 3
    with pytest.raises(CandidateScoringError):
        ProxyEvaluator(None, train, test, neg, metric=["Recall"], top_k=[n_neg + 2])


def test_sampled_evaluate_equals_the_reference_candidate_branch():
    """ProxyEvaluator(..., user_neg_test).evaluate(model) == a host re-enactment of cpp/uni_evaluator.py:132-140 (batches of 128,
    pad_sequences with -inf, the reference's compiled ranking of the device candidate scores, np.mean), bit for bit; the two
    halves of metric_rows(shard=(r, 2)) add up to the unsharded rows; tie_order id agrees on rows without ties."""
    from oracle import eval_oracle as ev
    from elimrec_amd import ProxyEvaluator
    if ev.ref_lib() is None:
        pytest.skip("oracle/_ref/libref_eval.so was not built (needs the reference sources at build time)")
    g, model, train, test, neg = _sampled_setup("kwai", 30, dup=False)
    metric, K = ["Precision", "Recall", "NDCG"], [5, 10]
    mids = [1, 2, 4]
    for ptype in ("TE", "TIE"):
        model.fusion_mode, model.predict_type = "rubi", ptype
        ev_ = ProxyEvaluator(None, train, test, neg, metric=metric, top_k=K)
        final, buf = ev_.evaluate(model)
        users = list(test.keys())
        parts = []
        for a in range(0, len(users), 128):
            bu = users[a:a + 128]
            parts.append(_ref_rank(model, bu, test, neg, mids, 10)[1])
        want = np.mean(np.concatenate(parts, 0), axis=0).reshape(3, 10)[:, np.array(K) - 1].reshape(-1)
        assert np.array_equal(final, want), (final, want)
        rows = ev_.evaluator.metric_rows(model, users).cpu().numpy()
        halves = [ev_.evaluator.metric_rows(model, users, shard=(r, 2), reduce=False).cpu().numpy() for r in range(2)]
        assert np.array_equal(halves[0] + halves[1], rows)
        ev_.evaluator.tie_order = "id"
        assert np.array_equal(ev_.evaluator.metric_rows(model, users).cpu().numpy(), rows)


def test_negative_sampler_contract():
    """n_neg distinct ids per user, none excluded, all in range; the same seed gives the same draws; uniform over the allowed
    items (chi-square over many users sharing one exclusion list); the edge n_neg = I - |excl| - 1."""
    from elimrec_amd import ops
    rng = np.random.default_rng(0)
    I, n_users, n_neg = 60, 300, 12
    excl = [np.unique(rng.integers(0, I, size=int(rng.integers(0, 40)))) for _ in range(n_users)]
    ptr = np.cumsum([0] + [len(e) for e in excl]).astype(np.int64)
    items = np.concatenate(excl).astype(np.int32)
    out = torch.empty(n_users, n_neg, dtype=torch.int32, device=DEV)
    got = ops.sample_negatives(_t(ptr), _t(items), I, n_neg, 11, out).cpu().numpy()
    for u in range(n_users):
        assert len(set(got[u].tolist())) == n_neg
        assert got[u].min() >= 0 and got[u].max() < I
        assert not set(got[u].tolist()) & set(excl[u].tolist())
    again = ops.sample_negatives(_t(ptr), _t(items), I, n_neg, 11, torch.empty_like(out)).cpu().numpy()
    assert np.array_equal(got, again)
    other = ops.sample_negatives(_t(ptr), _t(items), I, n_neg, 12, torch.empty_like(out)).cpu().numpy()
    assert not np.array_equal(got, other)
    # uniformity: 6000 users with the same 10 excluded ids of 40, 5 draws each
    e = np.sort(rng.choice(40, size=10, replace=False)).astype(np.int32)
    n = 6000
    ptr2 = (np.arange(n + 1) * 10).astype(np.int64)
    draws = ops.sample_negatives(_t(ptr2), _t(np.tile(e, n)), 40, 5, 3, torch.empty(n, 5, dtype=torch.int32, device=DEV)).cpu().numpy()
    counts = np.bincount(draws.ravel(), minlength=40)
    assert counts[e].sum() == 0
    allowed = np.setdiff1d(np.arange(40), e)
    exp = n * 5 / len(allowed)
    chi2 = float(((counts[allowed] - exp) ** 2 / exp).sum())
    assert chi2 < 70.0, chi2          # 29 degrees of freedom: P(chi2 > 70) < 1e-4
    assert all(len(set(r.tolist())) == 5 for r in draws[:500])
    # edge: every allowed id but one
    edge = ops.sample_negatives(_t(ptr[:2]), _t(items[:ptr[1]]), I, I - int(ptr[1]) - 1, 5,
                                torch.empty(1, I - int(ptr[1]) - 1, dtype=torch.int32, device=DEV)).cpu().numpy()[0]
    assert len(set(edge.tolist())) == len(edge) and not set(edge.tolist()) & set(excl[0].tolist()) and edge.max() < I
    with pytest.raises(ValueError, match="not enough integers"):
        ops.sample_negatives(_t(ptr[:2]), _t(items[:ptr[1]]), I, I - int(ptr[1]), 5,
                             torch.empty(1, I - int(ptr[1]), dtype=torch.int32, device=DEV))


def test_synthetic_dataset_negatives_and_predict_candidates_device_form():
    """SyntheticDataset draws its negatives in memory on first use: valid == test, ascending, outside every split."""
    from elimrec_amd import SyntheticDataset
    ds = SyntheticDataset(120, 200, 2400, feat_dims=(4, 4, 4), seed=2)
    neg = ds.get_user_test_neg_dict(15)
    assert ds.get_user_valid_neg_dict(15) is neg and len(neg) == 120
    seen = ds.exclusion_csr()
    for u, items in neg.items():
        assert items == sorted(set(items)) and len(items) == 15
        assert not set(items) & set(seen[1][seen[0][u]:seen[0][u + 1]].tolist())


def test_driver_runs_sampled_evaluation(tmp_path):
    """main.py with --rec.evaluate.neg=100 --eval_candidates=sampled: one epoch, finite sampled metrics in the log."""
    cmd = [sys.executable, "main.py", "--data.input.dataset=synthetic", "--alpha=0.5", "--synthetic_shape=[300,500,6000]",
           "--synthetic_dims=[16,8,12]", "--recdim=32", "--loss=bpr_loss", "--batch_size=512", "--num_epoch=2", "--test_step=1", "--verbose=1",
           "--rec.evaluate.neg=100", "--eval_candidates=sampled", "--path=%s" % str(tmp_path / "ck")]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    text = r.stdout + r.stderr
    lines = [ln for ln in text.splitlines() if "[TIE]" in ln and "R@" in ln]
    assert lines, text[-2000:]
    vals = [float(x) for x in re.findall(r"[-+]?\d*\.\d+(?:[eE][-+]?\d+)?|nan|inf", lines[-1])]
    assert vals and all(np.isfinite(vals)) and max(vals) > 0.0, lines[-1]
