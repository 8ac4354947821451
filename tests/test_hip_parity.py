"""Parity of the HIP path (through the C ABI) against the golden vectors captured from the
reference and against the CPU oracle on seeded inputs. Needs a real MI355X: `-m gpu`."""
import collections
import os
import numpy as np
import pytest
import torch

from helpers import assert_grad_close, build_model_from_fixture, csr_dict, load_golden, rel_err, sub
from helpers import reference_lists as _reference_lists, tie_free as _tie_free

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


# ----------------------------------------------------------------------------- golden fixtures
@pytest.fixture(params=["exact", "fast"])
def eval_math(request):
    """Both evaluator math modes explicitly (elimrec_score_set_math): EXACT = IEEE division + libm expf; FAST (the default)
    = v_exp_f32 / v_rcp_f32 + Newton step, every score within 1.2e-7 of EXACT."""
    from elimrec_amd import _lib
    lib = _lib.load()
    before = int(lib.elimrec_score_get_math())
    lib.elimrec_score_set_math(0 if request.param == "exact" else 1)
    yield request.param
    lib.elimrec_score_set_math(before)


def test_training_steps_match_reference(fixture_name):
    """loss to 1e-5 abs, every parameter gradient to 1e-4 rel (north_star tolerance), the same
    set of parameters receives a gradient, parameters after Adam steps to 2e-5 abs."""
    from elimrec_amd import FusedAdam
    g = load_golden(fixture_name)
    model, cfg = build_model_from_fixture(g, DEV)
    opt = FusedAdam(model.parameters(), lr=float(g["lr"]), weight_decay=float(g["weight_decay"]))
    steps = int(g["steps"])
    for t in range(1, steps + 1):
        u, p, n = (_t(g["step%d/%s" % (t, k)]) for k in ("users", "pos", "neg"))
        loss = model.bpr_loss(u, p, n)
        opt.zero_grad()
        loss.backward(retain_graph=True)
        assert abs(loss.cpu().item() - float(g["step%d/loss" % t])) < 1e-5, t
        if t == 1:
            assert rel_err(model.all_users.cpu(), g["fwd1/all_users"]) < 1e-4
            assert rel_err(model.all_items.cpu(), g["fwd1/all_items"]) < 1e-4
            ref = sub(g, "grad1")
            mine = {k: p_.grad for k, p_ in model.named_parameters() if p_.grad is not None}
            assert set(mine) == set(ref)
            for k, gr in ref.items():
                assert_grad_close(mine[k].cpu(), gr, k)
        opt.step()
        if t in (1, steps):
            sd = model.state_dict()
            for k, v in sub(g, "after%d" % t).items():
                assert np.abs(sd[k].cpu().numpy() - v).max() < 2e-5, (t, k)


def test_adam_kernel_given_reference_grads(fixture_name):
    from elimrec_amd import FusedAdam
    g = load_golden(fixture_name)
    model, _ = build_model_from_fixture(g, DEV)
    opt = FusedAdam(model.parameters(), lr=float(g["lr"]), weight_decay=float(g["weight_decay"]))
    ref = sub(g, "grad1")
    for k, p_ in model.named_parameters():
        if k in ref:
            p_.grad = _t(ref[k])
    opt.step()
    sd = model.state_dict()
    for k, v in sub(g, "after1").items():
        assert np.abs(sd[k].cpu().numpy() - v).max() <= 2.4e-7, k
        if k not in ref:
            assert np.array_equal(sd[k].cpu().numpy(), g["init/" + k])


def _load_cache(model, g):
    """Put the reference's cached tables (state after its last training forward) into Y."""
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


def test_predict_modes_match_reference(fixture_name, eval_math):
    g = load_golden(fixture_name)
    model, _ = build_model_from_fixture(g, DEV)
    _load_cache(model, g)
    users = g["eval_users"].tolist()
    for key, want in sub(g, "predict").items():
        model.fusion_mode, model.predict_type = key.split("/")
        got = model.predict(users)
        assert isinstance(got, torch.Tensor) and got.device.type == "cpu" and got.dtype == torch.float32
        assert got.shape == want.shape
        assert np.abs(got.numpy() - want).max() < 1e-5, key


def test_predict_after_training_uses_stale_tables(fixture_name):
    """End to end: train `steps` steps on the GPU, then predict() must match the reference's
    predict() (tables from the last forward, i.e. pre-update parameters)."""
    from elimrec_amd import FusedAdam
    g = load_golden(fixture_name)
    model, _ = build_model_from_fixture(g, DEV)
    opt = FusedAdam(model.parameters(), lr=float(g["lr"]), weight_decay=float(g["weight_decay"]))
    for t in range(1, int(g["steps"]) + 1):
        loss = model.bpr_loss(*(_t(g["step%d/%s" % (t, k)]) for k in ("users", "pos", "neg")))
        opt.zero_grad()
        loss.backward(retain_graph=True)
        opt.step()
    assert rel_err(model.all_users.cpu(), g["cache/all_users"]) < 1e-4
    model.fusion_mode, model.predict_type = "rubi", "TIE"
    got = model.predict(g["eval_users"].tolist()).numpy()
    assert np.abs(got - g["predict/rubi/TIE"]).max() < 1e-5


def test_batch_row_head_equals_full_tables(fixture_name):
    """--head_rows=batch (default: projections after the graph only at the batch's rows, full cached tables filled
    in on first use from the pre-update weights) against --head_rows=all (every row, every step): same losses,
    bit-identical parameters after training, identical stale-table predictions."""
    from helpers import FixtureDataset, fixture_argv, make_config
    from elimrec_amd import EliMRec, FusedAdam
    g = load_golden(fixture_name)
    out = {}
    for mode in ("batch", "all"):
        model = EliMRec(make_config(fixture_argv(g) + ["--head_rows=%s" % mode]), FixtureDataset(g))
        with torch.no_grad():
            for m in ("v", "a", "t"):
                if (m + "_feat") in g and hasattr(model, m + "_feat"):
                    getattr(model, m + "_feat").copy_(torch.from_numpy(g[m + "_feat"]))
        model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sub(g, "init").items()})
        model = model.to(DEV)
        if not model._folded:
            pytest.skip("fixture's adjacency is not bipartite: the graph tables are not folded")
        assert model._lazy == (mode == "batch")
        opt = FusedAdam(model.parameters(), lr=float(g["lr"]), weight_decay=float(g["weight_decay"]))
        losses = []
        for t in range(1, int(g["steps"]) + 1):
            loss = model.bpr_loss(*(_t(g["step%d/%s" % (t, k)]) for k in ("users", "pos", "neg")))
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(loss.item())
        if mode == "batch":
            assert model._tables_dirty            # nothing read the full tables during training
        model.fusion_mode, model.predict_type = "rubi", "TIE"
        pred = model.predict(g["eval_users"].tolist())
        out[mode] = (losses, {k: v.cpu().clone() for k, v in model.state_dict().items()}, pred,
                     model.all_users.cpu().clone(), model.all_s_embs["pre_fusion_item_v"].cpu().clone())
    assert out["batch"][0] == out["all"][0]
    for k, v in out["all"][1].items():
        assert torch.equal(out["batch"][1][k], v), k
    assert torch.equal(out["batch"][2], out["all"][2])
    assert torch.equal(out["batch"][3], out["all"][3]) and torch.equal(out["batch"][4], out["all"][4])


def test_step_regions_replayed_equal_eager(monkeypatch):
    """The step's regions two ways -- launched from Python every time, re-issued from the recorded C-ABI call
    lists (default; the native one-call program switched off so that the regions carry every step) -- give bit-identical
    parameters after several steps, including a change of batch size in between (regions are re-recorded against the new
    workspace buffers)."""
    from helpers import FixtureDataset, fixture_argv, make_config
    from elimrec_amd import ColumnShardEngine, ColumnShardTrainer, EliMRec, FusedAdam
    g = load_golden("ml3")
    u, p, n = (_t(g["step1/%s" % k]) for k in ("users", "pos", "neg"))
    sizes = [len(u)] * 5 + [len(u) - 7] * 2 + [len(u)] * 4
    monkeypatch.setenv("ELIMREC_NATIVE_STEP", "0")
    out = {}
    for mode in ("eager", "replay"):
        monkeypatch.setenv("ELIMREC_REPLAY", "0" if mode == "eager" else "1")
        model = EliMRec(make_config(fixture_argv(g)), FixtureDataset(g))
        model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sub(g, "init").items()})
        model = model.to(DEV)
        assert model._lazy and model._use_replay == (mode != "eager")
        trainer = ColumnShardTrainer(ColumnShardEngine(model), FusedAdam(model.parameters(), lr=float(g["lr"]), weight_decay=float(g["weight_decay"])))
        losses = [float(trainer.step(u[:b], p[:b], n[:b])) for b in sizes]
        assert trainer._native_state()["native_steps"] == 0
        out[mode] = (losses, {k: v.cpu().clone() for k, v in model.state_dict().items()})
    for mode in ("replay",):
        assert out[mode][0] == out["eager"][0], mode
        for k, v in out["eager"][1].items():
            assert torch.equal(out[mode][1][k], v), (mode, k)


def _my_rule_topk(scores, K):
    """Top-K under the device's stated tie rule: score descending, item id ascending."""
    return np.argsort(-scores, axis=1, kind="stable")[:, :K].astype(np.int32)


def _ulps(a, b):
    a = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def test_device_evaluator_matches_reference(fixture_name, eval_math):
    """SURVEY section 7 (ii), judged on the REFERENCE's scores (the fixture's masked score matrix of the whole test split):
      * rank by rank, the item the device puts at rank k has the same reference score as the item the reference puts
        there -- asserted for every row whose device scores equal the reference's bit for bit at those items;
      * rows without a tie at or across K: the device indices ARE the reference indices. Where they are not, the cause
        must be a device/reference score difference of a few ulp between two near-equal (not equal) scores: each such
        row is checked for exactly that and their number is bounded;
      * evaluate(): equal to 1e-7, no slack, to the metrics the oracle's metric port computes from the device's ranking --
        the ranking verified row by row above; and that ranking IS the reference scores' ranking under the device's tie
        rule (score desc, item id asc) except on the counted rows where a <= 4-ulp score difference moved two items."""
    from oracle import eval_oracle as ev
    g = load_golden(fixture_name)
    model, _ = build_model_from_fixture(g, DEV)
    _load_cache(model, g)
    model.fusion_mode, model.predict_type = "rubi", "TIE"
    users = g["evalbatch/users"].tolist()
    K = int(g["evalbatch/top_k"])
    mids = g["evalbatch/metric_ids"]
    evalr = model.test_evaluator.evaluator
    rows, idx, val = evalr.evaluate_batch(model, users, return_topk=True)
    idx = idx.cpu().numpy()
    ref_scores = g["evalbatch/masked_scores"]
    test = csr_dict(g, "test")
    tp, ti = ev.truth_to_csr([sorted(set(test[int(u)])) for u in users])
    _, ref_topk = ev.evaluate_matrix(ref_scores, tp, ti, mids, K)          # the reference's heap-order ranking
    mine_topk = _my_rule_topk(ref_scores, K)                              # reference scores, device tie rule
    dev_scores = torch.empty(len(users), model.num_items, device=DEV)
    train_ptr, train_items = evalr._batch_csr(users, evalr.user_pos_train, DEV, unique=False)
    model.predict_device(users, scores=dev_scores, train_ptr=train_ptr, train_items=train_items)
    dev_scores = dev_scores.cpu().numpy()
    assert np.array_equal(np.isinf(dev_scores), np.isinf(ref_scores))          # same items masked
    finite = ~np.isinf(ref_scores)
    assert np.abs(dev_scores[finite] - ref_scores[finite]).max() < 1e-5
    clean = _tie_free(ref_scores, K)
    assert clean.sum() > 0
    n_bitwise = n_moved = 0
    for r in range(len(users)):
        touched = np.union1d(idx[r], ref_topk[r])
        if np.array_equal(dev_scores[r][touched], ref_scores[r][touched]):
            n_bitwise += 1
            assert np.array_equal(ref_scores[r][idx[r]], ref_scores[r][ref_topk[r]]), r     # score-equivalent, rank by rank
            if clean[r]:
                assert np.array_equal(idx[r], ref_topk[r]), r                                 # tie-free: the same items
        elif clean[r] and not np.array_equal(idx[r], ref_topk[r]):
            # an ulp-level score difference reordered two near-equal reference scores: the swapped ranks hold reference
            # scores within 4 ulp of each other, and the device ranked by ITS scores correctly
            n_moved += 1
            assert _ulps(ref_scores[r][idx[r]], ref_scores[r][ref_topk[r]]).max() <= 4, r
        assert np.array_equal(dev_scores[r][idx[r]], -np.sort(-dev_scores[r])[:K]), r         # the device's own ranking is exact
    assert n_bitwise > 0
    assert n_moved <= max(1, len(users) // 20), n_moved
    # metric kernel on the device's ranking == the metric port on the same ranking
    want = ev.metrics_from_rank(idx, tp, ti, mids, K)
    assert np.abs(rows.cpu().numpy() - want).max() < 1e-6
    # evaluate() against the metrics recomputed from the reference scores under the device's tie rule
    moved = int((idx != mine_topk).any(1).sum())
    for r in np.nonzero((idx != mine_topk).any(1))[0]:
        assert _ulps(ref_scores[r][idx[r]], ref_scores[r][mine_topk[r]]).max() <= 4, r
    assert moved <= max(1, len(users) // 20), moved
    n_metrics = len(mids)
    mean_of = lambda topk: ev.metrics_from_rank(topk, tp, ti, mids, K).mean(0).reshape(n_metrics, K)[:, evalr.top_show - 1].reshape(-1)
    res, buf = model.test()
    assert res.dtype == np.float32 and res.shape == (3,) and len(buf.split("\t")) == 3
    assert np.abs(res - mean_of(idx)).max() <= 1e-7, (res, mean_of(idx))
    if moved == 0:
        assert np.abs(res - mean_of(mine_topk)).max() <= 1e-7
    # TE: scores from the oracle (pinned to the reference's predict() to 2e-6), same recomputation
    from oracle import elimrec_oracle as eo
    from helpers import feats_of
    adj = eo.build_adj(g["train_u"], g["train_i"], int(g["num_users"]), int(g["num_items"]), str(g["adj_type"]))
    om = eo.OracleEliMRec(int(g["num_users"]), int(g["num_items"]), int(g["recdim"]), int(g["layer_num"]), adj, feats_of(g),
                          sub(g, "init"), float(g["alpha"]), dataset_name=str(g["dataset_name"]),
                          modality=str(g["modality"]), mm_fusion_mode=str(g["mm_fusion_mode"]), predict_type="TE")
    om.set_cache(g["cache/all_users"], g["cache/all_items"], {k: v for k, v in sub(g, "cache").items() if k.startswith("pre_fusion")})
    te = om.predict(users).numpy().astype(np.float32)
    train = csr_dict(g, "train")
    for r, u in enumerate(users):
        te[r, train.get(int(u), [])] = -np.inf
    te_topk = _my_rule_topk(te, K)
    model.predict_type = "TE"
    _, te_idx, _ = evalr.evaluate_batch(model, users, return_topk=True)
    te_idx = te_idx.cpu().numpy()
    te_moved = int((te_idx != te_topk).any(1).sum())
    for r in np.nonzero((te_idx != te_topk).any(1))[0]:
        assert np.abs(te[r][te_idx[r]] - te[r][te_topk[r]]).max() < 4e-6, r       # oracle scores are 2e-6 from the reference's
    assert te_moved <= max(1, len(users) // 20), te_moved
    res, _ = model.test()
    assert np.abs(res - mean_of(te_idx)).max() <= 1e-7
    if te_moved == 0:
        assert np.abs(res - mean_of(te_topk)).max() <= 1e-7
    # and the reference's own reported numbers differ from ours only through its heap tie order
    ref_per_user = ev.metrics_from_rank(ref_topk, tp, ti, mids, K).mean(0).reshape(n_metrics, K)[:, evalr.top_show - 1].reshape(-1)
    assert np.abs(ref_per_user - g["evaluate/TIE/test"]).max() < 1e-7


def test_tie_straddling_k_is_score_equivalent_to_the_reference_order():
    """Identical scores on both sides of the K boundary: the device keeps the lowest item ids (its stated rule), the
    reference's partial_sort_copy keeps whatever its heap order leaves -- different items, but rank by rank the same
    score, on the same score matrix."""
    from elimrec_amd import ops
    from oracle import eval_oracle as ev
    U, I, d, S, K = 8, 600, 16, 3, 10
    Cy = (1 + S) * d
    gen = torch.Generator().manual_seed(4)
    Y = torch.randn(U + I, Cy, generator=gen)
    Y[U + 40:U + 520] = Y[U + 40:U + 52].repeat(40, 1)        # 12 distinct rows x 40 copies: every score value 40 times
    users = torch.arange(U)
    ws = torch.empty(ops.score_workspace(U, U, I, S, K), dtype=torch.uint8, device=DEV)
    scores = torch.empty(U, I, device=DEV)
    idx = torch.empty(U, K, dtype=torch.int32, device=DEV)
    val = torch.empty(U, K, device=DEV)
    ptr = torch.zeros(U + 1, dtype=torch.int64, device=DEV)
    ops.score_topk(Y.to(DEV), U, I, users.to(DEV), d, S, 0b111, "rubi", "TIE", ws, scores=scores, K=K, topk_idx=idx,
                   topk_val=val, train_ptr=ptr, train_items=torch.zeros(1, dtype=torch.int32, device=DEV))
    sc, idx = scores.cpu().numpy(), idx.cpu().numpy()
    kth = -np.sort(-sc, axis=1)[:, K - 1:K + 1]
    assert (kth[:, 0] == kth[:, 1]).any()                     # a tie does straddle K on some rows
    tp, ti = ev.truth_to_csr([[1]] * U)
    _, ref_topk = ev.evaluate_matrix(sc, tp, ti, [1, 2, 4], K)
    assert (idx != ref_topk).any()                            # the two tie rules do pick different items here
    for r in range(U):
        assert np.array_equal(sc[r][idx[r]], sc[r][ref_topk[r]]), r
        assert np.array_equal(idx[r], _my_rule_topk(sc[r:r + 1], K)[0]), r


# ----------------------------------------------------------------------------- op-level vs oracle
def test_linear_fwd_and_bwd_w_vs_torch():
    from elimrec_amd import ops
    gen = torch.Generator().manual_seed(0)
    for (M, N, K, lda_pad) in [(1000, 64, 128, 0), (777, 32, 40, 24), (130, 96, 2048, 0), (5, 16, 8, 8), (4096, 64, 256, 0)]:
        A_full = torch.randn(M, K + lda_pad, generator=gen)
        W = torch.randn(N, K, generator=gen) * 0.1
        b = torch.randn(N, generator=gen)
        out_full = torch.zeros(M, N + 16)
        A_d, W_d, b_d, out_d = A_full.to(DEV), W.to(DEV), b.to(DEV), out_full.to(DEV)
        ops.linear_fwd(A_d[:, :K], W_d, b_d, out_d[:, 8:8 + N])
        want = A_full[:, :K].double() @ W.double().T + b.double()
        got = out_d.cpu()
        assert rel_err(got[:, 8:8 + N], want) < 2e-6
        assert got[:, :8].abs().max() == 0 and got[:, 8 + N:].abs().max() == 0   # neighbours untouched
        # weight gradient: out[i,j] = sum_r A2[r,i] * B2[idx[r], j]
        G = torch.randn(M, N, generator=gen)
        idx = torch.randint(0, M, (M,), generator=gen, dtype=torch.int32)
        ws = torch.empty(ops.linear_bwd_w_workspace(M, N, K), dtype=torch.uint8, device=DEV)
        gw = torch.empty(N, K, device=DEV)
        gb = torch.empty(N, device=DEV)
        ops.linear_bwd_w(G.to(DEV), A_d[:, :K], gw, ws, colsum=gb)
        assert rel_err(gw.cpu(), G.double().T @ A_full[:, :K].double()) < 5e-6
        assert rel_err(gb.cpu(), G.double().sum(0)) < 5e-6
        rng = torch.tensor([M // 5, M - 3], dtype=torch.int32, device=DEV)
        ops.linear_bwd_w(G.to(DEV), A_d[:, :K], gw, ws, row_index=idx.to(DEV), rng=rng, colsum=gb)
        lo, hi = M // 5, M - 3
        want = G[lo:hi].double().T @ A_full[idx[lo:hi].long(), :K].double()
        assert rel_err(gw.cpu(), want) < 5e-6
        gw2 = gw.clone()
        ops.linear_bwd_w(G.to(DEV), A_d[:, :K], gw2, ws, row_index=idx.to(DEV), rng=rng, accumulate=True)
        assert rel_err(gw2.cpu(), 2 * want) < 5e-6
        # bitwise reproducible
        gw3 = torch.empty_like(gw)
        ops.linear_bwd_w(G.to(DEV), A_d[:, :K], gw3, ws, row_index=idx.to(DEV), rng=rng)
        assert torch.equal(gw3, gw)


def _random_graph(n, nnz, seed):
    import scipy.sparse as sp
    rs = np.random.RandomState(seed)
    r = rs.randint(n, size=nnz)
    c = (rs.zipf(1.6, size=nnz) - 1) % n          # skewed columns
    m = sp.csr_matrix((rs.rand(nnz).astype(np.float32), (r, c)), shape=(n, n))
    m.sum_duplicates()
    m.sort_indices()
    return m


@pytest.mark.parametrize("C,L", [(256, 3), (128, 2), (64, 1), (512, 3), (48, 4), (256, 0)])
def test_propagate_vs_oracle(C, L):
    from elimrec_amd import ops
    n = 3000
    m = _random_graph(n, 40000, seed=C + L).tolil()
    m[17, :] = 0                                   # an empty row
    m[5, :] = 0.01                                 # a very long row (n non-zeros)
    m = m.tocsr().astype(np.float32)
    m.eliminate_zeros()
    m.sort_indices()
    X0 = torch.randn(n, C, generator=torch.Generator().manual_seed(1))
    csr = ops.Csr.from_scipy(m, DEV, C=C, threshold=64)
    X0d = X0.to(DEV)
    t0, t1, out = torch.empty_like(X0d), torch.empty_like(X0d), torch.empty_like(X0d)
    ops.propagate(csr, X0d, L, t0, t1, out)
    coo = m.tocoo()
    A = torch.sparse_coo_tensor(np.vstack([coo.row, coo.col]), coo.data, (n, n)).double()
    x = X0.double()
    acc = x.clone()
    for _ in range(L):
        x = torch.sparse.mm(A, x)
        acc += x
    want = acc / (L + 1)
    assert rel_err(out.cpu(), want) < 2e-6
    assert torch.equal(X0d.cpu(), X0)              # X0 left intact
    out2 = torch.empty_like(out)
    ops.propagate(csr, X0d, L, t0, t1, out2)
    assert torch.equal(out, out2)                  # deterministic
    assert csr._split is not None and csr._split.n_long >= 1
    plain = ops.Csr.from_scipy(m, DEV)             # no row-split plan: one wave per row
    ops.propagate(plain, X0d, L, t0, t1, out2)
    assert rel_err(out2.cpu(), want) < 2e-6


def test_in_launch_row_combine_is_bitwise_equal_to_fixup_launch():
    """The split rows of the power-law head are combined either by a separate fix-up launch or, by
    default, inside the gather launch by the wave that finishes a row's last segment (agent-scope
    release/acquire + ticket counter). Same summation order => identical bits, every time, at the
    full Tiktok shape (hundreds of split rows, thousands of segment waves racing)."""
    from elimrec_amd import SyntheticDataset, _lib, ops
    from elimrec_amd.model import create_adj_mat
    ds = SyntheticDataset(36656, 76085, 720829, feat_dims=(4, 4, 4), seed=0)
    tu, ti = ds.get_train_interactions()
    adj = create_adj_mat(tu, ti, ds.num_users, ds.num_items, "pre")
    U, I, d, M = ds.num_users, ds.num_items, 64, 4
    P = ops.Csr.from_scipy(adj[:U, U:], DEV, C=d * M)
    Q = ops.Csr.from_scipy(adj[U:, :U], DEV, C=d * M)
    assert Q._split is not None and Q._split.n_long > 100
    g = torch.Generator(device=DEV).manual_seed(0)
    Eu = torch.randn(U, d, device=DEV, generator=g)
    XI = torch.randn(I, d * M, device=DEV, generator=g)
    ws = torch.empty(ops.bipartite_workspace(U, I, d, M), dtype=torch.uint8, device=DEV)
    lib = _lib.load()
    ref = torch.empty(U + I, d * M, device=DEV)
    lib.elimrec_set_ticket_fixup(0)
    try:
        ops.propagate_bipartite(P, Q, U, I, d, M, 3, Eu, XI, ref, ws)
    finally:
        lib.elimrec_set_ticket_fixup(1)
    out = torch.empty_like(ref)
    for it in range(25):
        out.fill_(float("nan"))
        ops.propagate_bipartite(P, Q, U, I, d, M, 3, Eu, XI, out, ws)
        assert torch.equal(out, ref), it
        assert int(Q._split_tensors[5].abs().sum()) == 0          # ticket counters back to zero


def test_propagate_linearity_at_tiktok_shape():
    """Size-independent property at the full BASELINE shape: P(aX + bZ) == aP(X) + bP(Z), and
    <P(X), Z> == <X, P^T(Z)> for the symmetric 'pre' adjacency (self-adjointness used by backward)."""
    from elimrec_amd import SyntheticDataset, ops
    from elimrec_amd.model import create_adj_mat
    ds = SyntheticDataset(36656, 76085, 720829, feat_dims=(4, 4, 4), seed=0)
    tu, ti = ds.get_train_interactions()
    adj = create_adj_mat(tu, ti, ds.num_users, ds.num_items, "pre")
    csr = ops.Csr.from_scipy(adj, DEV, C=256)
    n, C = adj.shape[0], 256
    g = torch.Generator(device=DEV).manual_seed(0)
    X, Z = torch.randn(n, C, device=DEV, generator=g), torch.randn(n, C, device=DEV, generator=g)
    t0, t1 = torch.empty_like(X), torch.empty_like(X)
    PX, PZ, PXZ = torch.empty_like(X), torch.empty_like(X), torch.empty_like(X)
    ops.propagate(csr, X, 3, t0, t1, PX)
    ops.propagate(csr, Z, 3, t0, t1, PZ)
    ops.propagate(csr, 0.5 * X - 2.0 * Z, 3, t0, t1, PXZ)
    assert rel_err((0.5 * PX - 2.0 * PZ).cpu(), PXZ.cpu()) < 1e-5
    a = (PX.double() * Z.double()).sum().item()
    b = (X.double() * PZ.double()).sum().item()
    assert abs(a - b) < 1e-6 * max(abs(a), 1.0)


def test_bpr_head_and_segment_reduce_vs_torch_autograd():
    from elimrec_amd import ops
    gen = torch.Generator().manual_seed(3)
    for (U, I, d, nb, B) in [(200, 300, 64, 4, 257), (50, 60, 32, 2, 64), (40, 40, 256, 4, 33), (64, 64, 16, 3, 100)]:
        Y = torch.randn(U + I, nb * d, generator=gen)
        Y[3] = 0.0                                                  # a zero row exercises the eps branch
        u = torch.randint(0, U, (B,), generator=gen)
        u[:5] = 3
        p = torch.randint(0, I, (B,), generator=gen)
        n = torch.randint(0, I, (B,), generator=gen)
        w = [1.0, 0.5, 0.0, 0.25][:nb]
        Yr = Y.clone().double().requires_grad_(True)
        total = 0
        F = torch.nn.functional
        for k in range(nb):
            blk = Yr[:, k * d:(k + 1) * d]
            a, pp, nn_ = F.normalize(blk[u], dim=1), F.normalize(blk[U + p], dim=1), F.normalize(blk[U + n], dim=1)
            total = total + w[k] * torch.mean(F.softplus((a * nn_).sum(1) - (a * pp).sum(1)))
        total.backward()
        Yd = Y.to(DEV)
        loss_rows = torch.empty(B, device=DEV)
        grad_rows = torch.empty(3 * B, nb * d, device=DEV)
        keys = torch.empty(3 * B, dtype=torch.int32, device=DEV)
        ops.bpr_head(Yd, U, I, u.to(DEV), p.to(DEV), n.to(DEV), d, w, loss_rows, grad_rows, keys)
        loss = torch.empty((), device=DEV)
        ops.fixed_order_sum(loss_rows, loss)
        assert abs(loss.item() - total.item()) < 2e-6
        act = torch.empty(3 * B, dtype=torch.int32, device=DEV)
        red = torch.zeros(3 * B, nb * d, device=DEV)
        seg = torch.zeros(8, dtype=torch.int32, device=DEV)
        ws = torch.empty(ops.segment_reduce_workspace(3 * B), dtype=torch.uint8, device=DEV)
        ops.segment_reduce_rows(grad_rows, keys, U, act, red, seg, ws)
        info = seg.cpu().tolist()
        want_rows = np.unique(np.concatenate([u.numpy(), U + p.numpy(), U + n.numpy()]))
        assert info[0] == len(want_rows) and info[1] == int((want_rows < U).sum())
        assert info[2:] == [0, info[1], info[1], info[0], 0, info[0]]
        assert np.array_equal(act.cpu().numpy()[:info[0]], want_rows)
        dense = torch.zeros(U + I, nb * d, dtype=torch.float64)
        dense[act[:info[0]].cpu().long()] = red[:info[0]].cpu().double()
        gref = Yr.grad.clone()
        assert torch.isfinite(dense[3]).all()
        assert rel_err(dense[3], gref[3]) < 1e-5     # zero-norm row: the v/eps branch (values ~1e9)
        gref[3] = 0
        dense[3] = 0
        assert rel_err(dense, gref) < 1e-5
        red2 = torch.zeros_like(red)
        ops.segment_reduce_rows(grad_rows, keys, U, act, red2, seg, ws, scale=torch.full((1,), 2.0, device=DEV))
        assert torch.equal(red2[:info[0]], 2 * red[:info[0]])       # deterministic + scale


@pytest.mark.parametrize("n,key_space,hot", [(6144, 112741, 0), (12288, 112741, 700), (300, 97, 40), (1, 5, 0),
                                             (49152, 600000, 3000), (98304, 112741, 2500), (8193, 8200, 9)])
def test_one_workgroup_segment_plan_equals_sorted_plan(n, key_space, hot):
    """The bitmap planner (keys < key_space known; one workgroup up to 8192 slots, the device-wide form of the same phases
    above that) against the radix-sort planner: same active rows, seg_info, slot -> segment map and bit-identical segment
    sums (member lists in ascending slot order), including member lists long enough for the cooperative rank sort (`hot`
    slots share one key)."""
    from elimrec_amd import ops
    gen = torch.Generator().manual_seed(n + key_space)
    keys = torch.randint(0, key_space, (n,), generator=gen, dtype=torch.int32)
    if hot:
        keys[torch.randperm(n, generator=gen)[:hot]] = int(keys[0])
        keys[torch.randperm(n, generator=gen)[:hot // 2]] = int(keys[1])
    split = key_space // 3
    rows = torch.randn(n, 8, generator=gen)
    keys_d, rows_d = keys.to(DEV), rows.to(DEV)
    res = []
    for ks in (key_space, 0):
        ws = torch.empty(ops.segment_plan_workspace(n), dtype=torch.uint8, device=DEV)
        act = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        seg = torch.zeros(8, dtype=torch.int32, device=DEV)
        slot_seg = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        red = torch.zeros(n, 8, device=DEV)
        ops.segment_plan(keys_d, split, ks, act, seg, slot_seg, ws)
        ops.segment_apply(rows_d, seg, red, ws)
        na = int(seg[0])
        res.append((act[:na].cpu(), seg.cpu(), slot_seg.cpu(), red[:na].cpu()))
    uniq = torch.unique(keys.long())
    assert torch.equal(res[0][0].long(), uniq) and int(res[0][1][1]) == int((uniq < split).sum())
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)
    assert torch.equal(uniq[res[0][2].long()], keys.long())
    want = torch.zeros(len(uniq), 8, dtype=torch.float64).index_add_(0, res[0][2].long(), rows.double())
    assert (res[0][3].double() - want).abs().max() < 1e-4


def test_fused_segment_apply_head_bwd_equals_two_launches():
    """segment_apply + head_bwd_input as one launch: bitwise the same dY and dOut rows; and the planner's key bitmap
    marks exactly the active rows."""
    from elimrec_amd import ops
    gen = torch.Generator().manual_seed(5)
    U, I, d, S, n = 300, 500, 64, 3, 777
    C, Cy = (1 + S) * d, (1 + S) * d
    keys = torch.randint(0, U + I, (n,), generator=gen, dtype=torch.int32).to(DEV)
    rows = torch.randn(n, Cy, generator=gen).to(DEV)
    wu, wi = torch.randn(d, C, generator=gen).to(DEV), torch.randn(d, C, generator=gen).to(DEV)
    heads = [torch.randn(d, d, generator=gen).to(DEV) for _ in range(S)]
    scale = torch.full((1,), 0.37, device=DEV)
    ws = torch.empty(ops.segment_plan_workspace(n), dtype=torch.uint8, device=DEV)
    act = torch.zeros(n, dtype=torch.int32, device=DEV)
    seg = torch.zeros(8, dtype=torch.int32, device=DEV)
    slot_seg = torch.zeros(n, dtype=torch.int32, device=DEV)
    bitmap = torch.full(((U + I + 31) // 32 + 2,), -1, dtype=torch.int32, device=DEV)
    ops.segment_plan(keys, U, U + I, act, seg, slot_seg, ws, key_bitmap=bitmap)
    na = int(seg[0])
    bits = torch.zeros(U + I, dtype=torch.bool)
    bits[act[:na].long().cpu()] = True
    words = bitmap[:(U + I + 31) // 32].cpu().numpy().view(np.uint32)
    got = np.unpackbits(words.view(np.uint8), bitorder="little")[:U + I].astype(bool)
    assert np.array_equal(got, bits.numpy())
    dY1, dY2 = torch.zeros(n, Cy, device=DEV), torch.zeros(n, Cy, device=DEV)
    out1, out2 = torch.zeros(n, C, device=DEV), torch.zeros(n, C, device=DEV)
    ops.segment_apply(rows, seg, dY1, ws, scale=scale)
    ops.head_bwd_input(dY1, act, seg, U, d, C, [1, 2, 3], wu, wi, heads, 1.0, None, compact=out1)
    ops.segment_apply_head_bwd(rows, act, seg, dY2, ws, U, d, C, [1, 2, 3], wu, wi, heads, out2, scale=scale)
    assert torch.equal(dY1[:na], dY2[:na]) and torch.equal(out1[:na], out2[:na])


def test_sampler_contract_on_device():
    from elimrec_amd import PairwiseSamplerV2, SyntheticDataset
    ds = SyntheticDataset(400, 300, 6000, feat_dims=(4, 4, 4), seed=9)
    smp = PairwiseSamplerV2(ds, batch_size=512, device=DEV, seed=7)
    train = ds.get_user_train_dict()
    us, ps, ns, nb = [], [], [], 0
    for bu, bp, bn in smp:
        assert bu.device.type == "cuda" and bu.dtype == torch.int64 and len(bu) == len(bp) == len(bn) <= 512
        us.append(bu.cpu()); ps.append(bp.cpu()); ns.append(bn.cpu()); nb += 1
    assert nb == len(smp)
    u, p, n = torch.cat(us).numpy(), torch.cat(ps).numpy(), torch.cat(ns).numpy()
    assert len(u) == smp.num_trainings
    sets = {k: set(v) for k, v in train.items()}
    assert all(int(a) in sets for a in u)
    assert all(int(b) in sets[int(a)] for a, b in zip(u, p))
    assert all(int(c) not in sets[int(a)] and 0 <= c < ds.num_items for a, c in zip(u, n))
    # users uniform over users with >= 1 training item (chi-square, 5 sigma)
    counts = np.bincount(u, minlength=ds.num_users)[sorted(sets)]
    exp = len(u) / len(sets)
    chi2 = ((counts - exp) ** 2 / exp).sum()
    assert abs(chi2 - len(sets)) < 5 * np.sqrt(2 * len(sets))
    # negatives uniform over the catalogue
    cn = np.bincount(n, minlength=ds.num_items)
    assert cn.min() > 0 and cn.max() < 4 * len(n) / ds.num_items
    # positives uniform, with replacement, over the drawn user's training items (data/sampler.py:113-115): Pearson chi-square over
    # all (user, training item) cells of 24 further epochs (about 20 draws expected per cell), 5 sigma
    uu, pp = [u], [p]
    for _ in range(24):
        eu, ep, _ = smp.sample_epoch()
        uu.append(eu.cpu().numpy()); pp.append(ep.cpu().numpy())
    uu, pp = np.concatenate(uu), np.concatenate(pp)
    drawn = np.bincount(uu, minlength=ds.num_users)
    cell = collections.Counter(zip(uu.tolist(), pp.tolist()))
    chi2, dof = 0.0, 0
    for a, items in sets.items():
        if drawn[a] == 0 or len(items) < 2:
            continue
        e = drawn[a] / len(items)
        chi2 += sum((cell.get((a, it), 0) - e) ** 2 / e for it in items)
        dof += len(items) - 1
    assert dof > 1000 and abs(chi2 - dof) < 5 * np.sqrt(2 * dof), (chi2, dof)
    # a new epoch draws a new stream; the same (seed, epoch) replays
    u2, _, _ = smp.sample_epoch()
    assert not np.array_equal(u2.cpu().numpy(), u)
    smp2 = PairwiseSamplerV2(ds, batch_size=512, device=DEV, seed=7)
    assert np.array_equal(smp2.sample_epoch()[0].cpu().numpy(), u)


def test_rank_metrics_and_topk_known_answers():
    """Device top-K + metric kernels against the reference's own outputs (tests/golden/metrics.npz)."""
    from elimrec_amd import ops
    from oracle import eval_oracle as ev
    g = load_golden("metrics")
    for c in range(int(g["n_cases"])):
        s, k = g["case%d/scores" % c], int(g["case%d/top_k" % c])
        tp, ti = g["case%d/truth_ptr" % c], g["case%d/truth_items" % c]
        _, ref_topk = ev.evaluate_matrix(s, tp, ti, [1, 2, 3, 4, 5], k)
        out = torch.empty(s.shape[0], 5 * k, device=DEV)
        ops.rank_metrics(_t(ref_topk), _t(tp), _t(ti), [1, 2, 3, 4, 5], out)
        assert np.abs(out.cpu().numpy() - g["case%d/result" % c]).max() < 1e-7, c   # same ranking -> same metrics


def test_driver_runs_epochs_with_eval_and_checkpoint(tmp_path):
    """main.py's Net.run on a small synthetic data set: trains, validates every test_step epochs,
    saves the best checkpoint with the reference's state_dict keys, reports TE and TIE test lines."""
    import sys
    from helpers import ROOT
    sys.path.insert(0, ROOT)
    import importlib
    main = importlib.import_module("main")
    from elimrec_amd import Configurator, set_seed
    import os
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        args = Configurator(os.path.join(ROOT, "NeuRec.properties"), default_section="hyperparameters",
                            argv=["main.py", "--data.input.dataset=synthetic", "--alpha=0.5", "--loss=bpr_loss",
                                  "--synthetic_shape=[300,500,6000]", "--synthetic_dims=[16,8,12]", "--recdim=32",
                                  "--batch_size=512", "--num_epoch=4", "--test_step=2", "--verbose=0",
                                  "--path=%s" % str(tmp_path / "ck")])
        set_seed(args["seed"])
        net = main.Net(args)
        best, final = net.run()
    finally:
        os.chdir(cwd)
    assert best["TIE"] > 0 and final["TE"].strip().startswith("[TE]") and final["TIE"].strip().startswith("[TIE]")
    ck = torch.load(net.recommender.getFileName(), map_location="cpu")
    assert set(ck.keys()) == set(net.recommender.state_dict().keys())
    assert "embedding_user.weight" in ck and "s_dense_t.bias" in ck


@pytest.mark.parametrize("L", [1, 2, 3, 4])
@pytest.mark.parametrize("d,M", [(64, 4), (32, 2), (16, 3), (128, 4), (256, 2)])
def test_bipartite_propagation_equals_full_propagation(L, d, M):
    """Forward: Out from the bipartite (wide + narrow chain) kernels == Out from the generic
    full-table kernels == fp64 reference. Backward: the adjoint pair (gXI, gE_u) == the gradients
    obtained by propagating the full gradient table with A^T. Non-symmetric blocks (gcmc-like)."""
    import scipy.sparse as sp
    from elimrec_amd import ops
    U, I = 700, 1100
    rs = np.random.RandomState(L * 100 + d + M)
    nnz = 9000
    ru, ci = rs.randint(U, size=nnz), (rs.zipf(1.5, size=nnz) - 1) % I
    P = sp.csr_matrix((rs.rand(nnz).astype(np.float32), (ru, ci)), shape=(U, I))
    P.sum_duplicates()
    Q = sp.csr_matrix(P.T.multiply(rs.rand(I, 1).astype(np.float32) + 0.5)).astype(np.float32)   # not P^T
    A = sp.bmat([[None, P], [Q, None]]).tocsr().astype(np.float32)
    C = d * M
    gen = torch.Generator().manual_seed(5)
    Eu, XI = torch.randn(U, d, generator=gen), torch.randn(I, C, generator=gen)
    X0 = torch.cat([Eu.repeat(1, M), XI]).contiguous()
    # reference in fp64
    Ad = torch.sparse_coo_tensor(np.vstack(A.nonzero()), np.asarray(A[A.nonzero()]).ravel(), A.shape).double()
    x = X0.double()
    acc = x.clone()
    for _ in range(L):
        x = torch.sparse.mm(Ad, x)
        acc += x
    want = acc / (L + 1)
    # full-table HIP path
    full = ops.Csr.from_scipy(A, DEV, C=C, threshold=32)
    X0d = X0.to(DEV)
    t0, t1, out_full = torch.empty_like(X0d), torch.empty_like(X0d), torch.empty_like(X0d)
    ops.propagate(full, X0d, L, t0, t1, out_full)
    # bipartite HIP path
    Pd, Qd = ops.Csr.from_scipy(P, DEV, C=C, threshold=32), ops.Csr.from_scipy(Q, DEV, C=C, threshold=32)
    ws = torch.empty(ops.bipartite_workspace(U, I, d, M), dtype=torch.uint8, device=DEV)
    out_bip = torch.empty_like(X0d)
    ops.propagate_bipartite(Pd, Qd, U, I, d, M, L, Eu.to(DEV), XI.to(DEV), out_bip, ws)
    assert rel_err(out_full.cpu(), want) < 2e-6
    assert rel_err(out_bip.cpu(), want) < 2e-6
    from elimrec_amd import _lib
    _lib.load().elimrec_set_concurrency(1)          # d-column chain on the side stream: same bits
    try:
        out_side = torch.empty_like(X0d)
        ops.propagate_bipartite(Pd, Qd, U, I, d, M, L, Eu.to(DEV), XI.to(DEV), out_side, ws)
        torch.cuda.synchronize()
        assert torch.equal(out_side, out_bip)
    finally:
        _lib.load().elimrec_set_concurrency(0)
    # ---- adjoint: sparse G (60 active rows), garbage elsewhere (must never be read)
    act = np.sort(rs.choice(U + I, size=60, replace=False)).astype(np.int32)
    G = torch.full((U + I, C), float("nan"))
    G[act.astype(np.int64)] = torch.randn(len(act), C, generator=gen)
    Gz = torch.nan_to_num(G, nan=0.0).double()
    g = Gz.clone()
    accg = g.clone()
    At = Ad.t().coalesce()
    for _ in range(L):
        g = torch.sparse.mm(At, g)
        accg += g
    gX0 = accg / (L + 1)
    want_gXI = gX0[U:]
    want_gEu = gX0[:U].view(U, M, d).sum(1)
    n_max = 100
    act_d = torch.zeros(n_max, dtype=torch.int32, device=DEV)
    act_d[:len(act)] = torch.from_numpy(act).to(DEV)
    seg = torch.tensor([len(act), int((act < U).sum()), 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=DEV)
    Gd = G.to(DEV)
    H = torch.full((U + I, d), float("nan"), device=DEV)
    ops.blocksum_rows(Gd, act_d, seg, d, M, H)
    PT, QT = ops.Csr.from_scipy(P.T.tocsr(), DEV, C=C, threshold=32), ops.Csr.from_scipy(Q.T.tocsr(), DEV, C=C, threshold=32)
    gXI = torch.empty(I, C, device=DEV)
    gEu = torch.empty(U, d, device=DEV)
    ops.propagate_bipartite_bwd(PT, QT, U, I, d, M, L, Gd, H, act_d, seg, gXI, gEu, ws)
    assert torch.isfinite(gXI).all() and torch.isfinite(gEu).all()
    assert rel_err(gXI.cpu(), want_gXI) < 5e-6
    assert rel_err(gEu.cpu(), want_gEu) < 5e-6


def test_model_paths_agree_on_gcmc_adjacency():
    """adj_type=gcmc is bipartite but NOT symmetric: the bipartite path (with explicit P^T/Q^T
    blocks) must give the same loss and gradients as the generic full-table path and the oracle."""
    from helpers import FixtureDataset, fixture_argv, make_config, feats_of
    from elimrec_amd import EliMRec
    from oracle import elimrec_oracle as eo
    g = load_golden("ml3")
    argv = [a for a in fixture_argv(g) if not a.startswith("--adj_type")] + ["--adj_type=gcmc"]
    u, p, n = (_t(g["step1/%s" % k]) for k in ("users", "pos", "neg"))
    res = {}
    for mode in ("auto", "bipartite", "full"):
        cfg = make_config(argv + ["--propagation=%s" % mode])
        model = EliMRec(cfg, FixtureDataset(g))
        model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sub(g, "init").items()})
        model = model.to(DEV)
        assert model._bipartite == (mode != "full") and model._folded == (mode == "auto") and not model._adj_symmetric
        loss = model.bpr_loss(u, p, n)
        loss.backward()
        res[mode] = (loss.item(), {k: q.grad.cpu() for k, q in model.named_parameters() if q.grad is not None})
    adj = eo.build_adj(g["train_u"], g["train_i"], int(g["num_users"]), int(g["num_items"]), "gcmc")
    feats = {k: eo.OracleEliMRec.normalize_features(v) for k, v in feats_of(g).items()}
    om = eo.OracleEliMRec(int(g["num_users"]), int(g["num_items"]), int(g["recdim"]), int(g["layer_num"]), adj, feats,
                          sub(g, "init"), float(g["alpha"]))
    ol = om.bpr_loss(g["step1/users"], g["step1/pos"], g["step1/neg"])
    ol.backward()
    for mode in ("auto", "bipartite", "full"):
        assert abs(res[mode][0] - float(ol)) < 1e-5
        assert set(res[mode][1]) == set(om.grads())
        for k, v in om.grads().items():
            assert_grad_close(res[mode][1][k], v, (mode, k))


# ----------------------------------------------------------------------------- BASELINE.json shapes
def _full_shape_step(U, I, E, dims, recdim, B, dataset_name, extra_argv=()):
    """One full training step at a BASELINE.json shape: HIP path vs the CPU oracle on identical
    synthetic data, parameters and triplets (loss 1e-5 abs, every gradient 1e-4 rel)."""
    import os
    from helpers import make_config
    from elimrec_amd import EliMRec, SyntheticDataset, set_seed
    from oracle import elimrec_oracle as eo
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    cfg = make_config(["--data.input.dataset=%s" % dataset_name, "--alpha=0.5", "--loss=bpr_loss", "--recdim=%d" % recdim,
                       "--verbose=0"] + list(extra_argv))
    ds = SyntheticDataset(U, I, E, feat_dims=dims, seed=1, name=dataset_name)
    set_seed(7)
    model = EliMRec(cfg, ds)
    init = {k: v.detach().clone().numpy() for k, v in model.state_dict().items()}
    model = model.to(DEV)
    g = torch.Generator().manual_seed(3)
    train = ds.train_matrix.tocoo()
    pick = torch.randint(0, train.nnz, (B,), generator=g).numpy()
    u = torch.from_numpy(train.row[pick].astype(np.int64))
    p = torch.from_numpy(train.col[pick].astype(np.int64))
    n = torch.randint(0, I, (B,), generator=g)
    loss = model.bpr_loss(u.to(DEV), p.to(DEV), n.to(DEV))
    loss.backward()
    tu, ti = ds.get_train_interactions()
    adj = eo.build_adj(tu, ti, U, I, cfg["adj_type"])
    mods = ["v"] if dataset_name == "kwai" else ["v", "a", "t"]
    feats = {m: eo.OracleEliMRec.normalize_features(getattr(ds, m + "_feat")) for m in mods}
    om = eo.OracleEliMRec(U, I, recdim, cfg["layer_num"], adj, feats, init, cfg["alpha"], dataset_name=dataset_name)
    ol = om.bpr_loss(u, p, n)
    ol.backward()
    assert abs(loss.item() - float(ol.detach())) < 1e-5
    mine = {k: q.grad.cpu() for k, q in model.named_parameters() if q.grad is not None}
    want = om.grads()
    assert set(mine) == set(want)
    truth = None
    if U * recdim <= 1 << 20:       # small shapes: the same step in fp64, the arbiter of rows where fp32 sums cancel
        om64 = eo.OracleEliMRec(U, I, recdim, cfg["layer_num"], adj, feats, init, cfg["alpha"], dataset_name=dataset_name,
                                dtype=torch.float64)
        om64.bpr_loss(u, p, n).backward()
        truth = om64.grads()
    for k, v in want.items():
        assert_grad_close(mine[k], v, k, truth=None if truth is None else truth[k])
    model._test_case = dict(cfg=cfg, ds=ds, init=init, batch=(u, p, n), loss=loss.item(), grads=mine)
    return model, om


@pytest.mark.parametrize("L,recdim,B,dims", [(1, 64, 257, (24, 8, 12)), (2, 32, 1000, (36, 4, 20)), (4, 64, 513, (8, 8, 8)),
                                             (3, 16, 64, (100, 12, 4)), (2, 128, 300, (16, 16, 16)), (3, 64, 1, (8, 8, 8)),
                                             (3, 32, 3, (8, 12, 4))])
def test_small_shapes_layers_and_widths_vs_oracle(L, recdim, B, dims):
    """Layer counts 1..4 (L = 1 runs the eager tables, L = 2 ends on the hop that forms N02, L = 4 adds a second
    user-side term to the shared part), recdim 16..128 (lane groups of 4..32, VALU and MFMA head kernels), ragged
    feature widths and batch sizes: one step vs the oracle, then predict() through the lazily materialised tables."""
    model, om = _full_shape_step(700, 1900, 9000, dims, recdim, B, "synthetic", extra_argv=["--layer_num=%d" % L])
    assert model._lazy == (L >= 2)
    users = list(range(0, 700, 13))[:40]
    for ptype in ("normal", "TIE"):
        model.predict_type = om.predict_type = ptype
        assert np.abs(model.predict(users).numpy() - om.predict(users).numpy()).max() < 1e-5


def test_full_tiktok_shape_step_vs_oracle():
    """BASELINE.json configs[1]: |U|=36 656, |I|=76 085, 128-d x3, recdim 64, B=2048."""
    model, om = _full_shape_step(36656, 76085, 720829, (128, 128, 128), 64, 2048, "synthetic")
    # and the cached tables feed the same counterfactual scores (TIE) for a block of users
    users = list(range(0, 36656, 300))[:64]
    model.predict_type = om.predict_type = "TIE"
    assert np.abs(model.predict(users).numpy() - om.predict(users).numpy()).max() < 1e-5


def test_full_tiktok_shape_with_bf16_feature_storage():
    """BASELINE.json configs[1] as labelled ("bf16"): the V / A / T feature constants STORED in bf16 (--feature_dtype=bf16),
    all arithmetic fp32, at the full Tiktok shape. Two statements: (1) what the mode computes -- the fp32 engine on constants
    rounded to bf16, to the last bits of c's hi + lo split (loss 2e-6, gradients 1e-4 row-wise); (2) the mode's stated
    tolerance against the unrounded reference arithmetic (the oracle): loss 2e-3 abs, every gradient 2e-2 max-norm and row
    by row."""
    from helpers import make_config
    from elimrec_amd import EliMRec, set_seed
    model32, om = _full_shape_step(36656, 76085, 720829, (128, 128, 128), 64, 2048, "synthetic")
    case = model32._test_case
    u, p, n = (t.to(DEV) for t in case["batch"])
    want = om.grads()
    res = {}
    for mode in ("stored", "rounded"):
        argv = ["--data.input.dataset=synthetic", "--alpha=0.5", "--loss=bpr_loss", "--recdim=64", "--verbose=0"]
        set_seed(7)
        model = EliMRec(make_config(argv + (["--feature_dtype=bf16"] if mode == "stored" else [])), case["ds"])
        model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in case["init"].items()})
        model = model.to(DEV)
        eng = model.plugin.ensure_engine()
        assert eng.feature_dtype == ("bf16" if mode == "stored" else "f32")
        if mode == "rounded":
            fold = model._ws["fold"]
            for k in model._mods:
                fold[k].copy_(fold[k].to(torch.bfloat16).float())
        loss = model.bpr_loss(u, p, n)
        loss.backward()
        res[mode] = (loss.item(), {k: q.grad.cpu().clone() for k, q in model.named_parameters() if q.grad is not None})
    assert abs(res["stored"][0] - res["rounded"][0]) < 2e-6
    assert set(res["stored"][1]) == set(res["rounded"][1]) == set(want)
    for k, v in res["rounded"][1].items():
        assert_grad_close(res["stored"][1][k], v, ("bf16 storage vs fp32 engine on rounded constants", k))
    assert res["stored"][0] != case["loss"]                                  # the storage really is 16-bit
    assert abs(res["stored"][0] - float(om.bpr_loss(*case["batch"]).detach())) < 2e-3
    for k, v in want.items():
        assert_grad_close(res["stored"][1][k], v, ("bf16 storage vs the oracle", k), rel=2e-2)


def test_full_kwai_shape_step_vs_oracle():
    """BASELINE.json configs[2], reference-parity variant: id + V only (dataset name 'kwai'), D_v = 2048."""
    _full_shape_step(7010, 86483, 298492, (2048,), 64, 2048, "kwai")


def test_full_movielens_shape_step_vs_oracle():
    """BASELINE.json configs[0]: MovieLens shape, D = (2048, 128, 100), recdim 64, batch 1024."""
    _full_shape_step(55485, 5986, 1239508, (2048, 128, 100), 64, 1024, "movielens")


def test_data_parallel_math_on_one_gpu():
    """What the ranks of a 2-rank job compute (elimrec_amd/dist.py: the unfolded row-major forms) emulated on one GPU: the
    whole backward on the concatenated head-gradient rows of both ranks equals the single-GPU step on the whole batch."""
    g = load_golden("ml3")
    extra = ["--head_rows=all"]
    u, p, n = (_t(g["step1/%s" % k]) for k in ("users", "pos", "neg"))
    half = (len(u) // 2)
    whole, _ = build_model_from_fixture(g, DEV, extra_argv=extra)
    assert not whole._lazy
    loss_w, rows_w = whole.forward_local(u[:2 * half], p[:2 * half], n[:2 * half])
    grads_w = {k: v.clone() for k, v in whole.backward_global(rows_w, torch.ones(1, device=DEV)).items()}
    dp, _ = build_model_from_fixture(g, DEV, extra_argv=extra)
    dp._workspace(half, 6 * half)
    all_keys = torch.cat([dp.batch_keys(u[r * half:(r + 1) * half], p[r * half:(r + 1) * half],
                                        n[r * half:(r + 1) * half]).clone() for r in range(2)])
    rows, losses = [], []
    for r in range(2):
        sl = slice(r * half, (r + 1) * half)
        loss, gr = dp.forward_local(u[sl], p[sl], n[sl], all_keys=all_keys, rank=r, world_size=2)
        rows.append(gr.clone()); losses.append(loss.clone())
    grads_dp = dp.backward_global(torch.cat(rows), torch.full((1,), 0.5, device=DEV))
    assert abs(float(loss_w) - float((losses[0] + losses[1]) / 2)) < 1e-6
    assert set(grads_w) == set(grads_dp)
    for k in grads_w:
        assert rel_err(grads_dp[k].cpu(), grads_w[k].cpu()) < 1e-5, k
    lazy, _ = build_model_from_fixture(g, DEV)
    with pytest.raises(RuntimeError, match="column-shard engine"):
        lazy.forward_local(u, p, n)


def test_kwai_shape_v_plus_t_variant_vs_oracle():
    """BASELINE.json configs[2] as stated ("V+T only"): id + V + T tables (M = 3, two single-modal heads)
    via --feature_modalities=vt. The reference itself cannot run this combination, so this checks the HIP
    path against the oracle's generalisation only (unpinned; see oracle/elimrec_oracle.py)."""
    import os
    from helpers import make_config
    from elimrec_amd import EliMRec, SyntheticDataset, set_seed
    from oracle import elimrec_oracle as eo
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    U, I, B = 7010, 86483, 2048
    cfg = make_config(["--data.input.dataset=kwai_vt", "--alpha=0.5", "--loss=bpr_loss", "--verbose=0",
                       "--feature_modalities=vt", "--modality=vt"])
    ds = SyntheticDataset(U, I, 298492, feat_dims=(2048, 4, 128), seed=1, name="kwai_vt")
    set_seed(5)
    model = EliMRec(cfg, ds)
    assert model.M == 3 and model.S == 2 and not hasattr(model, "a_dense")
    init = {k: v.detach().clone().numpy() for k, v in model.state_dict().items()}
    model = model.to(DEV)
    g = torch.Generator().manual_seed(3)
    train = ds.train_matrix.tocoo()
    pick = torch.randint(0, train.nnz, (B,), generator=g).numpy()
    u = torch.from_numpy(train.row[pick].astype(np.int64)); p = torch.from_numpy(train.col[pick].astype(np.int64))
    n = torch.randint(0, I, (B,), generator=g)
    loss = model.bpr_loss(u.to(DEV), p.to(DEV), n.to(DEV))
    loss.backward()
    tu, ti = ds.get_train_interactions()
    adj = eo.build_adj(tu, ti, U, I, cfg["adj_type"])
    feats = {m: eo.OracleEliMRec.normalize_features(getattr(ds, m + "_feat")) for m in "vt"}
    om = eo.OracleEliMRec(U, I, cfg["recdim"], cfg["layer_num"], adj, feats, init, cfg["alpha"], modality="vt", mods="vt")
    ol = om.bpr_loss(u, p, n)
    ol.backward()
    assert abs(loss.item() - float(ol.detach())) < 1e-5
    mine = {k: q.grad.cpu() for k, q in model.named_parameters() if q.grad is not None}
    assert set(mine) == set(om.grads())
    for k, v in om.grads().items():
        assert_grad_close(mine[k], v, k)
    users = list(range(0, U, 111))[:48]
    for ptype in ("TE", "TIE"):
        model.predict_type = om.predict_type = ptype
        assert np.abs(model.predict(users).numpy() - om.predict(users).numpy()).max() < 1e-5


def test_block_spmm_on_a_column_window():
    """elimrec_block_spmm on a strided column window of wider tables == fp64 reference; columns outside
    the window are untouched."""
    import scipy.sparse as sp
    from elimrec_amd import ops
    rs = np.random.RandomState(4)
    R, S_, W, ld = 900, 1300, 48, 160
    m = sp.random(R, S_, density=0.01, random_state=rs, format="csr", dtype=np.float32)
    m = (m + sp.csr_matrix((np.ones(S_, np.float32), (np.zeros(S_, int), np.arange(S_))), shape=(R, S_))).tocsr()  # one long row
    A = ops.Csr.from_scipy(m, DEV, C=ld, threshold=64)
    g = torch.Generator().manual_seed(2)
    Xin, Add = torch.randn(S_, ld, generator=g), torch.randn(R, ld, generator=g)
    Xout, Acc = torch.full((R, ld), 7.0), torch.full((R, ld), 9.0)
    Xin_d, Add_d, Xout_d, Acc_d = (t.to(DEV) for t in (Xin, Add, Xout, Acc))
    c0 = 32
    ops.block_spmm(A, Xin_d[:, c0:c0 + W], Xout=Xout_d[:, c0:c0 + W], add1=Add_d[:, c0:c0 + W],
                   acc_out=Acc_d[:, c0:c0 + W], scale=0.5)
    want = torch.from_numpy(m.astype(np.float64) @ Xin[:, c0:c0 + W].double().numpy())
    assert rel_err(Xout_d[:, c0:c0 + W].cpu(), want) < 2e-6
    assert rel_err(Acc_d[:, c0:c0 + W].cpu(), (want + Add[:, c0:c0 + W].double()) * 0.5) < 2e-6
    for t, v in ((Xout_d, 7.0), (Acc_d, 9.0)):
        assert (t[:, :c0] == v).all() and (t[:, c0 + W:] == v).all()


def test_topk_paths_agree_with_stable_sort():
    """Device top-K = first K of a stable sort by (score desc, item id asc), whichever internal path runs:
    continuous scores (two-sweep select), massive ties and rows with fewer than K unmasked items (K-round
    fallback), K from 1 to 100."""
    from elimrec_amd import ops
    U, I, d, S = 40, 5000, 16, 3
    Cy = (1 + S) * d
    g = torch.Generator().manual_seed(11)
    Yr = torch.randn(U + I, Cy, generator=g)
    Yt = Yr.clone()
    Yt[U:] = Yt[U:U + 7].repeat((I + 6) // 7, 1)[:I]            # only 7 distinct item rows -> massive ties
    users = torch.arange(0, 33)
    B = len(users)
    # row 5: everything but 4 items masked; row 6: nothing masked
    ptr = torch.zeros(B + 1, dtype=torch.int64)
    masked = torch.tensor([i for i in range(I) if i not in (17, 4000, 3, 999)], dtype=torch.int32)
    ptr[6:] = len(masked)
    for Y in (Yr, Yt):
        for K in (1, 10, 50, 100):
            Yd = Y.to(DEV)
            ws = torch.empty(ops.score_workspace(B, U, I, S, K), dtype=torch.uint8, device=DEV)
            scores = torch.empty(B, I, device=DEV)
            idx = torch.empty(B, K, dtype=torch.int32, device=DEV)
            val = torch.empty(B, K, device=DEV)
            ops.score_topk(Yd, U, I, users.to(DEV), d, S, 0b111, "rubi", "TIE", ws, scores=scores, K=K, topk_idx=idx,
                           topk_val=val, train_ptr=ptr.to(DEV), train_items=masked.to(DEV))
            sc = scores.cpu().numpy()
            assert np.isinf(sc[5]).sum() == I - 4 and not np.isinf(sc[6]).any()
            order = np.argsort(-sc, axis=1, kind="stable")[:, :K]
            assert np.array_equal(idx.cpu().numpy(), order), (K, Y is Yt)
            assert np.array_equal(val.cpu().numpy(), np.take_along_axis(sc, order, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("with_scores,d,I", [(True, 64, 3000), (False, 64, 3000), (False, 128, 3000), (True, 32, 3000),
                                             (False, 64, 40000), (False, 32, 33000)])
def test_tile_guided_topk_at_recdim_64(with_scores, d, I):
    """The evaluator's own configuration (recdim 32 / 64 / 128: 16-user-per-wave scorer, selection from tile maxima, bitmap masking)
    against a stable sort of the full masked score matrix: continuous scores and massive ties; rows with nothing, a few,
    hundreds (K + masked > 256 group maxima -> fall-back) and all-but-4 items masked; 200 users (two user groups per
    launch); with the caller's score matrix and with the private one (top-K only). I > 16384 without a score matrix: the
    catalogue is scored in chunks (no [B x I] block in the workspace), per-chunk top-K lists merged -- the same lists.
    Absolute accuracy: see test_score_fp64_gpu.py."""
    from elimrec_amd import ops
    U, S = 260, 3
    Cy = (1 + S) * d
    g = torch.Generator().manual_seed(5)
    Yr = torch.randn(U + I, Cy, generator=g) * 0.3
    Yt = Yr.clone()
    Yt[U:] = Yt[U:U + 9].repeat((I + 8) // 9, 1)[:I]            # 9 distinct item rows -> massive ties
    users = torch.arange(0, 200)
    B = len(users)
    lists = [[] for _ in range(B)]
    lists[3] = [5, 17, I - 1, 1024]
    lists[5] = [i for i in range(I) if i not in (17, 2000, 3, 999)]
    lists[7] = list(range(0, 900, 3))                            # 300 masked items
    lists[8] = [11, 11, 12]                                      # a duplicate
    rng = np.random.default_rng(0)
    for b in range(20, 200):
        lists[b] = rng.choice(I, size=int(rng.integers(0, 40)), replace=False).tolist()
    ptr = torch.zeros(B + 1, dtype=torch.int64)
    ptr[1:] = torch.tensor(np.cumsum([len(x) for x in lists]))
    items = torch.tensor([i for x in lists for i in x], dtype=torch.int32)
    for Y in (Yr, Yt):
        Yd = Y.to(DEV)
        ref = torch.empty(B, I, device=DEV)
        ws = torch.empty(ops.score_workspace(B, U, I, S, 1), dtype=torch.uint8, device=DEV)
        ops.score_topk(Yd, U, I, users.to(DEV), d, S, 0b111, "rubi", "TIE", ws, scores=ref, train_ptr=ptr.to(DEV),
                       train_items=items.to(DEV))
        sc = ref.cpu().numpy()
        for b in (3, 5, 7, 8):
            assert np.isinf(sc[b]).sum() == len(set(lists[b]))
        for K in (1, 10, 50, 100):
            ws = torch.empty(ops.score_workspace(B, U, I, S, K, topk_only=not with_scores), dtype=torch.uint8, device=DEV)
            if not with_scores and I > 16384:
                assert ws.numel() < B * I * 4            # no [B x I] score block
            scores = torch.empty(B, I, device=DEV) if with_scores else None
            idx = torch.empty(B, K, dtype=torch.int32, device=DEV)
            val = torch.empty(B, K, device=DEV)
            ops.score_topk(Yd, U, I, users.to(DEV), d, S, 0b111, "rubi", "TIE", ws, scores=scores, K=K, topk_idx=idx,
                           topk_val=val, train_ptr=ptr.to(DEV), train_items=items.to(DEV))
            if with_scores:
                assert np.array_equal(scores.cpu().numpy(), sc)
            order = np.argsort(-sc, axis=1, kind="stable")[:, :K]
            got = idx.cpu().numpy()
            full = np.isfinite(np.take_along_axis(sc, order, 1)).all(1)      # rows with at least K unmasked items
            assert np.array_equal(got[full], order[full]), (K, Y is Yt)
            assert np.array_equal(val.cpu().numpy()[full], np.take_along_axis(sc, order, 1)[full])
            assert not full[5] or K <= 4


@pytest.mark.gpu
def test_fast_evaluation_math_is_close_and_ranks_alike():
    """elimrec_score_set_math(1), the default: sigmoids through v_exp_f32 (two-float argument product) and v_rcp_f32 + one
    Newton step, reciprocal norms. Scores within 4e-7 of the EXACT mode (IEEE division, libm expf) in all three fusion
    modes; top-K lists differ only where two EXACT scores are closer than that.
    Absolute accuracy: see test_score_fp64_gpu.py."""
    from elimrec_amd import _lib, ops
    lib = _lib.load()
    U, I, d, S, K = 130, 4000, 64, 3, 20
    g = torch.Generator().manual_seed(9)
    Y = (torch.randn(U + I, (1 + S) * d, generator=g) * 0.4).to(DEV)
    Y[U:U + 40] *= 6.0                              # dot products beyond +-88: the saturated ends of the sigmoid
    users = torch.arange(0, 128).to(DEV)
    ws = torch.empty(ops.score_workspace(128, U, I, S, K), dtype=torch.uint8, device=DEV)
    before = int(lib.elimrec_score_get_math())
    assert before == 1 or os.environ.get("ELIMREC_EVAL_MATH", "")[:1] in ("e", "0")
    try:
        for mode in ("rubi", "hm", "sum"):
            for ptype in ("normal", "TE", "TIE"):
                out = {}
                for fast in (0, 1):
                    lib.elimrec_score_set_math(fast)
                    sc = torch.empty(128, I, device=DEV)
                    idx = torch.empty(128, K, dtype=torch.int32, device=DEV)
                    ops.score_topk(Y, U, I, users, d, S, 0b111, mode, ptype, ws, scores=sc, K=K, topk_idx=idx)
                    out[fast] = (sc.cpu().numpy(), idx.cpu().numpy())
                e, f = out[0][0], out[1][0]
                assert np.isfinite(f).all() and np.abs(e - f).max() < 4e-7, (mode, ptype, np.abs(e - f).max())
                for r in np.nonzero((out[0][1] != out[1][1]).any(1))[0]:
                    a, b = out[0][1][r], out[1][1][r]
                    assert np.abs(e[r][a] - e[r][b]).max() < 8e-7, (mode, ptype, r)
    finally:
        lib.elimrec_score_set_math(before)


@pytest.mark.gpu
def test_evaluator_results_do_not_depend_on_the_users_per_launch(monkeypatch):
    """The device evaluator scores 1024 users per launch where the reference's test_batch_size is 128: same metric rows."""
    g = load_golden("ml3")
    model, _ = build_model_from_fixture(g, DEV)
    _load_cache(model, g)
    model.fusion_mode, model.predict_type = "rubi", "TIE"
    evalr = model.test_evaluator.evaluator
    users = list(evalr.user_pos_test.keys())
    res = {}
    for blk in (7, 128, 4096):
        evalr.block_users = blk
        res[blk], _ = evalr.evaluate(model, users[:])
    assert np.array_equal(res[7], res[128]) and np.array_equal(res[128], res[4096])


@pytest.mark.gpu
def test_rank_sharded_evaluation_equals_one_process():
    """Multi-GPU validation: every rank scores a contiguous slice of the users and the zero-filled metric-row matrices
    are summed (all_reduce) -- simulated here by adding the W matrices on one GPU: bitwise the single-process rows."""
    g = load_golden("ml3")
    model, _ = build_model_from_fixture(g, DEV)
    _load_cache(model, g)
    model.fusion_mode, model.predict_type = "rubi", "TIE"
    evalr = model.test_evaluator.evaluator
    users = list(evalr.user_pos_test.keys())
    whole = evalr.metric_rows(model, users)
    for W in (2, 3, 8):
        parts = [evalr.metric_rows(model, users, shard=(r, W), reduce=False) for r in range(W)]
        assert torch.equal(sum(parts[1:], parts[0]), whole), W
    res, buf = evalr.evaluate(model)
    assert np.array_equal(res, np.mean(whole.cpu().numpy(), axis=0).reshape(evalr.metrics_num, evalr.max_top)[:, evalr.top_show - 1].reshape(-1))


@pytest.mark.gpu
@pytest.mark.parametrize("d,K", [(48, 10), (64, 300), (256, 10), (64, 10)])
def test_topk_only_workspace_fits_any_recdim_and_k(d, K):
    """top-K only at I > 16384 with a recdim outside the 16-user-per-wave scorer's set (48, 256) or
    K > 256 takes the whole-catalogue form; ops.score_workspace(..., topk_only=True, d=d) asks the library's own predicate
    and returns a workspace that fits (the reference accepts any recdim and any K, models/EliMRec.py:96-113). The lists
    equal a stable sort of the full masked score matrix.
    Absolute accuracy: see test_score_fp64_gpu.py."""
    from elimrec_amd import ops
    U, I, S = 40, 20000, 3
    g = torch.Generator().manual_seed(d + K)
    Y = (torch.randn(U + I, (1 + S) * d, generator=g) * 0.3).to(DEV)
    users = torch.arange(0, 33).to(DEV)
    B = 33
    ptr = torch.zeros(B + 1, dtype=torch.int64)
    masked = torch.tensor([5, 17, 19999, 1024], dtype=torch.int32)
    ptr[4:] = len(masked)
    ref = torch.empty(B, I, device=DEV)
    ws = torch.empty(ops.score_workspace(B, U, I, S, K), dtype=torch.uint8, device=DEV)
    ops.score_topk(Y, U, I, users, d, S, 0b111, "rubi", "TIE", ws, scores=ref, train_ptr=ptr.to(DEV), train_items=masked.to(DEV))
    sc = ref.cpu().numpy()
    need = ops.score_workspace(B, U, I, S, K, topk_only=True, d=d)
    chunked_bytes = ops.score_workspace(B, U, I, S, K, topk_only=True)
    if d in (32, 64, 128) and K <= 256:      # the chunked layout (+ one chunk's bf16 pieces for the recdim 32 / 64 scorer)
        assert chunked_bytes <= need <= chunked_bytes + 16384 * 3 * (1 + S) * d * 2 + 16384 * S * 4 + 512     # (+ its inverse item norms)
    else:                                    # the whole-catalogue layout (recdim 32 / 64: + room for one chunk's bf16 pieces, which
        full = ops.score_workspace(B, U, I, S, K)              # a score MATRIX of a catalogue beyond one chunk is scored through)
        assert full <= need <= full + (16384 * 3 * (1 + S) * d * 2 + 16384 * S * 4 + 512 if d in (32, 64) else 0)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    idx = torch.empty(B, K, dtype=torch.int32, device=DEV)
    val = torch.empty(B, K, device=DEV)
    ops.score_topk(Y, U, I, users, d, S, 0b111, "rubi", "TIE", ws, K=K, topk_idx=idx, topk_val=val, train_ptr=ptr.to(DEV),
                   train_items=masked.to(DEV))
    order = np.argsort(-sc, axis=1, kind="stable")[:, :K]
    from elimrec_amd import _lib
    # (recdim 32 / 64 with a workspace sized for the recdim: every call shape -- K beyond 256 too, since round 6 -- goes through the
    #  chunk launches on the bf16 matrix cores; `sc` above came from a workspace without room for the pieces: the fp32 form)
    b3 = d in (32, 64) and _lib.load().elimrec_score_get_math() == 1 and _lib.load().elimrec_score_get_bf16x3() == 1
    if not b3:
        assert np.array_equal(idx.cpu().numpy(), order)
        assert np.array_equal(val.cpu().numpy(), np.take_along_axis(sc, order, 1))
    else:       # the chunked form ran on the bf16 matrix cores (three-piece splits): the same scores to fp32 round-off
        got_i, got_v = idx.cpu().numpy(), val.cpu().numpy()
        assert np.abs(got_v - np.take_along_axis(sc, got_i, 1)).max() < 2.4e-7
        for r in np.nonzero((got_i != order).any(1))[0]:
            assert np.abs(sc[r][got_i[r]] - sc[r][order[r]]).max() < 4.8e-7, r
    # the reference's order on the same call shapes (K = 300: the whole-catalogue form with the item-by-item scan; recdim 48 / 256:
    # the generic scorer's masked matrix): the oracle's ranking of the matrix the SAME workspace shape returns
    ws_m = torch.empty(ops.score_workspace(B, U, I, S, K, d=d), dtype=torch.uint8, device=DEV)
    ops.score_topk(Y, U, I, users, d, S, 0b111, "rubi", "TIE", ws_m, scores=ref, train_ptr=ptr.to(DEV), train_items=masked.to(DEV))
    want = _reference_lists(ref.cpu().numpy(), K)
    ops.score_topk(Y, U, I, users, d, S, 0b111, "rubi", "TIE", ws, K=K, topk_idx=idx, topk_val=val, train_ptr=ptr.to(DEV),
                   train_items=masked.to(DEV), tie_order="reference")
    assert np.array_equal(idx.cpu().numpy(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 32])
@pytest.mark.parametrize("mode", ["rubi", "hm", "sum"])
def test_bf16x3_scorer_matches_exact_math(d, mode):
    """The FAST scorer of the evaluator's own configuration (chunked top-K, recdim 32 / 64) on the bf16 matrix cores --
    fp32 operands split exactly into three bf16 pieces, six piece products per dot product, fp32 accumulation -- against the
    EXACT mode (fp32 MFMA, IEEE division, libm expf) over a 40 000-item catalogue, normal / TE / TIE: every returned score
    within 2.4e-7 of the EXACT score of the same (user, item) -- FAST's own 1.2e-7 + the split form's round-off --, the top-20
    lists identical except where two EXACT scores are closer than 4.8e-7, masked items never returned; with the switch off the
    fp32-MFMA FAST scorer gives its own (equally close) lists.
    Absolute accuracy: see test_score_fp64_gpu.py."""
    from elimrec_amd import _lib, ops
    lib = _lib.load()
    U, I, S, K, B = 300, 40000, 3, 20, 200
    g = torch.Generator().manual_seed(d)
    Y = (torch.randn(U + I, (1 + S) * d, generator=g) * 0.4).to(DEV)
    Y[U:U + 40] *= 6.0                              # saturated sigmoids
    users = torch.randperm(U, generator=g)[:B].to(DEV)
    rng = np.random.default_rng(3)
    lists = [sorted(rng.choice(I, size=int(rng.integers(0, 50)), replace=False).tolist()) for _ in range(B)]
    ptr = np.zeros(B + 1, np.int64); ptr[1:] = np.cumsum([len(x) for x in lists])
    items = np.array([i for x in lists for i in x], np.int32)
    math0, b30 = int(lib.elimrec_score_get_math()), int(lib.elimrec_score_get_bf16x3())
    try:
        for ptype in ("normal", "TE", "TIE"):
            lib.elimrec_score_set_math(0)
            ref = torch.empty(B, I, device=DEV)
            ws = torch.empty(ops.score_workspace(B, U, I, S, K), dtype=torch.uint8, device=DEV)
            ops.score_topk(Y, U, I, users, d, S, 0b111, mode, ptype, ws, scores=ref, train_ptr=_t(ptr), train_items=_t(items))
            exact = ref.cpu().numpy()
            order = np.argsort(-exact, axis=1, kind="stable")[:, :K]
            lib.elimrec_score_set_math(1)
            out = {}
            for b3 in (1, 0):
                lib.elimrec_score_set_bf16x3(b3)
                ws = torch.empty(ops.score_workspace(B, U, I, S, K, topk_only=True, d=d), dtype=torch.uint8, device=DEV)
                idx = torch.empty(B, K, dtype=torch.int32, device=DEV)
                val = torch.empty(B, K, device=DEV)
                ops.score_topk(Y, U, I, users, d, S, 0b111, mode, ptype, ws, K=K, topk_idx=idx, topk_val=val, train_ptr=_t(ptr),
                               train_items=_t(items))
                gi, gv = idx.cpu().numpy(), val.cpu().numpy()
                at = np.take_along_axis(exact, gi, 1)
                assert np.isfinite(at).all(), (ptype, b3)                                  # no masked item in a list
                assert np.abs(gv - at).max() < 2.4e-7, (ptype, b3, np.abs(gv - at).max())
                for r in np.nonzero((gi != order).any(1))[0]:
                    assert np.abs(exact[r][gi[r]] - exact[r][order[r]]).max() < 4.8e-7, (ptype, b3, r)
                out[b3] = gv
            assert not np.array_equal(out[0], out[1]) or ptype == "normal"                 # two different arithmetic paths did run
    finally:
        lib.elimrec_score_set_math(math0)
        lib.elimrec_score_set_bf16x3(b30)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,ptype,d,reps", [("hm", "TIE", 64, 400), ("rubi", "TIE", 64, 100), ("sum", "TIE", 64, 100), ("hm", "TE", 64, 100),
                                                ("hm", "TIE", 32, 200), ("rubi", "normal", 32, 50)])
def test_bf16x3_scorer_is_stable_over_repeated_launches(mode, ptype, d, reps):
    """The same top-20 call, `reps` times on fresh workspaces: every launch returns the bits of the first, and the first
    is within 2.4e-7 of the EXACT scores. (Built with the SLP vectoriser's packed-fp32 forms, score_t16b_kernel<2,4,2,1,64>
    -- TIE, hm -- returned 1.0 for the 16 items of one tile on lanes 48-63 of one accumulator row about once in 150
    launches, more often early in a process; csrc/Makefile builds eval.hip without them.)
    Absolute accuracy: see test_score_fp64_gpu.py."""
    from elimrec_amd import _lib, ops
    lib = _lib.load()
    U, I, S, K, B = 300, 40000, 3, 20, 200
    g = torch.Generator().manual_seed(d)
    Y = (torch.randn(U + I, (1 + S) * d, generator=g) * 0.4).to(DEV)
    users = torch.randperm(U, generator=g)[:B].to(DEV)
    rng = np.random.default_rng(3)
    lists = [sorted(rng.choice(I, size=int(rng.integers(0, 50)), replace=False).tolist()) for _ in range(B)]
    ptr = np.zeros(B + 1, np.int64); ptr[1:] = np.cumsum([len(x) for x in lists])
    items = np.array([i for x in lists for i in x], np.int32)
    tp, ti = _t(ptr), _t(items)
    math0, b30 = int(lib.elimrec_score_get_math()), int(lib.elimrec_score_get_bf16x3())
    try:
        lib.elimrec_score_set_math(0)
        ref = torch.empty(B, I, device=DEV)
        ws = torch.empty(ops.score_workspace(B, U, I, S, K), dtype=torch.uint8, device=DEV)
        ops.score_topk(Y, U, I, users, d, S, 0b111, mode, ptype, ws, scores=ref, train_ptr=tp, train_items=ti)
        lib.elimrec_score_set_math(1)
        lib.elimrec_score_set_bf16x3(1)
        nbytes = ops.score_workspace(B, U, I, S, K, topk_only=True, d=d)
        first, differing = None, torch.zeros((), dtype=torch.int64, device=DEV)
        for rep in range(reps):
            ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
            idx = torch.empty(B, K, dtype=torch.int32, device=DEV)
            val = torch.empty(B, K, device=DEV)
            ops.score_topk(Y, U, I, users, d, S, 0b111, mode, ptype, ws, K=K, topk_idx=idx, topk_val=val, train_ptr=tp, train_items=ti)
            if first is None:
                first = (idx, val)
                assert (val - torch.gather(ref, 1, idx.long())).abs().max() < 2.4e-7
            else:
                differing += ((idx != first[0]).any() | (val != first[1]).any()).long()
        assert int(differing) == 0
    finally:
        lib.elimrec_score_set_math(math0)
        lib.elimrec_score_set_bf16x3(b30)


@pytest.mark.gpu
@pytest.mark.parametrize("d,ptype,W", [(64, "TIE", 3), (64, "TE", 2), (48, "TIE", 4), (128, "TIE", 2), (32, "normal", 5)])
def test_item_sharded_scoring_equals_whole_catalogue(d, ptype, W, eval_math):
    """elimrec_score_topk_shard on W emulated item shards (uneven blocks): phase 1 row sums added in rank order (the
    all_reduce), phase 2 scores / top-K per shard, elimrec_topk_merge of the W lists. The concatenated shard scores equal
    the whole-catalogue call's to 2e-7 (the NDE mean is the same sum split into W fixed-order partial sums), masks land on
    the same items, and the merged top-K IS the stable (score desc, id asc) ranking of those scores.
    Absolute accuracy: see test_score_fp64_gpu.py."""
    from elimrec_amd import ops
    U, I, S, K, B = 90, 7000, 3, 20, 70
    g = torch.Generator().manual_seed(d + W)
    Y = (torch.randn(U + I, (1 + S) * d, generator=g) * 0.3).to(DEV)
    users = torch.randperm(U, generator=g)[:B].to(DEV)
    rng = np.random.default_rng(1)
    lists = [sorted(rng.choice(I, size=int(rng.integers(0, 60)), replace=False).tolist()) for _ in range(B)]
    ptr = np.zeros(B + 1, np.int64); ptr[1:] = np.cumsum([len(x) for x in lists])
    items = np.array([i for x in lists for i in x], np.int32)
    whole = torch.empty(B, I, device=DEV)
    ws = torch.empty(ops.score_workspace(B, U, I, S, K), dtype=torch.uint8, device=DEV)
    ops.score_topk(Y, U, I, users, d, S, 0b111, "rubi", ptype, ws, scores=whole, train_ptr=_t(ptr), train_items=_t(items))
    bounds = [0] + sorted(rng.choice(np.arange(200, I - 200), size=W - 1, replace=False).tolist()) + [I]
    shards = []
    for o in range(W):
        i0, i1 = bounds[o], bounds[o + 1]
        Ysh = torch.cat([Y[:U], Y[U + i0:U + i1]]).contiguous()
        lp = np.zeros(B + 1, np.int64)
        loc = [[i - i0 for i in x if i0 <= i < i1] for x in lists]
        lp[1:] = np.cumsum([len(x) for x in loc])
        li = np.array([i for x in loc for i in x] + [0], np.int32)
        wsp = torch.empty(ops.score_workspace(B, U, i1 - i0, S, K), dtype=torch.uint8, device=DEV)
        shards.append((i0, i1, Ysh, _t(lp), _t(li), wsp))
    total = torch.zeros(B, device=DEV)
    for i0, i1, Ysh, lp, li, wsp in shards:                                   # phase 1 + the all_reduce, in rank order
        part = torch.zeros(B, device=DEV)
        ops.score_topk_shard(Ysh, U, i1 - i0, users, d, S, 0b111, "rubi", ptype, wsp, 1, part, I, i0)
        total += part
    cols, cand_i, cand_v = [], [], []
    for i0, i1, Ysh, lp, li, wsp in shards:
        sc = torch.empty(B, i1 - i0, device=DEV)
        idx = torch.empty(B, K, dtype=torch.int32, device=DEV)
        val = torch.empty(B, K, device=DEV)
        ops.score_topk_shard(Ysh, U, i1 - i0, users, d, S, 0b111, "rubi", ptype, wsp, 2, total, I, i0, scores=sc, K=K,
                             topk_idx=idx, topk_val=val, train_ptr=lp, train_items=li)
        cols.append(sc); cand_i.append(idx); cand_v.append(val)
    sharded = torch.cat(cols, dim=1).cpu().numpy()
    w = whole.cpu().numpy()
    assert np.array_equal(np.isinf(sharded), np.isinf(w))
    fin = ~np.isinf(w)
    assert np.abs(sharded[fin] - w[fin]).max() < 2e-7
    out_i = torch.empty(B, K, dtype=torch.int32, device=DEV)
    out_v = torch.empty(B, K, device=DEV)
    ops.topk_merge(torch.stack(cand_v, 1).reshape(B, W * K).contiguous(), torch.stack(cand_i, 1).reshape(B, W * K).contiguous(), K, out_i, out_v)
    order = np.argsort(-sharded, axis=1, kind="stable")[:, :K]
    assert np.array_equal(out_i.cpu().numpy(), order)
    assert np.array_equal(out_v.cpu().numpy(), np.take_along_axis(sharded, order, 1))


@pytest.mark.gpu
def test_device_evaluator_against_the_references_own_compiled_code(fixture_name):
    """oracle/_ref/libref_eval.so -- the reference's evaluate.h / metric.h / arg_topk.h compiled where they lie (never copied) --
    travels to the GPU box for this: the reference's C++ ranks and scores the DEVICE's own masked score matrix, and on every row
    where its heap-order top-K is the device's (score desc, id asc) top-K -- all rows without a tie at the K boundary -- the
    per-user metric rows agree bit for bit; the other rows hold the same scores rank by rank."""
    from oracle import eval_oracle as ev
    if ev.ref_lib() is None:
        pytest.skip("oracle/_ref/libref_eval.so was not built (needs /root/reference at build time)")
    g = load_golden(fixture_name)
    model, _ = build_model_from_fixture(g, DEV)
    _load_cache(model, g)
    model.fusion_mode, model.predict_type = "rubi", "TIE"
    users = g["evalbatch/users"].tolist()
    K = int(g["evalbatch/top_k"])
    mids = g["evalbatch/metric_ids"]
    evalr = model.test_evaluator.evaluator
    rows, idx, _ = evalr.evaluate_batch(model, users, return_topk=True)
    dev_scores = torch.empty(len(users), model.num_items, device=DEV)
    train_ptr, train_items = evalr._batch_csr(users, evalr.user_pos_train, DEV, unique=False)
    model.predict_device(users, scores=dev_scores, train_ptr=train_ptr, train_items=train_items)
    sc = np.ascontiguousarray(dev_scores.cpu().numpy())
    test = csr_dict(g, "test")
    tp, ti = ev.truth_to_csr([sorted(set(test[int(u)])) for u in users])
    ref_rows, ref_topk = ev.evaluate_matrix(sc.copy(), tp, ti, mids, K, use_ref=True)
    idx, rows = idx.cpu().numpy(), rows.cpu().numpy()
    # EVERY row whose K + 1 best scores are further apart than the two device scorers can differ (the evaluator's chunked bf16x3
    # form against the score-matrix form ranked here: 2.4e-7 each way) must carry the reference's list and metric row bit for bit;
    # only rows with a (near-)tie at or across the K boundary may differ, and then hold the same scores rank by rank
    top = -np.sort(-sc, axis=1)[:, :K + 1]
    clear = np.all(top[:, :-1] - top[:, 1:] > 1e-6, axis=1)
    assert clear.sum() >= len(users) // 2, clear.sum()              # (the criterion below is not vacuous)
    assert np.array_equal(idx[clear], ref_topk[clear]), np.nonzero(clear & ~(idx == ref_topk).all(1))[0]
    assert np.array_equal(rows[clear], np.asarray(ref_rows, np.float32).reshape(len(users), -1)[clear])
    same = (idx == ref_topk).all(1) & _tie_free(sc, K)
    assert np.array_equal(rows[same], np.asarray(ref_rows, np.float32).reshape(len(users), -1)[same])
    for r in np.nonzero(~same)[0]:
        assert np.abs(sc[r][idx[r]] - sc[r][ref_topk[r]]).max() <= 1e-6, r


@pytest.mark.gpu
def test_reference_tie_order_is_reproduced_on_request(fixture_name, eval_math):
    """--tie_order=reference (the default). The fixture's cached tables with groups of DUPLICATED item rows (equal rows score
    equally under every user, so ties sit inside the top-K and across its boundary for most users): with the device's own rule the
    lists differ from those of the reference's compiled evaluate.h on rows with ties; in reference order EVERY row -- tied or not --
    carries the reference's list, scores and metric row bit for bit, computed on the device inside the scoring call
    (ref_order_kernel), in both evaluation math modes: the lists are what the reference's code makes of the rows predict() returns."""
    from oracle import eval_oracle as ev
    if ev.ref_lib() is None:
        pytest.skip("oracle/_ref/libref_eval.so was not built (needs /root/reference at build time)")
    g = load_golden(fixture_name)
    model, _ = build_model_from_fixture(g, DEV)
    _load_cache(model, g)
    U = model.num_users
    Y = model._ws["Y"]
    rng = np.random.default_rng(5)
    for base in rng.choice(model.num_items, size=12, replace=False):          # every picked item gets three exact copies
        for dup in rng.choice(model.num_items, size=3, replace=False):
            Y[U + int(dup)] = Y[U + int(base)]
    model._publish_cache(Y)
    model.fusion_mode, model.predict_type = "rubi", "TIE"
    users = g["evalbatch/users"].tolist()
    K = int(g["evalbatch/top_k"])
    mids = g["evalbatch/metric_ids"]
    evalr = model.test_evaluator.evaluator
    dev_scores = torch.empty(len(users), model.num_items, device=DEV)
    train_ptr, train_items = evalr._batch_csr(users, evalr.user_pos_train, DEV, unique=False)
    model.predict_device(users, scores=dev_scores, train_ptr=train_ptr, train_items=train_items)
    sc = np.ascontiguousarray(dev_scores.cpu().numpy())
    test = csr_dict(g, "test")
    tp, ti = ev.truth_to_csr([sorted(set(test[int(u)])) for u in users])
    ref_rows, ref_topk = ev.evaluate_matrix(sc.copy(), tp, ti, mids, K, use_ref=True)
    ref_rows = np.asarray(ref_rows, np.float32).reshape(len(users), -1)
    _, port_topk = ev.evaluate_matrix(sc.copy(), tp, ti, mids, K)             # (the C restatement agrees with the reference's code)
    assert np.array_equal(port_topk, ref_topk)
    try:
        evalr.tie_order = "id"
        rows_id, idx_id, _ = evalr.evaluate_batch(model, users, return_topk=True)
        evalr.tie_order = "reference"
        rows_ref, idx_ref, val_ref = evalr.evaluate_batch(model, users, return_topk=True)
    finally:
        evalr.tie_order = "reference"
    tied = ~_tie_free(sc, K)
    assert tied.sum() >= 3
    assert not np.array_equal(idx_id.cpu().numpy(), ref_topk)                     # the device's rule IS another order on these rows
    assert np.array_equal(idx_id.cpu().numpy()[~tied], ref_topk[~tied])
    assert np.array_equal(idx_ref.cpu().numpy(), ref_topk)                        # ... and by default the reference's, everywhere
    assert np.array_equal(rows_ref.cpu().numpy(), ref_rows)
    assert np.array_equal(val_ref.cpu().numpy(), np.take_along_axis(sc, ref_topk.astype(np.int64), 1))
    # the same lists from the kernel over the materialised rows (elimrec_topk_reference_order_device)
    from elimrec_amd import ops
    oi = torch.empty(len(users), K, dtype=torch.int32, device=DEV)
    ov = torch.empty(len(users), K, device=DEV)
    ops.topk_reference_order(dev_scores, K, oi, ov)
    assert np.array_equal(oi.cpu().numpy(), ref_topk) and np.array_equal(ov.cpu().numpy(), val_ref.cpu().numpy())


@pytest.mark.gpu
def test_reference_order_kernel_known_answers_and_edge_rows():
    """ref_order_kernel (the reference's std::partial_sort_copy replayed by one wave per row) against the oracle, bit for bit on the
    ids AND on the order among equal scores: SURVEY section 4's known answer, a row of all-equal scores, ascending rows (every item
    enters the heap) and descending rows (none does), -inf (masked) scores inside the first K, K = 1 / K = I / even and odd K up
    to 1024, rows shorter than a 64-item step."""
    from elimrec_amd import ops
    rng = np.random.default_rng(11)

    def check(sc, K):
        sc = np.ascontiguousarray(sc, np.float32)
        want = _reference_lists(sc, K)
        oi = torch.empty(sc.shape[0], K, dtype=torch.int32, device=DEV)
        ov = torch.empty(sc.shape[0], K, device=DEV)
        ops.topk_reference_order(_t(sc), K, oi, ov)
        assert np.array_equal(oi.cpu().numpy(), want), (sc.shape, K)
        assert np.array_equal(ov.cpu().numpy(), np.take_along_axis(sc, want.astype(np.int64), 1))

    kat = np.array([[.5, .5, .5, .1, .9, .5]], np.float32)
    for K in (1, 2, 3, 4, 5, 6):
        check(kat, K)
    check(np.full((3, 1000), 0.25, np.float32), 10)                       # all equal: the order is the heap's alone
    check(np.full((2, 70), 0.25, np.float32), 70)
    for I in (5, 63, 64, 65, 200, 4097):
        base = rng.integers(0, 7, size=(6, I)).astype(np.float32) / 8     # eight distinct values: ties everywhere
        for K in sorted({1, 2, min(7, I), min(10, I), min(64, I), min(65, I), I if I <= 200 else 1024}):
            check(base, K)
    asc = np.tile(np.arange(3000, dtype=np.float32), (2, 1))
    check(asc, 10); check(asc[:, ::-1].copy(), 10); check(np.floor(asc / 7), 33)
    masked = rng.integers(0, 5, size=(8, 500)).astype(np.float32)
    masked[:, :12][rng.random((8, 12)) < 0.6] = -np.inf                   # masked items among the first K ids
    masked[rng.random(masked.shape) < 0.3] = -np.inf
    check(masked, 10); check(masked, 11)
    few = np.full((2, 300), -np.inf, np.float32)                          # fewer than K unmasked items: -inf ids in heap order
    few[:, [5, 17, 200]] = [0.5, 0.7, 0.5]
    check(few, 10)
    # a padded matrix (ld > I): rows cut out of a wider block
    wide = _t(rng.integers(0, 9, size=(5, 640)).astype(np.float32))
    oi = torch.empty(5, 10, dtype=torch.int32, device=DEV)
    ops.topk_reference_order(wide[:, :600], 10, oi)
    assert np.array_equal(oi.cpu().numpy(), _reference_lists(wide[:, :600].cpu().numpy(), 10))


@pytest.mark.gpu
def test_reference_order_at_the_tiktok_catalogue_with_early_training_scores():
    """SURVEY section 7's probe: early in training the TIE scores of 76 085 items span [0.4985, 0.5027] and take only ~17 k distinct
    fp32 values -- nearly every row ties inside its top-K. (a) the kernel over such rows, materialised; (b) the whole evaluator path
    at that catalogue size: test_reference_order_inside_the_scoring_call."""
    from elimrec_amd import ops
    rng = np.random.default_rng(3)
    I, K = 76085, 10
    levels = np.sort(rng.choice(np.arange(int(0.4985 * 2 ** 25), int(0.5027 * 2 ** 25)), size=17000, replace=False)).astype(np.float32) / 2 ** 25
    bell = np.clip(8500 + rng.standard_normal((32, I)) * 2100, 0, 16999).astype(np.int64)          # sparse upper tail: some ties in the top-K
    crowd = 16999 - np.minimum((np.abs(rng.standard_normal((32, I))) * 4000).astype(np.int64), 16999)   # the mode at the top: all tied
    sc = np.ascontiguousarray(levels[np.concatenate([bell, crowd])], np.float32)
    assert 36 <= (~_tie_free(sc, K)).sum()
    want = _reference_lists(sc, K)
    oi = torch.empty(64, K, dtype=torch.int32, device=DEV)
    ops.topk_reference_order(_t(sc), K, oi)
    assert np.array_equal(oi.cpu().numpy(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("d,I", [(64, 76085), (32, 40000), (128, 33000), (64, 9000)])
def test_reference_order_inside_the_scoring_call(d, I, eval_math):
    """elimrec_score_topk_ordered with tie_order = reference at catalogue sizes beyond one scorer chunk (the heap carried from chunk
    to chunk, tiles below the running threshold never stored, train items masked by bitmap) and below (one launch, tile-guided):
    the lists equal the oracle's ranking of the score matrix the SAME call shape returns -- one score form for lists and matrix,
    in both math modes (recdim 32 / 64 default math: six bf16 piece products, chunk by chunk for the matrix too) -- on tables
    with massive ties (nine distinct item rows), on early-training tables (scores crowded around 0.5: SURVEY section 7) and on
    continuous ones; K = 10 and 50; lists and matrix from one call as well."""
    from elimrec_amd import ops
    U, S = 150, 3
    Cy = (1 + S) * d
    g = torch.Generator().manual_seed(6)
    Yr = torch.randn(U + I, Cy, generator=g) * 0.3
    Yt = Yr.clone()
    Yt[U:] = Yt[U:U + 9].repeat((I + 8) // 9, 1)[:I]
    Ye = torch.round(torch.randn(U + I, Cy, generator=g) * 4) / 256           # tiny, coarsely quantised rows: colliding scores
    users = torch.arange(0, 140)
    B = len(users)
    rng = np.random.default_rng(1)
    lists = [rng.choice(I, size=int(rng.integers(0, 60)), replace=False).tolist() for _ in range(B)]
    lists[2] = list(range(0, 30))                                # the first K ids masked: -inf entries in the initial heap
    lists[4] = [i for i in range(I) if i % 1000 != 7]            # fewer unmasked items than K = 50... (I / 1000 of them)
    ptr = torch.zeros(B + 1, dtype=torch.int64)
    ptr[1:] = torch.tensor(np.cumsum([len(x) for x in lists]))
    items = torch.tensor([i for x in lists for i in x], dtype=torch.int32)
    ud, pd, itd = users.to(DEV), ptr.to(DEV), items.to(DEV)
    n_tied = 0
    for Y in (Yt, Ye, Yr):
        Yd = Y.to(DEV)
        ref = torch.empty(B, I, device=DEV)
        ws = torch.empty(ops.score_workspace(B, U, I, S, 1, d=d), dtype=torch.uint8, device=DEV)
        ops.score_topk(Yd, U, I, ud, d, S, 0b111, "rubi", "TIE", ws, scores=ref, train_ptr=pd, train_items=itd)
        sc = ref.cpu().numpy()
        for K in (10, 50):
            want = _reference_lists(sc, K)
            n_tied += int((~_tie_free(sc, K)).sum())
            ws = torch.empty(ops.score_workspace(B, U, I, S, K, topk_only=True, d=d), dtype=torch.uint8, device=DEV)
            if I > 16384:                                # no [B x I] score block: a [B x 16384] one
                assert ws.numel() <= ops.score_workspace(B, U, I, S, K, d=d) - B * (I - 16384) * 4
            idx = torch.empty(B, K, dtype=torch.int32, device=DEV)
            val = torch.empty(B, K, device=DEV)
            ops.score_topk(Yd, U, I, ud, d, S, 0b111, "rubi", "TIE", ws, K=K, topk_idx=idx, topk_val=val, train_ptr=pd,
                           train_items=itd, tie_order="reference")
            assert np.array_equal(idx.cpu().numpy(), want), (K, (idx.cpu().numpy() != want).any(1).nonzero())
            assert np.array_equal(val.cpu().numpy(), np.take_along_axis(sc, want.astype(np.int64), 1))
            # the device's own rule on the same call shape: the stable sort of the same matrix (rows with K unmasked items)
            ops.score_topk(Yd, U, I, ud, d, S, 0b111, "rubi", "TIE", ws, K=K, topk_idx=idx, topk_val=val, train_ptr=pd, train_items=itd)
            order = np.argsort(-sc, axis=1, kind="stable")[:, :K]
            full = np.isfinite(np.take_along_axis(sc, order, 1)).all(1)
            assert np.array_equal(idx.cpu().numpy()[full], order[full])
            # lists and matrix from ONE call
            ws = torch.empty(ops.score_workspace(B, U, I, S, K, d=d), dtype=torch.uint8, device=DEV)
            both = torch.empty(B, I, device=DEV)
            ops.score_topk(Yd, U, I, ud, d, S, 0b111, "rubi", "TIE", ws, scores=both, K=K, topk_idx=idx, topk_val=val, train_ptr=pd,
                           train_items=itd, tie_order="reference")
            assert torch.equal(both, ref) and np.array_equal(idx.cpu().numpy(), want)
    assert n_tied >= 2 * B                                       # (the tie rule was exercised on most rows of two of the tables)
    assert ops.score_range_violations(reset=True) == 0           # ... and no launch saw a score outside rubi TIE's [0.2689, 0.7311]


@pytest.mark.gpu
def test_every_scoring_call_checks_the_scores_it_returns_against_the_range_of_its_predict_type(monkeypatch):
    """The permanent guard behind round 3's fault (one launch in 49 000 returned 1.0 on sixteen lanes): every scoring call ends with
    a check of the scores it returns in its K-lists -- a wrongly HIGH score necessarily enters its user's list -- against the interval
    its (predict type, fusion mode) can produce (rubi TIE: sigma([-1, 1]) = [0.2689, 0.7311]) and of its TIE row means against
    (0, 1); offending user rows are counted on the device and the evaluator reads the count after every pass. Clean tables: zero,
    in every mode. The check itself over crafted lists; the evaluator's reaction (fp32 scorer + the pass again, then an error)."""
    from elimrec_amd import _lib, ops
    lib = _lib.load()
    g = load_golden("kwai")
    model, _ = build_model_from_fixture(g, DEV)
    _load_cache(model, g)
    users = g["evalbatch/users"].tolist()
    ops.score_range_violations(reset=True)
    for mode in ("rubi", "hm", "sum"):
        for ptype in ("normal", "TE", "TIE"):
            model.fusion_mode, model.predict_type = mode, ptype
            sc = model.predict(users).numpy()
            model.test()
            assert ops.score_range_violations(reset=True) == 0, (mode, ptype)
            if mode == "rubi":
                lo, hi = (0.2689414, 0.7310586) if ptype == "TIE" else (0.5, 0.7310586)
                assert sc.min() >= lo - 1e-6 and sc.max() <= hi + 1e-6, (ptype, sc.min(), sc.max())
    # the check over crafted lists: round 3's signature, a NaN, a score below the range, a bad row mean; fillers are not scores
    val = torch.full((6, 4), 0.6, device=DEV)
    idx = torch.arange(24, dtype=torch.int32, device=DEV).view(6, 4).contiguous()
    val[1, 0] = 1.0
    val[2, 3] = float("nan")
    val[3, 2] = 0.2
    val[4, 1], idx[4, 1] = -float("inf"), 7              # the reference order's masked filler
    val[5, 3], idx[5, 3] = -float("inf"), -1             # the id order's "no candidate"
    ops.score_range_check(val, idx, "TIE", "rubi")
    assert ops.score_range_violations(reset=True) == 3
    ops.score_range_check(val, idx, "TIE", "hm")         # [0, 1]: only the NaN
    assert ops.score_range_violations(reset=True) == 1
    ops.score_range_check(val, idx, "TE", "rubi")        # [0.5, 0.7311]: 1.0, NaN, 0.2
    assert ops.score_range_violations(reset=True) == 3
    mean = torch.tensor([0.5, 0.5, 0.5, 0.5, 0.0, float("nan")], device=DEV)
    ops.score_range_check(torch.full((6, 4), 0.6, device=DEV), idx.clamp(min=0), "TIE", "rubi", row_mean=mean)
    assert ops.score_range_violations(reset=True) == 2
    # the evaluator: a count behind a pass under the default scorer -> fp32 scorer, the pass again; a count again -> an error
    model.fusion_mode, model.predict_type = "rubi", "TIE"
    evalr = model.test_evaluator.evaluator
    b0 = int(lib.elimrec_score_get_bf16x3())
    calls = []
    real = ops.score_range_violations
    try:
        lib.elimrec_score_set_bf16x3(1)
        monkeypatch.setattr(ops, "score_range_violations", lambda reset=True: (calls.append(1), real(reset), 2 if len(calls) == 1 else 0)[2])
        want, _ = model.test()
        assert len(calls) == 2 and int(lib.elimrec_score_get_bf16x3()) == 0 and evalr.range_violations == 2
        monkeypatch.setattr(ops, "score_range_violations", lambda reset=True: (real(reset), 5)[1])
        with pytest.raises(FloatingPointError, match="left the range"):
            model.test()
    finally:
        monkeypatch.setattr(ops, "score_range_violations", real)
        lib.elimrec_score_set_bf16x3(b0)
        ops.score_range_violations(reset=True)


@pytest.mark.gpu
def test_evaluator_cross_checks_the_default_scorer_against_the_fp32_scorer(monkeypatch):
    """The first evaluation of a run (and every 16th after it; here: every one) re-scores its first users with the fp32-MFMA scorer:
    on healthy hardware no row differs; a scorer that returns a wrong score (injected here: the first launch's best score
    overwritten, the signature of round 3's fault) is counted, the process falls back to the fp32 scorer and the pass is scored
    again -- its results are the fp32 scorer's."""
    from elimrec_amd import _lib
    lib = _lib.load()
    g = load_golden("kwai")                      # recdim 64: the bf16 x 3 scorer's shape
    model, _ = build_model_from_fixture(g, DEV)
    _load_cache(model, g)
    model.fusion_mode, model.predict_type = "rubi", "TIE"
    evalr = model.test_evaluator.evaluator
    assert evalr.scorer_check_every == 16
    evalr.scorer_check_every = 1
    math0, b0 = int(lib.elimrec_score_get_math()), int(lib.elimrec_score_get_bf16x3())
    try:
        lib.elimrec_score_set_math(1)
        lib.elimrec_score_set_bf16x3(1)
        clean, _ = model.test()
        assert evalr.scorer_checked_rows > 0 and evalr.scorer_mismatch_rows == 0
        real = model.predict_device
        state = {"n": 0}

        def faulty(*a, **kw):
            idx, val = real(*a, **kw)
            state["n"] += 1
            if state["n"] == 1 and val is not None:
                val[0, 0] = 1.0
            return idx, val
        monkeypatch.setattr(model, "predict_device", faulty)
        again, _ = model.test()
        assert evalr.scorer_mismatch_rows == 1 and int(lib.elimrec_score_get_bf16x3()) == 0
        assert np.abs(np.asarray(again) - np.asarray(clean)).max() < 1e-6       # the re-scored pass: the fault is not in the results
    finally:
        lib.elimrec_score_set_math(math0)
        lib.elimrec_score_set_bf16x3(b0)
