"""Hard-negative sampling without a GPU: the float64 model of tests/hardneg_model.py on hand-worked examples, and the argument
errors of the sampler, the model front and the wrappers, all raised before anything touches a device."""
import inspect

import numpy as np
import pytest
import torch

import hardneg_model as hm
from helpers import FixtureDataset, build_model_from_fixture, load_golden

R = 1.0 / np.sqrt(2.0)


def test_model_on_a_hand_worked_example():
    U = np.array([[1.0, 0.0], [0.0, 2.0]])
    T = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [0.0, 0.0], [-1.0, 0.0]])          # item 3: a zero row, cosine 0
    users = [0, 1, 1]
    cands = np.array([[1, 2, 2, 4],             # a duplicate id holding the maximum: the lowest of its columns
                      [5, 3, 0, -1],            # two unlisted entries (5 = the item rows, -1); items 3 and 0 tie at 0
                      [2, 1, 0, 1]])
    s = hm.scores(U, T, [1.0], users, cands)
    want = np.array([[0.0, R, R, -1.0], [-np.inf, 0.0, 0.0, -np.inf], [R, 1.0, 0.0, 1.0]])
    assert np.array_equal(np.isneginf(s), np.isneginf(want))
    np.testing.assert_allclose(np.where(np.isneginf(s), 0.0, s), np.where(np.isneginf(want), 0.0, want), rtol=0, atol=1e-15)
    col, ids, best, margin = hm.pick(s, cands)
    assert col.tolist() == [1, 1, 1] and ids.tolist() == [2, 3, 1]
    np.testing.assert_allclose(best, [R, 0.0, 1.0], atol=1e-15)
    np.testing.assert_allclose(margin, [R - 0.0, 0.0, 1.0 - R], atol=1e-15)              # to the best candidate with ANOTHER id


def test_model_weights_blocks_and_rows_without_a_pick():
    U = np.array([[1.0, 0.0, 0.0, 1.0]])                                                  # two blocks of two columns
    T = np.array([[1.0, 0.0, 1.0, 0.0], [0.0, 1.0, 0.0, 3.0]])                           # block cosines (1, 0) and (0, 1)
    cands = np.array([[0, 1], [1, 0], [7, -3], [0, 0]])
    users = [0, 0, 0, 1]                                                                  # user 1 is outside the table
    for w, want in (((1.0, 0.5), [[1.0, 0.5], [0.5, 1.0]]), ((0.0, 2.0), [[0.0, 2.0], [2.0, 0.0]]), ((1.0, 0.0), [[1.0, 0.0], [0.0, 1.0]])):
        s = hm.scores(U, T, w, users, cands)
        np.testing.assert_allclose(s[:2], want, atol=1e-15)
        assert np.isneginf(s[2:]).all()
        col, ids, best, margin = hm.pick(s, cands)
        assert col[2:].tolist() == [-1, -1] and ids[2:].tolist() == [-1, -1] and np.isneginf(best[2:]).all() and np.isposinf(margin[2:]).all()
        assert ids[:2].tolist() == ([0, 0] if w[0] else [1, 1])
    one = hm.pick(hm.scores(U, T, (1.0, 0.5), [0], np.array([[1, 1, 1]])), np.array([[1, 1, 1]]))
    assert one[0].tolist() == [0] and np.isposinf(one[3]).all()                           # M copies of one id: column 0, no rival


def test_uniform_defaults_are_unchanged():
    from elimrec_amd import PairwiseSamplerV2, ops
    params = list(inspect.signature(PairwiseSamplerV2.__init__).parameters.values())[1:]
    assert [(p.name, p.default) for p in params[:8]] == [
        ("dataset", inspect.Parameter.empty), ("neg_num", 1), ("batch_size", 1024), ("shuffle", True), ("drop_last", False),
        ("device", None), ("seed", 2022), ("shard", None)]
    assert [(p.name, p.default) for p in params[8:]] == [("neg_sampling", "uniform"), ("neg_candidates", 8), ("neg_space", "fused"),
                                                         ("model", None)]
    assert ops.HARD_NEG_MAX_CANDIDATES == 64
    s = PairwiseSamplerV2(FixtureDataset(load_golden("ml3")))
    assert s.neg_sampling == "uniform" and s.model is None and s.last_stats is None and s.epoch == 0


def test_argument_errors_come_before_any_gpu_use():
    from elimrec_amd import PairwiseSamplerV2, ops
    g = load_golden("ml3")
    data = FixtureDataset(g)
    model, _ = build_model_from_fixture(g, "cpu")
    with pytest.raises(ValueError, match="model"):
        PairwiseSamplerV2(data, neg_sampling="hard")
    for bad in (0, 65, -1, 2.5):
        with pytest.raises(ValueError, match="neg_candidates"):
            PairwiseSamplerV2(data, neg_sampling="hard", neg_candidates=bad, model=model)
    with pytest.raises(ValueError, match="neg_sampling"):
        PairwiseSamplerV2(data, neg_sampling="hardest", model=model)
    with pytest.raises(ValueError, match="space"):
        PairwiseSamplerV2(data, neg_sampling="hard", neg_space="x", model=model)
    with pytest.raises(NotImplementedError):
        PairwiseSamplerV2(data, neg_num=2, neg_sampling="hard", model=model)
    ok = PairwiseSamplerV2(data, neg_sampling="hard", neg_candidates=64, neg_space="loss", model=model)
    assert ok.neg_candidates == 64 and not model.has_cached_tables()
    users, cands = torch.zeros(3, dtype=torch.int64), torch.zeros(3, 4, dtype=torch.int32)
    with pytest.raises(ValueError, match="space"):
        model.hard_negatives_device(users, cands, space="x")
    with pytest.raises(RuntimeError):                                            # a good space on a CPU model: no CPU path
        model.hard_negatives_device(users, cands)
    # the spaces' weights: one per block of the cached Y
    S = model.S
    assert model.hard_negative_weights("fused") == [1.0] + [0.0] * S
    for h, m in enumerate(model._mods):
        assert model.hard_negative_weights(m) == [1.0 if b == 1 + h else 0.0 for b in range(1 + S)]
    assert model.hard_negative_weights("loss") == [float(w) for w in model._block_weights()]
    kept = model.predict_type
    model.predict_type = "normal"
    try:
        assert model.hard_negative_weights("loss") == model.hard_negative_weights("fused")
    finally:
        model.predict_type = kept
    # the wrappers
    i32 = torch.zeros(4, dtype=torch.int32)
    for bad in (0, 65):
        with pytest.raises(ValueError, match="n_cand"):
            ops.sample_triplet_candidates(i32, torch.zeros(5, dtype=torch.int64), i32, 10, 3, 1, 0, bad, users, users, cands)
    table, sq = torch.zeros(5, 8), torch.zeros(5, 2)
    with pytest.raises(ValueError, match="blocks"):
        ops.pick_hard_negatives(table, sq, table, sq, [], users, cands, users)
    with pytest.raises(ValueError, match="blocks"):
        ops.pick_hard_negatives(table, sq, table, sq, [1.0] * 9, users, cands, users)
    with pytest.raises(ValueError, match="equal blocks"):
        ops.pick_hard_negatives(table, sq, table, sq, [1.0] * 3, users, cands, users)
    with pytest.raises(ValueError, match="d % 4"):
        ops.pick_hard_negatives(torch.zeros(5, 6), torch.zeros(5, 1), table, sq, [1.0], users, cands, users)
