"""Effect breakdown, host side (no GPU): the float64 model's score columns against score_model.predict, the column names, and
explain()'s argument checks, which run before anything touches the device."""
import numpy as np
import pytest
import torch

import effects_model as em
import score_model as sm
from helpers import build_model_from_fixture, load_golden


@pytest.mark.parametrize("fusion", ["rubi", "hm", "sum"])
def test_model_score_columns_are_predict(fusion):
    """Columns 4 / 5 of the model == score_model.predict(..., "TE" / "TIE") at the listed ids, exactly, in float64; padding NaN."""
    U, I, d, S = 7, 61, 8, 3
    Y = sm.make_table("benign", U, I, d, S, seed=1).double()
    users = torch.tensor([0, 3, 3, 6, 2])
    rng = np.random.default_rng(0)
    lists = [rng.integers(0, I, size=n).tolist() for n in (0, 1, 15, 17, 33)]
    for mask in (0b111, 0b101):
        got = em.effects(Y, U, users, d, S, mask, fusion, lists)
        assert got.dtype == torch.float64 and got.shape == (5, 33, 6 + S)
        ub, ib = sm.blocks(Y, U, users, d, S)
        a, z = sm.logits(ub, ib), sm.cosines(ub, ib)
        for col, ptype in ((4, "TE"), (5, "TIE")):
            want = sm.predict(a, z, mask, fusion, ptype)
            for b, c in enumerate(lists):
                assert torch.equal(got[b, :len(c), col], want[b, c])
                assert torch.isnan(got[b, len(c):]).all()
        assert torch.equal(got[2, :15, 1], torch.sigmoid(a[2]).mean().expand(15))


def test_effect_columns():
    from elimrec_amd import ops
    assert ops.effect_columns(("v", "a", "t")) == ("ui", "mean_ui", "te", "nde", "score_te", "score_tie", "cos_v", "cos_a", "cos_t")
    assert ops.effect_columns(()) == em.BASE


def test_explain_argument_errors_fire_without_a_gpu():
    g = load_golden("ml3")
    model, _ = build_model_from_fixture(g, "cpu")
    users = [0, 1, 2]
    with pytest.raises(ValueError, match="exactly one"):
        model.explain(users)
    with pytest.raises(ValueError, match="exactly one"):
        model.explain(users, candidate_items=[[1], [2], [3]], top_k=3)
    with pytest.raises(ValueError, match="one candidate list per user"):
        model.explain(users, candidate_items=[[1], [2]])
    with pytest.raises(IndexError):
        model.explain(users, candidate_items=[[1], [model.num_items], [3]])
    with pytest.raises(IndexError):
        model.explain(users, candidate_items=[[1], [-1], [3]])
    with pytest.raises(ValueError, match="top_k"):
        model.explain(users, top_k=0)


def test_effects_entry_is_declared_bound_and_registered():
    from elimrec_amd import _lib, torch_ops
    assert "elimrec_score_effects" in _lib.SIGNATURES and hasattr(_lib.load(), "elimrec_score_effects")
    assert hasattr(torch_ops.load(), "score_effects") and "score_effects" in torch_ops.OPS


def test_effect_report_argument_checks():
    from elimrec_amd.evaluator import EffectReport
    train, test = {0: [1], 1: [2, 3, 4]}, {0: [3], 1: [5]}
    rep = EffectReport(None, train, test, 2, group_view=[1, 5])
    assert rep.group_labels == ["all:".ljust(12), "(0,1]:".ljust(12), "(1,5]:".ljust(12)] and rep.users == [0, 1]
    with pytest.raises(ValueError):
        EffectReport(None, train, test, 0)
    g = load_golden("ml3")
    model, _ = build_model_from_fixture(g, "cpu")
    assert model.effect_reporter is None and model.effect_report() is None
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--effect_report=4", "--group_view=[1,3,5]"])
    assert model.effect_reporter.top_k == 4 and len(model.effect_reporter.group_labels) == 3
