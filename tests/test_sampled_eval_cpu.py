"""Sampled-negative evaluation, host side (no GPU): the negatives file of the reference's format, the --eval_candidates switch,
the reference's "not enough integers" condition, and the new C ABI / torch op entries."""
import os

import numpy as np
import pytest

from helpers import build_model_from_fixture, load_golden


def _toy_dataset(tmp_path, **extra):
    from elimrec_amd import Dataset
    d = tmp_path / "dataset"
    d.mkdir(exist_ok=True)
    (d / "toy.train").write_text("10,7\n10,3\n20,7\n30,5\n")
    (d / "toy.test").write_text("20,3\n30,9\n")
    (d / "toy.valid").write_text("10,9\n40,5\n")
    conf = {"data.input.dataset": "toy", "data.input.path": str(d), "data.convert.separator": ",",
            "data.column.format": "UI", "splitter": "given", "user_min": 0, "item_min": 0, "with_item_vat": False}
    conf.update(extra)
    return Dataset(conf), d


def test_negative_file_of_the_reference_format_is_read_back_ascending(tmp_path):
    """<path>/_tmp_<name>/<name>_<splitter>_u<user_min>_i<item_min>.neg<N> (data/dataset.py:66-73, 270-300): no header, user id
    then N item ids (remapped), data.convert.separator. Read lazily on the first call; lists ascending; valid dict == test dict."""
    ds, d = _toy_dataset(tmp_path, **{"rec.evaluate.neg": 2})
    fn = ds.neg_file(2)
    assert fn == os.path.join(str(d), "_tmp_toy", "toy_given_u0_i0.neg2")
    assert not os.path.exists(os.path.dirname(fn))           # nothing is written by a run that never asks
    os.makedirs(os.path.dirname(fn))
    rows = np.array([[0, 2, 1], [1, 3, 2], [2, 1, 0], [3, 3, 1]], dtype=np.int64)     # written as np.savetxt(fmt='%d') does
    np.savetxt(fn, rows, fmt="%d", delimiter=",")
    test = ds.get_user_test_neg_dict()                         # n_neg from rec.evaluate.neg
    assert test == {0: [1, 2], 1: [2, 3], 2: [0, 1], 3: [1, 3]}
    assert ds.get_user_valid_neg_dict() == test
    assert ds.get_user_test_neg_dict(2) is test                # drawn / read once
    ds0, _ = _toy_dataset(tmp_path, **{"rec.evaluate.neg": 0})
    assert ds0.get_user_test_neg_dict() is None and ds0.get_user_valid_neg_dict() is None


def test_not_enough_integers_is_rejected_on_the_host():
    """util/cython/random_choice.pyx:35-37: I - |exclusion| <= n_neg raises before any launch."""
    from elimrec_amd import SyntheticDataset, ops
    ptr = np.array([0, 3, 5], dtype=np.int64)
    ops.check_negative_room(ptr, 10, 6)                        # 10 - 3 = 7 > 6
    with pytest.raises(ValueError, match="not enough integers"):
        ops.check_negative_room(ptr, 10, 7)
    with pytest.raises(ValueError, match="greater than 'high'"):
        ops.check_negative_room(ptr, 3, 1)
    ds = SyntheticDataset(40, 30, 400, feat_dims=(4, 4, 4), seed=3)
    most = int(np.diff(ds.exclusion_csr()[0]).max())
    with pytest.raises(ValueError, match="not enough integers"):
        ds.get_user_test_neg_dict(30 - most)


def test_eval_candidates_switch():
    """--eval_candidates=full (default): the evaluators get no negatives, whatever rec.evaluate.neg says (the reference's driver
    passes None); sampled with rec.evaluate.neg = 0 is an error."""
    g = load_golden("ml3")
    model, _ = build_model_from_fixture(g, "cpu")
    assert model.valid_evaluator.evaluator.user_neg_test is None and model.test_evaluator.evaluator.user_neg_test is None
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--rec.evaluate.neg=5", "--eval_candidates=full"])
    assert model.valid_evaluator.evaluator.user_neg_test is None
    with pytest.raises(ValueError):
        build_model_from_fixture(g, "cpu", extra_argv=["--eval_candidates=sampled"])
    with pytest.raises(ValueError):
        build_model_from_fixture(g, "cpu", extra_argv=["--eval_candidates=some"])


def test_sampled_evaluator_rejects_k_beyond_the_candidates():
    """max(top_k) > rec.evaluate.neg + 1 raises by name, decided over the whole negative dict (not per user block)."""
    from elimrec_amd import ProxyEvaluator
    from elimrec_amd.evaluator import CandidateScoringError
    train, test = {0: [1], 1: [2]}, {0: [3], 1: [4]}
    neg = {0: [5, 6, 7], 1: [5, 6, 8]}
    ev = ProxyEvaluator(None, train, test, neg, metric=["Recall"], top_k=[4])
    assert ev.evaluator.user_neg_test is neg
    with pytest.raises(CandidateScoringError):
        ProxyEvaluator(None, train, test, neg, metric=["Recall"], top_k=[5])


def test_new_entries_are_declared_bound_and_registered():
    from elimrec_amd import _lib, torch_ops
    for name in ("elimrec_score_candidates", "elimrec_sample_negatives"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    ns = torch_ops.load()
    assert hasattr(ns, "score_candidates") and hasattr(ns, "sample_negatives")
