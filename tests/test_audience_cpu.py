"""Audience lists without a GPU: the bindings, the host checks of ops.AudienceQuery, the argument errors of EliMRec.audience, the
report's pure functions against tests/audience_model.py, and the float32 model's own lists under the list rules the GPU tests use."""
import numpy as np
import pytest
import torch

import audience_model as am
import score_model as sm
from helpers import build_model_from_fixture, load_golden


def test_bindings():
    from elimrec_amd import Audience, _lib, ops, torch_ops
    lib = _lib.load()
    for name in ("elimrec_audience_topk", "elimrec_audience_topk_workspace", "elimrec_audience_topk_chunk", "elimrec_audience_topk_tile",
                 "elimrec_audience_hits"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.elimrec_abi_version() == 2
    assert ops.audience_topk_workspace(8192, 36656, 10) > 0 and ops.audience_topk_workspace(0, 5, 3) > 0     # host-only size query
    chunks = -(-36656 // ops.AUDIENCE_CHUNK)
    assert ops.audience_topk_workspace(7, 36656, 10) == 2 * (-(-7 * chunks * 10 * 4 // 16) * 16)
    assert ops.AUDIENCE_MAX_K == 256 and ops.AUDIENCE_TILE >= 16 and ops.AUDIENCE_CHUNK % 16 == 0
    assert Audience._fields == ("users", "scores")
    ns = torch_ops.load()
    assert hasattr(ns, "audience_topk") and "audience_topk" in torch_ops.OPS
    with pytest.raises(NotImplementedError):
        ns.audience_topk(torch.zeros(6, 8), 2, 4, torch.zeros(1, dtype=torch.int32), None, None, 4, 1, 1, 0, 1, 1, None, None, 4)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.audience_topk(torch.zeros(6, 8), 2, 4, [0], 4, 1, 1, "rubi", "TE", 1, torch.zeros(1, 1, dtype=torch.int32))


def test_audience_query_validation():
    from elimrec_amd import ops
    q = ops.AudienceQuery([3, 0, 3], 4, 6, "cpu", [0, 2, 2, 3], [5, 5, 0])
    assert (q.n_items, q.n_users, q.n_queries) == (4, 6, 3)
    assert q.items.dtype == torch.int32 and q.items.tolist() == [3, 0, 3]
    assert q.excl_ptr.dtype == torch.int64 and q.excl_ptr.tolist() == [0, 2, 2, 3] and q.excl_users.tolist() == [5, 5, 0]
    assert ops.AudienceQuery([], 4, 6, "cpu").n_queries == 0
    with pytest.raises(IndexError):
        ops.AudienceQuery([4], 4, 6, "cpu")
    with pytest.raises(IndexError):
        ops.AudienceQuery([-1], 4, 6, "cpu")
    with pytest.raises(IndexError):
        ops.AudienceQuery([0], 4, 6, "cpu", [0, 1], [6])
    with pytest.raises(ValueError):
        ops.AudienceQuery([0, 1], 4, 6, "cpu", [0, 2, 1], [1])           # not monotone
    with pytest.raises(ValueError):
        ops.AudienceQuery([0, 1], 4, 6, "cpu", [0, 1, 1], [1, 2])        # ptr[Q] != len
    with pytest.raises(ValueError):
        ops.AudienceQuery([0, 1], 4, 6, "cpu", [0, 1], [1])              # Q + 1 entries
    with pytest.raises(ValueError):
        ops.AudienceQuery([0], 4, 6, "cpu", excl_ptr=[0, 0])
    with pytest.raises(ValueError):
        ops.AudienceQuery([0], 4, 6, "cpu", excl_users=[])
    with pytest.raises(TypeError):
        ops.AudienceQuery([0.5], 4, 6, "cpu")


def test_model_argument_errors():
    g = load_golden("ml3")
    model, _ = build_model_from_fixture(g, "cpu")
    for k in (0, 257):
        with pytest.raises(ValueError):
            model.audience([0], k)
    with pytest.raises(IndexError):
        model.audience([model.num_items], 3)
    with pytest.raises(IndexError):
        model.audience([0], 3, exclude={0: [model.num_users]})
    with pytest.raises(RuntimeError, match="no CPU fallback|HIP|GPU"):
        model.audience([0], 3)
    assert model.audience_reporter is None
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--audience_report=5", "--item_group_view=[1,4]"])
    rep = model.audience_reporter
    assert rep.k == 5 and len(rep.group_labels) >= 2 and rep.group_labels[0].startswith("all:")
    test = model.dataset.get_user_test_dict()
    assert rep.items == sorted({int(i) for items in test.values() for i in items})
    for bad in ("-1", "257"):
        with pytest.raises(ValueError):
            build_model_from_fixture(g, "cpu", extra_argv=["--audience_report=" + bad])


def test_item_rows_against_the_numpy_model():
    from elimrec_amd import reports
    from elimrec_amd.evaluator import AUDIENCE_COLUMNS, AudienceReport        # noqa: F401  (re-exported)
    assert reports.AUDIENCE_COLUMNS == ("hit", "first", "act", "score")
    assert reports.AUDIENCE_EXPOSURE_COLUMNS == ("users", "coverage", "gini", "entropy")
    # item 0: two of three test users listed; item 1: no listed test user; item 2: fillers, user 4 listed here and for item 0;
    # item 3: a list of fillers only; item 4: no test users at all
    lists = np.array([[4, 1, 7], [2, 3, 0], [4, -1, -1], [-1, -1, -1], [5, 6, -1]], dtype=np.int32)
    scores = np.array([[0.9, 0.8, 0.7], [0.6, 0.5, 0.4], [0.75, -np.inf, -np.inf], [-np.inf] * 3, [0.3, 0.2, -np.inf]], dtype=np.float32)
    ptr = np.array([0, 3, 5, 6, 7, 7], dtype=np.int64)
    users = np.array([1, 4, 6, 5, 7, 4, 2], dtype=np.int32)
    length = np.array([3, 1, 4, 1, 5, 9, 2, 6], dtype=np.int64)
    got = reports.audience_item_rows(lists, scores, ptr, users, length)
    want = am.item_rows(lists, scores, ptr, users, length)
    assert got.dtype == np.float64 and got.shape == (5, 4)
    assert np.allclose(got, want, rtol=1e-15, atol=0, equal_nan=True)
    assert got[0, 0] == 2 / 3 and got[0, 1] == 1 and got[0, 2] == (5 + 1 + 6) / 3
    assert got[1, 0] == 0 and got[1, 1] == 0
    assert got[2, 0] == 1 and got[2, 2] == 5 and got[2, 3] == 0.75
    assert got[3, 0] == 0 and np.isnan(got[3, 2]) and np.isnan(got[3, 3])
    assert np.isnan(got[4, 0]) and got[4, 1] == 0
    # the exposure side: user 4 holds two of the nine listed slots
    counts = np.bincount(lists[lists >= 0], minlength=8)
    table = reports.exposure_summary(counts, [np.arange(8)])[:, :4]
    assert table[0, 0] == 8 and table[0, 1] == 8 / 8 and counts[4] == 2


@pytest.mark.parametrize("family", ["benign", "saturated", "zero"])
def test_the_float32_model_stays_inside_the_list_rules(family):
    """The reference side itself: the float32 model's top-K passes rules 1-4 against the float64 model, for the shapes' seeds the
    GPU tests use (audience_cases in test_audience_gpu.py draws the same tables)."""
    U, I, d, S, mask = 300, 40, 20, 3, 5
    Y = sm.make_table(family, U, I, d, S, 11)
    items = [0, 3, 7, 39, 3]
    excl = [[], range(U), [1, 1, 2], [], [5]]
    ok = am.eligible_mask(U, len(items), excl)
    for ptype, fusion in sm.PAIRS:
        s64 = am.columns(Y.double(), U, items, d, S, mask, fusion, ptype).numpy()
        s32 = am.columns(Y, U, items, d, S, mask, fusion, ptype).numpy()
        for K in (1, 10, 65):
            idx, val = am.topk32(s32, ok, K)
            am.check_lists(idx, val, s64, s32, ok, K, False, (family, ptype, fusion, K))
            assert (idx[1] == -1).all()


@pytest.mark.parametrize("case", range(9))
def test_the_float32_model_passes_the_gpu_cases(case):
    """The same check over the shapes, seeds, items and exclusion lists of tests/test_audience_gpu.py (with the models' own TIE mean):
    a seed at which the float32 yardstick itself left the rules would have to be replaced before any GPU run."""
    import test_audience_gpu as tg
    name, family, U, Q, K, d, S, mask, pairs, modes = tg._shapes()[case]
    Y = sm.make_table(family, U, tg.I_CAT, d, S, 11 + case)
    items, excl = tg._items(Q), tg._excl_for(U, Q, np.random.default_rng(5 + case))
    ok = am.eligible_mask(U, Q, excl)
    for ptype, fusion in pairs:
        s64 = am.columns(Y.double(), U, items, d, S, mask, fusion, ptype).numpy()
        s32 = am.columns(Y, U, items, d, S, mask, fusion, ptype).numpy()
        idx, val = am.topk32(s32, ok, K)
        am.check_lists(idx, val, s64, s32, ok, K, False, (name, ptype, fusion))


def test_the_rising_case_has_no_near_ties():
    """A condition on the inputs of test_audience_gpu.py's rising case, met here: under both of its scorings every column's scores
    rise strictly with the user id, and no two eligible users are closer than the comparison's near-tie allowance (2 tol)."""
    import test_audience_gpu as tg
    U, Q, d = tg.RISING_U, tg.RISING_Q, tg.RISING_D
    items, excl = list(range(Q)), am.rising_excl(U, Q)
    ok = am.eligible_mask(U, Q, excl)
    for ptype, fusion, S, mask in tg.RISING_SCORINGS:
        Y = am.rising_table(U, tg.I_CAT, d, S)
        s64 = am.columns(Y.double(), U, items, d, S, mask, fusion, ptype).numpy()
        s32 = am.columns(Y, U, items, d, S, mask, fusion, ptype).numpy()
        assert (np.diff(s64, axis=0) > 0).all(), (ptype, fusion)
        tol = max(sm.tolerance(torch.from_numpy(s64[:, q]), torch.from_numpy(s32[:, q]), True)[0] for q in range(Q))
        gap = am.min_gap(s64, ok)
        print("audience rising %s/%s: smallest gap %.3g, allowance %.3g" % (ptype, fusion, gap, 2 * tol))
        assert gap > 2 * tol, (ptype, fusion, gap, tol)
