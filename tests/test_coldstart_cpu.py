"""The host side of the cold-start paths: kappa for the five adjacency types, the sort-and-search model of ops.rank_values against
brute force on the shared cases, and the report's pure table functions."""
import numpy as np
import pytest

import coldstart_cases as cc
import coldstart_model as cm


@pytest.mark.parametrize("adj_type", ["plain", "norm", "gcmc", "pre", "mean"])
def test_isolated_row_scale(adj_type):
    from elimrec_amd import reports
    for L in (0, 1, 2, 3, 4, 6):
        k = reports.isolated_row_scale(adj_type, L)
        assert isinstance(k, float) and np.float32(k) == k            # a float32 value
        inv = np.float32(1.0) / np.float32(L + 1)
        if adj_type in ("plain", "gcmc", "pre"):
            assert k == float(inv)                                    # (x + 0) * inv: the hops add zero rows
        else:
            acc = np.float32(1.0)
            for _ in range(L):
                acc = np.float32(acc + np.float32(1.0))
            assert k == float(np.float32(acc * inv))                  # L + 1 copies in hop order, times inv
        assert abs(k - cm.isolated_row_scale(adj_type, L)) <= 2.0 ** -23
    with pytest.raises(ValueError):
        reports.isolated_row_scale(adj_type, -1)


def test_isolated_row_scale_is_the_mean_of_an_isolated_node():
    """kappa against the adjacency itself: the row of a node without edges in mean_k A^k, for every type."""
    from elimrec_amd.model import create_adj_mat
    U, I, L = 3, 4, 3
    tu, ti = [0, 1, 1, 2], [0, 0, 1, 2]                               # item 3 has no edge
    for adj_type in ("plain", "norm", "gcmc", "pre", "mean"):
        A = create_adj_mat(tu, ti, U, I, adj_type).toarray().astype(np.float64)
        acc, P = np.eye(U + I), np.eye(U + I)
        for _ in range(L):
            P = A @ P
            acc = acc + P
        row = (acc / (L + 1))[U + 3]
        want = np.zeros(U + I)
        want[U + 3] = cm.isolated_row_scale(adj_type, L)
        assert np.allclose(row, want, atol=1e-12), adj_type


@pytest.mark.parametrize("family", cc.FAMILIES)
def test_model_equals_brute_force(family):
    rng = np.random.default_rng(cc.FAMILIES.index(family))
    met_skip = set()
    for case, I in enumerate((1, 3, 4, 5, 17)):
        for with_skip in (False, True):
            x, ptr, vals, skip = cc.make(family, I, 8, rng, case, with_skip)
            got, want = cm.rank_values(x, ptr, vals, skip), cm.rank_values_brute(x, ptr, vals, skip)
            assert np.array_equal(got, want), (family, I, with_skip)
            assert ((want == -1) == ~np.isfinite(vals)).all()
            assert (~np.isfinite(vals)).any() and np.isfinite(vals).any()
            if with_skip:
                plain = cm.rank_values_brute(x, ptr, vals, None)
                fin = np.isfinite(vals)
                met_skip |= set(np.unique((plain - want)[fin & (skip >= 0)]).tolist())
                assert (plain == want)[skip < 0].all()
    if family != "equal":                                             # (every column of "equal" beats or misses alike)
        assert met_skip == {0, 1}                                     # a skipped column that does and one that does not beat the value


def test_model_rules():
    x = np.array([[0.0, -0.0, 1.0, -np.inf, 1.0]], dtype=np.float32)
    ptr = np.array([0, 7])
    vals = np.array([0.0, -0.0, 1.0, 2.0, -5.0, np.nan, -np.inf], dtype=np.float32)
    assert cm.rank_values(x, ptr, vals).tolist() == [4, 4, 2, 0, 4, -1, -1]          # behind equal scores; -inf never counts
    assert cm.rank_values(x, ptr, vals, np.array([2, 3, 2, -1, 0, 0, 0])).tolist() == [3, 4, 1, 0, 3, -1, -1]
    assert cm.among(np.array([[1.0, 2.0, 1.0, 3.0]])).tolist() == [[2, 1, 3, 0]]


def test_report_table_functions():
    from elimrec_amd import reports
    train = {0: [0, 1], 1: [1], 2: [0]}
    test = {0: [2, 3], 1: [3, 0], 2: [1]}
    items, pairs = reports.cold_test_items(train, test, 5)
    assert items.tolist() == [2, 3]                                   # 4 has no test interaction, 0 / 1 have training interactions
    assert pairs == [(0, 2), (0, 3), (1, 3)]
    none_items, none_pairs = reports.cold_test_items(train, {0: [1], 1: [0]}, 5)
    assert none_items.size == 0 and not none_pairs
    assert "no cold test item" in reports.format_coldstart(None, None, None)
    columns = ("items", "pairs", "rank", "pct", "rr", "hit@2")
    rank = np.array([0, 3, 1], dtype=np.int64)
    n_cand = np.array([3, 3, 4], dtype=np.int64)
    row = reports.coldstart_row(rank, n_cand, [2], 2)
    want = [2, 3, rank.mean(), np.mean(rank / (n_cand - 1.0)), np.mean(1.0 / (rank + 1.0)), np.mean(rank < 2)]
    assert np.allclose(row, want, rtol=1e-6)
    buf = reports.format_coldstart(columns, ["catalogue:".ljust(12)], np.asarray([row]))
    assert buf.startswith("columns:") and "catalogue:" in buf and "%.8f" % want[2] in buf
