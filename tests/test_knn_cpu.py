"""Cosine neighbours, host side (no GPU): the numpy model's self-checks, the host-only entry points of csrc/knn.hip, the column names
and the argument checks that run before anything touches the device."""
import types

import numpy as np
import pytest
import torch

import knn_model as km
from helpers import build_model_from_fixture, load_golden


def test_model_against_triple_loops():
    rng = np.random.default_rng(5)
    for n, d in ((1, 4), (2, 4), (5, 8), (6, 12)):
        T = rng.standard_normal((n, d))
        T[0] = 0.0 if n > 2 else T[0]                              # a zero row: the floor, not a division by zero
        assert np.allclose(km.cos64(T), km.cos64_loops(T), rtol=0, atol=1e-15)
        assert np.allclose(km.cos64(T, [n - 1]), km.cos64(T)[n - 1:], rtol=0, atol=1e-15)


def test_model_tie_order_and_masking():
    s = np.asarray([[0.5, 1.0, 0.5, -np.inf, 1.0, 0.5]])
    ids, vals = km.topk64(s, 4)
    assert ids.tolist() == [[1, 4, 0, 2]] and vals.tolist() == [[1.0, 1.0, 0.5, 0.5]]
    ids, vals = km.topk64(s, 8)
    assert ids.tolist() == [[1, 4, 0, 2, 5, -1, -1, -1]] and np.isneginf(vals[0, 5:]).all()
    m = km.masked(np.ones((2, 4)), [1, 3], True, [[0, 0, 2], []])
    assert np.isneginf(m).tolist() == [[True, True, True, False], [False, False, False, True]]
    assert km.topk64(m, 2)[0].tolist() == [[3, -1], [0, 1]]
    assert km.overlap([[3, 1, -1], [0, 1, 2], [-1, -1, -1]], [[1, 3, 5], [5, 6, -1], [-1, -1, -1]]).tolist() == [2, 0, 0]


def test_model_report_rows():
    ids = np.asarray([[[1, 2], [0, -1], [-1, -1]], [[2, 1], [2, 0], [0, 1]]])
    vals = np.where(ids >= 0, 0.5, -np.inf)
    rows = km.report_rows(ids, vals, [4, 0, 2], 2)
    assert rows.dtype == np.float32 and rows.shape == (3, 5)
    assert rows[0].tolist() == [1.0, 0.5, 0.5, 1.0, 1.0] and rows[1].tolist() == [0.5, 0.5, 0.5, 4.0, 3.0]
    assert np.isnan(rows[2, :2]).all() and np.isnan(rows[2, 3]) and rows[2, 2] == 0.5 and rows[2, 4] == 2.0


def test_workspace_chunk_and_tile_without_a_gpu():
    from elimrec_amd import _lib, ops
    lib = _lib.load()
    chunk, tile = lib.elimrec_cosine_topk_chunk(), lib.elimrec_cosine_topk_tile()
    assert chunk > 0 and tile > 0 and chunk % 16 == 0
    assert ops.KNN_CHUNK == chunk and ops.KNN_TILE == tile
    ws = lib.elimrec_cosine_topk_workspace
    base = ws(10, chunk, 10)
    assert base >= 10 * 10 * 8
    assert ws(11, chunk, 10) >= base and ws(10, chunk + 1, 10) > base and ws(10, chunk, 11) > base
    assert ws(10, 3 * chunk, 10) >= 3 * base - 64 and ws(1, 1, 1) > 0
    assert ops.cosine_topk_workspace(10, chunk, 10) == base


def test_cpu_tensors_are_refused():
    from elimrec_amd import ops
    T = torch.zeros(8, 4)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.cosine_topk(T, torch.zeros(8), [0, 1], 2, torch.zeros(2, 2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.list_overlap(torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32))


def test_neighbour_columns():
    from elimrec_amd import ops
    assert ops.neighbour_columns(("v", "a", "t")) == ("overlap_v", "overlap_a", "overlap_t", "cos_fused", "cos_v", "cos_a", "cos_t",
                                                      "pop_fused", "pop_v", "pop_a", "pop_t")
    assert ops.neighbour_columns(("v",)) == ("overlap_v", "cos_fused", "cos_v", "pop_fused", "pop_v")
    assert ops.neighbour_columns(()) == ("cos_fused", "pop_fused")


def test_neighbour_query_checks():
    from elimrec_amd import ops
    for bad in ([5], [-1], [0, 7]):
        with pytest.raises(IndexError):
            ops.NeighbourQuery(bad, 5, "cpu")
    with pytest.raises(IndexError):
        ops.NeighbourQuery([0, 1], 5, "cpu", [0, 1, 2], [0, 5])
    with pytest.raises(ValueError):
        ops.NeighbourQuery([0, 1], 5, "cpu", [0, 1], [0])          # Q + 1 pointers
    with pytest.raises(ValueError):
        ops.NeighbourQuery([0, 1], 5, "cpu", [0, 2, 1], [0])       # ascending, ending at len
    with pytest.raises(ValueError):
        ops.NeighbourQuery([0, 1], 5, "cpu", [0, 0, 0], None)
    with pytest.raises(TypeError):
        ops.NeighbourQuery([0.5], 5, "cpu")
    q = ops.NeighbourQuery([3, 3, 0], 5, "cpu", [0, 2, 2, 3], [4, 4, 1])
    assert q.n_queries == 3 and q.n_rows == 5 and q.rows.dtype == torch.int32 and q.excl_ptr.tolist() == [0, 2, 2, 3]


def test_neighbour_report_checks():
    from elimrec_amd.evaluator import NeighbourReport
    ds = types.SimpleNamespace(num_items=6, num_users=3)
    train = {0: [1, 2], 1: [2], 2: []}
    for bad in (0, -1, 257, 1.5, True):
        with pytest.raises(ValueError):
            NeighbourReport(ds, train, bad)
    for bad in ([], [0, 3], [3, 3], (1, 4)):
        with pytest.raises((TypeError, ValueError)):
            NeighbourReport(ds, train, 3, item_group_view=bad)
    with pytest.raises(TypeError):
        NeighbourReport(ds, [1, 2], 3)
    rep = NeighbourReport(ds, train, 3, item_group_view=[1])
    assert rep.item_counts.tolist() == [0, 1, 2, 0, 0, 0] and rep.block_items == 8192
    assert [x.strip() for x in rep.group_labels] == ["all:", "cold:", "(0,1]:", "(1,inf):"]
    assert [p.tolist() for p in rep._positions] == [[0, 1, 2, 3, 4, 5], [0, 3, 4, 5], [1], [2]]


def test_basic_model_switch():
    g = load_golden("ml3")
    model, _ = build_model_from_fixture(g, "cpu")
    assert model.neighbour_reporter is None
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--neighbour_report=5", "--item_group_view=[1,4]"])
    assert model.neighbour_reporter.k == 5 and len(model.neighbour_reporter.group_labels) >= 2
    with pytest.raises(ValueError):
        build_model_from_fixture(g, "cpu", extra_argv=["--neighbour_report=-1"])
    for space in ("x", "fusedd", None):
        with pytest.raises(ValueError):
            model._neighbour_space(space)
    assert model._neighbour_space("fused") == 0 and model._neighbour_space(model._mods[0]) == 1
    from elimrec_amd import Neighbours
    assert Neighbours._fields == ("ids", "scores")


def test_the_rising_case_has_no_near_ties():
    """A condition on the inputs of test_knn_gpu.py's rising case, met here: every query's scores rise strictly with the candidate
    id, and no two candidates of a query are closer than the comparison's near-tie allowance (2 tol)."""
    n, d, Q = 4096 + 17, 32, 17
    T, rows, excl = km.rising_case(n, d, Q)
    assert len(excl) == Q and not excl[0] and len(excl[1]) == 300
    s = km.cos64(T, rows)
    assert (np.diff(s, axis=1) > 0).all()
    for exclude_self in (True, False):
        gap = km.min_gap(km.masked(s, rows, exclude_self, excl))
        print("knn rising, exclude_self=%d: smallest gap %.3g, allowance %.3g" % (exclude_self, gap, 2 * km.tol(d)))
        assert gap > 2 * km.tol(d)
