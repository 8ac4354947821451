"""What the iALS baseline decides on the host (no GPU): the float64 model of tests/als_model.py against plain loops, the loss by
the Gram trick against the sum over all pairs, and every argument error of ops.AlsIndex, ops.als_solve, ops.cross_topk, fit_ials,
recommend_ials and the report's switches -- each raised before the device is required."""
import os

import numpy as np
import pytest
import torch

import als_model as am
from helpers import ROOT

PTR = np.asarray([0, 3, 3, 5, 9, 10], dtype=np.int64)                       # 5 rows over 7 fixed rows, one of them empty
NBR = np.asarray([0, 2, 6, 1, 2, 0, 3, 4, 5, 6], dtype=np.int32)


def _factors(n, d, seed):
    return (0.3 * np.random.default_rng(seed).standard_normal((n, d))).astype(np.float32)


def test_solve_rows_against_a_triple_loop():
    F, d, conf = _factors(7, 4, 0), 4, 3.0
    reg = np.asarray([0.1, 0.2, 0.3, 0.4, 0.5])
    got = am.solve_rows(PTR, NBR, F, reg, conf, np.arange(5))
    F64 = F.astype(np.float64)
    for r in range(5):
        A, b = np.zeros((d, d)), np.zeros(d)
        for a_ in range(d):
            for c in range(d):
                for j in range(7):
                    A[a_, c] += F64[j, a_] * F64[j, c]
                for j in NBR[PTR[r]:PTR[r + 1]]:
                    A[a_, c] += conf * F64[j, a_] * F64[j, c]
            A[a_, a_] += reg[r]
            for j in NBR[PTR[r]:PTR[r + 1]]:
                b[a_] += (1.0 + conf) * F64[j, a_]
        want = np.linalg.solve(A, b) if PTR[r + 1] > PTR[r] else np.zeros(d)
        assert np.abs(got[r] - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert (got[1] == 0).all() and am.cond(PTR, NBR, F, reg, conf, np.arange(5)).max() < 1e6


@pytest.mark.parametrize("d", [16, 48, 64])
def test_the_gpu_solve_cases_are_well_conditioned(d):
    """The precondition of the solve bound in tests/test_als_gpu.py, from the model alone: with the ridges of als_model.solve_reg
    every cond(A_r) of every GPU case stays <= 1e6."""
    from elimrec_amd import ops
    for seed in (0, 1, 2, 3):
        ptr, nbr, F = am.solve_case(d, ops.ALS_CHUNK, seed)
        assert sorted(np.diff(ptr).tolist()) == sorted([0, 1, 2, ops.ALS_CHUNK - 1, ops.ALS_CHUNK, ops.ALS_CHUNK + 1, 3 * ops.ALS_CHUNK + 5, am.N_FIXED, 7, 0])
        for conf in am.SOLVE_CONFS:
            for kind in am.SOLVE_REGS:
                assert am.cond(ptr, nbr, F, am.solve_reg(kind, ptr), conf, np.arange(ptr.size - 1)).max() <= 1e6, (d, seed, conf, kind)


def test_objective_by_the_gram_trick_is_the_sum_over_all_pairs():
    X, Y = _factors(5, 4, 1), _factors(7, 4, 2)
    reg_x, reg_y = am.ridge(PTR, 0.05, 0.5), np.full(7, 0.05)
    for conf in (0.0, 1.0, 40.0):
        a = am.objective(PTR, NBR, X, Y, reg_x, reg_y, conf)
        b = am.objective_all_pairs(PTR, NBR, X, Y, reg_x, reg_y, conf)
        assert abs(a - b) <= 1e-12 * abs(b)
    assert np.array_equal(am.ridge(PTR, 0.05, 0.0), np.full(5, 0.05)) and am.ridge(PTR, 0.05, 1.0)[0] == 0.05 * 4


def test_the_model_fit_descends():
    lists = [[0, 2, 6, 2], [], [1, 2], [0, 3, 4, 5], [6]]
    X, Y, obj, conds = am.fit(lists, 7, factors=16, iters=4, reg=0.05)
    assert X.dtype == np.float32 and obj.shape == (8,) and (np.diff(obj) <= 1e-9 * obj[:-1]).all() and conds.max() < 1e6
    ptr, nbr, t_ptr, t_nbr = am.graph(lists, 7)
    assert np.array_equal(ptr, PTR) and np.array_equal(nbr, NBR) and t_ptr[-1] == 10 and t_nbr[:2].tolist() == [0, 3]


def test_als_index_checks():
    from elimrec_amd import ops
    ix = ops.AlsIndex(PTR, NBR, 5, 7, "cpu")
    assert ix.deg.tolist() == [3, 0, 2, 4, 1] and ix.by_degree.tolist() == [3, 0, 2, 4, 1] and ix.n_edges == 10
    repeated, descending, outside = NBR.copy(), NBR.copy(), NBR.copy()
    repeated[1] = 0
    descending[3:5] = [2, 1]
    outside[9] = 7
    with pytest.raises(ValueError, match="strictly ascending.*row 0 lists 0, then 0"):
        ops.AlsIndex(PTR, repeated, 5, 7, "cpu")
    with pytest.raises(ValueError, match="strictly ascending.*row 2 lists 2, then 1"):
        ops.AlsIndex(PTR, descending, 5, 7, "cpu")
    with pytest.raises(IndexError, match=r"nbr spans \[0, 7\]"):
        ops.AlsIndex(PTR, outside, 5, 7, "cpu")
    with pytest.raises(ValueError, match="ascend from 0"):
        ops.AlsIndex(np.asarray([0, 3, 2, 5, 9, 10]), NBR, 5, 7, "cpu")
    with pytest.raises(ValueError, match="n \\+ 1 = 5 entries"):
        ops.AlsIndex(PTR, NBR, 4, 7, "cpu")
    ops.AlsIndex(np.asarray([0, 1, 2]), np.asarray([5, 5]), 2, 7, "cpu")     # equal ids in two lists are no repeated edge


def test_als_solve_checks_come_before_the_device():
    from elimrec_amd import ops
    ix = ops.AlsIndex(PTR, NBR, 5, 7, "cpu")

    def call(d=16, reg=0.1, conf=1.0, rows=None, n_fixed=7):
        return ops.als_solve(ix, torch.zeros(n_fixed, d), torch.zeros(d, d, dtype=torch.float64), reg, conf, torch.zeros(5, d), rows=rows)
    for d in (20, 80, 8):
        with pytest.raises(ValueError, match="16 <= d <= 64"):
            call(d=d)
    with pytest.raises(ValueError, match="reg is finite and >= 0"):
        call(reg=-0.5)
    with pytest.raises(ValueError, match="reg is finite and >= 0"):
        call(reg=np.asarray([0.1, 0.1, np.inf, 0.1, 0.1]))
    with pytest.raises(ValueError, match="one entry per row"):
        call(reg=np.ones(4))
    for conf in (float("nan"), -1.0, float("inf")):
        with pytest.raises(ValueError, match="conf is finite and >= 0"):
            call(conf=conf)
    with pytest.raises(IndexError, match=r"rows span \[0, 5\]"):
        call(rows=[0, 5])
    with pytest.raises(ValueError, match="F must be"):
        call(n_fixed=6)
    with pytest.raises(TypeError):
        ops.als_solve(None, torch.zeros(7, 16), None, 0.1, 1.0, None)
    with pytest.raises(RuntimeError, match="HIP device tensor"):           # everything else is in order: now the device is required
        call()


def test_cross_topk_checks_come_before_the_device():
    from elimrec_amd import ops
    Tq, T = torch.zeros(3, 8), torch.zeros(5, 8)
    with pytest.raises(ValueError, match="1 <= K <= 256"):
        ops.cross_topk(Tq, None, T, None, [0], 257, None)
    with pytest.raises(ValueError, match="d % 4 == 0"):
        ops.cross_topk(torch.zeros(3, 6), None, torch.zeros(5, 6), None, [0], 2, None)
    with pytest.raises(ValueError, match="share d"):
        ops.cross_topk(torch.zeros(3, 4), None, T, None, [0], 2, None)
    with pytest.raises(ValueError, match="one entry per row"):
        ops.cross_topk(Tq, torch.ones(4), T, None, [0], 2, None)
    with pytest.raises(IndexError, match=r"query rows span \[0, 3\], the query table has 3 rows"):
        ops.cross_topk(Tq, None, T, None, [0, 3], 2, None)
    with pytest.raises(IndexError, match=r"excluded rows span \[1, 5\], the table has 5 rows"):
        ops.cross_topk(Tq, None, T, None, [0, 2], 2, None, excl_ptr=[0, 1, 2], excl_rows=[1, 5])
    with pytest.raises(ValueError, match="excl_ptr and excl_rows"):
        ops.cross_topk(Tq, None, T, None, [0], 2, None, excl_ptr=[0, 0])
    query = ops.CrossQuery([0, 2], 3, 5, "cpu", [0, 1, 3], [4, 4, 0])        # rows 3..4 of T are candidates, not queries
    assert query.n_queries == 2 and query.n_query_rows == 3 and query.n_rows == 5
    with pytest.raises(IndexError, match="was checked for"):
        ops.cross_topk(Tq, None, torch.zeros(4, 8), None, query, 2, None)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        ops.cross_topk(Tq, None, T, None, query, 2, None)


def test_fit_parameters_and_switches():
    from elimrec_amd import ops
    from elimrec_amd.basic_model import baseline_sources
    from elimrec_amd.model import EliMRec
    assert ops._ials_params("x") == (64, 15, 1.0, 0.01, 0.0, 2022) == EliMRec._ials_params()
    for bad in (dict(factors=40), dict(factors=80), dict(factors=16.0), dict(iters=0), dict(iters=101), dict(iters=True), dict(conf=-1.0),
                dict(conf=float("nan")), dict(reg=0.0), dict(reg=float("inf")), dict(reg_scale=-0.1), dict(reg_scale=1.5), dict(seed=-1)):
        with pytest.raises(ValueError):
            EliMRec._ials_params(**bad)
    assert baseline_sources("[co,rp3,ials]") == ("co", "rp3", "ials")
    with pytest.raises(ValueError):
        baseline_sources("[ials,ials]")


def test_model_and_report_refuse_before_the_device():
    from helpers import build_model_from_fixture, load_golden
    g = load_golden("ml3")
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--baseline_report=10", "--baseline_sources=[co,ials]", "--baseline_factors=32",
                                                              "--baseline_iters=4", "--baseline_conf=2.0", "--baseline_reg=0.5",
                                                              "--baseline_reg_scale=0.25"])
    assert model.baseline_reporter.sources == ("co", "ials") and model.baseline_reporter.ials_params[:5] == (32, 4, 2.0, 0.5, 0.25)
    with pytest.raises(ValueError, match="factors"):
        model.fit_ials(factors=40)
    with pytest.raises(ValueError, match="iters"):
        model.fit_ials(iters=0)
    with pytest.raises(ValueError, match="K must be"):
        model.recommend_ials([0], 0)
    with pytest.raises(ValueError, match="K must be"):
        model.recommend_ials([0], 257)
    with pytest.raises(ValueError, match="reg"):
        model.recommend_ials([0], 5, reg=-1.0)
    with pytest.raises(IndexError):
        model.recommend_ials([model.num_users], 5)
    with pytest.raises(IndexError):
        model.recommend_ials([0], 5, exclude={0: [model.num_items]})
    assert tuple(model.recommend_ials([], 5).ids.shape) == (0, 5)
    for switch in ("--baseline_factors=40", "--baseline_iters=0", "--baseline_conf=-1.0", "--baseline_reg=0.0", "--baseline_reg_scale=2.0"):
        with pytest.raises(ValueError, match="baseline_factors"):
            build_model_from_fixture(g, "cpu", extra_argv=[switch])
    with pytest.raises(ValueError, match="'ials'"):
        build_model_from_fixture(g, "cpu", extra_argv=["--baseline_report=10", "--baseline_sources=[co,als]"])


def test_exports():
    from elimrec_amd import _lib, ops, torch_ops
    header = open(os.path.join(ROOT, "include", "elimrec_hip.h")).read()
    for name in ("elimrec_als_solve", "elimrec_als_chunk", "elimrec_cross_topk", "elimrec_cross_topk_workspace"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name) and name + "(" in header
    assert "als.hip" in open(os.path.join(ROOT, "elimrec_amd", "csrc", "Makefile")).read()
    assert ops.ALS_CHUNK == _lib.load().elimrec_als_chunk() >= 16 and ops.ALS_FACTORS == (16, 32, 48, 64)
    ns = torch_ops.load()
    assert hasattr(ns, "als_solve") and hasattr(ns, "cross_topk") and {"als_solve", "cross_topk"} <= set(torch_ops.OPS)
