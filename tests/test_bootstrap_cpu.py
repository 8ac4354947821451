"""The bootstrap without a GPU: the numpy model of tests/bootstrap_model.py -- Philox4x32-10 against Random123's known answers, the
statistics of the draw contract --, reports.bootstrap_summary on hand-worked replicates, and the argument errors of the entry
point, the wrappers, the report and the switch, all raised before anything touches a device."""
import ctypes
import types

import numpy as np
import pytest
import torch

import bootstrap_model as bm
from helpers import build_model_from_fixture, load_golden

SEED = 2022


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10."""
    zero = bm.philox4x32((0, 0, 0, 0), (0, 0))
    assert [int(x) for x in zero] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    ones = bm.philox4x32((0xffffffff,) * 4, (0xffffffff, 0xffffffff))
    assert [int(x) for x in ones] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    both = bm.philox4x32((np.array([0, 0xffffffff]),) * 4, (0, 0))            # arrays: one counter per entry
    assert both.shape == (2, 4) and [int(x) for x in both[0]] == [int(x) for x in zero]


def test_positions_follow_the_counter_layout():
    for n_g in (1, 2, 3, 5, 7, 64, 65):
        pos = bm.positions(SEED, 3, 2, n_g)
        assert pos.shape == (n_g,) and pos.min() >= 0 and pos.max() < n_g
        for t in (0, n_g - 1):
            word = int(bm.philox4x32((t >> 2, 3, 2, 0x626F6F74), (SEED & 0xffffffff, SEED >> 32))[t & 3])
            assert pos[t] == (word * n_g) >> 32
    assert bm.positions(SEED, 0, 0, 0).size == 0
    assert not np.array_equal(bm.positions(SEED, 0, 0, 64), bm.positions(SEED, 1, 0, 64))
    assert not np.array_equal(bm.positions(SEED, 0, 0, 64), bm.positions(SEED, 0, 1, 64))
    assert not np.array_equal(bm.positions(SEED, 0, 0, 64), bm.positions(SEED + (1 << 32), 0, 0, 64))     # the key's high word


def test_positions_are_uniform():
    """n_g = 7, R = 20 000: the chi-square of the position counts stays below 22.46, the 99.9 % point of chi2(6)."""
    n_g, R = 7, 20000
    counts = np.zeros(n_g)
    for r in range(R):
        counts += np.bincount(bm.positions(SEED, r, 0, n_g), minlength=n_g)
    expect = R * n_g / n_g
    chi2 = ((counts - expect) ** 2 / expect).sum()
    print("chi-square of the position counts: %.2f" % chi2)
    assert chi2 < 22.46


def test_replicates_have_the_standard_error_of_the_mean():
    """n = 1000 values integers(0, 1025) / 1024, R = 4000: the replicates' standard deviation within 5 % of std(ddof=0) / sqrt(n)
    (the ratio's own sampling error is 1 / sqrt(2 R) = 1.1 %), their mean within 4 se / sqrt(R) of the sample mean."""
    n, R = 1000, 4000
    x = (np.random.default_rng(0).integers(0, 1025, n) / 1024.0).astype(np.float32)
    reps = bm.means(x[:, None], [0, n], np.arange(n), R, SEED)[:, 0, 0]
    se = x.astype(np.float64).std(ddof=0) / np.sqrt(n)
    ratio, z = reps.std(ddof=1) / se, (reps.mean() - x.astype(np.float64).mean()) / (se / np.sqrt(R))
    print("replicate sd / se = %.4f, z of the replicates' mean = %.2f" % (ratio, z))
    assert abs(ratio - 1.0) < 0.05 and abs(z) < 4.0


def test_model_means_on_a_hand_worked_example():
    rows = np.array([[1.0, 8.0], [2.0, 16.0], [4.0, 32.0]], dtype=np.float32)
    ptr, listed = [0, 3, 3, 5], [0, 1, 2, 2, 2]
    out = bm.means(rows, ptr, listed, 3, SEED)
    assert out.shape == (3, 3, 2) and np.isnan(out[:, 1]).all()
    assert (out[:, 2] == [4.0, 32.0]).all()                                  # a group listing one row twice: always that row
    for r in range(3):
        pos = bm.positions(SEED, r, 0, 3)
        assert out[r, 0, 0] == rows[pos, 0].astype(np.float64).sum() / 3 and out[r, 0, 1] == 8 * out[r, 0, 0]     # columns stay paired
    diff = bm.means(rows, ptr, listed, 3, SEED, rows_b=rows * 3, exact=True)
    assert np.array_equal(diff[:, 0], 2 * out[:, 0]) and np.array_equal(diff[:, 2], 2 * out[:, 2])


def test_bootstrap_summary_by_hand():
    from elimrec_amd.evaluator import bootstrap_summary
    reps = np.zeros((5, 3, 2))
    reps[:, 0, 0] = [1.0, 2.0, 3.0, 4.0, 5.0]
    reps[:, 0, 1] = [-1.0, 0.0, 0.0, 2.0, 3.0]
    reps[:, 1, 0] = [-2.0, -1.0, -4.0, -3.0, -5.0]
    reps[:, 1, 1] = 0.0
    reps[:, 2, :] = np.nan
    point = np.arange(6, dtype=np.float32).reshape(3, 2)
    s = bootstrap_summary(reps, point, level=0.5)
    assert s._fields == ("mean", "se", "lo", "hi", "p") and all(x.shape == (3, 2) and x.dtype == np.float64 for x in s)
    assert s.mean[:2].tolist() == [[0.0, 1.0], [2.0, 3.0]]
    np.testing.assert_allclose(s.se[0], [np.sqrt(2.5), np.sqrt(2.7)], rtol=1e-15)
    # quantiles 0.25 and 0.75 of five sorted values: positions 1 and 3
    assert (s.lo[0, 0], s.hi[0, 0]) == (2.0, 4.0) and (s.lo[0, 1], s.hi[0, 1]) == (0.0, 2.0) and (s.lo[1, 0], s.hi[1, 0]) == (-4.0, -2.0)
    # p: (#{<= 0}, #{>= 0}) = (0, 5) -> 2 / 6; (3, 4) -> min(1, 2 * 4 / 6) = 1; (5, 0) -> 2 / 6; all zero -> 1
    np.testing.assert_allclose(s.p[:2], [[2.0 / 6.0, 1.0], [2.0 / 6.0, 1.0]], rtol=1e-15)
    assert s.se[1, 1] == 0.0 and s.lo[1, 1] == s.hi[1, 1] == 0.0
    assert all(np.isnan(x[2]).all() for x in s)
    wide = bootstrap_summary(reps, point)                                   # 0.025 / 0.975: linear interpolation between neighbours
    np.testing.assert_allclose([wide.lo[0, 0], wide.hi[0, 0]], [1.1, 4.9], rtol=1e-14)
    one = bootstrap_summary(reps[:1], point)
    assert np.isnan(one.se).all() and one.lo[0, 0] == one.hi[0, 0] == 1.0
    for level in (0.0, 1.0, -0.1, 1.5, float("nan"), None, "0.9", True):
        with pytest.raises(ValueError):
            bootstrap_summary(reps, point, level=level)
    with pytest.raises(ValueError):
        bootstrap_summary(reps, point[:2])
    with pytest.raises(ValueError):
        bootstrap_summary(reps[0], point)


def test_numpy_column_means_do_not_depend_on_the_other_columns():
    """SignificanceReport takes UniEvaluator's np.mean over the compacted rows: per column the bits of the mean over the whole block."""
    wide = np.random.default_rng(1).random((5003, 20), dtype=np.float32)
    cols = [1, 4, 19]
    assert np.mean(wide, axis=0)[cols].tobytes() == np.mean(np.ascontiguousarray(wide[:, cols]), axis=0).tobytes()


def test_limits_and_form_rule():
    from elimrec_amd import _lib, ops
    lib = _lib.load()
    assert lib.elimrec_abi_version() == 2
    assert ops.BOOTSTRAP_MAX_COLUMNS == lib.elimrec_bootstrap_max_columns() == 16
    assert ops.BOOTSTRAP_TILE == lib.elimrec_bootstrap_replicate_tile() == 16
    assert ops.bootstrap_rows_in_lds(0, 1) and ops.bootstrap_rows_in_lds(8192, 1) and not ops.bootstrap_rows_in_lds(8193, 1)
    assert ops.bootstrap_rows_in_lds(512, 16) and not ops.bootstrap_rows_in_lds(513, 16) and not ops.bootstrap_rows_in_lds(40000, 1)
    for n_g, C in ((-1, 1), (2 ** 31, 1), (5, 0), (5, 17)):
        with pytest.raises(ValueError):
            ops.bootstrap_rows_in_lds(n_g, C)


def test_entry_point_refuses_bad_arguments_before_it_looks_at_a_pointer():
    from elimrec_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(8)                                                 # a non-null pointer nothing may read
    good = dict(rows=one, rows_b=None, n=10, C=3, ld=3, ptr=one, grows=one, listed=10, G=2, R=5, out=one, ld_out=3, lds=1)
    for kw in (dict(R=0), dict(R=-1), dict(R=2 ** 31), dict(C=0), dict(C=17), dict(C=-1), dict(n=-1), dict(n=2 ** 31), dict(listed=-1),
               dict(listed=2 ** 31), dict(G=0), dict(ld=2), dict(ld_out=2), dict(lds=2), dict(ptr=None), dict(out=None), dict(rows=None),
               dict(grows=None), dict(n=0), dict(R=2 ** 31 - 1, G=2 ** 30)):
        a = dict(good)
        a.update(kw)
        rc = lib.elimrec_bootstrap_means(a["rows"], a["rows_b"], a["n"], a["C"], a["ld"], a["ptr"], a["grows"], a["listed"], a["G"], a["R"],
                                         SEED, a["out"], a["ld_out"], a["lds"], None)
        assert rc == 10001 and b"bootstrap_means" in lib.elimrec_last_error(), (kw, rc)            # ELIMREC_E_BADARG
    for kw in (dict(ptr=None), dict(out=None), dict(rows=None), dict(grows=None)):
        a = dict(good)
        a.update(kw)
        lib.elimrec_bootstrap_means(a["rows"], a["rows_b"], a["n"], a["C"], a["ld"], a["ptr"], a["grows"], a["listed"], a["G"], a["R"], SEED,
                                    a["out"], a["ld_out"], a["lds"], None)
        assert b"null pointer" in lib.elimrec_last_error() or b"there are none" in lib.elimrec_last_error()


def test_wrapper_errors_that_need_no_device():
    from elimrec_amd import ops
    rows = torch.zeros(6, 3)
    ptr, listed = [0, 4, 6], [0, 1, 2, 3, 4, 5]
    for R in (0, -1, 2 ** 31, 2.5, True, None):
        with pytest.raises(ValueError, match="R must"):
            ops.bootstrap_means(rows, ptr, listed, R, SEED)
    for seed in (-1, 2 ** 64, 1.5, True, None):
        with pytest.raises(ValueError, match="seed"):
            ops.bootstrap_means(rows, ptr, listed, 4, seed)
    with pytest.raises(TypeError, match="float32"):
        ops.bootstrap_means(rows.double(), ptr, listed, 4, SEED)
    with pytest.raises(ValueError, match="unit column stride"):
        ops.bootstrap_means(torch.zeros(3, 6).t(), ptr, listed, 4, SEED)
    with pytest.raises(ValueError, match="unit column stride"):
        ops.bootstrap_means(torch.zeros(6), ptr, listed, 4, SEED)
    with pytest.raises(ValueError, match="at least one column"):
        ops.bootstrap_means(torch.zeros(6, 0), ptr, listed, 4, SEED)
    for b in (torch.zeros(6, 4), torch.zeros(5, 3), torch.zeros(6, 6)[:, :3]):
        with pytest.raises(ValueError, match="rows_b"):
            ops.bootstrap_means(rows, ptr, listed, 4, SEED, rows_b=b)
    with pytest.raises(TypeError, match="float32"):
        ops.bootstrap_means(rows, ptr, listed, 4, SEED, rows_b=rows.double())
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.bootstrap_means(rows.numpy(), ptr, listed, 4, SEED)
    for bad_ptr, bad_rows in (([0], []), ([1, 6], listed), ([0, 7], listed), ([0, 5, 4, 6], listed)):
        with pytest.raises(ValueError, match="group_ptr"):
            ops.bootstrap_means(rows, bad_ptr, bad_rows, 4, SEED)
    for bad_rows in ([0, 1, 2, 3, 4, 6], [-1, 1, 2, 3, 4, 5]):
        with pytest.raises(IndexError, match="row indices span"):
            ops.bootstrap_means(rows, ptr, bad_rows, 4, SEED)
    with pytest.raises(TypeError, match="integers"):
        ops.bootstrap_means(rows, ptr, [0.5] * 6, 4, SEED)
    index = ops.GroupIndex(ptr, listed, 6, "cpu")
    with pytest.raises(ValueError, match="carries its own rows"):
        ops.bootstrap_means(rows, index, listed, 4, SEED)
    with pytest.raises(IndexError, match="was checked for"):
        ops.bootstrap_means(rows[:5], index, None, 4, SEED)
    for out in (torch.zeros(4, 2, 3), torch.zeros(4, 2, 4, dtype=torch.float64), torch.zeros(4, 2, 6, dtype=torch.float64)[:, :, :3]):
        with pytest.raises(ValueError, match="out must"):
            ops.bootstrap_means(rows, index, None, 4, SEED, out=out)
    with pytest.raises(RuntimeError, match="HIP device"):                       # everything host-checkable is fine: no CPU path
        ops.bootstrap_means(rows, index, None, 4, SEED)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.bootstrap_means(rows, index, None, 4, SEED, out=torch.zeros(4, 2, 3, dtype=torch.float64), rows_b=rows)


def test_torch_ops_are_registered():
    from elimrec_amd import torch_ops
    ns = torch_ops.load()
    for name in ("bootstrap_means", "bootstrap_diff_means"):
        assert hasattr(ns, name) and name in torch_ops.OPS


def test_significance_report_checks():
    from elimrec_amd.evaluator import SignificanceReport, SignificanceTables, UniEvaluator
    ds = types.SimpleNamespace(num_items=6, num_users=4)
    train = {0: [1, 2], 1: [2], 2: [], 3: [0, 1, 2, 3]}
    test = {0: [3], 2: [4, 5], 3: [5]}
    for bad in (0, -1, 2 ** 31, 2.5, True, None):
        with pytest.raises(ValueError, match="replicates"):
            SignificanceReport(ds, train, test, [1, 3], replicates=bad)
    for bad in (0.0, 1.0, -0.5, 2, None, "0.9", True):
        with pytest.raises(ValueError, match="level"):
            SignificanceReport(ds, train, test, [1, 3], level=bad)
    for bad in (-1, 2 ** 64, 0.5, None, True):
        with pytest.raises(ValueError, match="seed"):
            SignificanceReport(ds, train, test, [1, 3], seed=bad)
    with pytest.raises((TypeError, ValueError)):
        SignificanceReport(ds, train, test, [1, 3], group_view=[3, 3])
    with pytest.raises(TypeError):
        SignificanceReport(ds, [1, 2], test, [1, 3])
    with pytest.raises(ValueError):
        SignificanceReport(ds, train, test, [1, 3], metric=["Recal"])
    with pytest.raises(TypeError, match="UniEvaluator"):
        SignificanceReport(ds, train, test, [1, 3], evaluator=object())
    rep = SignificanceReport(ds, train, test, [1, 3], metric=["Recall", "NDCG"], group_view=[2, 10], replicates=50, level=0.9, seed=7)
    assert (rep.replicates, rep.level, rep.seed, rep.users, rep.name) == (50, 0.9, 7, [0, 2, 3], "significance")
    assert rep.columns == ("Recall@1", "Recall@3", "NDCG@1", "NDCG@3") and rep._shown.tolist() == [0, 2, 3, 5]
    assert [x.strip() for x in rep.group_labels] == ["all:", "(0,2]:", "(2,10]:"]
    assert [p.tolist() for p in rep._positions] == [[0, 1, 2], [0, 1], [2]]
    assert SignificanceTables._fields == ("columns", "labels", "mean", "se", "lo", "hi", "p")
    ev = UniEvaluator(ds, train, test, metric=["MAP"], top_k=4)
    handed = SignificanceReport(ds, train, test, 4, evaluator=ev)
    assert handed.evaluator is ev and handed.users is ev.default_users() and handed.columns == ("MAP@1", "MAP@2", "MAP@3", "MAP@4")
    assert (handed.replicates, handed.level, handed.seed) == (2000, 0.95, 2022)
    with pytest.raises(TypeError):
        rep.evaluate(object())
    with pytest.raises(ValueError, match="metric_rows"):
        rep.evaluate(None, rows=torch.zeros(3, 5))
    with pytest.raises(ValueError, match="metric_rows"):
        rep.shift(torch.zeros(3, 4), torch.zeros(2, 4))


def test_basic_model_switches():
    g = load_golden("ml3")
    model, _ = build_model_from_fixture(g, "cpu")
    assert model.significance_reporter is None
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--significance_report=0", "--significance_level=7"])
    assert model.significance_reporter is None
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--significance_report=300", "--group_view=[2,4]", "--tie_order=id"])
    rep = model.significance_reporter
    assert (rep.replicates, rep.level, rep.seed) == (300, 0.95, 2022) and len(rep.group_labels) >= 2
    assert rep.evaluator is not model.test_evaluator.evaluator.evaluator and rep.evaluator.tie_order == "id"
    assert rep.users == model.test_evaluator.evaluator.evaluator.default_users()
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--significance_report=5", "--significance_level=0.8", "--significance_seed=11"])
    rep = model.significance_reporter
    assert (rep.replicates, rep.level, rep.seed) == (5, 0.8, 11) and rep.evaluator.tie_order == model.test_evaluator.evaluator.tie_order
    for bad in (["--significance_report=-2"], ["--significance_report=2.5"], ["--significance_report=%d" % 2 ** 31],
                ["--significance_report=5", "--significance_level=0"], ["--significance_report=5", "--significance_level=1"],
                ["--significance_report=5", "--significance_level=1.5"], ["--significance_report=5", "--significance_seed=-1"],
                ["--significance_report=5", "--significance_seed=0.5"]):
        with pytest.raises(ValueError):
            build_model_from_fixture(g, "cpu", extra_argv=bad)
