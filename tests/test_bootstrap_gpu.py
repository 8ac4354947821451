"""The bootstrap on the device: the kernel (csrc/bootstrap.hip) against the numpy model of tests/bootstrap_model.py, and what is
built on it: ops.bootstrap_means, torch.ops.elimrec.bootstrap_means / bootstrap_diff_means, reports.SignificanceReport and
--significance_report.

Where every value is a small integer or a multiple of 2^-10 in [0, 1], every partial sum of at most 2^31 of them is exact in
float64 whatever its order, and the kernel must give the model's BITS. For other values the bound is the textbook one for a
float64 sum of n terms in any order, |error| <= (n - 1) 2^-53 sum |x|: with n <= 1000 that is below 1.2e-13 mean |x| after the
division, so 1e-12 mean |x| over the drawn values holds with room for the division's own rounding -- against math.fsum, the exactly
rounded sum. Every input block is a column slice of a wider NaN matrix whose base is offset by one float (ld > C, no 16-byte
alignment), and the output lies between canaries: a read or a write outside shows up. The kernel has no workspace."""
import functools

import numpy as np
import pytest
import torch

import bootstrap_model as bm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, CANARY, PAD = 2022, -777.0, 9


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _slice(rows):
    """rows as rows 0 .. n - 1, columns 1 .. C of a [n + 1 x C + 3] NaN matrix on the device: the base is one float past an aligned
    address."""
    n, C = rows.shape
    wide = np.full((n + 1, C + 3), np.nan, dtype=np.float32)
    wide[:n, 1:1 + C] = rows
    view = _t(wide)[:n, 1:1 + C]
    assert view.stride(0) == C + 3 and view.data_ptr() % 16 == 4
    return view


def _run(rows, ptr, listed, R, seed=SEED, rows_b=None, lds=True):
    """One ops.bootstrap_means call between canaries -> float64 [R x G x C] on the host."""
    from elimrec_amd import ops
    G, C = len(ptr) - 1, rows.shape[1]
    flat = torch.full((R * G * C + 2 * PAD,), CANARY, dtype=torch.float64, device=DEV)
    out = flat[PAD:PAD + R * G * C].view(R, G, C)
    got = ops.bootstrap_means(_slice(rows), np.asarray(ptr, dtype=np.int64), np.asarray(listed, dtype=np.int32), R, seed, out=out,
                              rows_b=_slice(rows_b) if rows_b is not None else None, lds=lds)
    assert got is out
    host = flat.cpu().numpy()
    assert (host[:PAD] == CANARY).all() and (host[-PAD:] == CANARY).all()
    return host[PAD:-PAD].reshape(R, G, C).copy()


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _grid(n, C, seed=0):
    """Multiples of 2^-10 in [0, 1]: every sum of them is exact."""
    return (np.random.default_rng(seed).integers(0, 1025, (n, C)) / 1024.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _normal(n, C, seed=1):
    return np.random.default_rng(seed).standard_normal((n, C)).astype(np.float32)


SIZES = (1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1025)


def test_small_groups_draw_the_models_positions():
    """rows = identity: out * n_g counts how often every position was drawn."""
    from elimrec_amd import ops
    L = ops.BOOTSTRAP_MAX_COLUMNS
    sizes = [s for s in SIZES if s <= L] + [L]
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    listed = np.concatenate([np.arange(s) for s in sizes])
    R = 9
    out = _run(np.eye(L, dtype=np.float32), ptr, listed, R)
    for g, s in enumerate(sizes):
        for r in range(R):
            assert (out[r, g] * s).tolist() == np.bincount(bm.positions(SEED, r, g, s), minlength=L).tolist(), (s, r)


def test_larger_groups_draw_the_models_positions():
    """Columns i, i^2 and the bits of i: integer sums, exact in float64 -- bit for bit the model, whatever n_g % 4 is."""
    n = max(SIZES)
    i = np.arange(n)
    rows = np.stack([i, i * i] + [(i >> b) & 1 for b in range(11)], axis=1).astype(np.float32)
    assert rows.shape[1] == 13 and rows[:, 1].max() < 2 ** 24
    ptr = np.concatenate([[0], np.cumsum(SIZES)])
    listed = np.concatenate([np.arange(s)[::-1] for s in SIZES])                # (reversed: position j is row s - 1 - j)
    out = _run(rows, ptr, listed, 5)
    assert _same(out, bm.means(rows, ptr, listed, 5, SEED))


GROUPS_PTR = [0, 300, 420, 420, 600, 604]            # all, a part, an EMPTY group in the middle, another part, one row four times


def _groups():
    listed = np.concatenate([np.arange(300), np.arange(0, 120), np.arange(120, 300), [7, 7, 7, 7]])
    return GROUPS_PTR, listed


@pytest.mark.parametrize("C", [1, 3, 4, 5, 16, 17, 35])
def test_exact_values_are_the_models_bits(C):
    """C up to and beyond the column limit (the wrapper's slices), G = 5 with overlapping groups, an empty one and a repeated row,
    R one beyond the replicate tile."""
    from elimrec_amd import ops
    assert ops.BOOTSTRAP_MAX_COLUMNS == 16 and ops.BOOTSTRAP_TILE == 16
    rows = _grid(300, C)
    ptr, listed = _groups()
    out = _run(rows, ptr, listed, 17)
    want = bm.means(rows, ptr, listed, 17, SEED)
    assert np.isnan(out[:, 2]).all() and _same(out, want)
    assert (out[:, 4] == rows[7].astype(np.float64)).all()


@pytest.mark.parametrize("R", [1, 7])
def test_one_group_and_few_replicates(R):
    rows = _grid(40, 3, seed=3)
    out = _run(rows, [0, 40], np.arange(40), R)
    assert _same(out, bm.means(rows, [0, 40], np.arange(40), R, SEED))
    assert _same(out, _run(rows, [0, 40], np.arange(40), R, seed=SEED + (1 << 40))) is False        # the key's high word counts


def test_random_values_stay_within_the_float64_bound():
    rows = _normal(300, 5)
    ptr, listed = _groups()
    out = _run(rows, ptr, listed, 17)
    want = bm.means(rows, ptr, listed, 17, SEED, exact=True)
    scale = bm.means(np.abs(rows), ptr, listed, 17, SEED, exact=True)
    live = [0, 1, 3, 4]
    err = np.abs(out - want)[:, live] / scale[:, live]
    print("largest |error| / mean |x| against fsum: %.3g" % err.max())
    assert err.max() <= 1e-12 and np.isnan(out[:, 2]).all()


def test_both_forms():
    """A group on each side of ops.bootstrap_rows_in_lds in one call (two launches), and one small group through both forms."""
    from elimrec_amd import ops
    big, small = 40000, 50
    assert not ops.bootstrap_rows_in_lds(big, 1) and ops.bootstrap_rows_in_lds(small, 1)
    rows = _grid(big, 1, seed=4)
    ptr, listed = [0, big, big + small], np.concatenate([np.arange(big), np.arange(100, 100 + small)])
    out = _run(rows, ptr, listed, 4)
    assert _same(out, bm.means(rows, ptr, listed, 4, SEED))
    assert _same(out, _run(rows, ptr, listed, 4, lds=False))
    noisy = _normal(300, 5)                                                     # inexact sums: the two forms share one order
    gp, gl = _groups()
    assert all(ops.bootstrap_rows_in_lds(n, 5) for n in np.diff(gp))
    assert _same(_run(noisy, gp, gl, 17), _run(noisy, gp, gl, 17, lds=False))
    assert _same(_run(noisy, gp, gl, 17, rows_b=noisy[::-1].copy()), _run(noisy, gp, gl, 17, rows_b=noisy[::-1].copy(), lds=False))


def test_a_replicates_bits_depend_on_its_own_inputs_only():
    rows = _normal(300, 35)
    ptr, listed = _groups()
    first = _run(rows, ptr, listed, 7)
    assert _same(first, _run(rows, ptr, listed, 7))                             # twice
    assert _same(first, _run(rows, ptr, listed, 64)[:7])                        # R
    # the other groups' contents: group 3 keeps its index and its rows
    other = np.concatenate([np.arange(299, -1, -1), np.arange(100, 220), np.arange(120, 300), [9, 8, 7, 6]])
    assert _same(first[:, 3], _run(rows, ptr, other, 7)[:, 3]) and not _same(first[:, 0], _run(rows, ptr, other, 7)[:, 0])
    # more groups behind it, fewer listed rows in front of it
    ptr2, listed2 = [0, 0, 0, 0, 180, 180, 480], np.concatenate([np.arange(120, 300), np.arange(300)])
    assert _same(first[:, 3], _run(rows, ptr2, listed2, 7)[:, 3])
    # a column alone, in a narrow slice and inside the wide block (columns 0 .. 15, 16 .. 31, 32 .. 34 are three launches)
    for c in (0, 15, 16, 34):
        assert _same(first[:, :, c], _run(rows[:, c:c + 1].copy(), ptr, listed, 7)[:, :, 0]), c
    assert _same(first[:, :, 14:19], _run(rows[:, 14:19].copy(), ptr, listed, 7))


def test_paired_differences():
    ptr, listed = _groups()
    a, b = _grid(300, 5, seed=5), _grid(300, 5, seed=6)
    assert _same(_run(a, ptr, listed, 17, rows_b=b), bm.means(a, ptr, listed, 17, SEED, rows_b=b))
    x, y = _normal(300, 17), _normal(300, 17, seed=2)
    out = _run(x, ptr, listed, 7, rows_b=y)
    want = bm.means(x, ptr, listed, 7, SEED, rows_b=y, exact=True)
    scale = bm.means(np.abs(y.astype(np.float64) - x).astype(np.float32), ptr, listed, 7, SEED, exact=True)
    live = [0, 1, 3, 4]
    assert (np.abs(out - want)[:, live] / scale[:, live]).max() <= 1e-12
    zero = _run(x, ptr, listed, 7, rows_b=x.copy())
    assert (zero[:, live] == 0.0).all() and np.isnan(zero[:, 2]).all()


def test_non_finite_rows():
    ptr, listed = _groups()
    rows = _grid(300, 3, seed=7)
    rows[11, 1] = np.nan
    out = _run(rows, ptr, listed, 17)
    for g in (0, 1, 3):
        seg = listed[ptr[g]:ptr[g + 1]]
        drawn = np.array([(seg[bm.positions(SEED, r, g, seg.size)] == 11).any() for r in range(17)])
        assert np.array_equal(np.isnan(out[:, g, 1]), drawn) and not np.isnan(out[:, g, [0, 2]]).any()
        assert drawn.any() == (g != 3)
    rows[11, 1], rows[20, 0], rows[30, 0], rows[40, 2] = 0.5, np.inf, -np.inf, -np.inf
    out = _run(rows, ptr, listed, 17)
    want = bm.means(rows, ptr, listed, 17, SEED)
    assert np.array_equal(out, want, equal_nan=True) and np.isposinf(out).any() and np.isneginf(out).any()
    assert np.array_equal(np.isnan(out), np.isnan(want))


def test_torch_ops():
    from elimrec_amd import ops, torch_ops
    torch_ops.load()
    ptr, listed = _groups()
    a, b = _slice(_normal(300, 17)), _slice(_normal(300, 17, seed=2))
    gp, gl = _t(np.asarray(ptr, dtype=np.int64)), _t(np.asarray(listed, dtype=np.int32))
    one = torch.ops.elimrec.bootstrap_means(a, gp, gl, 17, SEED)
    assert one.dtype == torch.float64 and tuple(one.shape) == (17, 5, 17)
    assert _same(one.cpu().numpy(), ops.bootstrap_means(a, ptr, listed, 17, SEED).cpu().numpy())
    two = torch.ops.elimrec.bootstrap_diff_means(a, b, gp, gl, 17, SEED)
    assert _same(two.cpu().numpy(), ops.bootstrap_means(a, ops.GroupIndex(ptr, listed, 300, DEV), None, 17, SEED, rows_b=b).cpu().numpy())
    with pytest.raises(RuntimeError, match="row indices span"):
        torch.ops.elimrec.bootstrap_means(a, gp, gl + 1, 17, SEED)
    with pytest.raises(RuntimeError, match="R < 2"):
        torch.ops.elimrec.bootstrap_means(a, gp, gl, 0, SEED)


def _forward(extra=()):
    from helpers import build_model_from_fixture, load_golden
    g = load_golden("ml3")
    model, _ = build_model_from_fixture(g, DEV, extra_argv=extra)
    model.bpr_loss(_t(g["step1/users"]), _t(g["step1/pos"]), _t(g["step1/neg"]))
    return model


@pytest.mark.parametrize("view", [None, [2, 4]])
def test_significance_report(view):
    from elimrec_amd.evaluator import GroupedEvaluator, SignificanceReport, UniEvaluator, bootstrap_summary
    model = _forward()
    ds = model.dataset
    train, test = ds.get_user_train_dict(), ds.get_user_test_dict()
    topk = [1, 3, 5]
    report = SignificanceReport(ds, train, test, topk, metric=["Recall", "NDCG"], group_view=view, replicates=200, level=0.9, seed=5)
    G, Cs, n = len(report.group_labels), 6, len(report.users)
    assert (G > 1) == (view is not None)
    kept = {}
    for effect in ("TE", "TIE"):
        model.predict_type = effect
        rows, columns = kept[effect] = report.metric_rows(model)
        assert columns == ("Recall@1", "Recall@3", "Recall@5", "NDCG@1", "NDCG@3", "NDCG@5") and tuple(rows.shape) == (n, Cs)
        final, buf = report.evaluate(model, kept[effect])
        assert final.columns == columns and final.labels == report.group_labels and final.p is None
        assert all(x.shape == (G, Cs) for x in (final.mean, final.se, final.lo, final.hi)) and final.mean.dtype == np.float32
        # the point estimates: the evaluators' own numbers of the same pass, bit for bit
        uni = UniEvaluator(ds, train, test, metric=["Recall", "NDCG"], top_k=topk)
        assert final.mean[0].tobytes() == np.asarray(uni.evaluate(model)[0], dtype=np.float32).tobytes()
        if view is not None:
            grouped = GroupedEvaluator(ds, train, test, metric=["Recall", "NDCG"], group_view=view, top_k=topk)
            assert grouped.group_labels == report.group_labels[1:]
            assert final.mean[1:].tobytes() == np.asarray(grouped.evaluate(model)[0], dtype=np.float32).tobytes()
        # the spread: the model's replicates of these rows through bootstrap_summary
        ptr = np.concatenate([[0], np.cumsum([p.size for p in report._positions])])
        listed = np.concatenate(report._positions)
        want = bootstrap_summary(bm.means(rows.cpu().numpy(), ptr, listed, 200, 5, exact=True), final.mean, 0.9)
        for name in ("se", "lo", "hi"):
            np.testing.assert_allclose(getattr(final, name), getattr(want, name), rtol=1e-9, atol=1e-15)
        assert (final.lo <= final.hi).all() and (final.se >= 0).all()
        lines = buf.split("\n")
        assert len(lines) == 1 + 4 * G and lines[0].startswith("columns:") and all(c in lines[0] for c in columns)
        assert [ln.split("\t")[0].strip() for ln in lines[1:5]] == ["all: mean", "all: se", "all: lo", "all: hi"]
        assert report.evaluate(model)[1] == buf                                  # the pass repeats: the same rows, the same table
    same, buf = report.shift(kept["TE"], kept["TE"])
    assert all((x == 0).all() for x in (same.mean, same.se, same.lo, same.hi)) and (same.p == 1.0).all()
    assert [ln.split("\t")[0].strip() for ln in buf.split("\n")[1:6]] == ["all: mean", "all: se", "all: lo", "all: hi", "all: p"]
    moved, _ = report.shift(kept["TE"], kept["TIE"])
    a, b = kept["TE"][0].cpu().numpy(), kept["TIE"][0].cpu().numpy()
    np.testing.assert_allclose(moved.mean[0], (b.astype(np.float64) - a).mean(0), rtol=1e-6, atol=1e-7)
    want = bootstrap_summary(bm.means(a, ptr, listed, 200, 5, rows_b=b, exact=True), moved.mean, 0.9)
    for name in ("se", "lo", "hi", "p"):
        np.testing.assert_allclose(getattr(moved, name), getattr(want, name), rtol=1e-9, atol=1e-15)
    with pytest.raises(ValueError):
        report.shift(kept["TE"], kept["TIE"][0][:-1])


def test_driver_switch(tmp_path):
    from test_lists_gpu import _driver
    off, ev0, te0 = _driver(tmp_path / "a", ["--group_view=[10,30]"])
    assert not any("bootstrap" in ln or "metric intervals" in ln for ln in off)
    on, ev1, te1 = _driver(tmp_path / "b", ["--group_view=[10,30]", "--significance_report=200"])
    added = [k for k, ln in enumerate(on) if ln.startswith("  [TE] metric intervals (200 replicates, 95 %):\n")
             or ln.startswith("  [TIE] metric intervals (200 replicates, 95 %):\n")
             or ln.startswith("  [TE->TIE] metric difference, paired bootstrap:\n")]
    assert len(added) == 3 and [ln for k, ln in enumerate(on) if k not in added] == off      # with the switch off: the log as it was
    te, tie, shift = added
    assert on[te - 1].startswith("  [TE] by training interactions") and on[te + 1].startswith("  [TIE]\t") and shift == len(on) - 1
    for k in (te, tie):
        assert all(w in on[k] for w in ("\nall: mean", "\nall: se", "\nall: lo", "\nall: hi", "\n(0,10]: mean", "Recall@")) and "all: p" not in on[k]
    assert "\nall: p" in on[shift] and "\n(10,30]: p" in on[shift]
    metric_lines = lambda log: [ln for ln in log if ln.startswith("  [TE]\t") or ln.startswith("  [TIE]\t")]     # noqa: E731
    assert len(metric_lines(on)) == 2 and metric_lines(on) == metric_lines(off)
    assert ev0.tobytes() == ev1.tobytes() and te0.tobytes() == te1.tobytes()
