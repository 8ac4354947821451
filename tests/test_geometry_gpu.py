"""The embedding-geometry kernels on the device (csrc/geometry.hip) against the float64 model of tests/geometry_model.py, and what
is built on them: ops.uniformity_sum / row_gram, EliMRec.geometry_device / embedding_geometry / alignment,
evaluator.GeometryReport, --geometry_report, torch.ops.elimrec.uniformity_sum / row_gram.

Tolerances are derived, not measured.
Uniformity: |log(S / pairs) - model| <= 2 t (d + 4) 2^-23 + 4 * 2^-23: the worst-case fp32 error of a cosine of unit rows times
the slope 2 t of the exponent, plus 2 ulp each for expf and for the fp32 rounding of its argument; every term's relative error is
within that, so the mean's is; the float64 sum adds nothing visible.
Gram: the products of the fp32 unit rows are exact in float64, so only the order of n additions differs from the model's:
|dG_ab| <= n 2^-52 sum |x^_a x^_b|, likewise for m.
Alignment: twice the cosine's error, (d + 4) 2^-22."""
import numpy as np
import pytest
import torch

import geometry_model as gm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _consts():
    from elimrec_amd import ops
    return ops.GEOMETRY_TILE, ops.GEOMETRY_CHUNK, ops.GEOMETRY_SEGMENT


def _rows(n_rows, d, seed, zero=()):
    rng = np.random.default_rng(seed)
    T = rng.standard_normal((n_rows, d)).astype(np.float32) * rng.uniform(0.5, 3.0, (n_rows, 1)).astype(np.float32)
    T[list(zero)] = 0.0
    return T


def _tol(t, d):
    return 2.0 * t * (d + 4) * 2.0 ** -23 + 4 * 2.0 ** -23


def _uni(T, sq, rows, t=2.0, table=None, norms=None):
    from elimrec_amd import ops
    S, pairs, n_valid = ops.uniformity_sum(_t(T) if table is None else table, _t(sq) if norms is None else norms,
                                           _t(np.asarray(rows, dtype=np.int32)), t)
    return S, pairs, n_valid, ops.uniformity_value(S, pairs)


def _check_uni(T, sq, rows, t=2.0, **kw):
    S, pairs, n_valid, uni = _uni(T, sq, rows, t, **kw)
    wS, wpairs, wn, wuni = gm.uniformity_model(T, sq, rows, t)
    print("uniformity n=%d d=%d t=%g: got %.12g want %.12g diff %.3g tol %.3g" % (len(rows), T.shape[1], t, uni, wuni, abs(uni - wuni),
                                                                                _tol(t, T.shape[1])))
    assert (pairs, n_valid) == (wpairs, wn)
    if wn < 2:
        assert S == 0.0 and np.isnan(uni)
    else:
        assert abs(uni - wuni) <= _tol(t, T.shape[1])
    return S, pairs, n_valid, uni


# --------------------------------------------------------------------------- uniformity
@pytest.mark.parametrize("d", [4, 32, 64, 68, 128, 256])
def test_uniformity_sizes(d):
    TILE, CHUNK, _ = _consts()
    sizes = [0, 1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1] + ([CHUNK + 1] if d == 4 else [])
    T = _rows(max(sizes), d, 100 + d)
    sq = gm.sqnorms(T)
    for n in sizes:
        _check_uni(T, sq, np.arange(n), 2.0)
    _check_uni(T, sq, np.arange(2 * TILE + 1), 0.5)


@pytest.mark.parametrize("d", [4, 64, 68])
def test_uniformity_of_a_column_slice_with_strided_norms(d):
    TILE, _, _ = _consts()
    n = 2 * TILE + 1
    T = _rows(n, d, 7 + d, zero=(5,))
    sq = gm.sqnorms(T)
    wide = np.full((n + 2, d + 12), np.nan, dtype=np.float32)
    wide[1:1 + n, 8:8 + d] = T
    norms = np.full((n, 3), np.nan, dtype=np.float32)
    norms[:, 1] = sq
    table, nview = _t(wide)[1:1 + n, 8:8 + d], _t(norms)[:, 1]
    assert nview.stride(0) == 3 and table.stride(0) == d + 12
    for t in (0.5, 2.0):
        _check_uni(T, sq, np.arange(n), t, table=table, norms=nview)
    odd = np.full((n, d + 3), np.nan, dtype=np.float32)                       # a row stride that is no multiple of 4: no vector load
    odd[:, :d] = T
    _check_uni(T, sq, np.arange(n), 2.0, table=_t(odd)[:, :d])


@pytest.mark.parametrize("d", [4, 64, 68])
def test_uniformity_lists(d):
    TILE, _, _ = _consts()
    n_rows = 90
    T = _rows(n_rows, d, 31 + d, zero=(0, 17, 89))
    sq = gm.sqnorms(T)
    rng = np.random.default_rng(5)
    rows = rng.integers(0, n_rows, size=2 * TILE + 9)                        # repeated ids, rows without a norm
    rows[[3, 64, 100]] = -1
    rows[[0, 65, 136]] = [n_rows, n_rows + 1000, 2 ** 31 - 1]                # past the table
    rows[10] = -7
    S, pairs, n_valid, _ = _check_uni(T, sq, rows)
    assert n_valid < rows.size - 6
    _check_uni(T, sq, [0, 17, 89, -1, n_rows])                               # nothing valid
    _check_uni(T, sq, [0, 4, 17])                                            # one valid row: no pair
    _check_uni(T, sq, np.full(TILE + 3, -1))


def test_uniformity_fixed_cases():
    for d in (4, 64, 68):
        x = _rows(1, d, d)[0]
        T = np.stack([x, -x, 2 * x, np.zeros(d, dtype=np.float32)])
        sq = gm.sqnorms(T)
        for t in (0.5, 2.0):
            S, pairs, n, uni = _uni(T, sq, [0, 1], t)                        # antipodal
            assert (pairs, n) == (1, 2) and abs(uni + 4 * t) <= _tol(t, d)
            S, pairs, n, uni = _uni(T, sq, [0] * 70 + [2] * 70, t)          # all rows equal (up to scale)
            assert (pairs, n) == (140 * 139 // 2, 140) and abs(uni) <= _tol(t, d)
            S, pairs, n, uni = _uni(T, sq, [0, 0], t)                        # a repeated id contributes a pair
            assert (pairs, n) == (1, 2) and abs(uni) <= _tol(t, d)
            S, pairs, n, uni = _uni(T, sq, [0, 3, 1, 0], t)                  # (x, -x), (x, x), (-x, x)
            assert (pairs, n) == (3, 3) and abs(uni - np.log((2 * np.exp(-4.0 * t) + 1) / 3)) <= _tol(t, d)


@pytest.mark.parametrize("d", [64, 68])
def test_uniformity_invariance(d):
    TILE, CHUNK, _ = _consts()
    n = CHUNK + TILE + 5 if d == 64 else 2 * TILE + 1
    T = _rows(n + 40, d, 900 + d)
    sq = gm.sqnorms(T)
    rows = np.random.default_rng(1).permutation(n + 40)[:n]
    a, b = _uni(T, sq, rows), _uni(T, sq, rows)
    assert np.float64(a[0]).tobytes() == np.float64(b[0]).tobytes() and a[1:3] == b[1:3]      # two calls: the same bits
    r = _uni(T, sq, rows[::-1].copy())
    assert r[1:3] == a[1:3] and abs(r[0] - a[0]) <= a[1] * 2.0 ** -52 * a[0]
    assert abs(a[3] - gm.uniformity_model(T, sq, rows, 2.0)[3]) <= _tol(2.0, d)
    # a sub-list does not depend on what else is in the table: the same rows inside another table, at other ids
    sub = rows[:TILE + 7]
    small = T[sub]
    c = _uni(T, sq, sub)
    e = _uni(small, gm.sqnorms(small), np.arange(sub.size))
    assert np.float64(c[0]).tobytes() == np.float64(e[0]).tobytes() and c[1:3] == e[1:3]


# --------------------------------------------------------------------------- Gram
def _check_gram(T, sq, rows, table=None, norms=None):
    from elimrec_amd import ops
    d = T.shape[1]
    G, m, n_valid = ops.row_gram(_t(T) if table is None else table, _t(sq) if norms is None else norms, _t(np.asarray(rows, dtype=np.int32)))
    assert G.dtype == m.dtype == torch.float64 and tuple(G.shape) == (d, d) and tuple(m.shape) == (d,)
    G, m = G.cpu().numpy(), m.cpu().numpy()
    wG, wm, wn, A, a = gm.gram_model(T, sq, rows)
    assert n_valid == wn
    assert np.array_equal(G, G.T)                                            # exactly symmetric
    n = max(len(rows), 1)
    assert (np.abs(G - wG) <= n * 2.0 ** -52 * A).all() and (np.abs(m - wm) <= n * 2.0 ** -52 * a).all()
    if wn:
        assert abs(np.trace(G) / wn - 1.0) <= (d + 4) * 2.0 ** -23
    return G, m, n_valid


@pytest.mark.parametrize("d", [4, 64, 68, 256])
def test_gram_sizes(d):
    _, _, SEG = _consts()
    sizes = [1, SEG - 1] if d == 256 else [1, SEG - 1, SEG, SEG + 1, 2 * SEG + 3]
    T = _rows(max(sizes), d, 300 + d, zero=(3,) if max(sizes) > 3 else ())
    sq = gm.sqnorms(T)
    for n in sizes:
        _check_gram(T, sq, np.arange(n))
    G, m, n_valid = _check_gram(T, sq, [])
    assert n_valid == 0 and not G.any() and not m.any()


@pytest.mark.parametrize("d", [4, 68])
def test_gram_lists_and_forms(d):
    _, _, SEG = _consts()
    n_rows = 90
    T = _rows(n_rows, d, 77 + d, zero=(0, 17))
    sq = gm.sqnorms(T)
    rows = np.random.default_rng(9).integers(0, n_rows, size=SEG + 41)
    rows[[3, 64, 500]] = -1
    rows[[0, 65, 520]] = [n_rows, n_rows + 1000, 2 ** 31 - 1]
    G, m, n_valid = _check_gram(T, sq, rows)
    assert 0 < n_valid < rows.size - 6
    _check_gram(T, sq, [0, 17, -1, n_rows])                                  # nothing valid
    wide = np.full((n_rows + 2, d + 12), np.nan, dtype=np.float32)
    wide[1:1 + n_rows, 8:8 + d] = T
    norms = np.full((n_rows, 3), np.nan, dtype=np.float32)
    norms[:, 1] = sq
    G2, m2, _ = _check_gram(T, sq, rows, table=_t(wide)[1:1 + n_rows, 8:8 + d], norms=_t(norms)[:, 1])
    assert G2.tobytes() == G.tobytes() and m2.tobytes() == m.tobytes()       # the bits do not depend on the table's form


def test_torch_ops_return_what_the_ops_return():
    from elimrec_amd import ops, torch_ops
    t_ops = torch_ops.load()
    TILE, _, _ = _consts()
    T = _rows(2 * TILE + 1, 64, 4, zero=(2,))
    sq = gm.sqnorms(T)
    rows = _t(np.r_[np.arange(2 * TILE + 1), -1, 5].astype(np.int32))
    S, pairs, n_valid = ops.uniformity_sum(_t(T), _t(sq), rows, 0.5)
    s2, counts = t_ops.uniformity_sum(_t(T), _t(sq), rows, 0.5)
    assert s2.cpu().numpy().tobytes() == np.float64(S).tobytes() and counts.cpu().tolist() == [pairs, n_valid]
    G, m, n = ops.row_gram(_t(T), _t(sq), rows)
    g2, m2, c2 = t_ops.row_gram(_t(T), _t(sq), rows)
    assert torch.equal(G, g2) and torch.equal(m, m2) and c2.cpu().tolist() == [n]
    with pytest.raises(RuntimeError, match="0 < t <= 8"):
        t_ops.uniformity_sum(_t(T), _t(sq), rows, 0.0)


# --------------------------------------------------------------------------- the model and the report
def _forward(name, extra=()):
    from helpers import build_model_from_fixture, load_golden
    g = load_golden(name)
    model, _ = build_model_from_fixture(g, DEV, extra_argv=extra)
    model.bpr_loss(_t(g["step1/users"]), _t(g["step1/pos"]), _t(g["step1/neg"]))
    return model


def _host_tables(model):
    """(Y, sqn) of the cached tables copied to the host, the pending forward made real first."""
    sqn = model._block_sqnorms(model._cached_tables("the test needs"))
    return model._ws["Y"].cpu().numpy(), sqn.cpu().numpy()


def _space_tables(model, Y, sqn, side, h):
    lo, n = model._side_rows(side)
    d = model.latent_dim
    return Y[lo:lo + n, h * d:(h + 1) * d], sqn[lo:lo + n, h]


def _check_row(got, want, t, d):
    """One row of GEOMETRY_COLUMNS against the model's: n exact, uniformity within its bound, the spectrum columns -- float64
    eigenvalues of Gram matrices that agree to n 2^-52 -- to 1e-9."""
    assert got[0] == want[0]
    for k in range(1, 6):
        if np.isnan(want[k]):
            assert np.isnan(got[k]), (k, got, want)
        else:
            assert abs(got[k] - want[k]) <= (_tol(t, d) if k == 1 else 1e-9 * max(1.0, abs(want[k]))), (k, got, want)


@pytest.mark.parametrize("name", ["ml3", "kwai"])
def test_embedding_geometry_and_alignment(name):
    from helpers import build_model_from_fixture, load_golden
    from elimrec_amd.evaluator import GEOMETRY_COLUMNS, CandidateScoringError
    from elimrec_amd.model import Geometry
    fresh, _ = build_model_from_fixture(load_golden(name), DEV)
    with pytest.raises(RuntimeError):
        fresh.embedding_geometry()
    model = _forward(name)
    Y, sqn = _host_tables(model)
    d, spaces = model.latent_dim, ("fused",) + tuple(model._mods)
    assert len(spaces) == (2 if name == "kwai" else 4)
    for side in ("item", "user"):
        for t in (2.0, 0.5):
            got = model.embedding_geometry(side=side, t=t)
            assert isinstance(got, Geometry) and got.columns == GEOMETRY_COLUMNS and got.labels == spaces
            assert got.values.device.type == "cpu" and tuple(got.values.shape) == (len(spaces), 6) and got.values.dtype == torch.float64
            for h in range(len(spaces)):
                T, sq = _space_tables(model, Y, sqn, side, h)
                _check_row(got.values[h].numpy(), gm.geometry_row_model(T, sq, np.arange(T.shape[0]), t), t, d)
    T, sq = _space_tables(model, Y, sqn, "item", 1)
    sub = [5, 2, 2, 9, 0]
    one = model.embedding_geometry(space=spaces[1], rows=sub)
    assert one.labels == (spaces[1],) and tuple(one.values.shape) == (1, 6)
    _check_row(one.values[0].numpy(), gm.geometry_row_model(T, sq, sub, 2.0), 2.0, d)
    raw = model.geometry_device("item", spaces[1], _t(np.asarray(sub + [-1, 10 ** 6], dtype=np.int32)))
    assert all(x.is_cuda for x in raw) and int(raw[2].item()) == 5 and int(raw[1].item()) == 10
    # alignment: per space against the model, and bit for bit 2 - 2 x the score pick_hard_negatives returns
    U_, I = model.num_users, model.num_items
    rng = np.random.default_rng(3)
    users, items = rng.integers(0, U_, 50), rng.integers(0, I, 50)
    got = model.alignment(users, items)
    assert got.device.type == "cpu" and got.dtype == torch.float32 and tuple(got.shape) == (50, len(spaces))
    for h, s in enumerate(spaces):
        TU, squ = _space_tables(model, Y, sqn, "user", h)
        TI, sqi = _space_tables(model, Y, sqn, "item", h)
        want = gm.alignment_model(TU, squ, TI, sqi, users, items)
        assert np.abs(got[:, h].numpy().astype(np.float64) - want).max() <= (d + 4) * 2.0 ** -22
        score = model.hard_negatives_device(_t(users.astype(np.int64)), _t(items.astype(np.int32).reshape(-1, 1)), s)[2].cpu().numpy()
        assert got[:, h].numpy().tobytes() == (np.float32(2) - np.float32(2) * score).astype(np.float32).tobytes()
        assert model.alignment(users, items, space=s).numpy().tobytes() == got[:, h].contiguous().numpy().tobytes()
    model._eval_shard = object()
    try:
        with pytest.raises(CandidateScoringError):
            model.embedding_geometry()
    finally:
        model._eval_shard = None


@pytest.mark.parametrize("name,views", [("ml3", (None, None)), ("ml3", ([1, 3, 5], [1, 4])), ("kwai", ([2, 4], [2]))])
def test_geometry_report(name, views, monkeypatch):
    from elimrec_amd import ops
    from elimrec_amd.evaluator import GEOMETRY_COLUMNS, GeometryReport, GeometryTables
    model = _forward(name)
    train, test = model.dataset.get_user_train_dict(), model.dataset.get_user_test_dict()
    report = GeometryReport(model.dataset, train, test, group_view=views[0], item_group_view=views[1], t=0.5)
    calls = []
    real = ops.uniformity_sum_device
    monkeypatch.setattr(ops, "uniformity_sum_device", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    final, buf = report.evaluate(model)
    Y, sqn = _host_tables(model)
    d, spaces = model.latent_dim, ("fused",) + tuple(model._mods)
    n_sets = len(report.row_sets)
    assert isinstance(final, GeometryTables) and final.columns == GEOMETRY_COLUMNS and len(calls) == len(spaces) * n_sets
    assert final.values.shape == (len(spaces) * n_sets, 6) and (n_sets > 2) == (views[0] is not None)
    single = 0
    for h, s in enumerate(spaces):
        for k, (label, side, ids) in enumerate(report.row_sets):
            T, sq = _space_tables(model, Y, sqn, side, h)
            assert ids is None or ids.size > 0                                # an empty group is omitted
            want = gm.geometry_row_model(T, sq, np.arange(T.shape[0]) if ids is None else ids, 0.5)
            _check_row(final.values[h * n_sets + k], want, 0.5, d)
            assert final.labels[h * n_sets + k].startswith("%s %s" % (s, label.rstrip(":")))
            single += want[0] == 1 and np.isnan(final.values[h * n_sets + k][1])
    # alignment: the float64 mean of the pairs' fp32 values, rounded once; the pairs' values within (d + 4) 2^-22 of the model's
    assert final.align.shape == (2 * len(spaces), len(report.align_columns)) and final.align.dtype == np.float32
    for w, which in enumerate(("align_train", "align_test")):
        users, items, cols, positions = report._pairs[which]
        pair_rows = model.alignment(users, items).numpy()
        for h in range(len(spaces)):
            TU, squ = _space_tables(model, Y, sqn, "user", h)
            TI, sqi = _space_tables(model, Y, sqn, "item", h)
            want = gm.alignment_model(TU, squ, TI, sqi, users, items)
            row = final.align[2 * h + w]
            for c in range(len(report.align_columns)):
                if c in cols:
                    p = positions[cols.index(c)]
                    assert row[c] == np.float32(pair_rows[p, h].astype(np.float64).mean())
                    assert abs(float(row[c]) - want[p].mean()) <= (d + 4) * 2.0 ** -22 + 2.0 ** -23
                else:
                    assert np.isnan(row[c])                                  # a group without a pair
            assert final.align_labels[2 * h + w].startswith("%s %s" % (spaces[h], which))
        bare = [(sqn[users, h] == 0) | (sqn[model.num_users + items, h] == 0) for h in range(len(spaces))]
        assert [report.num_no_norm[(which, s)] for s in spaces] == [int(b.sum()) for b in bare]
    lines = buf.split("\n")
    assert lines[0].startswith("columns:") and all(c in lines[0] for c in GEOMETRY_COLUMNS)
    assert sum(ln.startswith("columns:") for ln in lines) == 2 and len(lines) == 2 + len(final.labels) + len(final.align_labels)
    # a second evaluate on the same table version launches nothing
    n_calls = len(calls)
    again, buf2 = report.evaluate(model)
    assert len(calls) == n_calls and buf2 == buf and again is final
    if views[0] is not None and name == "ml3":
        assert single >= 0


def test_a_group_with_a_single_row_has_no_uniformity():
    """A GeometryReport whose item view isolates single items: NaN uniformity and spectrum, n = 1, centre = 1."""
    from elimrec_amd.evaluator import GeometryReport
    model = _forward("ml3")
    train, test = model.dataset.get_user_train_dict(), model.dataset.get_user_test_dict()
    counts = np.bincount(np.asarray([i for v in train.values() for i in v], dtype=np.int64), minlength=model.num_items)
    alone = [int(c) for c in np.unique(counts) if c > 0 and (counts == c).sum() == 1]
    assert alone, "the fixture has an item whose training count no other item shares"
    c = alone[0]
    view = [c - 1, c] if c > 1 else [c]
    report = GeometryReport(model.dataset, train, test, item_group_view=view)
    final, _ = report.evaluate(model)
    label = "item (%d,%d]" % (c - 1 if c > 1 else 0, c)
    hits = [k for k, x in enumerate(final.labels) if label in x]
    assert len(hits) == 1 + len(model._mods)
    for k in hits:
        n, uni, erank, top1, rank99, centre = final.values[k]
        assert n == 1 and np.isnan(uni) and np.isnan(erank) and np.isnan(top1) and np.isnan(rank99) and abs(centre - 1) <= 2.0 ** -22


def test_driver_switch(tmp_path):
    from test_lists_gpu import _driver
    view = ["--group_view=[10,30]", "--item_group_view=[1,4]", "--neighbour_report=3"]
    off, ev0, te0 = _driver(tmp_path / "a", view)
    assert not any("[geometry]" in ln for ln in off)
    zero, ev2, te2 = _driver(tmp_path / "c", view + ["--geometry_report=0"])
    assert zero == off and ev0.tobytes() == ev2.tobytes() and te0.tobytes() == te2.tobytes()
    on, ev1, te1 = _driver(tmp_path / "b", view + ["--geometry_report=1", "--geometry_t=0.5"])
    added = [k for k, ln in enumerate(on) if ln.startswith("  [geometry]")]
    assert len(added) == 1 and added[0] == len(on) - 1                       # once, after both effects' lines and [neighbours]
    assert [ln for k, ln in enumerate(on) if k not in added] == off          # every other line is as it was
    block = on[added[0]]
    assert "t = 0.5" in block.split("\n")[0] and all(c in block for c in ("uniformity", "erank", "top1", "rank99", "centre"))
    assert all(x in block for x in ("fused user:", "fused item:", "fused align_train:", "fused align_test:", "item cold"))
    assert ev0.tobytes() == ev1.tobytes() and te0.tobytes() == te1.tobytes()
