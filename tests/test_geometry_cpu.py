"""The host side of the embedding geometry (no GPU): reports.spectrum_summary on constructed spectra, the numpy model of
tests/geometry_model.py by hand, every argument error of the ops, of EliMRec.embedding_geometry / alignment and of GeometryReport
before the device is needed, the --geometry_report switch, and the new entries in the header, the binding and the torch registry."""
import inspect
import os

import numpy as np
import pytest
import torch

import geometry_model as gm
from helpers import build_model_from_fixture, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------- the spectrum
@pytest.mark.parametrize("d", [4, 8, 64])
def test_spectrum_of_an_isotropic_space(d):
    from elimrec_amd.reports import spectrum_summary
    n = 1000
    erank, top1, rank99, centre = spectrum_summary(np.eye(d) * n / d, np.zeros(d), n)
    assert abs(erank - d) < 1e-9 * d and abs(top1 - 1.0 / d) < 1e-12 and centre == 0.0
    assert rank99 == np.ceil(0.99 * d - 1e-9)


def test_spectrum_of_a_rank_one_table():
    from elimrec_amd.reports import spectrum_summary
    d, n = 8, 50
    x = np.zeros(d)
    x[2] = 1.0
    X = np.outer(np.where(np.arange(n) % 2 == 0, 1.0, -1.0), x)              # +x and -x in turn: mean 0, one direction
    erank, top1, rank99, centre = spectrum_summary(X.T @ X, X.sum(0), n)
    assert abs(erank - 1.0) < 1e-12 and top1 == 1.0 and rank99 == 1.0 and centre == 0.0


def test_spectrum_of_collapsed_rows_and_of_too_few():
    from elimrec_amd.reports import spectrum_summary
    d, n = 8, 40
    x = np.full(d, 1.0 / np.sqrt(d))
    erank, top1, rank99, centre = spectrum_summary(n * np.outer(x, x), n * x, n)
    assert np.isnan(erank) and np.isnan(top1) and np.isnan(rank99) and abs(centre - 1.0) < 1e-12
    erank, top1, rank99, centre = spectrum_summary(np.outer(x, x), x, 1)
    assert np.isnan(erank) and np.isnan(top1) and np.isnan(rank99) and abs(centre - 1.0) < 1e-12
    assert all(np.isnan(v) for v in spectrum_summary(np.zeros((d, d)), np.zeros(d), 0))
    with pytest.raises(ValueError):
        spectrum_summary(np.zeros((d, d + 1)), np.zeros(d), 3)
    with pytest.raises(ValueError):
        spectrum_summary(np.zeros((d, d)), np.zeros(d + 1), 3)


def test_spectrum_of_two_unequal_directions():
    from elimrec_amd.reports import spectrum_summary
    d, n = 4, 100
    X = np.zeros((n, d))
    X[:90, 0] = np.where(np.arange(90) % 2 == 0, 1.0, -1.0)                  # variance 0.9 along e0, 0.1 along e1, mean 0
    X[90:, 1] = np.where(np.arange(10) % 2 == 0, 1.0, -1.0)
    erank, top1, rank99, centre = spectrum_summary(X.T @ X, X.sum(0), n)
    p = np.asarray([0.9, 0.1])
    assert abs(erank - np.exp(-(p * np.log(p)).sum())) < 1e-12 and abs(top1 - 0.9) < 1e-12 and rank99 == 2.0 and centre == 0.0


# --------------------------------------------------------------------------- the numpy model, by hand
def test_the_model_by_hand():
    T = np.asarray([[1, 0, 0, 0], [-2, 0, 0, 0], [0, 3, 0, 0], [0, 0, 0, 0]], dtype=np.float32)
    sq = gm.sqnorms(T)
    t = 2.0
    S, pairs, n, uni = gm.uniformity_model(T, sq, [0, 1], t)
    assert (pairs, n) == (1, 2) and abs(uni + 4 * t) < 1e-12                 # antipodal: cos = -1
    S, pairs, n, uni = gm.uniformity_model(T, sq, [0, 0, 3, -1, 9], t)      # a repeated id is a pair; no norm / -1 / past the table: skipped
    assert (pairs, n) == (1, 2) and abs(uni) < 1e-12
    S, pairs, n, uni = gm.uniformity_model(T, sq, [0, 1, 2], 0.5)
    assert (pairs, n) == (3, 3) and abs(S - (np.exp(-2.0) + 2 * np.exp(-1.0))) < 1e-12
    assert np.isnan(gm.uniformity_model(T, sq, [2], t)[3]) and gm.uniformity_model(T, sq, [], t)[1:3] == (0, 0)
    G, m, n, A, a = gm.gram_model(T, sq, [0, 1, 2, 3, 7])
    assert n == 3 and np.array_equal(G, np.diag([2.0, 1.0, 0, 0])) and np.array_equal(m, [0, 1.0, 0, 0]) and np.array_equal(A, G)
    al = gm.alignment_model(T, sq, T, sq, [0, 0, 0, 3], [0, 1, 2, 0])
    assert np.allclose(al, [0.0, 4.0, 2.0, 2.0], atol=1e-12)                 # a row without a norm: cosine 0


# --------------------------------------------------------------------------- the cell grid of uniformity_sum
def _grid_sizes():
    from elimrec_amd import ops
    TILE, CHUNK = ops.GEOMETRY_TILE, ops.GEOMETRY_CHUNK
    return TILE, CHUNK, [0, 1, TILE, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 3 * CHUNK + TILE + 1]


def test_live_cells_are_the_cells_that_hold_a_pair():
    """gm.live_cells against brute force over the positions: every (tile, chunk) that holds a pair p < q appears exactly once, in
    tile-major order. The definition (tile i meets the chunks c >= i * TILE // CHUNK) lists ONE cell brute force does not find, and
    only when n % TILE == 1: the diagonal cell of a last tile of a single position, which has no q behind its p. It is launched
    (and sized in the workspace) all the same and must add 0; no other cell without a pair may appear."""
    TILE, CHUNK, sizes = _grid_sizes()
    for n in sizes:
        cells = gm.live_cells(n, TILE, CHUNK)
        assert cells == sorted(set(cells))                                   # each once, tile-major
        idle = {((n - 1) // TILE, (n - 1) // CHUNK)} if n % TILE == 1 else set()
        assert set(cells) - gm.cells_with_a_pair(n, TILE, CHUNK) == idle and gm.cells_with_a_pair(n, TILE, CHUNK) <= set(cells)
    n = sizes[-1]                                                            # the size the device tests use
    cells = gm.live_cells(n, TILE, CHUNK)
    assert len(cells) == 290 and n == 6209 and cells[-2:] == [(96, 3), (97, 3)] and cells[256] == (80, 2)
    small = gm.live_cells(7, 2, 4)                                           # by hand: tiles of 2, chunks of 4
    assert small == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 1), (3, 1)] and gm.cells_with_a_pair(7, 2, 4) == set(small) - {(3, 1)}


def test_uniformity_workspace_is_one_float64_per_live_cell():
    """8 bytes per cell of gm.live_cells, rounded up to 16; an empty list keeps room for one cell (16 bytes)."""
    from elimrec_amd import ops
    TILE, CHUNK, sizes = _grid_sizes()
    for n in sizes:
        cells = max(1, len(gm.live_cells(n, TILE, CHUNK)))
        for d in (4, 64, 128):
            assert ops.uniformity_workspace(n, d) == (8 * cells + 15) // 16 * 16, (n, d)


def test_the_cell_sums_of_the_model_add_up():
    T = np.random.default_rng(0).standard_normal((150, 8)).astype(np.float32)
    sq = gm.sqnorms(T)
    rows = np.random.default_rng(1).permutation(150)[:139]
    S, pairs, n, uni = gm.uniformity_model(T, sq, rows, 2.0)
    S2, pairs2, n2, uni2, cells = gm.uniformity_model(T, sq, rows, 2.0, cells=(16, 64))
    assert (S2, pairs2, n2, uni2) == (S, pairs, n, uni) and len(cells) == len(gm.live_cells(139, 16, 64)) == 4 * 3 + 4 * 2 + 1
    assert abs(sum(cells) - S) <= 1e-12 * S and cells[-1] > 0
    X = gm.unit_rows(T, sq, rows).astype(np.float64)                         # cell (tile 5, chunk 2) by its definition
    want = sum(np.exp(4.0 * (X[p] @ X[q] - 1.0)) for p in range(80, 96) for q in range(128, 139))
    assert abs(cells[gm.live_cells(139, 16, 64).index((5, 2))] - want) <= 1e-12 * want


# --------------------------------------------------------------------------- argument errors before the device is needed
def test_the_temperature_just_past_the_limit_is_refused():
    from elimrec_amd import ops
    T, sq, rows = torch.zeros(8, 4), torch.zeros(8), torch.zeros(3, dtype=torch.int32)
    for bad in (8.0000001, float(np.nextafter(8.0, 9.0)), np.float64(8.0000001), float("inf")):
        with pytest.raises(ValueError, match="0 < t <= 8"):
            ops.uniformity_sum(T, sq, rows, t=bad)
    with pytest.raises(RuntimeError, match="HIP device tensor"):             # t = 8 passes the check; the tensors are refused next
        ops.uniformity_sum(T, sq, rows, t=8.0)


def test_ops_argument_errors_fire_without_a_gpu():
    from elimrec_amd import ops
    T, sq, rows = torch.zeros(8, 4), torch.zeros(8), torch.zeros(3, dtype=torch.int32)
    for bad in (0, -1.0, 8.5, float("nan"), True, "2"):
        with pytest.raises(ValueError, match="0 < t <= 8"):
            ops.uniformity_sum(T, sq, rows, t=bad)
    with pytest.raises(RuntimeError, match="HIP device tensor"):             # no CPU path
        ops.uniformity_sum(T, sq, rows)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        ops.row_gram(T, sq, rows)
    assert ops.GEOMETRY_MAX_T == 8.0
    assert np.isnan(ops.uniformity_value(0.0, 0)) and ops.uniformity_value(np.e, 1) == 1.0
    # the workspace queries are host arithmetic
    TILE, CHUNK, SEG = ops.GEOMETRY_TILE, ops.GEOMETRY_CHUNK, ops.GEOMETRY_SEGMENT
    assert CHUNK % TILE == 0 and TILE % 16 == 0 and SEG >= 64
    assert ops.uniformity_workspace(TILE, 64) == 16 and ops.uniformity_workspace(CHUNK + 1, 4) == (2 * (CHUNK // TILE) + 1) * 8 + 8
    assert ops.uniformity_workspace(10, 6) == 0 and ops.uniformity_workspace(-1, 64) == 0 and ops.uniformity_workspace(10, 260) == 0
    assert ops.row_gram_workspace(SEG + 1, 8) == 2 * (8 * 8 + 8) * 8 + 16 and ops.row_gram_workspace(10, 2) == 0


def test_model_argument_errors_fire_without_a_gpu():
    g = load_golden("ml3")
    model, _ = build_model_from_fixture(g, "cpu")
    for call in (model.embedding_geometry, lambda **kw: model.geometry_device(kw.pop("side", "item"), **kw)):
        with pytest.raises(ValueError, match="side must be"):
            call(side="items")
        with pytest.raises(ValueError, match="space must be"):
            call(space="x")
        with pytest.raises(ValueError, match="0 < t <= 8"):
            call(t=0.0)
        with pytest.raises(ValueError, match="0 < t <= 8"):
            call(t=9)
        with pytest.raises(IndexError):
            call(rows=[0, model.num_items])
        with pytest.raises(IndexError):
            call(rows=[-1])
        with pytest.raises(IndexError):
            call(side="user", rows=[model.num_users])
    with pytest.raises(ValueError, match="space must be"):
        model.alignment([0], [0], space="x")
    with pytest.raises(IndexError):
        model.alignment([model.num_users], [0])
    with pytest.raises(IndexError):
        model.alignment([0], [-1])
    with pytest.raises(ValueError, match="one item per user"):
        model.alignment([0, 1], [0])
    with pytest.raises(RuntimeError):                                        # a CPU model: no tables to read
        model.embedding_geometry()


def test_report_arguments_and_the_switch():
    from elimrec_amd.evaluator import GEOMETRY_COLUMNS, GeometryReport
    assert GEOMETRY_COLUMNS == ("n", "uniformity", "erank", "top1", "rank99", "centre")
    g = load_golden("ml3")
    model, _ = build_model_from_fixture(g, "cpu")
    assert model.geometry_reporter is None
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--geometry_report=0", "--geometry_t=99"])
    assert model.geometry_reporter is None
    train, test = model.dataset.get_user_train_dict(), model.dataset.get_user_test_dict()
    with pytest.raises(TypeError):
        GeometryReport(model.dataset, [], test)
    for bad in (0, 8.5, -2.0, "x"):
        with pytest.raises(ValueError, match="0 < t <= 8"):
            GeometryReport(model.dataset, train, test, t=bad)
    with pytest.raises(ValueError):
        GeometryReport(model.dataset, train, test, group_view=[3, 1])
    with pytest.raises(ValueError):
        GeometryReport(model.dataset, train, test, item_group_view=[0])
    with pytest.raises(IndexError):
        GeometryReport(model.dataset, train, {0: [model.num_items]})
    for bad in (["--geometry_report=2"], ["--geometry_report=1", "--geometry_t=0"], ["--geometry_report=1", "--geometry_t=8.5"]):
        with pytest.raises(ValueError):
            build_model_from_fixture(g, "cpu", extra_argv=bad)
    model, _ = build_model_from_fixture(g, "cpu", extra_argv=["--geometry_report=1", "--geometry_t=0.5", "--group_view=[1,3,5]",
                                                              "--item_group_view=[1,4]"])
    rep = model.geometry_reporter
    assert isinstance(rep, GeometryReport) and rep.t == 0.5 and rep.num_items == model.num_items
    assert [x[0] for x in rep.row_sets[:2]] == ["user", "item"] and all(x[0].startswith(("user (", "item ")) for x in rep.row_sets[2:])
    assert rep.align_columns[0] == "all:".ljust(12) and any(c.startswith("item ") for c in rep.align_columns)
    n_train = sum(len(v) for v in train.values())
    assert rep._pairs["align_train"][0].size == n_train and rep._pairs["align_test"][0].size == sum(len(v) for v in test.values())
    with pytest.raises(RuntimeError):                                        # a CPU model
        rep.evaluate(model)
    import main
    src = inspect.getsource(main.Net.__init__)
    assert "--geometry_report needs the whole cached tables on one rank: it is single-GPU" in src


def test_geometry_entries_are_declared_bound_and_registered():
    from elimrec_amd import _lib, ops, torch_ops
    header = open(os.path.join(ROOT, "include", "elimrec_hip.h")).read()
    for name in ("elimrec_uniformity_sum", "elimrec_gram_f64", "elimrec_uniformity_workspace", "elimrec_gram_workspace",
                 "elimrec_geometry_tile", "elimrec_geometry_chunk", "elimrec_geometry_segment"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name) and name + "(" in header
    for name in ("uniformity_sum", "row_gram"):
        assert hasattr(torch_ops.load(), name) and name in torch_ops.OPS
    assert (ops.GEOMETRY_TILE, ops.GEOMETRY_SEGMENT) == (64, 512) and ops.GEOMETRY_CHUNK == 2048
    assert "geometry.hip" in open(os.path.join(ROOT, "elimrec_amd", "csrc", "Makefile")).read()
