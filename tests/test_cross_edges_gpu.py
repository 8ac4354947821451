"""ops.cross_topk / elimrec_cross_topk (csrc/knn.hip with a query table of its own) at its edges, against the kernel's own
expression in np.float32 (knn_model.cross_lists32). The cases are tests/cross_cases.py's; tests/test_cross_cases_cpu.py shows
that each reaches what it is named for.

The model. Tables of small integers (|entry| <= 8, d <= 256) make every fp32 dot product exact in any order, and the score is
(dot * invq) * invc with inv = 1 / max(sqrt(sq), 1e-12f). csrc/Makefile builds with -O3 -ffp-contract=off -fno-slp-vectorize and
nothing that relaxes floating point (no -ffast-math, no -fno-hip-fp32-correctly-rounded-divide-sqrt, no denormal flush), so hipcc's
default holds: sqrtf and the division of cosine.h::inv_norm are correctly rounded (the kernel's code shows v_sqrt_f32 with its
one-ulp correction and the v_div_scale / v_div_fmas / v_div_fixup division). Hence the model predicts ids AND value bits for
arbitrary positive squared norms, and every comparison below is bit for bit: no case fell back to a tolerance. The squared norms
handed in are not the rows' own, and differ between the sides.

Every output is pre-filled with a sentinel and three rows longer than [Q x K]; the rows behind keep the sentinel (_run).

Non-finite scores. The matrix instruction runs a k-ordered fmaf chain whose products are not rounded, so finite rows cannot give
a NaN dot product: +inf plus a finite product stays +inf (knn_model.fma_chain_dot32; np.float32 multiplies and adds give NaN
for the same row, which the host test records). The NaN score comes from a candidate whose squared norm is +inf (inf * 0).

Mutations: each of these value-only changes of knn.hip was built apart, outside the tree, and run once against this file; all of
their reads stay inside the tests' allocations (_place: the wide tensors are sized for the longer side and the larger stride).
  (a) query rows read with a.ld for a.ldq: test_two_geometries_at_once, all 8 cases (nowhere else do the two strides differ).
  (b) the query-id guard takes a.n_rows for a.nq_rows: test_two_geometries_at_once[517-300-*] (the ids in [n_rows, nq_rows) turn
      into fillers), test_candidate_edges_around_a_stage (all three: 9 query rows against fewer candidates) and
      test_ids_outside_through_the_c_entry_point (the id in [nq_rows, n_rows) gets a list).
  (c) invq read with a.ld_sq for a.ld_sqq: test_two_geometries_at_once, all 8 cases.
  (d) invq taken from a.sq for a.sqq: 44 of the 69 tests -- every one with norms given on either side: test_two_geometries_at_once,
      test_the_four_norm_combinations but [False-False], test_d_ladder, both test_candidate_edges_*, test_partition_independence,
      test_ids_outside_through_the_c_entry_point, test_dirty_workspace_and_optional_output, test_cross_query_reuse.
  (e) the score formed as (acc * invc) * invq: 36 tests -- every bit-exact one with arbitrary norms on BOTH sides:
      test_two_geometries_at_once, test_the_four_norm_combinations[True-True], test_d_ladder, both test_candidate_edges_*,
      test_ids_outside_through_the_c_entry_point. (test_partition_independence compares runs with each other and rightly passes.)

Time: the whole file, 69 tests, took 3.7 s in pytest and 5.6 s of wall time with the interpreter's start on an MI355X; the slowest
test is test_two_geometries_at_once[517-300-True-10] at 0.75 s (the first call, which loads the library), then test_exclusions at
0.27 s (the linear scans of lists longer than a chunk); every other test is under 0.05 s."""
import numpy as np
import pytest
import torch

import cross_cases as cc
import knn_model as km

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDX_FILL, VAL_FILL = -7, 7.0


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _filled(shape, value=float("nan")):
    return torch.full(shape, value, dtype=torch.float32, device=DEV)


def _column(values, rows, ld, fill=float("nan")):
    """values as column 1 of a `fill`-filled [rows x ld] tensor (ld = 1: the head of a longer vector)."""
    wide = _filled((rows, ld), fill)
    view = wide[:len(values), 1 if ld > 1 else 0]
    view.copy_(_t(values))
    return view


def _place(case):
    """The case on the device: (Tq, sqq, T, sq). With a Geom each table is a block of a NaN-filled matrix of max(nq, n) + 4 rows and
    the norms are columns of NaN-filled tensors of twice as many rows; without one the tables are contiguous and the given norms
    are the heads of NaN-tailed vectors as long. So a row count, a stride or a norm pointer taken from the other side reads a NaN
    or another row's number, inside the allocation: the largest such index is (max(nq, n) - 1) * 3 + 1 < 2 (max(nq, n) + 4) * 2 for
    the norms and (nq - 1) * ld + 3 + d < (max(nq, n) + 4) * ldq for the query rows (cross_cases.Geom: ld < ldq)."""
    (nq, d), n, g = case.Tq.shape, case.T.shape[0], case.geom
    R = max(nq, n) + 4
    if g is None:
        Tq, T = _t(case.Tq), _t(case.T)
        sqq = None if case.sqq is None else _column(case.sqq, 2 * R, 1)
        sq = None if case.sq is None else _column(case.sq, 2 * R, 1)
        return Tq, sqq, T, sq
    assert g.q_off[1] + d <= g.ldq and g.t_off[1] + d <= g.ld and g.q_off[0] + nq <= R and g.t_off[0] + n <= R
    Tq = _filled((R, g.ldq))[g.q_off[0]:g.q_off[0] + nq, g.q_off[1]:g.q_off[1] + d]
    T = _filled((R, g.ld))[g.t_off[0]:g.t_off[0] + n, g.t_off[1]:g.t_off[1] + d]
    Tq.copy_(_t(case.Tq))
    T.copy_(_t(case.T))
    return Tq, _column(case.sqq, 2 * R, g.ld_sqq), T, _column(case.sq, 2 * R, g.ld_sq)


def _outputs(Q, K):
    idx = torch.full((Q + 3, K), IDX_FILL, dtype=torch.int32, device=DEV)
    val = torch.full((Q + 3, K), VAL_FILL, dtype=torch.float32, device=DEV)
    return idx, val


def _taken(idx, val, Q):
    """The lists as host arrays, once the rows behind [Q x K] are seen to keep their sentinels."""
    torch.cuda.synchronize()
    assert bool((idx[Q:] == IDX_FILL).all()) and (val is None or bool((val[Q:] == VAL_FILL).all()))
    return idx[:Q].cpu().numpy(), None if val is None else val[:Q].cpu().numpy()


def _run(dev, rows, K, excl=None, **kw):
    """ops.cross_topk on placed tensors; rows: host ids or a CrossQuery."""
    from elimrec_amd import ops
    Q = rows.n_queries if isinstance(rows, ops.CrossQuery) else len(rows)
    idx, val = _outputs(Q, K)
    ptr, flat = km.csr(excl) if excl is not None else (None, None)
    if not isinstance(rows, ops.CrossQuery):
        rows = np.asarray(rows, dtype=np.int32)
    ops.cross_topk(dev[0], dev[1], dev[2], dev[3], rows, K, idx, val, excl_ptr=ptr, excl_rows=flat, **kw)
    return _taken(idx, val, Q)


def _same(got, want, what=None):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(np.asarray(got[1], dtype=np.float32).view(np.int32), np.asarray(want[1], dtype=np.float32).view(np.int32)), what


def _model(case):
    return km.cross_lists32(case.Tq, case.sqq, case.T, case.sq, case.rows, case.K, case.excl, case.chain)


def _check(case):
    got = _run(_place(case), case.rows, case.K, case.excl)
    _same(got, _model(case))
    return got


@pytest.mark.parametrize("nq,n,aligned,K", cc.GEOMETRY)
def test_two_geometries_at_once(nq, n, aligned, K):
    case = cc.case(cc.geometry, nq, n, aligned, K)
    dev = _place(case)
    assert dev[0].stride(0) != dev[2].stride(0) and dev[1].stride(0) == 3 and dev[3].stride(0) == 2
    assert dev[0].data_ptr() % 16 != 0 and (dev[2].data_ptr() % 16 == 0 and dev[2].stride(0) % 4 == 0) == aligned == (dev[2].data_ptr() % 16 == 0)
    _same(_run(dev, case.rows, case.K, case.excl), _model(case))


@pytest.mark.parametrize("q_given,c_given", cc.NORMS)
def test_the_four_norm_combinations(q_given, c_given):
    _check(cc.case(cc.norm_combination, q_given, c_given))


@pytest.mark.parametrize("d,K", cc.LADDER)
def test_d_ladder(d, K):
    _check(cc.case(cc.ladder, d, K))


@pytest.mark.parametrize("Q,K", cc.QUERY_TILES)
def test_query_tile_edges(Q, K):
    case = cc.case(cc.query_tiles, Q, K)
    ids, vals = _check(case)
    _same((ids[Q - 1], vals[Q - 1]), (ids[0], vals[0]))
    if Q > 9:
        _same((ids[9], vals[9]), (ids[2], vals[2]))


@pytest.mark.parametrize("d,stage", cc.STAGE_D)
def test_candidate_edges_around_a_stage(d, stage):
    for n in cc.SMALL_N:
        ids, _ = _check(cc.case(cc.candidates, n, d))
        assert ((ids >= 0).sum(1) == min(n, 10)).all(), n


def test_candidate_edges_around_a_chunk():
    for n, d in cc.candidate_edges():
        if n > 100:
            _check(cc.case(cc.candidates, n, d))


@pytest.mark.parametrize("K,with_excl", cc.SCORE_RANGE)
def test_score_range(K, with_excl):
    case = cc.case(cc.score_range, K, with_excl)
    got = _check(case)
    _same(got, cc.score_range_closed_form(K, with_excl))


@pytest.mark.parametrize("d,K", cc.PARTITION)
def test_partition_independence(d, K):
    """A (query, row) pair's value bits do not depend on the table around the row, on the chunk and stage it is met in, or on the
    query's place in the grid. Random float tables; the values are also held to the float64 score within knn_model.tol(d) times the
    two rows' norms and reciprocal norms handed in (the fp32 dot product's worst case, scaled like the score)."""
    small, big = cc.case(cc.partition, d, K)
    m = min(K, cc.PART_ROWS)
    ids_s, vals_s = _run(_place(small), small.rows, K)
    ids_b, vals_b = _run(_place(big), big.rows, K)
    assert (ids_s[:, :m] >= 0).all() and (ids_s[:, m:] == -1).all()
    _same((ids_b[:, :m] - cc.PART_FILL, vals_b[:, :m]), (ids_s[:, :m], vals_s[:, :m]))
    assert (ids_b[:, m:] < cc.PART_FILL).all() and (ids_b[:, m:] >= 0).all()
    alone = _run(_place(small), small.rows[:1], K)
    for at in (0, 37, 64):
        _same((ids_s[at:at + 1], vals_s[at:at + 1]), alone, at)
    q64, c64 = small.Tq.astype(np.float64)[small.rows], small.T.astype(np.float64)
    scale = 1.0 / np.sqrt(small.sqq.astype(np.float64))[small.rows][:, None] / np.sqrt(small.sq.astype(np.float64))[None, :]
    s = (q64 @ c64.T) * scale
    bound = km.tol(d) * np.sqrt((q64 ** 2).sum(1))[:, None] * np.sqrt((c64 ** 2).sum(1))[None, :] * scale
    take = np.arange(len(small.rows))[:, None], ids_s[:, :m]
    assert (np.abs(vals_s[:, :m].astype(np.float64) - s[take]) <= bound[take]).all()
    assert (np.diff(vals_s[:, :m], axis=1) <= 0).all()


def _call_c(dev, nq, rows, K, excl=None):
    """elimrec_cross_topk itself: no host check stands between the ids and the kernel. dev: contiguous (Tq, sqq, T, sq)."""
    from elimrec_amd import _lib, ops
    lib = _lib.load()
    Tq, sqq, T, sq = dev
    n, d = T.shape
    Q = len(rows)
    rows_t = _t(np.asarray(rows, dtype=np.int64).astype(np.int32))
    idx, val = _outputs(Q, K)
    ws = torch.empty(int(lib.elimrec_cross_topk_workspace(Q, n, K)), dtype=torch.uint8, device=DEV)
    ptr_t = flat_t = None
    if excl is not None:
        ptr, flat = km.csr(excl)
        ptr_t, flat_t = _t(ptr), _t(flat if flat.size else np.zeros(1, dtype=np.int32))
    rc = lib.elimrec_cross_topk(Tq.data_ptr(), Tq.stride(0), nq, sqq.data_ptr(), sqq.stride(0), T.data_ptr(), T.stride(0), n, d, sq.data_ptr(),
                                sq.stride(0), rows_t.data_ptr(), Q, None if ptr_t is None else ptr_t.data_ptr(),
                                None if flat_t is None else flat_t.data_ptr(), K, idx.data_ptr(), val.data_ptr(), ws.data_ptr(), ws.numel(),
                                ops._stream())
    _lib.check(rc, "cross_topk")
    return _taken(idx, val, Q)


def test_ids_outside_through_the_c_entry_point():
    """The kernel's own guards (knn.hip: a query id < 0 or >= nq_rows is no query; the exclusion scan compares ids and indexes
    nothing with them). The query table and its norms are the heads of allocations as long as the candidate side's, finite behind
    nq: a guard that took n_rows for nq_rows would list candidates for the id in [nq_rows, n_rows)."""
    case, bad_queries, bad_excl = cc.outside_ids()
    (nq, d), n, K = case.Tq.shape, case.T.shape[0], case.K
    Tq = _filled((n + 4, d), 1.0)[:nq]
    Tq.copy_(_t(case.Tq))
    dev = (Tq, _column(case.sqq, n + 4, 1, 1.0), _t(case.T), _t(case.sq))
    want = _model(case)
    base = _call_c(dev, nq, case.rows, K)
    _same(base, want)
    for bad in bad_queries:
        for at in (5, 34):                                                    # inside a full 16-row group, and in the last, partial one
            rows = case.rows.copy()
            rows[at] = bad
            ids, vals = _call_c(dev, nq, rows, K)
            assert (ids[at] == -1).all() and np.isneginf(vals[at]).all(), (bad, at)
            keep = np.arange(len(rows)) != at
            _same((ids[keep], vals[keep]), (base[0][keep], base[1][keep]), (bad, at))
    every = _call_c(dev, nq, np.asarray(bad_queries), K)
    assert (every[0] == -1).all() and np.isneginf(every[1]).all()
    excl = [bad_excl if b % 2 == 0 else bad_excl[b % 5:] + bad_excl for b in range(len(case.rows))]
    _same(_call_c(dev, nq, case.rows, K, excl), base)
    mixed = [bad_excl[:2] + [int(want[0][b, 0])] + bad_excl[2:] for b in range(len(case.rows))]
    _same(_call_c(dev, nq, case.rows, K, mixed), km.cross_lists32(case.Tq, case.sqq, case.T, case.sq, case.rows, K, mixed))


@pytest.mark.parametrize("K", cc.EXCLUSIONS)
def test_exclusions(K):
    case = cc.case(cc.exclusions, K)
    ids, vals = _check(case)
    assert (ids[1] == -1).all() and np.isneginf(vals[1]).all() and (ids[2] < cc.chunk()).all()
    assert (ids[3] >= 0).sum() == K - 1 and (ids[4] >= 0).all() and (ids[5] >= 0).all()


@pytest.mark.parametrize("K", cc.NONFINITE)
def test_nonfinite_scores(K):
    """+inf ranks first, ties by id; -inf and NaN are no candidates (the kernel keeps what is > its threshold)."""
    case = cc.case(cc.nonfinite, K)
    ids, vals = _check(case)
    assert ids[0, :3].tolist() == [cc.NF_PLUS, cc.NF_CANCEL, cc.NF_PLUS2] and np.isposinf(vals[0, :3]).all()
    listed = ids[0][ids[0] >= 0]
    assert cc.NF_MINUS not in listed and cc.NF_ZERO_INV not in listed and np.isfinite(vals[0, 3:listed.size]).all()
    assert not np.isnan(vals).any() and np.isneginf(vals[ids < 0]).all()


def test_dirty_workspace_and_optional_output():
    from elimrec_amd import ops
    case = cc.plain()
    dev, Q, K = _place(case), len(case.rows), case.K
    want = _model(case)
    fresh = _run(dev, case.rows, K, case.excl)
    _same(fresh, want)
    need = ops.cosine_topk_workspace(Q, case.T.shape[0], K)
    ws = torch.full((need + 4096,), 0xFF, dtype=torch.uint8, device=DEV)
    _same(_run(dev, case.rows, K, case.excl, workspace=ws), want)
    ws.copy_(torch.randint(0, 256, (need + 4096,), dtype=torch.uint8, device=DEV, generator=torch.Generator(DEV).manual_seed(3)))
    _same(_run(dev, case.rows, K, case.excl, workspace=ws), want)
    # no value output
    idx, _ = _outputs(Q, K)
    ptr, flat = km.csr(case.excl)
    ops.cross_topk(dev[0], dev[1], dev[2], dev[3], case.rows.astype(np.int32), K, idx, None, excl_ptr=ptr, excl_rows=flat, workspace=ws)
    assert np.array_equal(_taken(idx, None, Q)[0], want[0])
    # Q = 0: nothing is launched, nothing is written
    idx, val = _outputs(0, K)
    ops.cross_topk(dev[0], dev[1], dev[2], dev[3], np.zeros(0, dtype=np.int32), K, idx, val)
    _taken(idx, val, 0)
    # an empty candidate table: every list is fillers, with and without the value output
    empty = (dev[0], dev[1], torch.empty((0, case.T.shape[1]), dtype=torch.float32, device=DEV), None)
    ids, vals = _run(empty, case.rows, K)
    assert (ids == -1).all() and np.isneginf(vals).all()
    idx, _ = _outputs(Q, K)
    ops.cross_topk(empty[0], empty[1], empty[2], None, case.rows.astype(np.int32), K, idx, None)
    assert (_taken(idx, None, Q)[0] == -1).all()


def test_cross_query_reuse():
    from elimrec_amd import ops
    case = cc.plain()
    dev = _place(case)
    (nq, _), n = case.Tq.shape, case.T.shape[0]
    ptr, flat = km.csr(case.excl)
    query = ops.CrossQuery(case.rows, nq, n, DEV, ptr, flat)
    for K in (5, 64, 100):
        want = km.cross_lists32(case.Tq, case.sqq, case.T, case.sq, case.rows, K, case.excl)
        _same(_run(dev, query, K), want, K)
        _same(_run(dev, case.rows, K, case.excl), want, K)
    idx, val = _outputs(len(case.rows), 5)
    with pytest.raises(IndexError):
        ops.cross_topk(dev[0][:nq - 1], dev[1][:nq - 1], dev[2], dev[3], query, 5, idx, val)
    with pytest.raises(IndexError):
        ops.cross_topk(dev[0], dev[1], dev[2][:n - 1], None, query, 5, idx, val)
    _taken(idx, val, 0)                                                       # the refusals wrote nothing
