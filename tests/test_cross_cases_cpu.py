"""The inputs of tests/test_cross_edges_gpu.py (no GPU): conditions on the cases of tests/cross_cases.py and on the float32 model
of tests/knn_model.py, not on the kernel -- each case reaches what it is named for."""
import numpy as np

import cross_cases as cc
import knn_model as km


def _lists(case):
    return km.cross_lists32(case.Tq, case.sqq, case.T, case.sq, case.rows, case.K, case.excl, case.chain)


def test_the_model_by_hand():
    """Two query rows, three candidates, d = 4. dots: q0 = (1, 2, 0, 0) -> 4, 0, -2; q1 = (0, 0, 3, 0) -> 0, 3, 3.
    Norms 4 and 16 on the query side (inv 1/2, 1/4), 1, 4, 0 on the other (inv 1, 1/2, 1e12)."""
    Tq = np.asarray([[1, 2, 0, 0], [0, 0, 3, 0]], dtype=np.float32)
    T = np.asarray([[2, 1, 0, 0], [0, 0, 1, 5], [0, -1, 1, 0]], dtype=np.float32)
    sqq, sq = np.asarray([4, 16], dtype=np.float32), np.asarray([1, 4, 0], dtype=np.float32)
    assert km.inv_norm32(sq, 3).tolist() == [1.0, 0.5, float(np.float32(1.0) / np.float32(1e-12))] and km.inv_norm32(None, 2).tolist() == [1.0, 1.0]
    assert km.inv_norm32(np.asarray([1e-30, np.inf], dtype=np.float32), 2).tolist() == [float(np.float32(1.0) / np.float32(1e-12)), 0.0]
    e12 = np.float32(1.0) / np.float32(1e-12)
    s = km.cross_scores32(Tq, sqq, T, sq, [0, 1])
    assert s.dtype == np.float32 and s.tolist() == [[2.0, 0.0, float(np.float32(-1.0) * e12)], [0.0, 0.375, float(np.float32(0.75) * e12)]]
    assert km.cross_scores32(Tq, None, T, None, [1, 0]).tolist() == [[0.0, 3.0, 3.0], [4.0, 0.0, -2.0]]
    assert np.array_equal(km.cross_scores32(Tq, sqq, T, sq, [0, 1], chain=True), s)
    ids, vals = km.cross_lists32(Tq, None, T, None, [1, 0, 2, -1, 1], 2, [[], [0, 7, -3], [], [], [1]])
    assert ids.tolist() == [[1, 2], [1, 2], [-1, -1], [-1, -1], [2, 0]] and vals.dtype == np.float32
    assert vals[:2].tolist() == [[3.0, 3.0], [0.0, -2.0]] and np.isneginf(vals[2:4]).all() and vals[4].tolist() == [3.0, 0.0]
    # the swap of the two sides' norms is another number
    assert not np.array_equal(km.cross_scores32(Tq, sqq, T, sq, [0, 1]), km.cross_scores32(Tq, sq[:2], T, np.asarray([4, 16, 1], np.float32), [0, 1]))


def test_the_case_lists_are_the_issues():
    C = cc.chunk()
    assert sorted({d for d, _ in cc.LADDER}) == [4, 8, 20, 32, 36, 64, 68, 128, 132, 252, 256]
    assert {K for _, K in cc.LADDER} == {64, 65} and len(cc.LADDER) == 22
    for d, K in cc.LADDER:
        case = cc.case(cc.ladder, d, K)
        assert case.rows.size == 17 and case.T.shape == (C + 1, d) and case.K == K and case.Tq.shape[1] == d
    assert sorted(Q for Q, K in cc.QUERY_TILES if K <= 64) == [1, 15, 16, 17, 63, 64, 65, 129]
    assert sorted(Q for Q, K in cc.QUERY_TILES if K > 64) == [15, 16, 17, 33] and {K for _, K in cc.QUERY_TILES} == {10, 65}
    for Q, K in cc.QUERY_TILES:
        rows, tile = cc.case(cc.query_tiles, Q, K).rows, 64 if K <= 64 else 16
        assert rows.size == Q and rows[Q - 1] == rows[0] and (Q < 10 or rows[9] == rows[2])
        assert ((Q - 1) // tile > 0) == (Q > tile)                            # the repeat sits in another workgroup past one tile
    edges = cc.candidate_edges()
    for d, _ in cc.STAGE_D:
        assert sorted(n for n, dd in edges if dd == d and n < 100) == [1, 15, 16, 17, 31, 32, 33, 63, 64, 65]
    assert sorted(n for n, d in edges if n > 100) == [C - 1, C, C + 1, 3 * C + 5] and {d for n, d in edges if n > 100} == {64}
    assert [d for d, _ in cc.STAGE_D] == [64, 128, 20] and all(cc.case(cc.candidates, n, d).K <= 64 for n, d in edges)
    assert sorted({K for K, _ in cc.SCORE_RANGE}) == [1, 64, 65, 256] and {e for _, e in cc.SCORE_RANGE} == {False, True}
    assert len(cc.SCORE_RANGE) == 8 and {K for *_, K in cc.GEOMETRY} == {10, 65} and cc.NORMS == [(False, False), (True, False), (False, True), (True, True)]
    # every table: small integers unless the case says otherwise, n <= 3 C + 5, d % 4 == 0
    built = [cc.case(cc.geometry, *a) for a in cc.GEOMETRY] + [cc.case(cc.norm_combination, *a) for a in cc.NORMS]
    built += [cc.case(cc.ladder, *a) for a in cc.LADDER] + [cc.case(cc.query_tiles, *a) for a in cc.QUERY_TILES]
    built += [cc.case(cc.candidates, *a) for a in edges] + [cc.case(cc.exclusions, K) for K in cc.EXCLUSIONS] + [cc.outside_ids()[0], cc.plain()]
    for case in built:
        assert np.abs(case.Tq).max() <= 8 and np.abs(case.T).max() <= 8 and (case.Tq == np.rint(case.Tq)).all() and (case.T == np.rint(case.T)).all()
    built += [cc.case(cc.score_range, *a) for a in cc.SCORE_RANGE] + [c for a in cc.PARTITION for c in cc.case(cc.partition, *a)]
    built += [cc.case(cc.nonfinite, K) for K in cc.NONFINITE]
    for case in built:
        n, d = case.T.shape
        assert n <= 3 * C + 5 and d % 4 == 0 and 4 <= d <= 256 and case.Tq.shape[1] == d and 1 <= case.K <= 256
        assert case.sqq is None or (case.sqq.shape == (case.Tq.shape[0],) and case.sqq.dtype == np.float32)
        assert case.sq is None or (case.sq.shape == (n,) and case.sq.dtype == np.float32)
        assert case.rows.min() >= 0 and case.rows.max() < case.Tq.shape[0] and (case.excl is None or len(case.excl) == case.rows.size)
        # a side without norms next to a longer query table would let a mixed-up side read past a vector of n ones
        assert case.geom is not None or (case.sqq is not None and case.sq is not None) or case.Tq.shape[0] <= n


def test_geometry_cases_separate_the_two_sides():
    C = cc.chunk()
    seen = set()
    for nq, n_, aligned, K in cc.GEOMETRY:
        case = cc.case(cc.geometry, nq, n_, aligned, K)
        g, (n, d) = case.geom, case.T.shape
        seen.add((nq > n, aligned))
        assert g.ldq != d and g.ldq != g.ld and g.ld != d and g.q_off[0] % 2 == 1 and g.q_off[1] == 3
        assert (g.q_off[0] * g.ldq + g.q_off[1]) % 4 != 0                     # the query base is not 16-byte aligned
        assert ((g.t_off[0] * g.ld + g.t_off[1]) % 4 == 0 and g.ld % 4 == 0) == aligned
        assert g.ld_sqq > 1 and g.ld_sq > 1 and g.ld_sqq != g.ld_sq and g.ld < g.ldq and g.ld_sq < g.ld_sqq
        ids, _ = _lists(case)
        if nq > n:
            assert ((case.rows >= n) & (case.rows < nq)).sum() >= 2 and (ids[case.rows >= n] >= 0).all()
        else:
            assert n == C + 9 and (ids >= nq).any() and (ids >= C).any()      # candidates the query table has no row for, both chunks
        assert not np.array_equal(case.sqq[:20], case.sq[:20])
    assert seen == {(True, True), (True, False), (False, True), (False, False)}


def test_norm_cases_reach_the_floor_and_the_zero_rows():
    floor = float(np.float32(1.0) / np.float32(1e-12))
    both = cc.case(cc.norm_combination, True, True)
    assert both.sqq[2] == 0 and both.sqq[5] == np.float32(1e-30) and both.sq[3] == 0 and both.sq[77] == np.float32(1e-30)
    assert km.inv_norm32(both.sqq, 40)[[2, 5]].tolist() == [floor] * 2 and km.inv_norm32(both.sq, 600)[[3, 77]].tolist() == [floor] * 2
    assert not both.Tq[7].any() and not both.T[100].any() and both.rows[:3].tolist() == [2, 5, 7]
    lists = {}
    for q_given, c_given in cc.NORMS:
        case = cc.case(cc.norm_combination, q_given, c_given)
        assert (case.sqq is not None) == q_given and (case.sq is not None) == c_given
        assert np.array_equal(case.Tq, both.Tq) and np.array_equal(case.T, both.T) and np.array_equal(case.rows, both.rows)
        lists[q_given, c_given] = _lists(case)
    # the floored candidates head the lists they are in; the four combinations give four different results
    ids, vals = lists[True, True]
    floored = np.isin(ids, [3, 77])
    floored[2] = False                                                        # (the zero query row lists candidate 3 with a score of 0)
    assert floored.sum() >= 10 and (np.diff(floored.astype(np.int8), axis=1) <= 0).all() and vals[floored].min() > 1e9
    keys = list(lists)
    assert all(not np.array_equal(lists[a][1], lists[b][1]) for i, a in enumerate(keys) for b in keys[:i])
    assert (lists[True, True][1][2] == 0).all()                               # the zero query row: every score is 0, ids decide


def test_score_range_closed_forms_agree_with_the_model():
    C = cc.chunk()
    for K, with_excl in cc.SCORE_RANGE:
        case = cc.case(cc.score_range, K, with_excl)
        n = case.T.shape[0]
        assert n == 3 * C + 5 and case.T[:, 0].tolist() == list(range(n)) and not case.T[:, 1:].any() and case.sqq is None and case.sq is None
        s = km.cross_scores32(case.Tq, None, case.T, None, [0, 1, 2])
        assert (np.diff(s[0]) > 0).all() and (np.diff(s[1]) < 0).all() and not s[2].any() and s[0, -1] == n - 1
        ids, vals = _lists(case)
        want_ids, want_vals = cc.score_range_closed_form(K, with_excl)
        assert np.array_equal(ids, want_ids) and np.array_equal(vals.view(np.int32), want_vals.view(np.int32))
        if with_excl:
            plain_ids = cc.score_range_closed_form(K, False)[0]
            assert all(set(case.excl[b]) == set(plain_ids[b, :3].tolist()) or K < 3 for b in range(3))
            assert all(set(case.excl[b]) == set(cc.score_range_closed_form(3, False)[0][b].tolist()) for b in range(3))


def test_partition_fillers_score_below_the_shared_rows():
    for d, K in cc.PARTITION:
        small, big = cc.case(cc.partition, d, K)
        assert small.T.shape == (200, d) and big.T.shape == (4200, d) and np.array_equal(big.T[4000:], small.T)
        assert np.array_equal(big.sq[4000:], small.sq) and np.array_equal(big.rows, small.rows) and small.rows.size == 65
        assert small.rows[0] == small.rows[37] == small.rows[64]
        assert (small.T != np.rint(small.T)).any()                            # random floats
        T64, q64 = big.T.astype(np.float64), big.Tq.astype(np.float64)
        s = (q64 @ T64.T) / np.sqrt(big.sqq.astype(np.float64))[:, None] / np.sqrt(big.sq.astype(np.float64))[None, :]
        assert (s[:, :4000].max(1) < s[:, 4000:].min(1) - 1000.0).all()       # every filler far below every shared row, for every query
        assert 4000 < cc.chunk() < 4200                                       # the shared rows straddle a chunk boundary


def test_exclusion_cases_leave_what_they_say():
    C = cc.chunk()
    for K in cc.EXCLUSIONS:
        case = cc.case(cc.exclusions, K)
        n = case.T.shape[0]
        left = [n - len(set(e)) for e in case.excl]
        assert n == C + 50 and len(case.excl[0]) > n and left == [5, 0, C, K - 1, K, K + 1, n]
        assert min(case.excl[2]) == C and max(case.excl[2]) == n - 1
        ids, _ = _lists(case)
        assert (ids >= 0).sum(1).tolist() == [min(K, x) for x in left]
    case, bad_queries, bad_excl = cc.outside_ids()
    nq, n = case.Tq.shape[0], case.T.shape[0]
    assert nq < n and bad_queries == [-1, -2 ** 31, nq, 2 ** 31 - 1, 150] and nq <= 150 < n
    assert all(not 0 <= e < n for e in bad_excl) and {-1, n, 2 ** 31 - 1, -2 ** 31} <= set(bad_excl)


def test_nonfinite_rows_give_the_three_scores():
    """In np.float32 arithmetic (every product rounded, then added) the three rows give +inf, -inf and NaN; in the fmaf chain of the
    matrix instruction the cancelling row stays at +inf, and the row with the infinite squared norm is the NaN."""
    case = cc.case(cc.nonfinite, 3)
    assert np.isfinite(case.Tq).all() and np.isfinite(case.T).all() and case.sqq is None
    q = case.Tq[0]
    with np.errstate(all="ignore"):
        got = []
        for i in (cc.NF_PLUS, cc.NF_MINUS, cc.NF_CANCEL):
            acc = np.float32(0)
            for k in range(8):
                acc = np.float32(acc + np.float32(q[k] * case.T[i, k]))
            got.append(acc)
    assert got[0] == np.inf and got[1] == -np.inf and np.isnan(got[2])
    s = km.cross_scores32(case.Tq, None, case.T, case.sq, [0, 1], chain=True)
    assert s[0, cc.NF_PLUS] == np.inf and s[0, cc.NF_PLUS2] == np.inf and s[0, cc.NF_MINUS] == -np.inf and s[0, cc.NF_CANCEL] == np.inf
    assert np.isnan(s[0, cc.NF_ZERO_INV]) and np.isfinite(np.delete(s[0], [5, 9, 13, 17, 21])).all() and np.isfinite(s[1]).all()
    for K in cc.NONFINITE:
        ids, vals = _lists(cc.case(cc.nonfinite, K))
        assert ids[0, :3].tolist() == [5, 13, 21] and np.isposinf(vals[0, :3]).all() and np.array_equal(ids[0], ids[2])
        listed = ids[0][ids[0] >= 0]
        assert 9 not in listed and 17 not in listed and (K < 40 or listed.size == 38) and np.isfinite(vals[1][ids[1] >= 0]).all()
