"""The dense form of the co-interaction neighbours (csrc/cooccur.hip, cooccur_dense_kernel) past one row and one cut per workgroup,
and the outer edges of the LDS form, on the graphs of tests/cooccur_cases.py (tests/test_cooccur_cpu.py shows, without a device,
that each graph reaches the mechanism it is named for). Everything is exact: idx and cnt equal, val bit for bit, against
cooccur_model.topk; no tolerance anywhere. Every output is pre-filled with a sentinel and allocated PAD rows longer than [Q x K]:
the rows behind keep the sentinel.

  test_many_rows                      2 G + 81 dense rows on G workgroups: up to 3 rows per workgroup on one counter row, s_n / s_thr
                                      reset between them, the workspace zero afterwards and good for a second call
  test_rows_among_lds_rows            interleaved: one workgroup serves dense positions 0, 3, 6 and two serve none (the s_flag skip);
                                      second_pass: G = 1 and the row waits in the second pass of the `base` loop
  test_the_list_is_cut_again_and_again  rising / flat_desc: 4 cuts, each raising the threshold, nothing dropped; falling / flat_asc:
                                      one cut, everything after it dropped; flat_*: the id in the key's low word alone decides
  test_lds_form_edges                 wrap: probing past the table's last slot; full_list: 2047 candidates, the network over the
                                      whole list; sort_sizes: 63 / 64 / 65 / 128 / 129 / 1024 / 1025 candidates

What a wrong kernel fails here (value-only changes of cooccur.hip, each built apart and run once against this file; none of them
is part of the tree):
  s_thr not reset per row             8 fail: test_many_rows (all five), test_rows_among_lds_rows[interleaved-*]
  the c swap dropped from co_sort     15 fail: test_many_rows (all five), test_rows_among_lds_rows (all six),
                                      test_lds_form_edges[wrap-*, sort_sizes-*] (the graphs with counts 1 and 2)
  the probe stops at the table's end  2 fail: test_lds_form_edges[wrap-256, wrap-5] -- run as "a candidate whose probe finds the last
                                      slot taken is dropped"; a clamp to the last slot itself never ends once that slot is taken
                                      by another key, so that form was not run
  key >= thr in pass 2                none fails, and none can: a key is (score, ~id) and an id is claimed once per row, so a
                                      candidate's key never equals a kept one's and the threshold 0 is below every key -- the
                                      change computes the same function. Its neighbour "the score word alone must exceed the
                                      threshold's" was run in its place: 16 fail, among them all four
                                      test_the_list_is_cut_again_and_again[flat_desc-*] and test_lds_form_edges[full_list-*]

Measured on an MI355X: the file's 33 tests take 3.0 s in all, start-up included; the slowest, test_many_rows[65-count] (the first to
build a graph and call the device), 0.35 s, every other under 0.1 s."""
import numpy as np
import pytest
import torch

import cooccur_cases as cc
from test_cooccur_gpu import DEV, MEASURES, Graph, _same

pytestmark = pytest.mark.gpu
PAD = 3                                                       # rows allocated behind [Q x K]
_GRAPHS = {}


def _graph(name):
    if name not in _GRAPHS:
        case = cc.case(name)
        _GRAPHS[name] = Graph(case.users, case.n_query)
    return _GRAPHS[name]


def _run(g, rows, K, measure, lds, workspace=None):
    """One call into sentinel-filled outputs of Q + PAD rows; the rows behind [Q x K] keep the sentinel."""
    from elimrec_amd import ops
    Q = len(rows)
    idx = torch.full((Q + PAD, K), 77, dtype=torch.int32, device=DEV)
    val = torch.full((Q + PAD, K), 7.0, dtype=torch.float32, device=DEV)
    cnt = torch.full((Q + PAD, K), 77, dtype=torch.int32, device=DEV)
    ops.cooccur_topk(g.index, np.asarray(rows, dtype=np.int64), K, idx, val, cnt, measure=measure, lds=lds, workspace=workspace)
    idx, val, cnt = idx.cpu().numpy(), val.cpu().numpy(), cnt.cpu().numpy()
    assert (idx[Q:] == 77).all() and (val[Q:] == 7.0).all() and (cnt[Q:] == 77).all(), (measure, K, lds, "rows behind the output")
    return idx[:Q], val[:Q], cnt[:Q]


def _check(g, rows, K, measure, lds, workspace=None):
    got = _run(g, rows, K, measure, lds, workspace)
    _same(got, g.want(rows, K, measure), (measure, K, lds))
    return got


def _fillers(got, n):
    """Row r lists min(n[r], K) candidates, then -1 / -inf / 0."""
    idx, val, cnt = got
    for r, m in enumerate(n):
        m = min(int(m), idx.shape[1])
        assert (idx[r, :m] >= 0).all() and (cnt[r, :m] >= 1).all() and np.isfinite(val[r, :m]).all()
        assert (idx[r, m:] == -1).all() and np.isneginf(val[r, m:]).all() and (cnt[r, m:] == 0).all()


@pytest.mark.parametrize("K,measure", [(65, "count"), (65, "cosine"), (65, "jaccard"), (1, "cosine"), (256, "jaccard")])
def test_many_rows(K, measure):
    from elimrec_amd import ops
    g, rows = _graph("many_rows"), cc.case("many_rows").rows
    G = ops.COOCCUR_GROUPS
    assert len(rows) > 2 * G and (g.index.walk[rows] > ops.COOCCUR_SLOTS // 2).all()
    need = ops.cooccur_workspace(len(rows), g.n_query)
    assert need == G * g.n_query * 4
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    got = _check(g, rows, K, measure, False, ws)
    assert not ws.any().item()
    back = _run(g, rows[::-1], K, measure, False, ws)         # the same counter rows, every row on another workgroup
    assert not ws.any().item()
    _same(tuple(x[::-1] for x in back), got, "rows reversed")
    if K == 65:
        _same(_run(g, rows, K, measure, True), got, "lds=True: every row is past the limit")
        assert (got[0] >= 0).all()


@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("name", ["interleaved", "second_pass"])
def test_rows_among_lds_rows(name, measure):
    from elimrec_amd import ops
    g, rows = _graph(name), cc.case(name).rows
    dense = np.flatnonzero(g.index.walk[rows] > ops.COOCCUR_SLOTS // 2).tolist()
    assert dense == ([0, 3, 6] if name == "interleaved" else [cc.CO_THREADS + 14])
    for K in (256, 5):
        got = _check(g, rows, K, measure, True)
        _same(_run(g, rows, K, measure, False), got, "lds=False")
        back = _run(g, rows[::-1], K, measure, True)
        _same(tuple(x[::-1] for x in back), got, "rows reversed")
        for p in dense:
            alone = _run(g, [rows[p]], K, measure, True)
            _same(alone, tuple(x[p:p + 1] for x in got), "the row alone")
    if name == "second_pass":
        empty = np.flatnonzero(g.index.walk[rows] == 0)
        assert empty.size == 12
        _fillers(tuple(x[empty] for x in got), [0] * 12)


@pytest.mark.parametrize("K", [1, 64, 255, 256])
@pytest.mark.parametrize("name", ["rising", "falling", "flat_desc", "flat_asc"])
def test_the_list_is_cut_again_and_again(name, K):
    from elimrec_amd import ops
    g, rows = _graph(name), cc.case(name).rows
    assert not ops.cooccur_rows_in_lds(int(g.index.walk[rows[0]]))
    for measure in (("count",) if name.startswith("flat") else ("cosine", "jaccard")):
        got = _check(g, rows, K, measure, False)
        _same(_run(g, rows, K, measure, True), got, "lds=True")
        assert (got[0] >= 0).all() and (got[2] == 1).all()
        if name.startswith("flat"):
            assert got[0][0].tolist() == list(range(1, K + 1))


@pytest.mark.parametrize("K", [256, 5])
@pytest.mark.parametrize("name", ["wrap", "full_list", "sort_sizes"])
def test_lds_form_edges(name, K):
    from elimrec_amd import ops
    g, rows = _graph(name), cc.case(name).rows
    assert all(ops.cooccur_rows_in_lds(int(w)) for w in g.index.walk[rows])
    n = {"wrap": [48], "full_list": [ops.COOCCUR_SLOTS // 2 - 1]}.get(name) or [cc.SORT_SIZES[r] for r in rows]
    for measure in MEASURES:
        got = _check(g, rows, K, measure, True)
        _fillers(got, n)
        _same(_run(g, rows, K, measure, False), got, "lds=False")
        if name != "full_list" and K == 256:                  # counts 1 and 2 among the listed
            assert set(np.unique(got[2]).tolist()) - {0} == {1, 2}
