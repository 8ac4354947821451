"""The neighbour votes on the device (csrc/vote.hip) against the exact host model of tests/vote_model.py, and what is built on them:
ops.NeighbourLists / neighbour_vote_topk, torch.ops.elimrec.neighbour_vote_topk, EliMRec.neighbour_lists / recommend_knn /
knn_recommend_device, evaluator.BaselineReport.

The kernel is integer arithmetic up to one float64 product rounded once, so nothing here has a tolerance: idx and cnt are compared
exactly and val bit for bit, in both forms. The report's means are ops.group_metric_means' -- float64 sums rounded once -- and take
that op's own bound (tests/test_group_eval_gpu.py: one fp32 ulp of the float64 mean rounded once)."""
import ctypes

import numpy as np
import pytest
import torch

import vote_cases as vc
import vote_model as vm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), (what, "idx", got[0], want[0])
    assert np.array_equal(got[2], want[2]), (what, "cnt")
    assert got[1].dtype == np.float32 and got[1].view(np.int32).tobytes() == want[1].view(np.int32).tobytes(), (what, "val")


class Resident(object):
    """A case on the device, with the model's lists at K = 256 computed once per (users, exclude_history)."""

    def __init__(self, case):
        from elimrec_amd import ops
        self.case = case
        self.lists = ops.NeighbourLists(case.idx, case.val, DEV)
        self.hist = ops.HistoryIndex(*vm.csr_of(case.hist), DEV)
        self.excl = ops.HistoryIndex(*vm.csr_of(case.excl), DEV) if case.excl is not None else None
        self._want = {}

    def want(self, users, K, exclude_history=True):
        key = (tuple(users), exclude_history)
        if key not in self._want:
            self._want[key] = vm.topk(self.case.idx, self.case.val, self.case.hist, users, 256, self.case.excl, exclude_history)
        return tuple(x[:, :K] for x in self._want[key])

    def run(self, users, K, lds=True, exclude_history=True, workspace=None, hist=None):
        from elimrec_amd import ops
        B = len(users)
        idx = torch.full((B, K), 77, dtype=torch.int32, device=DEV)
        val = torch.full((B, K), 7.0, dtype=torch.float32, device=DEV)
        cnt = torch.full((B, K), 77, dtype=torch.int32, device=DEV)
        ops.neighbour_vote_topk(self.lists, hist or self.hist, np.asarray(users, dtype=np.int64), K, idx, val, cnt, excl=self.excl,
                                exclude_history=exclude_history, lds=lds, workspace=workspace)
        return idx.cpu().numpy(), val.cpu().numpy(), cnt.cpu().numpy()


_RESIDENT = {}


def _resident(name):
    if name not in _RESIDENT:
        _RESIDENT[name] = Resident(vc.case(name))
    return _RESIDENT[name]


@pytest.mark.parametrize("lds", [True, False])
@pytest.mark.parametrize("K", vc.KS)
@pytest.mark.parametrize("name", list(vc.BUILDERS))
def test_every_case_in_both_forms(name, K, lds):
    r = _resident(name)
    _same(r.run(r.case.users, K, lds=lds), r.want(r.case.users, K), (name, K, lds))


def test_lists_histories_and_selection_by_hand():
    r = _resident("basics")
    idx, val, cnt = r.run(r.case.users, 64)
    assert (idx[0] == -1).all() and np.isneginf(val[0]).all() and (cnt[0] == 0).all()          # an empty history
    assert idx[1].tolist()[:1] == [-1]                                                        # item 5 is voted for and left out
    assert idx[2, 0] == 6 and cnt[2, 0] == 2 and (idx[2, 1:] == -1).all()                     # a repeated id within a list
    assert (idx[8] == -1).all() and (idx[10] == -1).all() and (idx[11] == -1).all()           # all left out; fillers; outside the table
    assert cnt[5].max() >= 3                                                                  # a repeated history id votes again
    idx_h, _, _ = r.run(r.case.users, 64, exclude_history=False)
    _same(r.run(r.case.users, 64, exclude_history=False), r.want(r.case.users, 64, False), "exclude_history=False")
    assert not np.array_equal(idx_h, idx)


def test_fixed_point_by_hand():
    r = _resident("fixed_point")
    idx, val, cnt = r.run([0], 64)
    row = {int(i): (float(v), int(c)) for i, v, c in zip(idx[0], val[0], cnt[0]) if i >= 0}
    assert row[30] == (0.0, 1) and row[31] == (2.0 ** -23, 1) and row[37] == (2.0 ** -23, 1) and row[35] == (0.0, 2)
    assert row[32] == (float(np.float32(2 * int(vm.fixed(np.float32(1.0 / 3.0))) * 2.0 ** -24)), 2)
    assert row[33] == (-0.25, 1) and row[36] == (0.0, 1) and row[38] == (-2.0 ** -23, 1)     # halves tie to the even integer
    assert row[40][0] == row[41][0] == 1024.0 and idx[0].tolist()[:2] == [40, 41]            # sums 2^34 + 1 and 2^34 + 2, by id
    assert idx[0].tolist().index(30) < idx[0].tolist().index(35) < idx[0].tolist().index(36)  # three scores of 0, by id


def test_the_two_forms_at_the_cap():
    from elimrec_amd import ops
    r = _resident("at_the_cap")
    V = ops.vote_votes(r.lists, r.hist, r.excl)
    assert V.tolist() == [vc.CAP, 2 * 3 + 2, vc.CAP + 1, vc.CAP + 1]
    assert [ops.vote_rows_in_lds(v) for v in V] == [True, True, False, False]
    ws = torch.zeros(ops.vote_workspace(2, r.lists.n), dtype=torch.uint8, device=DEV)
    got = r.run(r.case.users, 64, workspace=ws)
    _same(got, r.want(r.case.users, 64), "interleaved")
    assert int(ws.count_nonzero()) == 0
    assert np.array_equal(got[0][2], got[0][3]) and got[1][2].tobytes() == got[1][3].tobytes()   # the history reversed
    with pytest.raises(ValueError, match="workspace needs"):
        r.run(r.case.users, 64, workspace=ws[:-16])


def _raw_call(r, users, K, n_dense_rows, ws):
    """elimrec_neighbour_vote_topk itself with lds off and a declared dense-row count of the caller's choosing: the grid is
    min(n_dense_rows, VOTE_GROUPS) workgroups, which loop over all B rows."""
    from elimrec_amd import _lib
    B = len(users)
    idx = torch.full((B, K), 77, dtype=torch.int32, device=DEV)
    val = torch.full((B, K), 7.0, dtype=torch.float32, device=DEV)
    cnt = torch.full((B, K), 77, dtype=torch.int32, device=DEV)
    u = torch.tensor(users, dtype=torch.int64, device=DEV)
    rc = _lib.load().elimrec_neighbour_vote_topk(r.lists.idx.data_ptr(), r.lists.val.data_ptr(), r.lists.n, r.lists.Kn, r.hist.ptr.data_ptr(),
                                                 r.hist.items.data_ptr(), r.hist.n_rows, r.excl.ptr.data_ptr(), r.excl.items.data_ptr(),
                                                 r.excl.n_rows, u.data_ptr(), B, K, 1, 0, n_dense_rows, idx.data_ptr(), val.data_ptr(),
                                                 cnt.data_ptr(), ws.data_ptr(), ws.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    return idx.cpu().numpy(), val.cpu().numpy(), cnt.cpu().numpy()


def test_dense_rows_share_a_workspace_row_and_leave_it_zero():
    from elimrec_amd import ops
    r = _resident("dense_rows")
    users = r.case.users
    ws = torch.zeros(ops.vote_workspace(2, r.lists.n), dtype=torch.uint8, device=DEV)
    assert ws.numel() == 2 * 70 * 12 and ops.vote_workspace(len(users), r.lists.n) > ws.numel()
    for K in vc.KS:
        _same(_raw_call(r, users, K, 2, ws), r.want(users, K), ("two workgroups", K))
        assert int(ws.count_nonzero()) == 0
    # the same workspace again, now through ops with all seven rows declared
    big = torch.zeros(ops.vote_workspace(len(users), r.lists.n), dtype=torch.uint8, device=DEV)
    _same(r.run(users, 64, lds=False, workspace=big), r.want(users, 64), "seven workgroups")
    assert int(big.count_nonzero()) == 0


@pytest.mark.parametrize("name", ["cut_rising", "cut_falling", "cut_flat"])
def test_the_cut_leaves_the_workspace_zero(name):
    from elimrec_amd import ops
    r = _resident(name)
    ws = torch.zeros(ops.vote_workspace(2, r.lists.n), dtype=torch.uint8, device=DEV)
    for K in vc.KS:
        _same(r.run(r.case.users, K, workspace=ws), r.want(r.case.users, K), (name, K))
        assert int(ws.count_nonzero()) == 0


@pytest.mark.parametrize("lds", [True, False])
def test_independence(lds):
    from elimrec_amd import ops
    r = _resident("basics")
    users = r.case.users
    base = r.run(users, 64, lds=lds)
    # the users permuted, repeated, alone
    rng = np.random.default_rng(2)
    perm = [int(u) for u in rng.permutation(users)] + [4, 4]
    got = r.run(perm, 64, lds=lds)
    for b, u in enumerate(perm):
        _same(tuple(x[b] for x in got), tuple(x[u] for x in base), ("permuted", u))
    for u in (4, 5, 7):
        alone = r.run([u], 64, lds=lds)
        _same(tuple(x[0] for x in alone), tuple(x[u] for x in base), ("alone", u))
    # every history permuted
    shuffled = [[h[i] for i in rng.permutation(len(h))] for h in r.case.hist]
    hist = ops.HistoryIndex(*vm.csr_of(shuffled), DEV)
    _same(r.run(users, 64, lds=lds, hist=hist), base, "histories permuted")


@pytest.mark.parametrize("name", ["basics", "at_the_cap", "hash_chain"])
def test_the_torch_op(name):
    from elimrec_amd import torch_ops
    r = _resident(name)
    users = r.case.users
    idx, val, cnt = torch_ops.load().neighbour_vote_topk(r.lists.idx, r.lists.val, r.hist.ptr, r.hist.items[:r.hist.n_entries], r.excl.ptr,
                                                        r.excl.items[:r.excl.n_entries], torch.tensor(users, device=DEV), 64)
    _same((idx.cpu().numpy(), val.cpu().numpy(), cnt.cpu().numpy()), r.run(users, 64), name)
    _same((idx.cpu().numpy(), val.cpu().numpy(), cnt.cpu().numpy()), r.want(users, 64), name)
    r = _resident("fixed_point")
    idx, val, cnt = torch_ops.load().neighbour_vote_topk(r.lists.idx, r.lists.val, r.hist.ptr, r.hist.items, None, None,
                                                        torch.tensor(r.case.users, device=DEV), 7)
    _same((idx.cpu().numpy(), val.cpu().numpy(), cnt.cpu().numpy()), r.want(r.case.users, 7), "no second CSR")
    with pytest.raises(IndexError):
        torch_ops.load().neighbour_vote_topk(r.lists.idx, r.lists.val, r.hist.ptr, r.hist.items, None, None, torch.tensor([99], device=DEV), 7)
    with pytest.raises(ValueError, match="overflow"):
        torch_ops.load().neighbour_vote_topk(r.lists.idx, r.lists.val * 2.0 ** 62, r.hist.ptr, r.hist.items, None, None,
                                             torch.tensor([0], device=DEV), 7)


# --------------------------------------------------------------------------- the model and the report
def _fixture(forward, extra=()):
    from helpers import build_model_from_fixture, load_golden
    g = load_golden("ml3")
    model, _ = build_model_from_fixture(g, DEV, extra_argv=list(extra))
    if forward:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        model.bpr_loss(t(g["step1/users"]), t(g["step1/pos"]), t(g["step1/neg"]))
    return model


def _tensors(x):
    return tuple(t.numpy() for t in x)


def test_recommend_knn_on_the_fixture():
    model = _fixture(True)
    I, U = model.num_items, model.num_users
    train = model.dataset.get_user_train_dict()
    users = list(range(0, U, 3)) + [1, 1]
    hist = [list(train.get(u, [])) for u in range(U)]
    for source, Kn in (("co", 50), ("co", 4), ("v", 6)):
        near = model.co_items(np.arange(I), Kn, "jaccard") if source == "co" else model.similar_items(np.arange(I), Kn, space=source)
        got = model.recommend_knn(users, 20, neighbours=Kn, source=source, measure="jaccard")
        want = vm.topk(near.ids.numpy(), near.scores.numpy(), hist, users, 20)
        _same(_tensors(got), want, (source, Kn))
        assert (got.ids >= 0).any()
    # the lists are kept: per (neighbours, measure) for "co", per table version for a space
    assert model.neighbour_lists("co", 4, "jaccard") is model.neighbour_lists("co", 4, "jaccard")
    assert model.neighbour_lists("co", 4, "jaccard") is not model.neighbour_lists("co", 4, "count")
    assert model.neighbour_lists("v", 6) is model.neighbour_lists("v", 6)
    # a history and an exclusion of the caller's
    mine = {0: [3, 4, 5, 3], 2: []}
    near = model.co_items(np.arange(I), 4, "cosine")
    got = model.recommend_knn([0, 2, 5], 7, neighbours=4, history=mine, exclude={0: [int(near.ids[3, 0])]})
    want = vm.topk(near.ids.numpy(), near.scores.numpy(), [mine[0], [], []], [0, 1, 2], 7, excl=[[int(near.ids[3, 0])], [], []])
    _same(_tensors(got), want, "history")
    assert (got.ids[1:] == -1).all() and int(near.ids[3, 0]) not in got.ids[0].tolist()
    # an untrained model serves "co", and refuses a space without tables
    fresh = _fixture(False)
    _same(_tensors(fresh.recommend_knn(users, 20, neighbours=4, measure="cosine")),
          vm.topk(near.ids.numpy(), near.scores.numpy(), hist, users, 20), "untrained")
    with pytest.raises(RuntimeError):
        fresh.recommend_knn([0], 5, source="v")


def _ulp_close(got, want):
    """One fp32 ulp of the float64 mean rounded once (ops.group_metric_means' bound)."""
    want32 = np.asarray(want, dtype=np.float64).astype(np.float32)
    return np.all(np.abs(np.asarray(got, dtype=np.float64) - want32.astype(np.float64)) <= np.spacing(np.abs(want32)).astype(np.float64))


@pytest.mark.parametrize("effect", ["TE", "TIE"])
def test_the_baseline_report_on_the_fixture(effect):
    from elimrec_amd.reports import exposure_summary
    model = _fixture(True, ["--baseline_report=20", "--baseline_sources=[co,v]", "--baseline_neighbours=7", "--group_view=[2,4]",
                            "--significance_report=50"])
    model.predict_type = effect
    rep, sig = model.baseline_reporter, model.significance_reporter
    final, buf = rep.evaluate(model)
    I, K = model.num_items, 20
    train, test = model.dataset.get_user_train_dict(), model.dataset.get_user_test_dict()
    users = rep.users
    assert users == sig.users and final.columns == rep.columns and final.table.shape == (2 * len(rep.group_labels), len(rep.columns))
    hist = [list(train.get(u, [])) for u in users]
    truth = [sorted(set(test[u])) for u in users]
    ev = rep.evaluator
    own = np.concatenate([idx.cpu().numpy() for _, _, _, idx in rep.top_lists(model, users, K, rep.block_users, rep.tie_order)])
    sig_rows = sig.metric_rows(model)
    for s, source in enumerate(rep.sources):
        near = model.co_items(np.arange(I), 7, "cosine") if source == "co" else model.similar_items(np.arange(I), 7, space=source)
        want_lists = vm.topk(near.ids.numpy(), near.scores.numpy(), hist, range(len(users)), K)[0]
        lists = rep.knn_lists(model, source)
        assert np.array_equal(lists.cpu().numpy(), want_lists) and (want_lists == -1).any() and (want_lists >= 0).any()
        metric = vm.metric_rows(want_lists[:, :ev.max_top], truth, ev.metrics)[:, rep._shown]
        rows, columns = rep.metric_rows(model, source)
        assert columns == sig.columns and rows.shape == sig_rows[0].shape and rows.is_contiguous()
        assert np.array_equal(rows.cpu().numpy(), metric)                    # per user bit for bit: a filler is a miss
        per_user = np.concatenate([metric, vm.list_columns(want_lists, own, rep.item_counts)], axis=1).astype(np.float64)
        for g, at in enumerate(rep._positions):
            got = final.table[s * len(rep.group_labels) + g]
            assert _ulp_close(got[:per_user.shape[1]], per_user[at].mean(axis=0)), (source, g)
            counts = np.bincount(want_lists[at][want_lists[at] >= 0], minlength=I)
            assert np.array_equal(got[per_user.shape[1]:], exposure_summary(counts, [np.arange(I)])[0, 1:4]), (source, g)
        shift, text = sig.shift((rows, columns), sig_rows)                   # model - baseline, paired per user
        assert _ulp_close(shift.mean[0], (sig_rows[0].cpu().numpy().astype(np.float32) - metric).astype(np.float64).mean(axis=0))
        assert shift.p is not None and "all: mean" in text
    assert buf.count("\n") == final.table.shape[0] and "co all:" in buf and "v all:" in buf
    assert rep.knn_lists(model, "co") is rep.knn_lists(model, "co")           # kept with the model's neighbour lists
