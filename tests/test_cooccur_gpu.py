"""The co-interaction neighbours on the device (csrc/cooccur.hip) against the exact host model of tests/cooccur_model.py, and what is
built on them: ops.CooccurIndex / cooccur_topk / cooccur_walk, EliMRec.co_items / co_users / co_neighbours_device,
evaluator.CoNeighbourReport, --co_report, torch.ops.elimrec.cooccur_topk.

The kernel is integer arithmetic up to one float64 expression rounded once, so nothing here has a tolerance: idx and cnt are compared
exactly and val bit for bit, for all three measures. The report's means are ops.group_metric_means' -- float64 sums rounded once --
and take that op's own bound (tests/test_group_eval_gpu.py: one fp32 ulp of the float64 mean rounded once)."""
import numpy as np
import pytest
import torch

import cooccur_model as cm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEASURES = ("count", "cosine", "jaccard")
HAND_USERS = [[0, 1, 2], [1, 2], [0, 2], [3]]                 # the 4 user x 5 item graph of tests/test_cooccur_cpu.py


class Graph(object):
    """A bipartite graph from the other side's lists (user -> items): both CSRs, the index on the device, the model's inputs."""

    def __init__(self, user_lists, n_query):
        from elimrec_amd import ops
        self.n_query, self.n_other = n_query, len(user_lists)
        self.o_ptr, self.o_nbr = cm.csr_of(user_lists)
        self.q_ptr, self.q_nbr = cm.transpose_csr(self.o_ptr, self.o_nbr, n_query)
        self.index = ops.CooccurIndex(self.q_ptr, self.q_nbr, self.o_ptr, self.o_nbr, n_query, self.n_other, DEV)
        self.walk = cm.walk(self.q_ptr, self.q_nbr, self.n_other)
        self._want = {}

    def want(self, rows, K, measure):
        """The model's lists: computed once per (rows, measure) at K = 256 and cut (a list's first K entries are its top-K)."""
        key = (tuple(int(r) for r in rows), measure)
        if key not in self._want:
            self._want[key] = cm.topk(self.q_ptr, self.q_nbr, self.n_other, rows, 256, measure)
        return tuple(x[:, :K] for x in self._want[key])

    def run(self, rows, K, measure, lds=True, workspace=None):
        from elimrec_amd import ops
        Q = len(rows)
        idx = torch.full((Q, K), 77, dtype=torch.int32, device=DEV)
        val = torch.full((Q, K), 7.0, dtype=torch.float32, device=DEV)
        cnt = torch.full((Q, K), 77, dtype=torch.int32, device=DEV)
        ops.cooccur_topk(self.index, np.asarray(rows, dtype=np.int64), K, idx, val, cnt, measure=measure, lds=lds, workspace=workspace)
        return idx.cpu().numpy(), val.cpu().numpy(), cnt.cpu().numpy()

    def check(self, rows, K, measure, lds=True, workspace=None):
        got = self.run(rows, K, measure, lds, workspace)
        _same(got, self.want(rows, K, measure), (measure, K, lds))
        return got


def _same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), (what, "idx")
    assert np.array_equal(got[2], want[2]), (what, "cnt")
    assert got[1].dtype == np.float32 and got[1].view(np.int32).tobytes() == want[1].view(np.int32).tobytes(), (what, "val")


_GRAPHS = {}


def _graph(name):
    if name not in _GRAPHS:
        _GRAPHS[name] = globals()["_make_" + name]()
    return _GRAPHS[name]


def _make_hand():
    return Graph(HAND_USERS, 5)


def _make_ties():
    rng = np.random.default_rng(11)
    return Graph([rng.choice(500, size=3, replace=False).tolist() for _ in range(300)], 500)


def _edge_shapes():
    from elimrec_amd import ops
    H = ops.COOCCUR_SLOTS // 2
    shapes = []
    for W in (H - 1, H, H + 1):
        m = next(m for m in range(3, 64) if W % m == 0)
        shapes.append((W, m, W // m))
    return shapes


def _make_edge():
    """Items 0, 1, 2 with W = SLOTS/2 - 1, SLOTS/2, SLOTS/2 + 1: item q has m users of degree W / m, who share nothing else by
    construction but meet at random among the other 1497 items."""
    rng = np.random.default_rng(5)
    users = []
    for q, (W, m, deg) in enumerate(_edge_shapes()):
        users += [[q] + (3 + rng.choice(1497, size=deg - 1, replace=False)).tolist() for _ in range(m)]
    return Graph(users, 1500)


def _make_collide():
    """A catalogue of 8 x SLOTS items. Item 0: one user holds it and the 8 items = 7 (mod SLOTS). Item 1: one user holds it and the
    1600 items whose id mod SLOTS lies in [100, 300) -- 200 runs of 8 keys with one home slot each -- and a second user holds it and
    every fourth of them: 1600 candidates with counts 1 and 2, W = 1601 + 401 = 2002, as many as the LDS form admits in this shape."""
    from elimrec_amd import ops
    S = ops.COOCCUR_SLOTS
    one = [7 + S * k for k in range(8)]
    many = [r + S * k for r in range(100, 300) for k in range(8)]
    return Graph([[0] + one, [1] + many, [1] + many[::4]], 8 * S)


def _make_repeat():
    return Graph([[0, 1, 1, 2], [0, 0, 2], [1, 2, 3]], 4)


# --------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("measure", MEASURES)
def test_hand_graph(measure):
    """The row itself is left out; item 3's only user has degree 1 (all fillers); item 4 has no user; a query id repeated."""
    from elimrec_amd import ops
    g = _graph("hand")
    rows = [0, 1, 2, 3, 4, 2, 0]
    for lds in (True, False):
        idx, val, cnt = g.check(rows, 3, measure, lds)
        assert idx.tolist() == [[2, 1, -1], [2, 0, -1], [0, 1, -1], [-1] * 3, [-1] * 3, [0, 1, -1], [2, 1, -1]]
        assert cnt.tolist() == [[2, 1, 0], [2, 1, 0], [2, 2, 0], [0] * 3, [0] * 3, [2, 2, 0], [2, 1, 0]]
        assert np.isneginf(val[3]).all() and np.isneginf(val[:, 2]).all()
    want0 = {"count": [2.0, 1.0], "cosine": [2 / np.sqrt(6.0), 0.5], "jaccard": [2 / 3.0, 1 / 3.0]}[measure]
    assert val[0, :2].tolist() == np.asarray(want0, dtype=np.float64).astype(np.float32).tolist()
    assert ops.cooccur_walk(g.index, rows).cpu().tolist() == [5, 5, 7, 1, 0, 7, 5] == g.index.walk[rows].tolist()
    # out_val / out_cnt are optional, an empty query launches nothing
    only = torch.empty(len(rows), 3, dtype=torch.int32, device=DEV)
    ops.cooccur_topk(g.index, rows, 3, only, measure=measure)
    assert np.array_equal(only.cpu().numpy(), idx)
    assert ops.cooccur_topk(g.index, [], 3, only) is only and np.array_equal(only.cpu().numpy(), idx)


@pytest.mark.parametrize("K", [1, 64, 65, 256])
def test_ties(K):
    """300 users x 500 items, every user's degree 3: most counts are 1 or 2, so the id decides; rows with fewer than K candidates."""
    g = _graph("ties")
    rows = np.arange(500)
    for measure in MEASURES:
        idx, val, cnt = g.check(rows, K, measure)
        if measure == "count":
            assert set(np.unique(cnt)) <= {0, 1, 2, 3} and (cnt == 1).sum() > (cnt >= 2).sum() > 0
            tied = (val[:, :-1] == val[:, 1:]) & (idx[:, 1:] >= 0) if K > 1 else np.zeros((1, 1), bool)
            assert K == 1 or (tied.any() and (idx[:, :-1][tied] < idx[:, 1:][tied]).all())
        if K >= 64:
            assert (idx[:, -1] < 0).any() and (idx[:, 0] >= 0).any()        # fewer than K candidates somewhere
    _same(g.run(rows, K, "cosine", lds=False), g.want(rows, K, "cosine"), "dense form")


def test_form_edge():
    """W = SLOTS/2 - 1, SLOTS/2 (the LDS form) and SLOTS/2 + 1 (the dense form): each with lds=True and lds=False, the same bits."""
    from elimrec_amd import ops
    g = _graph("edge")
    shapes = _edge_shapes()
    H = ops.COOCCUR_SLOTS // 2
    assert [W for W, _, _ in shapes] == [H - 1, H, H + 1] == g.walk[:3].tolist() == g.index.walk[:3].tolist()
    assert ops.cooccur_walk(g.index, [0, 1, 2]).cpu().tolist() == [H - 1, H, H + 1]
    assert [ops.cooccur_rows_in_lds(W) for W in g.walk[:3]] == [True, True, False]
    for measure in MEASURES:
        for K in (5, 256):
            for rows in ([0], [1], [2], [2, 1, 0]):
                a = g.check(rows, K, measure, lds=True)
                b = g.check(rows, K, measure, lds=False)
                _same(a, b, "the two forms")
    assert (g.want([2], 256, "count")[0] >= 0).all()                       # more than K candidates: the dense form cuts its list


def test_hash_collisions():
    from elimrec_amd import ops
    g = _graph("collide")
    assert g.n_query == 8 * ops.COOCCUR_SLOTS and g.q_nbr.size < 4000
    assert g.walk[:2].tolist() == [9, 2002] and ops.cooccur_rows_in_lds(2002)
    for measure in MEASURES:
        idx, val, cnt = g.check([0, 1], 256, measure)
        assert sorted(idx[0][idx[0] >= 0].tolist()) == [7 + ops.COOCCUR_SLOTS * k for k in range(8)]
        assert (idx[1] >= 0).all() and set(np.unique(cnt[1])) <= {1, 2}
        _same(g.run([0, 1], 256, measure, lds=False), (idx, val, cnt), "dense form")


def test_repeated_edges_give_the_product_count():
    """User 0 lists item 1 twice, user 1 lists item 0 twice: c(0, 1) = 1 x 2, c(0, 2) = 1 x 1 + 2 x 1, deg(0) = 3."""
    g = _graph("repeat")
    for lds in (True, False):
        idx, val, cnt = g.check([0, 1, 2, 3], 3, "count", lds)
        assert idx[0].tolist() == [2, 1, -1] and cnt[0].tolist() == [3, 2, 0]
        assert idx[3].tolist() == [1, 2, -1] and cnt[3].tolist() == [1, 1, 0]
        for measure in ("cosine", "jaccard"):
            g.check([0, 1, 2, 3], 3, measure, lds)
    assert g.index.deg.tolist() == [3, 3, 3, 1]


def test_dense_form_leaves_its_workspace_clean():
    from elimrec_amd import ops
    g = _graph("ties")
    first, second = np.arange(0, 250), np.arange(499, 249, -1)
    need = ops.cooccur_workspace(250, g.n_query)
    assert need == 250 * 500 * 4
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    g.check(first, 64, "jaccard", lds=False, workspace=ws)
    assert not ws.any().item()
    got = g.check(second, 64, "jaccard", lds=False, workspace=ws)
    assert not ws.any().item()
    _same(got, g.run(second, 64, "jaccard", lds=False), "fresh workspace")
    with pytest.raises(ValueError):
        g.run(first, 64, "jaccard", lds=False, workspace=ws[:need - 16])


@pytest.mark.parametrize("lds", [True, False])
def test_determinism(lds):
    g = _graph("ties")
    rows = np.arange(500)
    a = g.run(rows, 65, "cosine", lds)
    _same(g.run(rows, 65, "cosine", lds), a, "two calls")
    for q in (0, 17, 499):
        alone = g.run([q], 65, "cosine", lds)
        moved = g.run([3, q, 4, q], 65, "cosine", lds)
        for x, y, z in zip(alone, moved, a):
            assert x[0].tobytes() == y[1].tobytes() == y[3].tobytes() == z[q].tobytes()


def test_user_side_and_from_train():
    from elimrec_amd import ops
    rng = np.random.default_rng(3)
    train = {u: rng.choice(40, size=int(rng.integers(0, 9)), replace=False).tolist() for u in range(60)}
    u_ptr, u_items = cm.csr_of([train[u] for u in range(60)])
    i_ptr, i_users = cm.transpose_csr(u_ptr, u_items, 40)
    for side, (ptr, nbr, n, other) in (("item", (i_ptr, i_users, 40, 60)), ("user", (u_ptr, u_items, 60, 40))):
        index = ops.CooccurIndex.from_train(train, 60, 40, side, DEV)
        assert (index.n_query, index.n_other) == (n, other) and index.q_ptr.cpu().tolist() == ptr.tolist()
        rows = np.arange(n)
        idx = torch.empty(n, 7, dtype=torch.int32, device=DEV)
        val = torch.empty(n, 7, dtype=torch.float32, device=DEV)
        cnt = torch.empty(n, 7, dtype=torch.int32, device=DEV)
        ops.cooccur_topk(index, rows, 7, idx, val, cnt, measure="jaccard")
        _same((idx.cpu().numpy(), val.cpu().numpy(), cnt.cpu().numpy()), cm.topk(ptr, nbr, other, rows, 7, "jaccard"), side)
        has = (cm.topk(ptr, nbr, other, rows, 1, "count")[0][:, 0] >= 0)
        assert index.has_neighbour.tolist() == has.tolist()


def test_torch_op():
    from elimrec_amd import torch_ops
    torch_ops.load()
    g = _graph("edge")
    rows = [2, 0, 1, 7]
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(DEV)
    args = (t(g.q_ptr, np.int64), t(g.q_nbr, np.int32), t(g.o_ptr, np.int64), t(g.o_nbr, np.int32))
    for measure in MEASURES:
        idx, val, cnt = torch.ops.elimrec.cooccur_topk(*args, t(rows, np.int32), 9, measure)
        _same((idx.cpu().numpy(), val.cpu().numpy(), cnt.cpu().numpy()), g.want(rows, 9, measure), measure)
    with pytest.raises(IndexError):
        torch.ops.elimrec.cooccur_topk(*args, t([1500], np.int32), 9, "cosine")
    with pytest.raises(RuntimeError):
        torch.ops.elimrec.cooccur_topk(*args, t(rows, np.int32), 257, "cosine")
    with pytest.raises(RuntimeError):
        torch.ops.elimrec.cooccur_topk(*args, t(rows, np.int32), 9, "dice")


# --------------------------------------------------------------------------- the model and the report
def _fixture(name, forward):
    from helpers import build_model_from_fixture, load_golden
    g = load_golden(name)
    model, _ = build_model_from_fixture(g, DEV)
    if forward:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        model.bpr_loss(t(g["step1/users"]), t(g["step1/pos"]), t(g["step1/neg"]))
    return model


def _train_csr(model):
    train = model.dataset.get_user_train_dict()
    u_ptr, u_items = cm.csr_of([list(train.get(u, [])) for u in range(model.num_users)])
    i_ptr, i_users = cm.transpose_csr(u_ptr, u_items, model.num_items)
    return u_ptr, u_items, i_ptr, i_users


def test_co_items_on_an_untrained_fixture_model():
    model = _fixture("ml3", forward=False)                                   # no forward: no cached tables are needed
    u_ptr, u_items, i_ptr, i_users = _train_csr(model)
    items = np.arange(model.num_items)
    for measure in MEASURES:
        got = model.co_items(items, 10, measure)
        want = cm.topk(i_ptr, i_users, model.num_users, items, 10, measure)
        assert not got.ids.is_cuda and np.array_equal(got.ids.numpy(), want[0])
        assert got.scores.numpy().view(np.int32).tobytes() == want[1].view(np.int32).tobytes()
    users = [5, 0, model.num_users - 1, 5]
    got = model.co_users(users, 4)
    want = cm.topk(u_ptr, u_items, model.num_items, users, 4, "cosine")
    assert np.array_equal(got.ids.numpy(), want[0]) and got.scores.numpy().tobytes() == want[1].tobytes()
    with pytest.raises(IndexError):
        model.co_items([model.num_items], 3)
    with pytest.raises(ValueError):
        model.co_items([0], 257)


@pytest.mark.parametrize("view", [None, [1, 4]])
def test_co_neighbour_report(view):
    from elimrec_amd.evaluator import CoNeighbourReport, co_neighbour_columns
    from test_group_eval_gpu import _assert_1ulp
    model = _fixture("ml3", forward=True)
    train = model.dataset.get_user_train_dict()
    I, k = model.num_items, 5
    report = CoNeighbourReport(model.dataset, train, k, measure="jaccard", item_group_view=view)
    final, buf = report.evaluate(model)
    spaces = ("fused",) + tuple(model._mods)
    columns = co_neighbour_columns(model._mods)
    assert columns == ("n", "co_n", "co_score", "co_pop") + tuple("co_overlap_" + s for s in spaces)
    assert final.shape == (len(report.group_labels), len(columns)) and (len(report.group_labels) > 1) == (view is not None)
    # the numpy table formed from the device lists
    items = np.arange(I)
    co = model.co_items(items, k, "jaccard")
    lists = [model.similar_items(items, k, space=s).ids.numpy() for s in spaces]
    rows = cm.report_rows(co.ids.numpy(), co.scores.numpy(), report.item_counts, lists).astype(np.float32)
    _, _, i_ptr, i_users = _train_csr(model)
    has = cm.topk(i_ptr, i_users, model.num_users, items, 1, "count")[0][:, 0] >= 0
    assert report.has_neighbour.tolist() == has.tolist() and (rows[has, 0] >= 1).all() and (rows[~has, 0] == 0).all()
    for g, at in enumerate(report._positions):
        assert at.tolist() == [i for i in at if has[i]]
        assert final[g, 0] == at.size
        if at.size:
            want = rows[at].astype(np.float64).mean(0).astype(np.float32)
            print("group %d n=%d got %s want %s" % (g, at.size, final[g, 1:], want))
            _assert_1ulp(final[g, 1:], want, g)
        else:
            assert np.isnan(final[g, 1:]).all()
    assert final[0, 0] == has.sum() and 0 < final[0, 0]
    lines = buf.split("\n")
    assert lines[0].startswith("columns:") and all(c in lines[0] for c in columns) and len(lines) == 1 + len(report.group_labels)
    again, buf2 = report.evaluate(model)
    assert again is final and buf2 == buf                                     # kept per table version


def test_driver_switch(tmp_path):
    from test_lists_gpu import _driver
    view = ["--item_group_view=[1,4]", "--neighbour_report=3"]
    off, ev0, te0 = _driver(tmp_path / "a", view)
    assert not any("[co-neighbours]" in ln for ln in off)
    zero, ev2, te2 = _driver(tmp_path / "c", view + ["--co_report=0"])
    assert zero == off and ev0.tobytes() == ev2.tobytes() and te0.tobytes() == te2.tobytes()
    on, ev1, te1 = _driver(tmp_path / "b", view + ["--co_report=4", "--co_measure=jaccard"])
    added = [k for k, ln in enumerate(on) if ln.startswith("  [co-neighbours]")]
    assert len(added) == 1 and added[0] == len(on) - 1                       # once, after both effects' lines and [neighbours]
    assert [ln for k, ln in enumerate(on) if k not in added] == off          # every other line is as it was
    block = on[added[0]]
    assert "top-4" in block and "jaccard" in block.split("\n")[0]
    assert all(c in block for c in ("co_n", "co_score", "co_pop", "co_overlap_fused", "all:", "cold"))
    assert ev0.tobytes() == ev1.tobytes() and te0.tobytes() == te1.tobytes()
