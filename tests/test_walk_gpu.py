"""The weighted two-step walk on the device (csrc/walk.hip) against the exact host model of tests/walk_model.py, and what is built on
it: ops.walk_topk / rp3_weights, EliMRec.rp3_items / rp3_users / walk_neighbours_device, neighbour_lists / recommend_knn with source
"rp3", BaselineReport's rp3 rows, --baseline_sources=[co,rp3], torch.ops.elimrec.walk_topk.

The kernel is integer arithmetic up to one float64 expression rounded once, so nothing here has a tolerance: idx is compared exactly
and val bit for bit. The graphs of the dense form are those of tests/cooccur_cases.py (W picks the form here as it does there)."""
import numpy as np
import pytest
import torch

import cooccur_cases as cc
import cooccur_model as cm
import vote_model as vm
import walk_model as wm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HAND_USERS = [[0, 1, 2], [1, 2], [0, 2], [3]]                 # 4 users x 5 items: item 3's only user has degree 1, item 4 has no user
KINDS = {"rp3": (1.0, 0.6), "p3": (1.0, 0.0), "count": (0.0, 0.0), "steep": (4.0, 4.0)}


class Graph(object):
    """A bipartite graph from the other side's lists (user -> items): both CSRs, the index on the device, named weights."""

    def __init__(self, user_lists, n_query):
        from elimrec_amd import ops
        self.n_query, self.n_other = n_query, len(user_lists)
        self.o_ptr, self.o_nbr = cm.csr_of(user_lists)
        self.q_ptr, self.q_nbr = cm.transpose_csr(self.o_ptr, self.o_nbr, n_query)
        self.index = ops.CooccurIndex(self.q_ptr, self.q_nbr, self.o_ptr, self.o_nbr, n_query, self.n_other, DEV)
        self.walk = cm.walk(self.q_ptr, self.q_nbr, self.n_other)
        self._weights, self._want = {}, {}

    def weights(self, kind):
        """(ops.WalkWeights, its three host arrays). "rp3" / "p3" / "count" / "steep": ops.rp3_weights; "random": weights below 2^44,
        one in eight of them 0, scales in [0, 3), one in eight of them 0; "zero": every weight 0."""
        from elimrec_amd import ops
        if kind not in self._weights:
            if kind in KINDS:
                w = ops.rp3_weights(self.index, *KINDS[kind])
                host = wm.rp3_weights(np.diff(self.q_ptr), np.diff(self.o_ptr), *KINDS[kind])
                assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip((w.mid_weight, w.row_scale, w.col_scale), host))
            else:
                rng = np.random.default_rng(7)
                mid = rng.integers(1, 2 ** 44, size=self.n_other) * (rng.integers(0, 8, size=self.n_other) > 0)
                host = (mid * (kind != "zero"), rng.uniform(0.0, 3.0, self.n_query) * (rng.integers(0, 8, size=self.n_query) > 0),
                        rng.uniform(0.0, 3.0, self.n_query) * (rng.integers(0, 8, size=self.n_query) > 0))
                w = ops.WalkWeights(*host, DEV)
            self._weights[kind] = (w, host)
        return self._weights[kind]

    def want(self, rows, K, kind):
        """The model's lists: computed once per (rows, kind) at K = 256 and cut (a list's first K entries are its top-K)."""
        key = (tuple(int(r) for r in rows), kind)
        if key not in self._want:
            self._want[key] = wm.topk(self.q_ptr, self.q_nbr, self.n_other, rows, 256, *self.weights(kind)[1])
        return tuple(x[:, :K] for x in self._want[key])

    def run(self, rows, K, kind, lds=True, workspace=None):
        from elimrec_amd import ops
        Q = len(rows)
        idx = torch.full((Q, K), 77, dtype=torch.int32, device=DEV)
        val = torch.full((Q, K), 7.0, dtype=torch.float32, device=DEV)
        ops.walk_topk(self.index, np.asarray(rows, dtype=np.int64), K, self.weights(kind)[0], idx, val, lds=lds, workspace=workspace)
        return idx.cpu().numpy(), val.cpu().numpy()

    def check(self, rows, K, kind, lds=True, workspace=None):
        got = self.run(rows, K, kind, lds, workspace)
        _same(got, self.want(rows, K, kind), (kind, K, lds))
        return got


def _same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), (what, "idx")
    assert got[1].dtype == np.float32 and got[1].view(np.int32).tobytes() == want[1].view(np.int32).tobytes(), (what, "val")


_GRAPHS = {}


def _graph(name):
    if name not in _GRAPHS:
        _GRAPHS[name] = globals()["_make_" + name]() if "_make_" + name in globals() else Graph(cc.case(name).users, cc.case(name).n_query)
    return _GRAPHS[name]


def _make_hand():
    return Graph(HAND_USERS, 5)


def _make_ties():
    """300 users of degree 3 over 500 items: with beta = 0 a score is (the walks) x 3^-alpha x deg(q)^-alpha, so most scores tie."""
    rng = np.random.default_rng(11)
    return Graph([rng.choice(500, size=3, replace=False).tolist() for _ in range(300)], 500)


def _edge_shapes():
    from elimrec_amd import ops
    H = ops.WALK_SLOTS // 2
    shapes = []
    for W in (H - 1, H, H + 1):
        m = next(m for m in range(3, 64) if W % m == 0)
        shapes.append((W, m, W // m))
    return shapes


def _make_edge():
    """Items 0, 1, 2 with W = 2047, 2048, 2049: item q has m users of degree W / m, who meet at random among the other 1497 items."""
    rng = np.random.default_rng(5)
    users = []
    for q, (W, m, deg) in enumerate(_edge_shapes()):
        users += [[q] + (3 + rng.choice(1497, size=deg - 1, replace=False)).tolist() for _ in range(m)]
    return Graph(users, 1500)


def _make_repeat():
    return Graph([[0, 1, 1, 2], [0, 0, 2], [1, 2, 3]], 4)


# --------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("kind", ["rp3", "count", "random"])
def test_hand_graph(kind):
    """The row itself is left out; item 3's only user has degree 1 (a middle node that leads nowhere: fillers); item 4 is an empty
    row; a query id repeated."""
    from elimrec_amd import ops
    g = _graph("hand")
    rows = [0, 1, 2, 3, 4, 2, 0]
    for lds in (True, False):
        idx, val = g.check(rows, 3, kind, lds)
        assert sorted(idx[0].tolist()) == [-1, 1, 2] and sorted(idx[2].tolist()) == [-1, 0, 1] and idx[6].tolist() == idx[0].tolist()
        assert (idx[3] == -1).all() and (idx[4] == -1).all() and np.isneginf(val[3]).all() and np.isneginf(val[:, 2]).all()
        if kind == "rp3":                                                    # item 0: users 0 (degree 3) and 2 (degree 2)
            S = np.asarray([int(np.rint(2.0 ** 40 / 3.0)) + 2 ** 39, int(np.rint(2.0 ** 40 / 3.0))], dtype=np.int64)
            by_hand = ((S.astype(np.float64) * 2.0 ** -40) * 0.5) * np.asarray([3.0 ** -0.6, 2.0 ** -0.6])
            assert idx[0].tolist() == [2, 1, -1] and val[0, :2].tolist() == by_hand.astype(np.float32).tolist()
    # out_val is optional, an empty query launches nothing
    only = torch.empty(len(rows), 3, dtype=torch.int32, device=DEV)
    ops.walk_topk(g.index, rows, 3, g.weights(kind)[0], only)
    assert np.array_equal(only.cpu().numpy(), idx)
    assert ops.walk_topk(g.index, [], 3, g.weights(kind)[0], only) is only and np.array_equal(only.cpu().numpy(), idx)


def test_form_edge():
    """W = 2047, 2048 (the LDS form) and 2049 (the dense form): each with lds=True and lds=False, the same bits."""
    from elimrec_amd import ops
    g = _graph("edge")
    H = ops.WALK_SLOTS // 2
    assert H == 2048 and [W for W, _, _ in _edge_shapes()] == [H - 1, H, H + 1] == g.walk[:3].tolist() == g.index.walk[:3].tolist()
    assert [ops.walk_rows_in_lds(W) for W in g.walk[:3]] == [True, True, False]
    for kind in ("rp3", "random"):
        for K in (5, 256):
            for rows in ([0], [1], [2], [2, 1, 0]):
                a = g.check(rows, K, kind, lds=True)
                b = g.check(rows, K, kind, lds=False)
                _same(a, b, "the two forms")
    assert (g.want([2], 256, "rp3")[0] >= 0).all()                          # more than 256 candidates


@pytest.mark.parametrize("name", ["many_rows", "interleaved", "second_pass", "rising", "falling", "flat_desc", "wrap", "full_list", "sort_sizes"])
def test_the_cooccur_cases(name):
    """The dense form past one row and one cut per workgroup, hash chains that wrap, the list at its largest and the sort network's
    sizes (tests/cooccur_cases.py; tests/test_cooccur_cpu.py shows that the graphs do what they are named for -- W and the
    candidates' arrival order do not depend on the weights). K = 1, a K below and K = 256 at the list's longest."""
    case, g = cc.case(name), _graph(name)
    rows = list(case.rows)
    walks = g.walk[np.asarray(rows)]
    if name in ("rising", "falling", "flat_desc"):
        assert g.n_query - 1 == 5120 > 2 * cc.cap() and walks[0] > cc.cap()   # more than 2048 distinct candidates: the list is cut
    if name == "many_rows":
        assert len(rows) > 2 * cc.groups() and (walks > cc.cap()).all()     # more dense rows than workgroups
    if name == "full_list":
        assert walks.tolist() == [cc.cap()]
    for kind in ("rp3", "random"):
        for K in (1, 7, 256):
            got = g.check(rows, K, kind)
            if name not in ("many_rows", "rising", "falling", "flat_desc"):   # (those rows are dense whatever `lds` says)
                _same(g.run(rows, K, kind, lds=False), got, "the two forms")
    if name == "rising":                                                     # deg(j) falls along the arrival order: every cut raises the threshold
        idx = g.want(rows, 256, "rp3")[0]
        assert (cc.block_of(case)[idx[0]] == 4).all()


@pytest.mark.parametrize("K", [1, 64, 256])
def test_ties_are_decided_by_id(K):
    """beta = 0 and users of one degree: a score is (the number of walks) x a constant of the row, so most of a row's scores tie and
    the id decides; with K = 256 no row has that many candidates and fillers appear."""
    g = _graph("ties")
    assert (np.diff(g.o_ptr) == 3).all()
    rows = np.arange(500)
    idx, val = g.check(rows, K, "p3")
    _same(g.run(rows, K, "p3", lds=False), (idx, val), "dense form")
    if K > 1:
        tied = (val[:, :-1] == val[:, 1:]) & (idx[:, 1:] >= 0)
        assert tied.sum() > 100 and (idx[:, :-1][tied] < idx[:, 1:][tied]).all()
    if K == 256:
        assert (idx[:, -1] < 0).all() and (idx[:, 0] >= 0).any()
    g.check(rows, K, "steep")


def test_repeated_edges_are_walks_of_their_own():
    """User 0 lists item 1 twice, user 1 lists item 0 twice: item 0 reaches item 2 by 1 x 1 + 2 x 1 walks and item 1 by 1 x 2."""
    g = _graph("repeat")
    for lds in (True, False):
        idx, val = g.check([0, 1, 2, 3], 3, "count", lds)
        assert idx[0].tolist() == [2, 1, -1] and val[0].tolist() == [3.0, 2.0, -np.inf]
        assert idx[3].tolist() == [1, 2, -1] and val[3].tolist() == [1.0, 1.0, -np.inf]
        for kind in ("rp3", "random"):
            g.check([0, 1, 2, 3], 3, kind, lds)


def test_a_sum_of_zero_is_listed():
    """Weights of 0: a row one walk reaches is listed with score 0 -- the dense form marks the touched sum instead of adding --, so
    the lists hold the reachable rows in id order; and zeros among random weights and scales. The dense form runs on a caller's
    workspace, which the claims leave all zero: the mark bit of a weight of 0 is taken back with the word."""
    from elimrec_amd import ops
    g = _graph("ties")
    rows = np.arange(0, 500, 7)
    ws = torch.zeros(ops.walk_workspace(len(rows), g.n_query), dtype=torch.uint8, device=DEV)
    for lds in (True, False):
        idx, val = g.check(rows, 64, "zero", lds, workspace=None if lds else ws)
        assert not ws.any()
        count = g.want(rows, 64, "count")[0]
        assert (np.sort(np.where(count < 0, 2 ** 30, count), axis=1) == np.where(idx < 0, 2 ** 30, idx)).all()
        assert (val[idx >= 0] == 0.0).all() and (idx >= 0).sum() > 100 and (idx[:, -1] < 0).all()
        idx, val = g.check(rows, 64, "random", lds, workspace=None if lds else ws)
        assert not ws.any()
        assert (val[idx >= 0] == 0.0).any() and (val[idx >= 0] > 0.0).any()


@pytest.mark.parametrize("lds", [True, False])
def test_ids_outside_their_side(lds):
    """Through the C entry point, past the host's checks: a query id outside the side gives fillers; a neighbour id outside its side
    -- in either CSR -- is skipped. The model walks the edges that are left, each direction its own."""
    from elimrec_amd import _lib, ops
    rng = np.random.default_rng(13)
    users = [rng.choice(80, size=int(rng.integers(2, 12)), replace=False).tolist() for _ in range(60)]
    g = Graph(users, 80)
    w, host = g.weights("rp3")
    bad_q, bad_o = g.q_nbr.copy(), g.o_nbr.copy()
    bad_q[rng.choice(bad_q.size, size=25, replace=False)] = rng.choice([-1, -7, 60, 61, 2 ** 31 - 1], size=25)
    bad_o[rng.choice(bad_o.size, size=25, replace=False)] = rng.choice([-1, -7, 80, 81, 2 ** 31 - 1], size=25)
    rows = np.asarray([3, -1, 80, 79, 0, 2 ** 31 - 1, -2 ** 31, 17, 3], dtype=np.int64)
    inside = (rows >= 0) & (rows < 80)

    def kept(ptr, nbr, bound):                                               # the CSR without the entries outside [0, bound)
        ok = (nbr >= 0) & (nbr < bound)
        along = np.concatenate([[0], np.cumsum(ok)])
        return along[ptr], nbr[ok]

    K, Q = 9, rows.size
    want_idx, want_val = np.full((Q, K), -1, dtype=np.int32), np.full((Q, K), -np.inf, dtype=np.float32)
    q_kept = kept(g.q_ptr, bad_q, 60)
    want_idx[inside], want_val[inside] = wm.topk(q_kept[0], q_kept[1], 60, rows[inside], K, *host, back=kept(g.o_ptr, bad_o, 80))
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(DEV)
    dq, do, dr = t(bad_q, np.int32), t(bad_o, np.int32), t(rows, np.int32)
    idx = torch.full((Q, K), 77, dtype=torch.int32, device=DEV)
    val = torch.full((Q, K), 7.0, dtype=torch.float32, device=DEV)
    walk = torch.empty(Q, dtype=torch.int64, device=DEV)
    n_dense = 0 if lds else Q
    ws = torch.zeros(max(16, ops.walk_workspace(n_dense, 80)), dtype=torch.uint8, device=DEV)
    _lib.check(_lib.load().elimrec_walk_topk(g.index.q_ptr.data_ptr(), dq.data_ptr(), 80, g.index.o_ptr.data_ptr(), do.data_ptr(), 60,
                                             dr.data_ptr(), Q, K, w.mid_weight.data_ptr(), w.row_scale.data_ptr(), w.col_scale.data_ptr(),
                                             1 if lds else 0, n_dense, walk.data_ptr(), idx.data_ptr(), val.data_ptr(), ws.data_ptr(),
                                             ws.numel(), torch.cuda.current_stream().cuda_stream), "walk_topk")
    _same((idx.cpu().numpy(), val.cpu().numpy()), (want_idx, want_val), "ids outside")
    assert (want_idx[~inside] == -1).all() and (want_idx[inside][:, 0] >= 0).any() and not ws.any().item()
    clean = wm.topk(g.q_ptr, g.q_nbr, 60, rows[inside], K, *host)
    assert not np.array_equal(clean[0], want_idx[inside])                    # the lost edges do change the lists
    assert walk.cpu()[torch.from_numpy(~inside)].eq(0).all()


def test_both_sides_and_from_train():
    from elimrec_amd import ops
    rng = np.random.default_rng(3)
    train = {u: rng.choice(40, size=int(rng.integers(0, 9)), replace=False).tolist() for u in range(60)}
    u_ptr, u_items = cm.csr_of([train[u] for u in range(60)])
    i_ptr, i_users = cm.transpose_csr(u_ptr, u_items, 40)
    for side, (ptr, nbr, n, other) in (("item", (i_ptr, i_users, 40, 60)), ("user", (u_ptr, u_items, 60, 40))):
        index = ops.CooccurIndex.from_train(train, 60, 40, side, DEV)
        other_deg = np.bincount(nbr, minlength=other)
        assert index.deg_other.tolist() == other_deg.tolist()
        rows = np.arange(n)
        for alpha, beta in ((1.0, 0.6), (0.5, 2.0)):
            idx = torch.empty(n, 7, dtype=torch.int32, device=DEV)
            val = torch.empty(n, 7, dtype=torch.float32, device=DEV)
            ops.walk_topk(index, rows, 7, ops.rp3_weights(index, alpha, beta), idx, val)
            want = wm.topk(ptr, nbr, other, rows, 7, *wm.rp3_weights(np.diff(ptr), other_deg, alpha, beta))
            _same((idx.cpu().numpy(), val.cpu().numpy()), want, (side, alpha, beta))


@pytest.mark.parametrize("lds", [True, False])
def test_a_row_depends_on_nothing_else(lds):
    """A row's bits with its place in `rows`, with Q, and with a second call on the same workspace, which every call leaves zero."""
    from elimrec_amd import ops
    g = _graph("ties")
    rows = np.arange(500)
    need = ops.walk_workspace(500, g.n_query)
    assert need == 500 * 500 * 8
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    a = g.check(rows, 65, "rp3", lds, workspace=ws)
    assert not ws.any().item()
    _same(g.run(rows[::-1], 65, "rp3", lds, workspace=ws), tuple(x[::-1] for x in a), "reversed, on the same workspace")
    assert not ws.any().item()
    for q in (0, 17, 499):
        alone = g.run([q], 65, "rp3", lds)
        moved = g.run([3, q, 4, q], 65, "rp3", lds, workspace=ws)
        for x, y, z in zip(alone, moved, a):
            assert x[0].tobytes() == y[1].tobytes() == y[3].tobytes() == z[q].tobytes()
    if not lds:
        with pytest.raises(ValueError, match="workspace"):
            g.run(rows, 65, "rp3", lds, workspace=ws[:need - 16])


@pytest.mark.parametrize("name", ["edge", "ties", "repeat", "wrap", "rising", "interleaved"])
def test_counting_walks_gives_cooccur_topk(name):
    """alpha = beta = 0: every weight is 2^40 and every scale 1, so val == float(c): the lists of the existing kernel under "count",
    bit for bit."""
    from elimrec_amd import ops
    g = _graph(name)
    rows = np.asarray(cc.case(name).rows if name in cc.BUILDERS else np.arange(min(g.n_query, 500)), dtype=np.int64)
    for K in (1, 256):
        idx = torch.empty(rows.size, K, dtype=torch.int32, device=DEV)
        val = torch.empty(rows.size, K, dtype=torch.float32, device=DEV)
        ops.cooccur_topk(g.index, rows, K, idx, val, measure="count")
        _same(g.run(rows, K, "count"), (idx.cpu().numpy(), val.cpu().numpy()), (name, K))
    assert (idx >= 0).any().item()


def test_torch_op():
    from elimrec_amd import torch_ops
    torch_ops.load()
    g = _graph("edge")
    rows = [2, 0, 1, 7]
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(DEV)
    args = (t(g.q_ptr, np.int64), t(g.q_nbr, np.int32), t(g.o_ptr, np.int64), t(g.o_nbr, np.int32))
    for kind in ("rp3", "random"):
        w = g.weights(kind)[0]
        idx, val = torch.ops.elimrec.walk_topk(*args, t(rows, np.int32), 9, w.mid_weight, w.row_scale, w.col_scale)
        _same((idx.cpu().numpy(), val.cpu().numpy()), g.want(rows, 9, kind), kind)
    w = g.weights("rp3")[0]
    with pytest.raises(IndexError):
        torch.ops.elimrec.walk_topk(*args, t([1500], np.int32), 9, w.mid_weight, w.row_scale, w.col_scale)
    with pytest.raises(ValueError):
        torch.ops.elimrec.walk_topk(*args, t(rows, np.int32), 257, w.mid_weight, w.row_scale, w.col_scale)
    with pytest.raises(ValueError, match="overflow"):
        torch.ops.elimrec.walk_topk(*args, t(rows, np.int32), 9, w.mid_weight * 2 ** 20, w.row_scale, w.col_scale)     # 2^53 x 2049
    with pytest.raises(ValueError, match="negative"):
        torch.ops.elimrec.walk_topk(*args, t(rows, np.int32), 9, w.mid_weight - 2 ** 41, w.row_scale, w.col_scale)
    with pytest.raises(ValueError, match="finite"):
        torch.ops.elimrec.walk_topk(*args, t(rows, np.int32), 9, w.mid_weight, w.row_scale * float("inf"), w.col_scale)
    with pytest.raises(ValueError, match="one entry per"):
        torch.ops.elimrec.walk_topk(*args, t(rows, np.int32), 9, w.mid_weight[:-1], w.row_scale, w.col_scale)


# --------------------------------------------------------------------------- the model and the report
def _fixture(forward, extra=()):
    from helpers import build_model_from_fixture, load_golden
    g = load_golden("ml3")
    model, _ = build_model_from_fixture(g, DEV, extra_argv=list(extra))
    if forward:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        model.bpr_loss(t(g["step1/users"]), t(g["step1/pos"]), t(g["step1/neg"]))
    return model


def _train_csr(model):
    train = model.dataset.get_user_train_dict()
    u_ptr, u_items = cm.csr_of([list(train.get(u, [])) for u in range(model.num_users)])
    i_ptr, i_users = cm.transpose_csr(u_ptr, u_items, model.num_items)
    return u_ptr, u_items, i_ptr, i_users


def _host_rp3(ptr, nbr, n_other, rows, K, alpha, beta):
    return wm.topk(ptr, nbr, n_other, rows, K, *wm.rp3_weights(np.diff(ptr), np.bincount(nbr, minlength=n_other), alpha, beta))


def test_the_vote_scale():
    """One power of two for the block, the largest value into [0.5, 1); what the vote's 2^-24 still loses is counted."""
    from elimrec_amd.model import EliMRec
    ninf = -np.inf
    block = np.asarray([[0.75 * 2.0 ** -30, 2.0 ** -60, ninf], [2.0 ** -54, 2.0 ** -56, 0.0]], dtype=np.float32)
    val = torch.from_numpy(block.copy()).to(DEV)
    e, zero = EliMRec._vote_scale(val)
    assert (e, zero) == (30, 3 / 5) == wm.vote_scale(block)[::2]             # 2^-24 votes 1, 2^-26 rounds to 0: two tiny ones and the 0.0 are lost
    assert val.cpu().numpy().tobytes() == wm.vote_scale(block)[1].tobytes() and val[0, 0].item() == 0.75
    for flat in (np.full((2, 2), ninf, dtype=np.float32), np.zeros((2, 2), dtype=np.float32), np.asarray([[0.5, 0.25]], dtype=np.float32)):
        val = torch.from_numpy(flat.copy()).to(DEV)
        assert EliMRec._vote_scale(val) == (0, wm.vote_scale(flat)[2]) and val.cpu().numpy().tobytes() == flat.tobytes()
    val = torch.tensor([[1.5, 3.0]], device=DEV)
    assert EliMRec._vote_scale(val) == (-2, 0.0) and val.cpu().tolist() == [[0.375, 0.75]]


def test_rp3_items_and_recommend_knn_on_an_untrained_fixture_model():
    model = _fixture(forward=False)                                          # no forward: no cached tables are needed
    u_ptr, u_items, i_ptr, i_users = _train_csr(model)
    I, U = model.num_items, model.num_users
    items = np.arange(I)
    for alpha, beta in ((1.0, 0.6), (0.5, 0.0), (4.0, 4.0)):
        got = model.rp3_items(items, 10, alpha, beta)
        want = _host_rp3(i_ptr, i_users, U, items, 10, alpha, beta)
        assert not got.ids.is_cuda
        _same((got.ids.numpy(), got.scores.numpy()), want, ("items", alpha, beta))
    got = model.rp3_items(items, 10)                                         # the defaults
    _same((got.ids.numpy(), got.scores.numpy()), _host_rp3(i_ptr, i_users, U, items, 10, 1.0, 0.6), "defaults")
    users = [5, 0, U - 1, 5]
    got = model.rp3_users(users, 4)
    _same((got.ids.numpy(), got.scores.numpy()), _host_rp3(u_ptr, u_items, I, users, 4, 1.0, 0.6), "users")
    with pytest.raises(IndexError):
        model.rp3_items([I], 3)
    # the neighbour lists: one power of two, then the votes
    train = model.dataset.get_user_train_dict()
    hist = [list(train.get(u, [])) for u in range(U)]
    ask = list(range(0, U, 3)) + [1, 1]
    for Kn, alpha, beta in ((50, 1.0, 0.6), (4, 1.0, 0.6), (6, 4.0, 4.0)):
        near_idx, near_val = _host_rp3(i_ptr, i_users, U, items, Kn, alpha, beta)
        e, scaled, zero_votes = wm.vote_scale(near_val)
        lists = model.neighbour_lists("rp3", Kn, alpha=alpha, beta=beta)
        print("Kn %d alpha %g beta %g: scale 2^%d zero_votes %.6f" % (Kn, alpha, beta, lists.scale_exp, lists.zero_votes))
        assert (lists.scale_exp, lists.zero_votes) == (e, zero_votes)
        _same((lists.idx.cpu().numpy(), lists.val.cpu().numpy()), (near_idx, scaled), "lists")
        assert 0.5 <= scaled[np.isfinite(scaled)].max() < 1.0
        got = model.recommend_knn(ask, 20, neighbours=Kn, source="rp3", alpha=alpha, beta=beta)
        want = vm.topk(near_idx, scaled, hist, ask, 20)
        assert all(np.array_equal(a.numpy(), b) for a, b in zip(got, want)) and (got.ids >= 0).any()
        assert model.neighbour_lists("rp3", Kn, alpha=alpha, beta=beta) is lists                       # kept per (neighbours, alpha, beta)
    assert model.neighbour_lists("rp3", 4, alpha=1.0, beta=0.5) is not model.neighbour_lists("rp3", 4)
    co = model.neighbour_lists("co", 4)
    assert (co.scale_exp, co.zero_votes) == (0, None)
    assert model.neighbour_lists("co", 4, alpha=-1.0) is co                  # read by "rp3" alone


@pytest.mark.parametrize("effect", ["TE", "TIE"])
def test_the_baseline_report_with_rp3(effect):
    model = _fixture(True, ["--baseline_report=20", "--baseline_sources=[co,rp3]", "--baseline_neighbours=7", "--group_view=[2,4]",
                            "--significance_report=50", "--baseline_beta=0.4"])
    model.predict_type = effect
    rep, sig = model.baseline_reporter, model.significance_reporter
    assert (rep.alpha, rep.beta) == (1.0, 0.4)
    final, buf = rep.evaluate(model)
    G = len(rep.group_labels)
    assert final.table.shape == (2 * G, len(rep.columns)) and final.labels[G].startswith("rp3 all:")
    u_ptr, u_items, i_ptr, i_users = _train_csr(model)
    near_idx, near_val = _host_rp3(i_ptr, i_users, model.num_users, np.arange(model.num_items), 7, 1.0, 0.4)
    e, scaled, zero_votes = wm.vote_scale(near_val)
    train = model.dataset.get_user_train_dict()
    want_lists = vm.topk(near_idx, scaled, [list(train.get(u, [])) for u in rep.users], range(len(rep.users)), 20)[0]
    assert np.array_equal(rep.knn_lists(model, "rp3").cpu().numpy(), want_lists) and (want_lists >= 0).any()
    assert rep.rp3_info == (e, zero_votes)
    lines = buf.split("\n")
    assert len(lines) == 1 + 2 * G + 1 and lines[1 + G].startswith("rp3 all:") and lines[1].startswith("co all:")
    assert lines[-1] == "rp3: alpha=1 beta=0.4 scale=2^%d zero_votes=%.6f" % (e, zero_votes)
    overlap = final.table[G:, rep.columns.index("overlap")]
    assert ((overlap >= 0.0) & (overlap <= 1.0)).all()
    rows, columns = rep.metric_rows(model, "rp3")
    shift, text = sig.shift((rows, columns), sig.metric_rows(model))         # model - rp3, paired per user
    assert shift.p is not None and "all: mean" in text
    # the same report without rp3 reads as before: the co rows, and no line under the table
    alone = _fixture(True, ["--baseline_report=20", "--baseline_sources=[co]", "--baseline_neighbours=7", "--group_view=[2,4]"])
    alone.predict_type = effect
    final0, buf0 = alone.baseline_reporter.evaluate(alone)
    assert buf0.split("\n") == lines[:1 + G] and final0.table.tobytes() == final.table[:G].tobytes()


def test_driver_switch(tmp_path):
    from test_lists_gpu import _driver
    base = ["--baseline_report=10", "--baseline_neighbours=5", "--significance_report=20"]
    off, ev0, te0 = _driver(tmp_path / "a", base + ["--baseline_sources=[co]"])
    assert not any("rp3" in ln for ln in off)
    on, ev1, te1 = _driver(tmp_path / "b", base + ["--baseline_sources=[co,rp3]"])
    paired = [k for k, ln in enumerate(on) if ln.startswith("  [TE - rp3] metric difference") or ln.startswith("  [TIE - rp3] metric difference")]
    tables = [k for k, ln in enumerate(on) if "[baselines]" in ln.split("\n")[0]]
    assert len(paired) == 2 and len(tables) == 2 and [k for k, ln in enumerate(off) if "[baselines]" in ln.split("\n")[0]] == [k - i for i, k in enumerate(tables)]
    for k in tables:
        block = on[k].split("\n")
        rp3 = [ln for ln in block if ln.startswith("rp3")]
        assert len(rp3) == 2 and rp3[0].startswith("rp3 all:") and block[-1] == rp3[1] and rp3[1].startswith("rp3: alpha=1 beta=0.6 scale=2^")
        assert "zero_votes=" in rp3[1]
        assert block[1].startswith("columns:\t") and block[2].startswith("co all:")
        header = [c.strip() for c in block[1].split("\t")[1:]]
        cells = [float(c) for c in rp3[0].split("\t")[1:]]
        assert len(cells) == len(header) and 0.0 <= cells[header.index("overlap")] <= 1.0
        on[k] = "\n".join(ln for ln in block if not ln.startswith("rp3"))    # without the rp3 row and line: the run without rp3
    assert [ln for k, ln in enumerate(on) if k not in paired] == off
    assert ev0.tobytes() == ev1.tobytes() and te0.tobytes() == te1.tobytes()
