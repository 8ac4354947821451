"""New users on the device: ops.segment_row_sum (csrc/foldin.hip) against the float64 model of tests/foldin_model.py within the
bound float64 accumulation and one rounding give, its independence of the batch, its tie to the propagation kernel,
EliMRec.fold_in_users against an all-float64 restatement, the readers over the handle against the catalogue's own readers, and
the report with its switch.

Kernel bound per element: |got - want| <= 2^-23 |want| + n 2^-50 sum_j |w_j x_j| (the model's own float64 error sits inside the
second term: both sums are within n 2^-53 of the exact one)."""
import numpy as np
import pytest
import torch

import foldin_cases as fc
import foldin_model as fm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _chunk():
    from elimrec_amd import ops
    return ops.FOLDIN_CHUNK


def _run(buf, C, ptr, rows, w, row_offset=0):
    from elimrec_amd import ops
    table = _t(buf)[:, :C]
    out = torch.full((len(ptr) - 1, C), float("nan"), dtype=torch.float32, device=DEV)
    assert ops.segment_row_sum(table, ptr, rows, w, out, row_offset=row_offset) is out
    return out


# --------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("C", [8, 256, 320, 1280])
@pytest.mark.parametrize("family", fc.FAMILIES)
def test_segment_row_sum_against_float64(family, C):
    """Every list length around one chunk and around one round of the four waves in one call, repeated ids, a padded table whose
    padding holds NaN and a row offset (C = 320 / 1280: more than one column pass, the last one ragged at 320)."""
    chunk = _chunk()
    rng = np.random.default_rng(1000 * fc.FAMILIES.index(family) + C)
    pad, off = (0, 4)[C % 16 == 0 and C != 256], (0, 5)[C != 8]
    buf, ptr, rows, w = fc.make(family, C, chunk, rng, pad=pad, row_offset=off)
    lens = np.diff(ptr).tolist()
    assert lens == [1, chunk - 1, 0, chunk, chunk + 1, 4 * chunk - 1, 4 * chunk, 4 * chunk + 1]
    want, bound, _ = fm.segment_row_sum(buf[:, :C], ptr, rows, w, row_offset=off)
    got = _run(buf, C, ptr, rows, w, off).double().cpu().numpy()
    assert np.isfinite(got).all() and not got[2].any()                # (an empty list: zeros; a padding column read: NaN)
    err = np.abs(got - want)
    assert (err <= bound).all(), (family, C, np.argwhere(err > bound)[:4].tolist(), float((err / np.maximum(bound, 1e-300)).max()))


@pytest.mark.parametrize("Q", [1, 5])
def test_segment_row_sum_small_batches(Q):
    chunk = _chunk()
    rng = np.random.default_rng(Q)
    C, n_rows = 64, 23
    buf = fc.table("unit", n_rows, C, C, rng)
    ptr, rows, w = fc.lists("unit", [chunk + 3, 0, 2, 4 * chunk + 2, 1][:Q], n_rows, rng)
    want, bound, _ = fm.segment_row_sum(buf, ptr, rows, w)
    err = np.abs(_run(buf, C, ptr, rows, w).double().cpu().numpy() - want)
    assert (err <= bound).all()


def test_a_list_alone_equals_the_list_inside_the_batch():
    """A list's bits depend on its own entries, C and the table alone: every list of a batch, run as a batch of one, gives the
    rows of the batch call; a second call gives the same bits; device tensors and host arrays give the same call."""
    from elimrec_amd import ops
    chunk = _chunk()
    for C in (8, 320):
        rng = np.random.default_rng(C)
        buf, ptr, rows, w = fc.make("spread", C, chunk, rng)
        whole = _run(buf, C, ptr, rows, w)
        assert torch.equal(whole.view(torch.int32), _run(buf, C, ptr, rows, w).view(torch.int32))
        for q in range(len(ptr) - 1):
            lo, hi = int(ptr[q]), int(ptr[q + 1])
            alone = _run(buf, C, np.array([0, hi - lo]), rows[lo:hi], w[lo:hi])
            assert np.array_equal(alone.cpu().numpy().view(np.int32), whole[q:q + 1].cpu().numpy().view(np.int32)), (C, q)
        out = torch.empty_like(whole)
        ops.segment_row_sum(_t(buf)[:, :C], _t(ptr), _t(rows), _t(w), out)
        assert torch.equal(out.view(torch.int32), whole.view(torch.int32))


def test_segment_row_sum_refuses_on_the_host():
    from elimrec_amd import _lib, ops
    table = torch.zeros(6, 8, device=DEV)
    out = torch.full((2, 8), 7.0, device=DEV)
    rows, w = np.array([0, 5, 1], dtype=np.int32), np.ones(3, dtype=np.float32)
    calls = []
    _lib.record(calls)
    try:
        for ptr in ([0, 2, 1], [0, 3], [0, 1, 2], [1, 2, 3]):         # not ascending; Q + 1 entries; not to len(rows); not from 0
            with pytest.raises(ValueError):
                ops.segment_row_sum(table, ptr, rows, w, out)
        for bad in ([0, 6, 1], [0, -1, 1]):
            with pytest.raises(IndexError):
                ops.segment_row_sum(table, [0, 2, 3], np.array(bad, dtype=np.int32), w, out)
        with pytest.raises(IndexError):
            ops.segment_row_sum(table, [0, 2, 3], rows, w, out, row_offset=1)       # 5 is outside the window now
        with pytest.raises(IndexError):
            ops.segment_row_sum(table, [0, 2, 3], rows, w, out, row_offset=7)
        for bad in (np.array([1, np.inf, 1], dtype=np.float32), np.array([1, np.nan, 1], dtype=np.float32), w[:2]):
            with pytest.raises(ValueError):
                ops.segment_row_sum(table, [0, 2, 3], rows, bad, out)
        with pytest.raises(ValueError):
            ops.segment_row_sum(torch.zeros(6, 6, device=DEV), [0, 2, 3], rows, w, torch.zeros(2, 6, device=DEV))      # C % 4
        with pytest.raises(ValueError):
            ops.segment_row_sum(torch.zeros(6, 1284, device=DEV), [0, 2, 3], rows, w, torch.zeros(2, 1284, device=DEV))
        with pytest.raises(ValueError):
            ops.segment_row_sum(torch.zeros(6, 9, device=DEV)[:, :8], [0, 2, 3], rows, w, out)                          # row stride
        with pytest.raises(ValueError):
            ops.segment_row_sum(table, [0, 2, 3], rows, w, out[:, :4])
        empty = torch.empty(0, 8, device=DEV)
        assert ops.segment_row_sum(table, [0], rows[:0], w[:0], empty) is empty                                        # Q = 0
    finally:
        _lib.record(None)
    assert not calls and (out.cpu() == 7).all()                       # every refusal and Q = 0: no launch


def test_torch_op_equals_the_ctypes_binding():
    from elimrec_amd import torch_ops
    chunk = _chunk()
    rng = np.random.default_rng(9)
    buf, ptr, rows, w = fc.make("unit", 320, chunk, rng, pad=4, row_offset=3)
    want = _run(buf, 320, ptr, rows, w, 3)
    t = torch_ops.load()
    got = t.segment_row_sum(_t(buf)[:, :320], _t(ptr), _t(rows), _t(w), 3)
    assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), want.view(torch.int32))
    with pytest.raises(IndexError):
        t.segment_row_sum(_t(buf)[:, :320], _t(ptr), _t(rows + 37), _t(w), 3)
    with pytest.raises(RuntimeError):
        t.segment_row_sum(_t(buf)[:, :320], _t(ptr[::-1].copy()), _t(rows), _t(w), 3)
    with pytest.raises(RuntimeError):
        t.segment_row_sum(_t(buf)[:, :320], _t(ptr), _t(rows), _t(np.where(np.arange(w.size) == 3, np.inf, w).astype(np.float32)), 3)


# --------------------------------------------------------------------------- the fold-in
_MODELS = {}


def _model(name="ml3", d=8, adj=None, propagation=None, stepped=False, tag=None):
    """A small model over a golden fixture's graph and features (random seeded parameters), after compute() -- or, stepped, after
    one bpr_loss + backward + optimizer.step(): (model, the state dict the cached tables were built with)."""
    key = (name, d, adj, propagation, stepped, tag)                   # tag: a second model of the same kind
    if key in _MODELS:
        return _MODELS[key]
    from elimrec_amd import EliMRec, FusedAdam
    from helpers import FixtureDataset, fixture_argv, load_golden, make_config
    g = load_golden(name)
    drop = ("--recdim=", "--layer_num=") + (("--adj_type=",) if adj else ())
    argv = [a for a in fixture_argv(g) if not a.startswith(drop)] + ["--recdim=%d" % d, "--layer_num=3"]
    argv += ["--adj_type=%s" % adj] if adj else []
    argv += ["--propagation=%s" % propagation] if propagation else []
    torch.manual_seed(7)
    model = EliMRec(make_config(argv), FixtureDataset(g)).to(DEV)
    W = {k: v.detach().double().cpu().numpy() for k, v in model.state_dict().items()}
    if stepped:
        opt = FusedAdam(model.parameters(), lr=float(g["lr"]), weight_decay=float(g["weight_decay"]))
        loss = model.bpr_loss(_t(g["step1/users"]), _t(g["step1/pos"]), _t(g["step1/neg"]))
        opt.zero_grad()
        loss.backward(retain_graph=True)
        opt.step()
    else:
        with torch.no_grad():
            model.compute()
    _MODELS[key] = (model, W)
    return _MODELS[key]


def _histories(model, rng, n=9):
    I = model.num_items
    train = model.dataset.get_user_train_dict()
    own = [list(train[u]) for u in list(train)[:3]]
    return own + [[], [int(rng.integers(I))], [3, 3, 5, 3]] + [rng.integers(0, I, size=int(rng.integers(2, 40))).tolist() for _ in range(n - 6)]


@pytest.mark.parametrize("adj,propagation,stepped", [("pre", None, False), ("pre", "full", False), ("pre", None, True), ("plain", None, False),
                                                     ("gcmc", "bipartite", False), ("norm", None, False), ("mean", None, False)])
def test_fold_in_users_against_float64(adj, propagation, stepped):
    """Weights, sum, id term, user fusion Linear and heads restated in float64 from the float32 inputs (the cached layer-mean table,
    the weights the tables were built with), for every adjacency, the folded form and the unfolded ones, and after a training step
    (the copy of the weights taken before the update). Bound: the projections' (tests/test_coldstart_gpu.py), with OutNew's own error
    carried through |W|."""
    from elimrec_amd import reports
    model, W = _model(adj=adj, propagation=propagation, stepped=stepped)
    assert model._folded == (adj in ("pre", "plain", "gcmc") and propagation is None)
    U, d, L = model.num_users, model.latent_dim, model.n_layers
    rng = np.random.default_rng(3)
    hist = _histories(model, rng)
    ptr, items = fm.csr(hist)
    deg = reports.item_train_counts(model.dataset.get_user_train_dict(), model.num_items)
    for id_rows in (None, rng.standard_normal((len(hist), d)).astype(np.float32)):
        new = model.fold_in_users(hist, id_rows=id_rows)
        assert len(new) == len(hist) and new.table.shape == (len(hist) + model.num_items, model.Cy) and new.version == model._table_version
        out_items = model._ws["Out"][U:].double().cpu().numpy()
        ids = np.zeros((len(hist), d)) if id_rows is None else id_rows
        want, bound, out, out_bound = fm.fold_in_rows(out_items, ptr, items, fm.weights(adj, ptr, items, deg), ids,
                                                      fm.isolated_row_scale(adj, L), W, model._mods, d, model.mm_fusion_mode)
        err = np.abs(new.layer_mean.double().cpu().numpy() - out)
        assert (err <= out_bound).all(), (adj, "OutNew", float((err / out_bound).max()))
        err = np.abs(new.rows.double().cpu().numpy() - want)
        assert (err <= bound).all(), (adj, propagation, stepped, float((err / bound).max()))
        assert torch.equal(new.table[len(hist):].view(torch.int32), model._ws["Y"][U:].view(torch.int32))
        assert new.hist_ptr.cpu().tolist() == ptr.tolist() and new.hist_items[:items.size].cpu().tolist() == items.tolist()
    if stepped:                                                       # the stepped weights would give other rows: the copy matters
        live = {k: v.detach().double().cpu().numpy() for k, v in model.state_dict().items()}
        other = fm.fold_in_rows(out_items, ptr, items, fm.weights(adj, ptr, items, deg), ids, fm.isolated_row_scale(adj, L), live,
                                model._mods, d, model.mm_fusion_mode)[0]
        assert (np.abs(other - want) > 2 * bound).any()


def test_out_new_against_the_propagation_kernel():
    """'pre', training users folded in with their own histories: OutNew's row is row u of one hop over the layer-mean table,
    sum_i A[u, U + i] Out[U + i] -- there an fp32 sum of fp32 adjacency values, here float64 with the weights of
    reports.fold_in_weights. Bound: the fp32 sum's, n 2^-23 sum |w x|, for the users with n >= 3, where the weights' own rounding
    fits inside it. The two sides' weights differ by up to 2^-23 relative (tests/test_foldin_cpu.py): for n = 1 and 2 that one ulp is
    added, (n + 1) 2^-23 sum |w x| (weights 1, the hop's n products and n - 1 adds 1/2 each, this side's rounding 1/2 ulp)."""
    from elimrec_amd import ops, reports
    from elimrec_amd.model import create_adj_mat
    from helpers import load_golden
    model, _ = _model(adj="pre")
    g = load_golden("ml3")
    U, I, C = model.num_users, model.num_items, model.C
    Out = model._ws["Out"]
    csr = ops.Csr.from_scipy(create_adj_mat(g["train_u"], g["train_i"], U, I, "pre"), DEV, C=C)
    hop = torch.full_like(Out, float("nan"))
    ops.spmm_hop(csr, Out.contiguous(), Xout=hop)
    train = model.dataset.get_user_train_dict()
    distinct = [u for u in train if len(set(train[u])) == len(train[u])]
    short = [u for u in distinct if 1 <= len(train[u]) <= 2][:6]
    users = [u for u in distinct if len(train[u]) >= 3][:12] + short
    assert len(users) - len(short) >= 4 and len(short) >= 1
    ptr, items = fm.csr([train[u] for u in users])
    w = reports.fold_in_weights("pre", ptr, items, reports.item_train_counts(train, I))
    got = torch.empty(len(users), C, device=DEV)
    ops.segment_row_sum(Out, ptr, items.astype(np.int32), w, got, row_offset=U)
    mag = fm.segment_row_sum(Out[U:].double().cpu().numpy(), ptr, items, w)[2]
    err = np.abs(got.double().cpu().numpy() - hop[_t(np.asarray(users))].double().cpu().numpy())
    n = np.diff(ptr)[:, None]
    bound = np.where(n >= 3, n, n + 1) * 2.0 ** -23 * mag
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    new = model.fold_in_users([train[u] for u in users])
    assert torch.equal(new.layer_mean.view(torch.int32), got.view(torch.int32))


def test_fold_in_front_end():
    from elimrec_amd import _lib
    from elimrec_amd.ops import CandidateScoringError
    model, _ = _model()
    rng = np.random.default_rng(5)
    hist = _histories(model, rng, n=12)
    ids = rng.standard_normal((len(hist), model.latent_dim)).astype(np.float32)
    many = model.fold_in_users(hist, id_rows=ids)
    for q in (0, 3, 5, 11):                                           # one user or a batch: the same bits
        one = model.fold_in_users([hist[q]], id_rows=ids[q:q + 1])
        assert torch.equal(one.rows.view(torch.int32), many.rows[q:q + 1].view(torch.int32)), q
    # an empty history: OutNew = kappa x0; without id rows the rows come from the biases alone
    bare = model.fold_in_users([[]])
    assert not bare.layer_mean.any()
    W = model._table_W
    bias = torch.cat([W["embedding_user_after_GCN.bias"]] + [W["s_dense_%s.bias" % m] for m in model._mods])
    assert torch.equal(bare.rows[0].view(torch.int32), bias.view(torch.int32))
    from elimrec_amd import reports
    kappa = reports.isolated_row_scale("pre", model.n_layers)
    assert torch.equal(many.layer_mean[3], (_t(ids[3]) * kappa).repeat(model.C // model.latent_dim))
    # id_rows="mean": the mean embedding_user row of the users with a training interaction, for every new user
    mean = model.mean_user_id_row()
    train = model.dataset.get_user_train_dict()
    active = sorted(u for u in train if len(train[u]))
    want = model.embedding_user.weight.detach()[_t(np.asarray(active))].double().mean(0).float()
    assert torch.equal(mean.view(torch.int32), want.view(torch.int32))
    a = model.fold_in_users(hist, id_rows="mean")
    b = model.fold_in_users(hist, id_rows=mean.expand(len(hist), -1).cpu().numpy())
    assert torch.equal(a.rows.view(torch.int32), b.rows.view(torch.int32))
    calls = []
    _lib.record(calls)
    try:
        for bad in ([[0, model.num_items]], [[-1]]):
            with pytest.raises(IndexError):
                model.fold_in_users(bad)
        for kw in (dict(id_rows=ids[:, :4]), dict(id_rows=ids[:5]), dict(id_rows=ids * np.float32("inf")), dict(id_rows="median")):
            with pytest.raises(ValueError):
                model.fold_in_users(hist, **kw)
        empty = model.fold_in_users([])
    finally:
        _lib.record(None)
    assert not calls and len(empty) == 0 and empty.rows.shape == (0, model.Cy)   # the refusals and Q = 0: no launch
    assert model.predict_new_users(empty).shape == (0, model.num_items)
    assert model.recommend_new_users(empty, 3)[0].shape == (0, 3)
    assert model.similar_users_to_new(empty, 3).ids.shape == (0, 3)
    with pytest.raises(TypeError):
        model.predict_new_users(many.rows)
    # a stale handle
    twin, _ = _model(tag="twin")
    old = twin.fold_in_users(hist[:2])
    with torch.no_grad():
        twin.compute()
    with pytest.raises(RuntimeError, match="fold_in_users"):
        twin.predict_new_users(old)
    # item-sharded / lean tables are refused
    twin._lean = True
    try:
        with pytest.raises(CandidateScoringError):
            twin.fold_in_users(hist[:2])
    finally:
        twin._lean = False


# --------------------------------------------------------------------------- the readers
def test_predict_new_users_is_the_scorer_over_the_handle():
    from elimrec_amd import ops
    model, _ = _model()
    rng = np.random.default_rng(8)
    hist = _histories(model, rng)
    new = model.fold_in_users(hist, id_rows="mean")
    Q, U, I, d = len(hist), model.num_users, model.num_items, model.latent_dim
    try:
        for ptype in ("normal", "TE", "TIE"):
            model.predict_type = ptype
            got = model.predict_new_users_device(new, torch.empty(Q, I, device=DEV))
            table = torch.cat((new.rows, model._ws["Y"][U:]), 0).contiguous()
            sqn = ops.row_sqnorms(table, d, 1 + model.S, torch.empty(Q + I, 1 + model.S, device=DEV))
            ws = torch.empty(ops.score_workspace(Q, Q, I, model.S, 1, topk_only=False, d=d), dtype=torch.uint8, device=DEV)
            want = torch.empty(Q, I, device=DEV)
            ops.score_topk(table, Q, I, torch.arange(Q, device=DEV), d, model.S, model._head_mask(), model.fusion_mode, ptype, ws,
                           scores=want, sqnorm=sqn)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), ptype
            assert torch.equal(model.predict_new_users(new).view(torch.int32), want.cpu().view(torch.int32))
    finally:
        model.predict_type = "TIE"


def test_a_handle_holding_cached_user_rows_scores_as_predict():
    """The handle's rows overwritten with the cached rows of trained users: the readers give what the catalogue's readers give
    those users, bit for bit, under every predict type."""
    from elimrec_amd import ops
    model, _ = _model()
    users = [2, 0, 7, 11]
    train = model.dataset.get_user_train_dict()
    new = model.fold_in_users([list(train[u]) for u in users])
    new.table[:len(users)] = model._ws["Y"][_t(np.asarray(users))]
    ops.row_sqnorms(new.table, model.latent_dim, 1 + model.S, new.sqn)
    try:
        for ptype in ("normal", "TE", "TIE"):
            model.predict_type = ptype
            assert torch.equal(model.predict_new_users(new).view(torch.int32), model.predict(users).view(torch.int32)), ptype
            excl = {u: train[u] for u in users}
            idx, val = model.predict_device(_t(np.asarray(users)), top_k=6, train_ptr=new.hist_ptr, train_items=new.hist_items)
            ids, scores = model.recommend_new_users(new, 6)
            assert torch.equal(ids, idx.cpu()) and torch.equal(scores.view(torch.int32), val.cpu().view(torch.int32)), ptype
            items = [[1, 4, train[u][0]] for u in users]
            assert torch.equal(model.rank_items_for_new_users(new, items), model.rank_items(users, items, exclude=excl)), ptype
    finally:
        model.predict_type = "TIE"
    near = model.similar_users_to_new(new, 5)
    own = model.similar_users(users, 4)
    for q, u in enumerate(users):                                     # the trained user itself (cosine 1), then its own neighbours
        rest = [int(i) for i in near.ids[q].tolist() if i != u]
        assert u in near.ids[q].tolist() and rest[:4] == own.ids[q].tolist(), q
    assert int(near.ids.max()) < model.num_users


def test_recommend_new_users_masks_the_history():
    model, _ = _model()
    I = model.num_items
    hist = [[3, 3, 5, 3], [], [0, 1, 2], [7]]
    new = model.fold_in_users(hist, id_rows="mean")
    scores = model.predict_new_users(new).numpy()
    for k in (1, 9, min(256, I)):
        ids, val = model.recommend_new_users(new, k)
        open_ids, _ = model.recommend_new_users(new, k, exclude_history=False)
        more, _ = model.recommend_new_users(new, k, exclude={1: [4, 4], 3: [8]})
        for q, h in enumerate(hist):
            for masked, got in ((set(h), ids), (set(), open_ids), (set(h) | {1: {4}, 3: {8}}.get(q, set()), more)):
                row = scores[q].astype(np.float64).copy()
                row[list(masked)] = -np.inf
                order = np.lexsort((np.arange(I), -row))[:k]
                keep = row[order] > -np.inf                             # (k beyond the unmasked catalogue: the fillers are not compared)
                assert got[q].numpy()[keep].tolist() == order[keep].tolist(), (k, q)
            assert not set(ids[q].tolist()[:min(k, I - len(set(h)))]) & set(h)
            n_open = min(k, I - len(set(h)))
            assert np.array_equal(val[q].numpy()[:n_open], scores[q][ids[q].numpy()[:n_open]])
    ref_ids, _ = model.recommend_new_users(new, 5, tie_order="reference")
    assert ref_ids.shape == (4, 5)
    for bad in (0, I + 1, 257):
        with pytest.raises(ValueError):
            model.recommend_new_users(new, bad)
    with pytest.raises(ValueError):
        model.recommend_new_users(new, 3, tie_order="random")
    with pytest.raises(IndexError):
        model.recommend_new_users(new, 3, exclude={0: [I]})
    with pytest.raises(ValueError):
        model.similar_users_to_new(new, 0)
    with pytest.raises(ValueError):
        model.rank_items_for_new_users(new, [[0]])
    ranks = model.rank_items_for_new_users(new, [[3, 6], [2], [], [7, 0, 1]])
    assert ranks.shape == (4, 3) and ranks[0, 0] == -1 and ranks[3, 0] == -1 and ranks[2].tolist() == [-1, -1, -1]
    row = scores[1].astype(np.float64)
    assert int(ranks[1, 0]) == int(((row > row[2]) | ((row == row[2]) & (np.arange(I) < 2))).sum())


# --------------------------------------------------------------------------- the report
def test_newuser_report():
    from elimrec_amd import reports
    from elimrec_amd.evaluator import NEWUSER_VARIANTS, NewUserReport, UniEvaluator
    model, _ = _model()
    assert model.newuser_reporter is None                             # the switch is off by default
    ds = model.dataset
    train, test = ds.get_user_train_dict(), ds.get_user_test_dict()
    ks, k, d = [5, 20], 5, model.latent_dim
    rep = NewUserReport(ds, train, test, ks, group_view=[2, 4, 40], metric=["Recall"], k=k)
    rep.block_users = 16                                              # several user blocks
    assert rep.users == list(test.keys()) and len(rep.users) > 16 and len(rep.group_labels) > 1
    model.predict_type = "TIE"
    rows, lists = rep.user_rows(model)
    final, buf = rep.evaluate(model, rows)
    G, V, Cs = len(rep.group_labels), 3, len(ks)
    assert final.shape == (G, V, 1 + Cs + 2) and all((v + ":") in buf for v in NEWUSER_VARIANTS) and "Recall@20" in buf and buf.startswith("all:\n")
    assert rep.columns == ("users", "Recall@5", "Recall@20", "overlap", "cos")
    # trained: UniEvaluator.evaluate's own numbers, bit for bit (the all: block's metric columns are the evaluator's overall
    # expression over the same per-user rows); the group blocks are the float64 means of the evaluator's rows, rounded once
    ev = UniEvaluator(ds, train, test, metric=["Recall"], top_k=ks)
    ev.tie_order = rep.tie_order
    assert np.asarray(ev.evaluate(model)[0], dtype=np.float32).tobytes() == final[0, 0, 1:1 + Cs].tobytes()
    per_user = ev.metric_rows(model, rep.users).double().cpu().numpy()
    shown = per_user.reshape(len(rep.users), 1, ev.max_top)[:, :, ev.top_show - 1].reshape(len(rep.users), -1)
    for g, at in enumerate(rep._positions[1:], 1):
        assert np.allclose(final[g, 0, 1:1 + Cs], shown[at].mean(0), rtol=2.0 ** -23, atol=0), g
    assert (final[:, 0, 1 + Cs] == 1.0).all() and (np.abs(final[:, 0, 2 + Cs] - 1.0) <= 2.0 ** -22).all()
    assert final[:, 0, 0].tolist() == [float(p.size) for p in rep._positions] and (final[:, 1, 0] == final[:, 0, 0]).all()
    # history / history+mean_id: the numpy model on the device's lists and rows
    own_rows = model._ws["Y"][_t(np.asarray(rep.users)), :d].double().cpu().numpy()
    host_lists = lists.cpu().numpy()
    truth = [test[u] for u in rep.users]
    for v, id_rows in ((0, None), (1, None), (2, "mean")):
        fused = own_rows if v == 0 else model.fold_in_users([train[u] for u in rep.users], id_rows=id_rows).rows[:, :d].double().cpu().numpy()
        want_rows = fm.user_rows(fm.metrics_at(host_lists[v], truth, ks), host_lists[0], host_lists[v], k, own_rows, fused)
        assert np.allclose(rows[v].double().cpu().numpy(), want_rows, rtol=2.0 ** -23, atol=2.0 ** -24), v
        want = fm.table(want_rows, rep._positions)
        # (all: block, metric columns: the float32 mean of the float32 rows in user order, as the evaluator takes it -- the same bits)
        overall = np.mean(want_rows[:, :Cs].astype(np.float32), axis=0)
        assert overall.tobytes() == final[0, v, 1:1 + Cs].tobytes(), (v, overall, final[0, v])
        want[0, 1:1 + Cs] = overall
        assert np.allclose(final[:, v], want, rtol=2.0 ** -22, atol=2.0 ** -24), (v, final[:, v], want)
        if v:
            ids, _ = model.recommend_new_users(model.fold_in_users([train[u] for u in rep.users], id_rows=id_rows), 20, tie_order=rep.tie_order)
            assert np.array_equal(ids.numpy(), host_lists[v])         # the report's lists are the public reader's
    assert (final[0, 1:, 1 + Cs] < 1.0).all()                         # folding in does change the lists of this fixture
    delta, dbuf = rep.shift(final, final)
    assert not delta.any() and "d_Recall@5" in dbuf and "d_users" not in dbuf
    none = NewUserReport(ds, {}, test, ks)
    assert none.evaluate(model) == (None, reports.format_newuser(None, None, None))


def _net(tmp_path, extra):
    import importlib
    import os
    import sys
    from helpers import ROOT
    sys.path.insert(0, ROOT)
    main = importlib.import_module("main")
    from elimrec_amd import Configurator, set_seed
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        args = Configurator(os.path.join(ROOT, "NeuRec.properties"), default_section="hyperparameters",
                            argv=["main.py", "--data.input.dataset=synthetic", "--alpha=0.5", "--synthetic_shape=[60,200,1200]",
                                  "--synthetic_dims=[16,8,12]", "--recdim=32", "--loss=bpr_loss", "--batch_size=512", "--num_epoch=2",
                                  "--test_step=1", "--verbose=0", "--save_flag=0", "--path=%s" % str(tmp_path / "ck")] + list(extra))
        set_seed(args["seed"])
        return main.Net(args)
    finally:
        os.chdir(cwd)


class _Capture(object):
    def __init__(self):
        self.lines = []

    def log(self, *msg):
        self.lines.append("\t".join(str(m) for m in msg))


def _driver(tmp_path, extra):
    """(lines Net.test_all_effects() logs after a two-epoch synthetic run, evaluate()[0], test()[0], the net)."""
    import os
    from elimrec_amd import Logger
    from helpers import ROOT
    net = _net(tmp_path, extra)
    before = Logger.logger
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        net.run()
        cap = Logger.logger = _Capture()
        net.test_all_effects()
        rec = net.recommender
        rec.predict_type = "TIE"
        return cap.lines, np.asarray(rec.evaluate()[0]), np.asarray(rec.test()[0]), net
    finally:
        os.chdir(cwd)
        Logger.logger = before


def test_driver_switch(tmp_path):
    """With --newuser_report=K exactly three lines are added -- one under each effect's block and the TE->TIE table -- and with the
    switch off the log and the returned metrics are the other run's."""
    from elimrec_amd.evaluator import NEWUSER_VARIANTS
    view = ["--group_view=[10,30]", "--rank_report=1"]
    off, ev0, te0, net0 = _driver(tmp_path / "a", view)
    assert net0.newuser_report == 0 and net0.recommender.newuser_reporter is None and not any("[new users]" in ln for ln in off)
    on, ev1, te1, net1 = _driver(tmp_path / "b", view + ["--newuser_report=7"])
    rep = net1.recommender.newuser_reporter
    topks = [int(k) for k in net1.recommender.config["topks"]]
    assert net1.newuser_report == 7 and rep.k == 7 and len(rep.users) > 0 and rep.evaluator.top_show.tolist() == sorted(set(topks + [7]))
    added = [i for i, ln in enumerate(on) if "[new users]" in ln.split("\n")[0]]
    assert len(added) == 3 and [ln for i, ln in enumerate(on) if i not in added] == off
    te, tie, shift = added
    assert on[te].startswith("  [TE] [new users] ") and on[tie].startswith("  [TIE] [new users] ") and on[shift].startswith("  [TE->TIE] [new users]:\n")
    assert "catalogue rank" in on[te - 1] and "catalogue rank" in on[tie - 1] and on[shift + 1].startswith("  [TE->TIE] rank shift")
    for i in (te, tie):
        assert all((v + ":") in on[i] for v in NEWUSER_VARIANTS) and "@7" in on[i] and "overlap" in on[i] and "cos" in on[i]
        assert ("\nall:\n" in on[i]) == (len(rep.group_labels) > 1)
    assert "d_overlap" in on[shift] and "d_users" not in on[shift]
    assert ev0.tobytes() == ev1.tobytes() and te0.tobytes() == te1.tobytes()
    for bad in ("--newuser_report=-1", "--newuser_report=257"):
        with pytest.raises(ValueError, match="newuser_report"):
            _net(tmp_path / "c", [bad])
