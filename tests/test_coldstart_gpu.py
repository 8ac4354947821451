"""Cold-start items on the device: ops.rank_values (csrc/coldstart.hip) against the exact integer model of
tests/coldstart_model.py, EliMRec.fold_in_items against the cached rows of catalogue items without a training edge (a free yardstick:
a correct fold-in must reproduce them), the readers over the folded rows against the catalogue's own readers, and the report.

The count is an integer: int32 EQUALITY, at the segment and values-per-pass edges (placed from ops.RANK_VALUES_SEGMENT /
ops.RANK_VALUES_PER_PASS), on padded rows whose padding holds +inf (reading a padding column shows up as a wrong count).
Fold-in: with the default 'pre' adjacency (and 'plain' / 'gcmc': no diagonal) the isolated row is (x + 0) * inv in the propagation
kernels and kappa * x here, the same float32 product, and the projections are the same ops.linear_fwd_batched problems, so the rows
are compared BIT FOR BIT. 'norm' / 'mean' sum L + 1 copies of x before scaling: compared with the float64 model within the bound
tests/fp64_tools.py gives the projections."""
import numpy as np
import pytest
import torch

import coldstart_cases as cc
import coldstart_model as cm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _edges():
    from elimrec_amd import ops
    return ops.RANK_VALUES_SEGMENT, ops.RANK_VALUES_PER_PASS


def _padded(x, pad):
    B, I = x.shape
    lds = (I + 3) // 4 * 4 + pad
    host = np.full((B, lds), np.inf, dtype=np.float32)                # +inf in every padding column
    host[:, :I] = x
    return host


@pytest.mark.parametrize("family", cc.FAMILIES)
def test_rank_values_is_exact(family):
    from elimrec_amd import ops
    SEG, P = _edges()
    assert P == 1024 and SEG % 4 == 0
    rng = np.random.default_rng(cc.FAMILIES.index(family))
    met = set()
    for case, I in enumerate((1, 3, 4, 5, SEG - 1, SEG, SEG + 1)):
        with_skip, pad = case % 2 == 1 or I == SEG + 1, (0, 12)[case % 2]
        x, ptr, vals, skip = cc.make(family, I, P, rng, case, with_skip)
        lens = np.diff(ptr).tolist()
        assert {0, 1, P, P + 1} <= set(lens) and lens[2] == 0         # a ragged mix in one call, an empty row between listed ones
        want = cm.rank_values(x, ptr, vals, skip)
        assert ((want == -1) == ~np.isfinite(vals)).all() and (want == -1).any()
        if with_skip:
            plain = cm.rank_values(x, ptr, vals, None)
            met |= set(np.unique((plain - want)[np.isfinite(vals) & (skip >= 0)]).tolist())
        host = _padded(x, pad)
        block = _t(host)[:, :I]
        n = vals.size
        out = torch.full((n + 9,), 7, dtype=torch.int32, device=DEV)
        ops.rank_values(block, ptr, _t(vals), out, skip=skip)
        first = out.cpu().numpy()
        assert (first[n:] == 7).all(), (family, I)                    # nothing behind the last value is touched
        assert np.array_equal(first[:n], want), (family, I, np.flatnonzero(first[:n] != want)[:8])
        again = torch.full((n + 9,), 7, dtype=torch.int32, device=DEV)
        ops.rank_values(block, _t(ptr), _t(vals), again, skip=None if skip is None else _t(skip))
        assert torch.equal(again, out), (family, I)                   # the same counts whatever order the adds arrive in
        assert torch.equal(block.cpu(), torch.from_numpy(host[:, :I]))
    if family != "equal":
        assert met == {0, 1}                                          # a skipped column that beats the value and one that does not


def test_rank_values_on_rows_that_take_the_unaligned_form():
    """A row stride that is no multiple of 4 floats (and a base off the 16-byte grid) cannot take the 16-byte loads."""
    from elimrec_amd import ops
    SEG, P = _edges()
    rng = np.random.default_rng(11)
    I, lds = SEG + 6, SEG + 9
    x, ptr, vals, skip = cc.make("few", I, P, rng, 1, True)
    flat = torch.full((cc.B * lds + 1,), float("inf"), dtype=torch.float32, device=DEV)
    block = flat[1:].view(cc.B, lds)[:, :I]
    block.copy_(_t(x))
    out = torch.empty(vals.size, dtype=torch.int32, device=DEV)
    ops.rank_values(block, ptr, _t(vals), out, skip=skip)
    assert np.array_equal(out.cpu().numpy(), cm.rank_values(x, ptr, vals, skip))


def test_rank_values_refuses_on_the_host():
    from elimrec_amd import _lib, ops
    block = torch.zeros(2, 8, device=DEV)
    vals = torch.zeros(2, device=DEV)
    out = torch.full((4,), 7, dtype=torch.int32, device=DEV)
    calls = []
    _lib.record(calls)
    try:
        with pytest.raises(ValueError):
            ops.rank_values(block, [0, 2, 1], vals, out)              # not ascending
        with pytest.raises(ValueError):
            ops.rank_values(block, [0, 1], vals, out)                 # B + 1 entries
        with pytest.raises(ValueError):
            ops.rank_values(block, [0, 1, 3], vals, out)              # does not end at len(vals)
        with pytest.raises(IndexError):
            ops.rank_values(block, [0, 1, 2], vals, out, skip=[0, 8])
        with pytest.raises(IndexError):
            ops.rank_values(block, [0, 1, 2], vals, out, skip=[-2, 0])
        with pytest.raises(ValueError):
            ops.rank_values(block, [0, 1, 2], vals, out, skip=[0])
        with pytest.raises(ValueError):
            ops.rank_values(block, [0, 1, 2], vals, out[:1])          # out too short
        with pytest.raises(TypeError):
            ops.rank_values(block, [0, 1, 2], vals, out.float())
    finally:
        _lib.record(None)
    assert not calls                                                  # every refusal came before any launch
    assert (out.cpu() == 7).all()
    assert ops.rank_values(block, [0, 0, 0], vals[:0], out) is out    # nothing listed: nothing counted
    assert (out.cpu() == 7).all()


def test_torch_op_equals_the_ctypes_binding():
    from elimrec_amd import ops, torch_ops
    SEG, P = _edges()
    rng = np.random.default_rng(5)
    I = SEG + 5
    x, ptr, vals, skip = cc.make("masked", I, P, rng, 2, True)
    block = _t(_padded(x, 4))[:, :I]
    out = torch.empty(vals.size, dtype=torch.int32, device=DEV)
    ops.rank_values(block, ptr, _t(vals), out, skip=skip)
    t = torch_ops.load()
    got = t.rank_values(block, _t(ptr), _t(vals), _t(skip))
    assert got.dtype == torch.int32 and torch.equal(got, out)
    assert torch.equal(t.rank_values(block, _t(ptr), _t(vals), None), ops.rank_values(block, ptr, _t(vals), torch.empty_like(out)))
    with pytest.raises(IndexError):
        t.rank_values(block, _t(ptr), _t(vals), _t(np.full(vals.size, I, dtype=np.int32)))
    with pytest.raises(RuntimeError):
        t.rank_values(block, _t(ptr[::-1].copy()), _t(vals), None)


# --------------------------------------------------------------------------- the fold-in and its readers
_MODELS = {}


def _model(name, d, fusion="concat", adj=None, stepped=True):
    """A small model over a golden fixture's graph and features (random seeded parameters: recdim is the test's), after one
    bpr_loss + backward + optimizer.step(): (model, cold item ids -- the first one has a test interaction --, their id rows captured
    BEFORE the step)."""
    key = (name, d, fusion, adj, stepped)
    if key in _MODELS:
        return _MODELS[key]
    from elimrec_amd import EliMRec, FusedAdam
    from helpers import FixtureDataset, fixture_argv, load_golden, make_config
    g = load_golden(name)
    drop = ("--recdim=", "--mm_fusion_mode=", "--layer_num=") + (("--adj_type=",) if adj else ())
    argv = [a for a in fixture_argv(g) if not a.startswith(drop)] + ["--recdim=%d" % d, "--mm_fusion_mode=%s" % fusion, "--layer_num=3"]
    argv += ["--adj_type=%s" % adj] if adj else []
    torch.manual_seed(7)
    model = EliMRec(make_config(argv), FixtureDataset(g)).to(DEV)
    assert model.n_layers == 3 and model.latent_dim == d
    I = model.num_items
    trained = np.zeros(I, dtype=bool)
    trained[g["train_i"]] = True
    tested = np.zeros(I, dtype=bool)
    for items in model.dataset.get_user_test_dict().values():
        tested[np.asarray(items, dtype=np.int64)] = True
    cold = np.flatnonzero(~trained)
    with_test = np.flatnonzero(~trained & tested)
    assert cold.size >= 3 and with_test.size >= 1                     # the precondition: no skip, the fixtures have such items
    items = np.concatenate((with_test[:1], cold[cold != with_test[0]]))
    id_rows = model.embedding_item.weight.detach()[_t(items)].clone()
    if stepped:
        opt = FusedAdam(model.parameters(), lr=float(g["lr"]), weight_decay=float(g["weight_decay"]))
        loss = model.bpr_loss(_t(g["step1/users"]), _t(g["step1/pos"]), _t(g["step1/neg"]))
        opt.zero_grad()
        loss.backward(retain_graph=True)
        opt.step()
    _MODELS[key] = (model, items, id_rows)
    return _MODELS[key]


def _own_features(model, items):
    return {m: getattr(model, m + "_feat")[_t(items)] for m in model._mods}


def _cached_rows(model, items):
    assert model.all_items is not None                                # (materialises the tables of the last forward)
    return model._ws["Y"][model.num_users + _t(items)]


@pytest.mark.parametrize("name,d,fusion", [("ml3", 8, "concat"), ("ml3", 64, "mean"), ("kwai", 8, "mean"), ("kwai", 64, "concat")])
def test_fold_in_reproduces_the_cached_rows_of_items_without_an_edge(name, d, fusion):
    """The default 'pre' adjacency, L >= 2: bit for bit, after a training step (the tables materialise from the snapshot of the
    weights the forward used, NOT the stepped parameters) and after compute() (the live parameters)."""
    from fp64_tools import same_bits
    model, items, id_rows = _model(name, d, fusion)
    assert model.S == (1 if name == "kwai" else 3) and str(model.config["adj_type"]) == "pre"
    new = model.fold_in_items(_own_features(model, items), id_rows=id_rows, normalized=True)
    want = _cached_rows(model, items)
    assert float(want.abs().max()) > 0 and new.rows.shape == want.shape
    assert same_bits(new.rows.contiguous(), want.contiguous()), float((new.rows - want).abs().max())
    assert same_bits(new.table[:model.num_users].contiguous(), model._ws["Y"][:model.num_users].contiguous())
    live = model.fold_in_items(_own_features(model, items), id_rows=model.embedding_item.weight.detach()[_t(items)], normalized=True)
    assert not same_bits(live.rows.contiguous(), want.contiguous())   # (the step moved the weights: the snapshot matters)
    # ... and after compute(): the live views
    twin, items2, _ = _model(name, d, fusion, stepped=False)
    with torch.no_grad():
        twin.compute()
    new2 = twin.fold_in_items(_own_features(twin, items2), id_rows=twin.embedding_item.weight.detach()[_t(items2)], normalized=True)
    assert same_bits(new2.rows.contiguous(), _cached_rows(twin, items2).contiguous())
    with pytest.raises(RuntimeError, match="fold_in_items"):          # a stale handle
        with torch.no_grad():
            twin.compute()
        twin.predict_new_items([0], new2)


@pytest.mark.parametrize("adj", ["norm", "mean", "gcmc", "plain"])
def test_fold_in_against_float64_for_every_adjacency(adj):
    """'norm' / 'mean' give an isolated node the identity row: L + 1 copies of x summed before the scale, not bit-exact against
    kappa x. Every form: the fold-in AND the cached rows within the projections' float64 bound of the exact rows (two chained
    Linears: the second one's bound plus the first one's error carried through |W|)."""
    from fp64_tools import TINY, tau
    model, items, _ = _model("ml3", 8, "concat", adj=adj, stepped=False)
    with torch.no_grad():
        model.compute()
    ids = model.embedding_item.weight.detach()[_t(items)]
    feats = _own_features(model, items)
    new = model.fold_in_items(feats, id_rows=ids, normalized=True)
    W = {k: v.detach().double().cpu().numpy() for k, v in model.state_dict().items()}
    f = {m: v.double().cpu().numpy() for m, v in feats.items()}
    L, d, mods = model.n_layers, model.latent_dim, model._mods
    kappa = cm.isolated_row_scale(adj, L)
    want = cm.fold_in_rows(f, ids.double().cpu().numpy(), W, mods, d, kappa, "concat")
    # bound: Out blocks, then the fused Linear over C columns and the heads over d
    a = lambda x: np.abs(x)
    out_abs = [kappa * a(ids.double().cpu().numpy())]
    out_err = [tau(L + 2) * out_abs[0]]
    for m in mods:
        s = kappa * (a(f[m]) @ a(W[m + "_dense.weight"]).T + a(W[m + "_dense.bias"]))
        out_abs.append(s)
        out_err.append(tau(f[m].shape[1] + L + 2) * s)
    wi = a(W["embedding_item_after_GCN.weight"])
    bound = [tau(model.C) * (np.concatenate(out_abs, 1) @ wi.T + a(W["embedding_item_after_GCN.bias"])) + np.concatenate(out_err, 1) @ wi.T]
    for h, m in enumerate(mods):
        ws = a(W["s_dense_%s.weight" % m])
        bound.append(tau(d) * (out_abs[1 + h] @ ws.T + a(W["s_dense_%s.bias" % m])) + out_err[1 + h] @ ws.T)
    bound = np.concatenate(bound, 1) * (1 + 1e-3) + TINY
    for what, got in (("fold-in", new.rows), ("cached", _cached_rows(model, items))):
        err = np.abs(got.double().cpu().numpy() - want)
        assert (err <= bound).all(), (adj, what, float((err / bound).max()))
    if adj in ("gcmc", "plain"):                                      # no diagonal: the same product as the kernels'
        from fp64_tools import same_bits
        assert same_bits(new.rows.contiguous(), _cached_rows(model, items).contiguous())


def test_fold_in_front_end():
    from elimrec_amd import _lib
    from fp64_tools import same_bits
    import torch.nn.functional as F
    model, items, id_rows = _model("ml3", 8)
    rng = np.random.default_rng(3)
    raw = {m: torch.from_numpy(rng.standard_normal((17, getattr(model, m + "_feat").shape[1])).astype(np.float32)) for m in model._mods}
    ids = torch.from_numpy(rng.standard_normal((17, 8)).astype(np.float32))
    many = model.fold_in_items(raw, id_rows=ids)
    one = model.fold_in_items({m: v[5:6] for m, v in raw.items()}, id_rows=ids[5:6])
    assert len(many) == 17 and len(one) == 1 and many.table.shape == (model.num_users + 17, model.Cy)
    assert same_bits(one.rows.contiguous(), many.rows[5:6].contiguous())          # a row depends on its own inputs only
    given = model.fold_in_items({m: F.normalize(v, dim=1) for m, v in raw.items()}, id_rows=ids, normalized=True)
    assert same_bits(given.rows.contiguous(), many.rows.contiguous())
    zero = model.fold_in_items(raw)
    assert same_bits(zero.rows.contiguous(), model.fold_in_items(raw, id_rows=torch.zeros(17, 8)).rows.contiguous())
    calls = []
    _lib.record(calls)
    try:
        bad = dict(raw)
        bad["x"] = raw["v"]
        for features, kw in ((bad, {}), ({m: raw[m] for m in model._mods[1:]}, {}), ({m: v[:, :-4] for m, v in raw.items()}, {}),
                             (raw, dict(id_rows=ids[:, :4])), (raw, dict(id_rows=ids[:5])),
                             ({m: (v if m != "a" else torch.where(torch.arange(v.numel()).view_as(v) == 9, float("nan"), v)) for m, v in raw.items()}, {}),
                             (raw, dict(id_rows=ids * float("inf"))), ({m: v.long() for m, v in raw.items()}, {})):
            with pytest.raises(ValueError):
                model.fold_in_items(features, **kw)
        empty = model.fold_in_items({m: v[:0] for m, v in raw.items()})
    finally:
        _lib.record(None)
    assert not calls and len(empty) == 0 and empty.rows.shape == (0, model.Cy)   # the refusals and Q = 0: no launch
    assert model.predict_new_items([0, 1], empty).shape == (2, 0)
    with pytest.raises(TypeError):
        model.predict_new_items([0], many.rows)


@pytest.mark.parametrize("fusion_mode", ["rubi", "hm", "sum"])
def test_readers_of_a_folded_catalogue_item_equal_the_catalogue_readers(fusion_mode):
    model, items, id_rows = _model("ml3", 8)
    model.fusion_mode = fusion_mode
    new = model.fold_in_items(_own_features(model, items), id_rows=id_rows, normalized=True)
    users = list(range(0, model.num_users, 3))
    try:
        for ptype in ("normal", "TE", "TIE"):
            model.predict_type = ptype
            full = model.predict(users)
            got = model.predict_new_items(users, new)
            assert got.shape == (len(users), len(items))
            assert torch.equal(got.view(torch.int32), full[:, torch.from_numpy(items)].contiguous().view(torch.int32)), (fusion_mode, ptype)
            excl = {0: [1, 2], 2: [0]}
            a = model.audience_new_items(new, 5, exclude=excl)
            b = model.audience([int(i) for i in items], 5, exclude={int(items[q]): v for q, v in excl.items()})
            assert torch.equal(a.users, b.users) and torch.equal(a.scores.view(torch.int32), b.scores.view(torch.int32)), (fusion_mode, ptype)
    finally:
        model.predict_type, model.fusion_mode = "TIE", "rubi"


def test_similar_recommend_and_rank_with_new_items():
    model, items, id_rows = _model("ml3", 8)
    model.predict_type = "TIE"
    I, Q = model.num_items, len(items)
    new = model.fold_in_items(_own_features(model, items), id_rows=id_rows, normalized=True)
    # neighbours: the folded row is the catalogue row, so its list is the item itself (cosine of identical rows) + the item's own list
    for space in ("fused", "v"):
        near = model.similar_to_new_items(new, 6, space=space)
        own = model.similar_items([int(i) for i in items], 5, space=space)
        assert int(near.ids.max()) < I
        for q in range(Q):
            rest = [int(i) for i in near.ids[q].tolist() if i != int(items[q])]
            assert int(items[q]) in near.ids[q].tolist() and rest[:5] == own.ids[q].tolist()[:len(rest[:5])], (space, q)
    # recommend_with_new against a host merge by (score descending, id ascending), new item q under id I + q
    users = [0, 3, 4, 9, 11]
    train = model.dataset.get_user_train_dict()
    excl = {u: train.get(u, []) for u in users}
    block = model.predict(users).numpy().copy()
    for r, u in enumerate(users):
        block[r, excl[u]] = -np.inf
    vals = model.predict_new_items(users, new).numpy()
    both = np.concatenate((block, vals), axis=1)
    for k in (1, 7, 40):
        ids, scores = model.recommend_with_new(users, new, k, exclude=excl)
        for r in range(len(users)):
            order = np.lexsort((np.arange(I + Q), -both[r].astype(np.float64)))[:k]
            assert ids[r].tolist() == order.tolist(), (k, r)
            assert np.array_equal(scores[r].numpy(), both[r, order])
    assert (ids >= I).any()                                           # (the folded copies tie with their originals and follow them)
    for bad in (0, I + 1, 257):
        with pytest.raises(ValueError):
            model.recommend_with_new(users, new, bad, exclude=excl)
    # a user whose unmasked catalogue (items 3 and 8) is shorter than k: new items take the places of predict_device's fillers, and
    # -1 / -inf remain only where catalogue and new items together are fewer than k
    few = {0: [i for i in range(I) if i not in (3, 8)]}
    row = np.concatenate((model.predict([0]).numpy()[0, [3, 8]], vals[0]))
    names = np.asarray([3, 8] + list(range(I, I + Q)))
    ids2, scores2 = model.recommend_with_new([0], new, 5, exclude=few)
    order = np.lexsort((names, -row.astype(np.float64)))[:5]
    assert ids2[0].tolist() == names[order].tolist() and np.array_equal(scores2[0].numpy(), row[order])
    one = model.fold_in_items({m: v[:1] for m, v in _own_features(model, items).items()}, id_rows=id_rows[:1], normalized=True)
    ids3, scores3 = model.recommend_with_new([0], one, 5, exclude=few)
    order = np.lexsort((names[:3], -row[:3].astype(np.float64)))
    assert ids3[0].tolist() == names[:3][order].tolist() + [-1, -1]
    assert np.array_equal(scores3[0].numpy(), np.concatenate((row[:3][order], [-np.inf, -np.inf])).astype(np.float32))
    # rank_new_items against the exact model on the copied blocks
    ptr = np.arange(len(users) + 1, dtype=np.int64) * Q
    want = cm.rank_values(block, ptr, vals.reshape(-1)).reshape(len(users), Q)
    got = model.rank_new_items(users, new, exclude=excl)
    assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want)
    assert np.array_equal(model.rank_new_items(users, new, exclude=excl, among=True).numpy(), want + cm.among(vals))
    skip = model.rank_new_items_device(_t(np.asarray(users)), new, skip=items).cpu().numpy()
    plain = model.predict(users).numpy()
    assert np.array_equal(skip, cm.rank_values(plain, ptr, vals.reshape(-1), np.tile(items, len(users))).reshape(len(users), Q))
    old, model.RANK_BLOCK_BYTES = model.RANK_BLOCK_BYTES, 2 * ((I + 3) // 4 * 16)          # two users per block
    try:
        assert np.array_equal(model.rank_new_items(users, new, exclude=excl).numpy(), want)
    finally:
        model.RANK_BLOCK_BYTES = old


# --------------------------------------------------------------------------- the report
def test_coldstart_report():
    from elimrec_amd import reports
    from elimrec_amd.evaluator import ColdStartReport, RankReport
    model, _, _ = _model("ml3", 8)
    assert model.coldstart_reporter is None                           # the switch is off by default: nothing is built, nothing logged
    ds = model.dataset
    train, test = ds.get_user_train_dict(), ds.get_user_test_dict()
    ks = [5, 20]
    rep = ColdStartReport(ds, train, test, ks, group_view=[2, 4])
    cold, pairs = reports.cold_test_items(train, test, model.num_items)
    assert rep.num_pairs == len(pairs) > 0 and np.array_equal(rep.items, cold) and len(rep.group_labels) > 1
    model.predict_type = "TIE"
    final, buf = rep.evaluate(model)
    assert final.shape == (len(rep.group_labels), 3, 5 + len(ks)) and "catalogue:" in buf and "mean_id:" in buf
    # the pure numpy rows on the copied blocks
    users = rep.users
    block = model.predict(users).numpy().copy()
    for r, u in enumerate(users):
        block[r, train.get(u, [])] = -np.inf
    n_cand = rep.pair_n_cand.astype(np.int64)
    ptr = np.arange(len(users) + 1, dtype=np.int64) * cold.size
    import rank_model as rm
    ranks = [rm.ranks(block, rep.pair_ptr, rep.pair_items)]
    for variant in ("content", "mean_id"):
        new = rep.new_items(model, variant)
        vals = model.predict_new_items(users, new).numpy()
        full = cm.rank_values(block, ptr, vals.reshape(-1), np.tile(cold, len(users))).reshape(len(users), cold.size)
        ranks.append(full[rep.pair_user, rep.pair_q])
    for g, at in enumerate(rep._pair_pos):
        for v in range(3):
            want = reports.coldstart_row(ranks[v][at], n_cand[at], ks, np.unique(rep.pair_items[at]).size)
            # (per-pair values rounded to float32, their mean taken in float64 and rounded once: two float32 roundings)
            assert np.allclose(final[g, v], want, rtol=2.0 ** -22, atol=0), (g, v, final[g, v], want)
    # the catalogue row = the rank report's pair means restricted to the cold items
    only = {}
    for u, i in pairs:
        only.setdefault(u, []).append(i)
    rr = RankReport(ds, train, only, ks).evaluate(model)[0]
    assert np.array_equal(final[0, 0, 2:], rr.pairs[0][[0, 2, 1, 3, 4]])
    delta, dbuf = rep.shift(final, final)
    assert not delta.any() and "d_rank" in dbuf
    # a split without cold test items: one line
    warm = {u: [i for i in items if i not in set(cold.tolist())] for u, items in test.items()}
    none = ColdStartReport(ds, train, warm, ks)
    assert none.evaluate(model) == (None, reports.format_coldstart(None, None, None))


def test_fold_in_after_a_step_of_the_unfolded_forward():
    """'norm' has a diagonal: the model trains through the unfolded row-major forward, which builds its tables from the live weights
    and then steps them. The fold-in reads the copy taken before the update: the rows agree with the cached rows of the forward within
    twice the float64 bound of either (both are float32 evaluations of the same exact rows), and are NOT the rows of the stepped
    weights."""
    from elimrec_amd import FusedAdam
    from fp64_tools import TINY, same_bits, tau
    from helpers import load_golden
    model, items, _ = _model("kwai", 8, "concat", adj="norm", stepped=False)
    assert not model._lazy
    g = load_golden("kwai")
    W = {k: v.detach().double().cpu().numpy() for k, v in model.state_dict().items()}
    ids = model.embedding_item.weight.detach()[_t(items)].clone()
    opt = FusedAdam(model.parameters(), lr=float(g["lr"]), weight_decay=float(g["weight_decay"]))
    loss = model.bpr_loss(_t(g["step1/users"]), _t(g["step1/pos"]), _t(g["step1/neg"]))
    opt.zero_grad()
    loss.backward(retain_graph=True)
    opt.step()
    feats = _own_features(model, items)
    new = model.fold_in_items(feats, id_rows=ids, normalized=True)
    f = {m: v.double().cpu().numpy() for m, v in feats.items()}
    L, d, m = model.n_layers, model.latent_dim, "v"
    want = cm.fold_in_rows(f, ids.double().cpu().numpy(), W, model._mods, d, 1.0, "concat")
    a = np.abs
    out_abs = [a(ids.double().cpu().numpy()), a(f[m]) @ a(W["v_dense.weight"]).T + a(W["v_dense.bias"])]
    out_err = [tau(L + 2) * out_abs[0], tau(f[m].shape[1] + L + 2) * out_abs[1]]
    wi, ws = a(W["embedding_item_after_GCN.weight"]), a(W["s_dense_v.weight"])
    bound = np.concatenate([tau(model.C) * (np.concatenate(out_abs, 1) @ wi.T + a(W["embedding_item_after_GCN.bias"])) + np.concatenate(out_err, 1) @ wi.T,
                            tau(d) * (out_abs[1] @ ws.T + a(W["s_dense_v.bias"])) + out_err[1] @ ws.T], 1) * (1 + 1e-3) + TINY
    cached = _cached_rows(model, items)
    for what, got in (("fold-in", new.rows), ("cached", cached)):
        err = np.abs(got.double().cpu().numpy() - want)
        assert (err <= bound).all(), (what, float((err / bound).max()))
    live = model.fold_in_items(feats, id_rows=ids, normalized=True).rows.clone()
    model._table_W = model._ws["live_views"]                            # (what reading the stepped weights would give)
    try:
        stepped = model.fold_in_items(feats, id_rows=ids, normalized=True).rows
    finally:
        model._table_W = model._ws["snap_views"]
    assert same_bits(live.contiguous(), new.rows.contiguous()) and not same_bits(stepped.contiguous(), live.contiguous())


# --------------------------------------------------------------------------- the driver's switch
def _net(tmp_path, extra, shape="[60,200,1200]"):
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
                            argv=["main.py", "--data.input.dataset=synthetic", "--alpha=0.5", "--synthetic_shape=" + shape,
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


def _driver(tmp_path, extra, shape="[60,200,1200]"):
    """(lines Net.test_all_effects() logs after a two-epoch synthetic run, evaluate()[0], test()[0], the net)."""
    import os
    from elimrec_amd import Logger
    from helpers import ROOT
    net = _net(tmp_path, extra, shape)
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
    """With --coldstart_report=K exactly three lines are added -- one under each effect's block, behind the rank report's, and the
    TE->TIE table before the rank shift -- and with the switch off the log and the returned metrics are the other run's."""
    from elimrec_amd.evaluator import COLDSTART_VARIANTS
    view = ["--group_view=[10,30]", "--rank_report=1", "--list_report=5"]
    off, ev0, te0, net0 = _driver(tmp_path / "a", view)
    assert net0.coldstart_report == 0 and net0.recommender.coldstart_reporter is None and not any("cold test items" in ln for ln in off)
    on, ev1, te1, net1 = _driver(tmp_path / "b", view + ["--coldstart_report=7"])
    rep = net1.recommender.coldstart_reporter
    topks = [int(k) for k in net1.recommender.config["topks"]]
    assert net1.coldstart_report == 7 and rep.num_pairs > 0 and rep.ks == topks + [7] * (7 not in topks)
    added = [k for k, ln in enumerate(on) if "cold test items" in ln.split("\n")[0]]
    assert len(added) == 3 and [ln for k, ln in enumerate(on) if k not in added] == off
    te, tie, shift = added
    assert on[te].startswith("  [TE] cold test items (no training interaction):\n")
    assert on[tie].startswith("  [TIE] cold test items (no training interaction):\n") and on[shift].startswith("  [TE->TIE] cold test items:\n")
    assert "catalogue rank" in on[te - 1] and on[te - 1].startswith("  [TE]") and on[te + 1].startswith("  [TE] top-5 lists")
    assert "catalogue rank" in on[tie - 1] and on[tie - 1].startswith("  [TIE]") and on[tie + 1].startswith("  [TIE] top-5 lists")
    assert on[shift - 1].startswith("  [TIE]") and on[shift + 1].startswith("  [TE->TIE] rank shift")
    for k in (te, tie):
        assert all((v + ":") in on[k] for v in COLDSTART_VARIANTS) and "hit@7" in on[k] and "pairs" in on[k]
        assert ("\nall:\n" in on[k]) == (len(rep.group_labels) > 1)        # with user groups: one block per group, its label on a line
    assert "d_rank" in on[shift] and "d_hit@7" in on[shift] and "d_pairs" not in on[shift]
    assert ev0.tobytes() == ev1.tobytes() and te0.tobytes() == te1.tobytes()
    # the same switch on a plain run, and K among the topks: no column twice
    plain_off, ev2, te2, _ = _driver(tmp_path / "c", [])
    plain_on, ev3, te3, net3 = _driver(tmp_path / "d", ["--coldstart_report=%d" % topks[0]])
    assert net3.recommender.coldstart_reporter.ks == topks
    assert len(plain_off) == 2 and len(plain_on) == 5 and [plain_on[0], plain_on[2]] == plain_off
    assert plain_on[1].startswith("  [TE] cold test items") and plain_on[3].startswith("  [TIE] cold test items")
    assert plain_on[4].startswith("  [TE->TIE] cold test items") and "\nall:\n" not in plain_on[1]
    assert ev2.tobytes() == ev3.tobytes() and te2.tobytes() == te3.tobytes()


def test_driver_switch_without_cold_test_items_and_refusals(tmp_path):
    """A split in which every test item has a training interaction logs one line per place; a negative K and a world size above 1
    are refused at start-up."""
    from elimrec_amd import reports
    dense = "[60,40,1500]"
    off, ev0, te0, _ = _driver(tmp_path / "a", [], shape=dense)
    on, ev1, te1, net = _driver(tmp_path / "b", ["--coldstart_report=5"], shape=dense)
    assert net.recommender.coldstart_reporter.num_pairs == 0          # the precondition of this test: no cold test item
    line = reports.format_coldstart(None, None, None)
    assert len(off) == 2 and [on[0], on[2]] == off
    assert on[1:] == [on[1], on[2], "  [TIE] cold test items (no training interaction):\n" + line, "  [TE->TIE] cold test items:\n" + line]
    assert on[1] == "  [TE] cold test items (no training interaction):\n" + line and "\n" not in line
    assert ev0.tobytes() == ev1.tobytes() and te0.tobytes() == te1.tobytes()
    with pytest.raises(ValueError, match="coldstart_report"):
        _net(tmp_path / "c", ["--coldstart_report=-1"])
