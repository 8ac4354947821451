"""Hard-negative sampling on the device: the pick kernel (csrc/hardneg.hip) against the float64 model of tests/hardneg_model.py,
the candidate draw (csrc/sampler.hip) against the uniform draw, and what is built on them: EliMRec.hard_negatives_device,
PairwiseSamplerV2(neg_sampling="hard"), --neg_sampling=hard.

Tolerance of a score, tol = 4 (d + 8) 2^-24 * sum_b |w_b|: the worst-case fp32 bound of one cosine derived in
test_rerank_gpu.py's header ((2 d + 8) u for the cosine itself, u = 2^-24; twice that for a comparison of two), times the weight
sum -- the products w_b * cos_b and their additions add a few u of a value <= sum |w_b|, inside the d-independent part of the
bound. A bound, not a measurement: a pick can fall short of the float64 maximum by at most tol, a reported score is off by at
most tol / 2, and where the float64 margin to every candidate with another id exceeds tol the kernel must make the float64 pick.
The tables are column slices of wider matrices whose other columns and neighbouring rows hold NaN, the squared norms strided
columns of a NaN matrix, and every output lies between canaries: a read or a write outside shows up."""
import functools

import numpy as np
import pytest
import torch

import hardneg_model as hm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
USERS, ITEMS, SEED = 300, 500, 11
NS = (1, 63, 257, 1000)
CASES = ((1, 4, 1), (2, 20, 2), (5, 64, 4), (16, 64, 1), (17, 256, 2), (64, 64, 4), (8, 256, 4))          # M, d, blocks
CANARY_I, CANARY_F, PAD = 77, 7.0, 5


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def tol(d, w):
    return 4.0 * (d + 8) * 2.0 ** -24 * float(np.abs(np.asarray(w, dtype=np.float64)).sum())


def _weight_sets(blocks):
    sets = [[1.0] + [0.0] * (blocks - 1)]
    if blocks > 1:
        sets.append([0.0] * (blocks - 1) + [1.0])                             # a single head
    if blocks == 4:
        sets.append([1.0, 0.5, 0.0, 0.5])
    return sets


@functools.lru_cache(maxsize=None)
def _tables(d, blocks, col0=4):
    """300 user rows and 500 item rows of `blocks` blocks of N(0, 1) + 1.5 x one of 8 centres per block, fp32, row 11 of each side
    zero; each at row 2, column col0 of a wider NaN matrix (col0 = 3: the base is not 16-byte aligned and ld % 4 != 0), the squared
    norms at row 1, column 1 of a NaN matrix. -> (U, T float32 host, user view, user norms view, item view, item norms view)"""
    rng = np.random.default_rng(SEED + 1000 * d + blocks)
    host, views = [], []
    for rows in (USERS, ITEMS):
        centres = rng.standard_normal((8, blocks * d))
        X = (rng.standard_normal((rows, blocks * d)) + 1.5 * centres[rng.integers(0, 8, rows)]).astype(np.float32)
        X[11] = 0.0
        sq = (X.astype(np.float64).reshape(rows, blocks, d) ** 2).sum(2).astype(np.float32)
        wide = np.full((rows + 3, blocks * d + col0 + 4), np.nan, dtype=np.float32)
        wide[2:2 + rows, col0:col0 + blocks * d] = X
        sqw = np.full((rows + 2, blocks + 2), np.nan, dtype=np.float32)
        sqw[1:1 + rows, 1:1 + blocks] = sq
        host.append(X)
        views += [_t(wide)[2:2 + rows, col0:col0 + blocks * d], _t(sqw)[1:1 + rows, 1:1 + blocks]]
    assert (views[0].data_ptr() % 16 == 0) == (col0 == 4) and (views[0].stride(0) % 4 == 0) == (col0 == 4)
    return host[0], host[1], views[0], views[1], views[2], views[3]


def _triplets(n, M, rng, pool=ITEMS):
    users = rng.integers(0, USERS, n).astype(np.int64)
    cands = rng.integers(0, pool, (n, M)).astype(np.int32)
    return users, cands


def _run(tabs, w, users, cands, outputs=3):
    """One launch with canaries in front of and behind the [n] outputs -> (neg int64, pos int32, score float32) numpy."""
    from elimrec_amd import ops
    n = len(users)
    flat = [torch.full((n + 2 * PAD,), c, dtype=dt, device=DEV)
            for c, dt in ((CANARY_I, torch.int64), (CANARY_I, torch.int32), (CANARY_F, torch.float32))]
    views = [f[PAD:] for f in flat]
    ops.pick_hard_negatives(tabs[2], tabs[3], tabs[4], tabs[5], w, _t(np.asarray(users, dtype=np.int64)),
                            _t(np.asarray(cands, dtype=np.int32)).reshape(n, -1), views[0], *(views[1:] if outputs == 3 else ()))
    torch.cuda.synchronize()
    out = []
    for f, c in zip(flat[:outputs], (CANARY_I, CANARY_I, CANARY_F)):
        a = f.cpu().numpy()
        assert (a[:PAD] == c).all() and (a[PAD + n:] == c).all(), "entries outside [n] were written"
        out.append(a[PAD:PAD + n])
    return out


def _verify(score64, cands, got, t, what, max_unclear=0.01):
    """The certificate, the clear picks and the reported score of one launch against the float64 scores [n x M]."""
    neg, pos, val = got
    n = cands.shape[0]
    col, ids, best, margin = hm.pick(score64, cands)
    none = col < 0
    assert (neg[none] == -1).all() and (pos[none] == -1).all() and np.isneginf(val[none]).all(), (what, "rows without a pick")
    ok = ~none
    assert (pos[ok] >= 0).all() and (pos[ok] < cands.shape[1]).all()
    at = np.maximum(pos, 0)
    assert (neg[ok] == cands[np.arange(n), at][ok]).all(), (what, "out_pos does not index out_neg's id")
    picked = score64[np.arange(n), at]
    assert not np.isneginf(picked[ok]).any(), (what, "an unlisted candidate was picked")
    short = float((best[ok] - picked[ok]).max()) if ok.any() else 0.0
    off = float(np.abs(val[ok].astype(np.float64) - picked[ok]).max()) if ok.any() else 0.0
    clear = ok & (margin > t)
    # a row whose listed float64 scores are all equal (one candidate, copies of one id, the zero user row: every cosine exactly 0 in
    # fp32 too) is decided by the tie rule alone, exactly: it is checked below and does not count as unclear
    flat = ok & (np.where(np.isneginf(score64), best[:, None], score64) == best[:, None]).all(1)
    assert (pos[flat] == col[flat]).all(), (what, "equal scores: not the lowest listed column")
    unclear = float((ok & ~clear & ~flat).mean())
    print("pick_hard_negatives %s: pick below the float64 maximum by <= %.3e (bound %.3e), |out_score - float64| <= %.3e (bound %.3e), "
          "%.4f of the triplets unclear" % (what, short, t, off, t / 2, unclear))
    assert short <= t, (what, short, t)
    assert off <= t / 2, (what, off, t / 2)
    assert (neg[clear] == ids[clear]).all(), (what, "a clear pick is not the float64 pick")
    assert (pos[clear] == col[clear]).all(), (what, "out_pos is not the lowest column holding the picked id")
    assert unclear <= max_unclear, (what, unclear)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "M%d_d%d_b%d" % c)
def test_kernel_against_float64(case):
    M, d, blocks = case
    tabs = _tables(d, blocks)
    users, cands = _triplets(max(NS), M, np.random.default_rng(SEED + M))
    users[5], cands[7, 0] = 11, 11                                          # the zero rows
    for w in _weight_sets(blocks):
        score64 = hm.scores(tabs[0], tabs[1], w, users, cands)
        for n in NS:
            _verify(score64[:n], cands[:n], _run(tabs, w, users[:n], cands[:n]), tol(d, w), (case, tuple(w), n))


def test_misaligned_base_takes_the_scalar_row_load():
    M, d, blocks = 5, 64, 4
    tabs = _tables(d, blocks, col0=3)
    users, cands = _triplets(257, M, np.random.default_rng(SEED))
    users[5], cands[7, 0] = 11, 11
    for w in _weight_sets(blocks):
        _verify(hm.scores(tabs[0], tabs[1], w, users, cands), cands, _run(tabs, w, users, cands), tol(d, w), ("col0 = 3", tuple(w)))
    aligned = _tables(d, blocks)                                             # the same rows through the 16-byte loads: the same bits
    w = [1.0, 0.5, 0.0, 0.5]
    for a, b in zip(_run(tabs, w, users, cands), _run(aligned, w, users, cands)):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("d", (4, 64, 68, 128, 132, 192, 196, 256))
def test_width_edges(d):
    """Both sides of every boundary of NQ = ceil(d / 64), the float4s a lane holds: 3 triplets of M = 17 candidates (the 17th starts
    a second 16-column group), two blocks with one zero weight on either side, through the 16-byte and the scalar row loads."""
    M, blocks = 17, 2
    tabs, aligned = _tables(d, blocks, col0=3), _tables(d, blocks)
    users, cands = _triplets(3, M, np.random.default_rng(SEED + d))
    for w in ([0.0, 1.0], [1.0, 0.0]):
        got = _run(tabs, w, users, cands)
        _verify(hm.scores(tabs[0], tabs[1], w, users, cands), cands, got, tol(d, w), ("width edge", d, tuple(w)))
        for a, b in zip(got, _run(aligned, w, users, cands)):
            assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("case", ((17, 64, 4), (64, 20, 2), (5, 256, 1)), ids=lambda c: "M%d_d%d_b%d" % c)
def test_exact_properties(case):
    M, d, blocks = case
    tabs = _tables(d, blocks)
    w = [1.0, 0.5, 0.0, 0.5][:blocks]
    n = 257
    users, cands = _triplets(n, M, np.random.default_rng(SEED + 3), pool=40)          # few ids: duplicates in most rows
    neg, pos, val = _run(tabs, w, users, cands)
    # the M-wide launch = the lowest-column argmax over M one-column launches, bit for bit
    cols = [_run(tabs, w, users, cands[:, j:j + 1]) for j in range(M)]
    one = np.stack([c[2] for c in cols], 1)
    assert all((c[1] == 0).all() and (c[0] == cands[:, j]).all() for j, c in enumerate(cols))
    want = one.argmax(1)
    assert (pos == want).all() and (neg == cands[np.arange(n), want]).all()
    assert val.tobytes() == one[np.arange(n), want].tobytes()
    # the same triplets in another order, and embedded in a larger launch
    perm = np.random.default_rng(SEED + 4).permutation(n)
    for a, b in zip(_run(tabs, w, users[perm], cands[perm]), (neg, pos, val)):
        assert a.tobytes() == b[perm].tobytes()
    for a, b in zip(_run(tabs, w, users[100:163], cands[100:163]), (neg, pos, val)):
        assert a.tobytes() == b[100:163].tobytes()
    # M copies of one id: column 0
    same = np.repeat(cands[:, :1], M, 1)
    neg1, pos1, val1 = _run(tabs, w, users, same)
    assert (pos1 == 0).all() and (neg1 == same[:, 0]).all() and val1.tobytes() == one[:, 0].tobytes()
    # out_pos / out_score are optional
    assert _run(tabs, w, users, cands, outputs=1)[0].tobytes() == neg.tobytes()


@pytest.mark.parametrize("col0", (4, 3), ids=("aligned", "unaligned"))
def test_unlisted_entries(col0):
    M, d, blocks = 6, 20, 2
    tabs = _tables(d, blocks, col0)
    w = [1.0, 0.5]
    users, cands = _triplets(63, M, np.random.default_rng(SEED + 5))
    cands[0, [1, 4]] = (-1, ITEMS)                                           # unlisted entries among listed ones
    cands[1] = (-1, ITEMS, 2 ** 31 - 1, -2 ** 31, ITEMS + 7, -5)              # nothing listed
    cands[2, :5] = -1                                                        # only the last column is listed
    cands[3, 1:] = ITEMS                                                     # only the first
    users[4], users[5], users[6] = -1, USERS, 2 ** 40                        # users outside the table
    score64 = hm.scores(tabs[0], tabs[1], w, users, cands)
    neg, pos, val = got = _run(tabs, w, users, cands)
    _verify(score64, cands, got, tol(d, w), ("unlisted", col0))
    for r in (1, 4, 5, 6):
        assert neg[r] == -1 and pos[r] == -1 and np.isneginf(val[r])
    assert pos[0] not in (1, 4) and pos[2] == 5 and pos[3] == 0
    assert ((neg >= 0) & (neg < ITEMS) | (neg == -1)).all()


def test_empty_launch_and_torch_op():
    from elimrec_amd import ops, torch_ops
    tabs = _tables(20, 2)
    w = [1.0, 0.5]
    out = torch.full((4,), CANARY_I, dtype=torch.int64, device=DEV)
    ops.pick_hard_negatives(tabs[2], tabs[3], tabs[4], tabs[5], w, torch.zeros(0, dtype=torch.int64, device=DEV),
                            torch.zeros(0, 3, dtype=torch.int32, device=DEV), out)
    torch.cuda.synchronize()
    assert (out == CANARY_I).all()
    users, cands = _triplets(70, 9, np.random.default_rng(SEED + 6))
    want = _run(tabs, w, users, cands)
    got = torch_ops.load().pick_hard_negatives(tabs[2], tabs[3], tabs[4], tabs[5], w, _t(users), _t(cands))
    assert [tuple(g.shape) for g in got] == [(70,)] * 3 and [g.dtype for g in got] == [torch.int64, torch.int32, torch.float32]
    for g, x in zip(got, want):
        assert g.cpu().numpy().tobytes() == x.tobytes()
    with pytest.raises(RuntimeError):
        torch_ops.load().pick_hard_negatives(tabs[2], tabs[3], tabs[4], tabs[5], w, _t(users), _t(np.zeros((70, 65), np.int32)))
    with pytest.raises(ValueError):
        ops.pick_hard_negatives(tabs[2], tabs[3], tabs[4], tabs[5], w, _t(users), _t(np.zeros((70, 65), np.int32)), out)


# --------------------------------------------------------------------------- the candidate draw
def test_candidate_draw():
    from elimrec_amd import ops
    n_users, I, n, M, seed = 50, 40, 5000, 5, 2022
    rng = np.random.default_rng(SEED + 7)
    train = {u: np.sort(rng.permutation(I)[:rng.integers(1, 12)]) for u in range(1, n_users)}
    train[0] = np.delete(np.arange(I), 17)                                   # 39 of the 40 items: only item 17 is left
    ids = np.arange(n_users, dtype=np.int32)
    ptr = np.concatenate([[0], np.cumsum([len(train[u]) for u in ids])]).astype(np.int64)
    items = np.concatenate([train[u] for u in ids]).astype(np.int32)
    dev = (_t(ids), _t(ptr), _t(items))

    def uniform(epoch):
        u, p, q = (torch.empty(n, dtype=torch.int64, device=DEV) for _ in range(3))
        ops.sample_triplets(*dev, I, n, seed, epoch, u, p, q)
        return u.cpu().numpy(), p.cpu().numpy(), q.cpu().numpy()

    def draw(epoch, m=M):
        u = torch.full((n + 2 * PAD,), CANARY_I, dtype=torch.int64, device=DEV)
        p = u.clone()
        c = torch.full((n + 2 * PAD, m), CANARY_I, dtype=torch.int32, device=DEV)
        ops.sample_triplet_candidates(*dev, I, n, seed, epoch, m, u[PAD:PAD + n], p[PAD:PAD + n], c[PAD:PAD + n])
        torch.cuda.synchronize()
        for x in (u, p, c):
            x = x.cpu().numpy()
            assert (x[:PAD] == CANARY_I).all() and (x[PAD + n:] == CANARY_I).all()
        return u[PAD:PAD + n].cpu().numpy(), p[PAD:PAD + n].cpu().numpy(), c[PAD:PAD + n].cpu().numpy()

    u0, p0, q0 = uniform(3)
    u, p, c = draw(3)
    assert u.tobytes() == u0.tobytes() and p.tobytes() == p0.tobytes() and c[:, 0].astype(np.int64).tobytes() == q0.tobytes()
    assert (c >= 0).all() and (c < I).all()
    member = np.zeros((n_users, I), dtype=bool)
    for k, v in train.items():
        member[k, v] = True
    assert not member[u[:, None], c].any(), "a candidate is one of its user's training items"
    # the user holding 39 of 40 items: the rejection loop alone (510 draws find item 17 with probability 1 - 2.5e-6 per negative,
    # and with one id missing the fallback would give the same answer); test_sampler_gpu.py reaches the fallback
    assert (u == 0).any() and (c[u == 0] == 17).all()
    for j in range(1, M):
        assert (c[:, j] != c[:, 0]).any(), j
        for k in range(j):
            assert (c[:, j] != c[:, k]).any(), (j, k)
    u1, p1, c1 = draw(4)
    assert (u1 != u).any() and (c1 != c).any()
    uu, pp, c1col = draw(3, 1)                                               # one candidate: the uniform draw
    assert uu.tobytes() == u0.tobytes() and pp.tobytes() == p0.tobytes() and c1col[:, 0].astype(np.int64).tobytes() == q0.tobytes()
    wide = draw(3, 64)[2]                                                    # the widest draw keeps the narrower one's columns
    assert wide[:, :M].tobytes() == c.tobytes()


# --------------------------------------------------------------------------- the model, the sampler and the driver
def _forward(name="ml3"):
    from helpers import build_model_from_fixture, load_golden
    g = load_golden(name)
    model, _ = build_model_from_fixture(g, DEV)
    model.bpr_loss(_t(g["step1/users"]), _t(g["step1/pos"]), _t(g["step1/neg"]))
    return model


def test_model_front():
    from helpers import build_model_from_fixture, load_golden
    from elimrec_amd.evaluator import CandidateScoringError
    fresh, _ = build_model_from_fixture(load_golden("ml3"), DEV)
    rng = np.random.default_rng(SEED + 8)
    n, M = 400, 7
    users = rng.integers(0, fresh.num_users, n).astype(np.int64)
    cands = rng.integers(0, fresh.num_items, (n, M)).astype(np.int32)
    assert not fresh.has_cached_tables()
    with pytest.raises(RuntimeError):
        fresh.hard_negatives_device(_t(users), _t(cands))
    model = _forward()
    assert model.has_cached_tables()
    with pytest.raises(ValueError, match="space"):
        model.hard_negatives_device(_t(users), _t(cands), space="x")
    U, I, d, nb = model.num_users, model.num_items, model.latent_dim, 1 + model.S
    model.hard_negatives_device(_t(users), _t(cands))                       # (the tables are realised before Y is read back)
    Y = model._ws["Y"].cpu().numpy()
    alpha = float(model.config["alpha"])
    mask = model._head_mask()
    spaces = {"fused": [1.0] + [0.0] * model.S,
              "loss": [1.0] + [alpha if (mask >> h) & 1 and model.predict_type != "normal" else 0.0 for h in range(model.S)]}
    for h, m in enumerate(model._mods):
        spaces[m] = [1.0 if b == 1 + h else 0.0 for b in range(nb)]
    assert any(x != 0.0 for x in spaces["loss"][1:]), "the fixture trains no single-modal term: 'loss' would only repeat 'fused'"
    for space, w in spaces.items():
        got = [x.cpu().numpy() for x in model.hard_negatives_device(_t(users), _t(cands), space=space)]
        assert [g.dtype for g in got] == [np.int64, np.int32, np.float32]
        _verify(hm.scores(Y[:U, :nb * d], Y[U:U + I, :nb * d], w, users, cands), cands, got, tol(d, w), ("model", space))
    outs = (torch.empty(n, dtype=torch.int64, device=DEV), torch.empty(n, dtype=torch.int32, device=DEV), torch.empty(n, device=DEV))
    back = model.hard_negatives_device(_t(users), _t(cands), "loss", *outs)                 # outputs given by the caller
    want = model.hard_negatives_device(_t(users), _t(cands), space="loss")
    assert all(a is b for a, b in zip(back, outs)) and all(torch.equal(a, b) for a, b in zip(outs, want))
    model._eval_shard = object()
    try:
        with pytest.raises(CandidateScoringError):
            model.hard_negatives_device(_t(users), _t(cands))
    finally:
        model._eval_shard = None


def test_sampler():
    from helpers import FixtureDataset, build_model_from_fixture, load_golden
    from elimrec_amd import PairwiseSamplerV2, ops
    g = load_golden("ml3")
    data = FixtureDataset(g)
    fresh, _ = build_model_from_fixture(g, DEV)

    def epoch_of(sampler, epoch):
        sampler.epoch = epoch
        return [x.cpu().numpy() for x in sampler.sample_epoch()]

    uniform = PairwiseSamplerV2(data, device=DEV, seed=5)
    want = epoch_of(uniform, 2)
    hard = PairwiseSamplerV2(data, device=DEV, seed=5, neg_sampling="hard", neg_candidates=6, model=fresh)
    got = epoch_of(hard, 2)                                                  # no tables yet: the uniform epoch, bit for bit
    assert all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(got, want)) and hard.epoch == 3
    assert hard.last_stats["hard"] is False and hard.last_stats["moved"] == 0.0
    model = _forward()
    one = PairwiseSamplerV2(data, device=DEV, seed=5, neg_sampling="hard", neg_candidates=1, neg_space="loss", model=model)
    got = epoch_of(one, 2)                                                   # M = 1: the uniform epoch after a forward too
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
    assert one.last_stats["hard"] is True and one.last_stats["moved"] == 0.0 and one.last_stats["score_picked"] == one.last_stats["score_first"]
    train = data.get_user_train_dict()
    for space in ("fused", "loss"):
        hard = PairwiseSamplerV2(data, device=DEV, seed=5, neg_sampling="hard", neg_candidates=6, neg_space=space, model=model)
        u, p, q = epoch_of(hard, 2)
        assert u.tobytes() == want[0].tobytes() and p.tobytes() == want[1].tobytes() and q.dtype == np.int64
        n = hard.num_trainings
        cands = torch.empty(n, 6, dtype=torch.int32, device=DEV)
        ops.sample_triplet_candidates(*hard._dev, data.num_items, n, 5, 2, 6, torch.empty(n, dtype=torch.int64, device=DEV),
                                      torch.empty(n, dtype=torch.int64, device=DEV), cands)
        neg, pos, score = model.hard_negatives_device(_t(u), cands, space=space)
        first = model.hard_negatives_device(_t(u), cands[:, :1].contiguous(), space=space)[2]
        c = cands.cpu().numpy()
        assert c[:, 0].astype(np.int64).tobytes() == want[2].tobytes()
        assert q.tobytes() == neg.cpu().numpy().tobytes()
        assert (q[:, None] == c).any(1).all(), "a negative that is not one of its triplet's candidates"
        assert all(int(i) not in set(train[int(a)]) for a, i in zip(u, q)), "a negative that is a training item"
        assert (score >= first).all(), "a pick that scores below candidate 0"
        st = hard.last_stats
        assert st == dict(hard=True, moved=float((pos != 0).float().mean().item()), score_picked=float(score.mean().item()),
                          score_first=float(first.mean().item()))
        assert 0.0 < st["moved"] < 1.0 and st["score_picked"] > st["score_first"]
        print("hard epoch on the fixture, space %s: %s" % (space, st))
    batches = list(hard)
    assert len(batches) == len(hard) and sum(b[2].numel() for b in batches) == hard.num_trainings


def test_driver_switch(tmp_path):
    import os
    from elimrec_amd import Logger
    from test_lists_gpu import ROOT, _Capture, _net
    net = _net(tmp_path, ["--neg_sampling=hard", "--neg_candidates=4"])
    losses, train_epoch = [], net.train_epoch
    net.train_epoch = lambda batches: losses.append(train_epoch(batches)) or losses[-1]
    before, cwd = Logger.logger, os.getcwd()
    cap = Logger.logger = _Capture()
    os.chdir(ROOT)
    try:
        net.run()
    finally:
        os.chdir(cwd)
        Logger.logger = before
    lines = [ln for ln in cap.lines if ln.startswith("[hard negatives]")]
    assert len(lines) == 2 and lines[0] == "[hard negatives] uniform (no tables yet)", lines
    assert lines[1].startswith("[hard negatives] best of 4 in 'fused': ") and "moved" in lines[1]
    assert len(losses) == 2 and all(np.isfinite(x) for x in losses), losses
    with pytest.raises(ValueError, match="neg_sampling"):
        _net(tmp_path / "bad", ["--neg_sampling=hardest"])
