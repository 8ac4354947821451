"""csrc/sampler.hip against tests/sampler_model.py, bit for bit: sample_triplets_kernel, sample_triplet_candidates_kernel and
sample_negatives_kernel draw the Philox streams that include/elimrec_hip.h spells out, and PairwiseSamplerV2 and the data set's
evaluation negatives hand exactly those streams on. Every comparison is tobytes() equality; every output lies between canaries.

The inputs are those of tests/sampler_cases.py, whose reach conditions (computed by the model's records, also asserted in
test_sampler_cpu.py) say that the rejection loop's late rounds and second halves, draw_outside's fallback with its k = 0 exit, both
ends of a slice and of an exclusion list, duplicates against earlier rounds and within a round, and surplus ranks all occur.

Unreachable, not tested: the closing fallback of sample_negatives_kernel (2^16 rounds without n_neg distinct ranks). Dropping
duplicates in lane order makes the rounds one sequence of T = 64 * 2^16 = 4.19e6 draws; the call needs the fallback only if more than
M - n_neg ranks are still undrawn after them. The slowest admissible case is n_neg = NEG_MAX = 16000 of M = 16001 ranks (a coupon
collector stopped one short: M (H_M - 1) = 1.48e5 draws = 2.3e3 rounds on average): two given ranks are both undrawn with probability
(1 - 2 / M)^T = e^-524, and there are M^2 / 2 = 1.3e8 pairs, so P(fallback) < 1e-219 per user. A smaller n_neg or a larger M only
lowers it: no input of the ABI (n_neg <= NEG_MAX) reaches the branch."""
import numpy as np
import pytest
import torch

import sampler_cases as sc
import sampler_model as sm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY, PAD = 77, 5


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _between_canaries(shape, dtype):
    """A canary-filled buffer with PAD rows on either side of `shape` -> (buffer, the view to write)."""
    buf = torch.full((shape[0] + 2 * PAD,) + tuple(shape[1:]), CANARY, dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + shape[0]]


def _result(buf, n):
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:PAD] == CANARY).all() and (host[PAD + n:] == CANARY).all(), "a write outside the output"
    return host[PAD:PAD + n]


def _device_graph(name):
    ids, ptr, items, I = sc.graph(name)
    return (_t(ids), _t(ptr), _t(items)), I


def _triplets(dev, I, n, seed, epoch):
    from elimrec_amd import ops
    bufs = [_between_canaries((n,), torch.int64) for _ in range(3)]
    ops.sample_triplets(*dev, I, n, seed, epoch, *(view for _, view in bufs))
    return [_result(buf, n) for buf, _ in bufs]


def _candidates(dev, I, n, seed, epoch, M):
    from elimrec_amd import ops
    bufs = [_between_canaries((n,), torch.int64), _between_canaries((n,), torch.int64), _between_canaries((n, M), torch.int32)]
    ops.sample_triplet_candidates(*dev, I, n, seed, epoch, M, *(view for _, view in bufs))
    return [_result(buf, n) for buf, _ in bufs]


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == np.ascontiguousarray(want).tobytes()


def _stream_pairs(name):
    """Every (seed, epoch) on the ordinary graph; on the dense ones (255 model rounds per triplet) every epoch under one seed and
    every seed under two epochs."""
    if name == "ordinary":
        return [(s, e) for s in sc.SEEDS for e in sc.EPOCHS]
    return [(2022, e) for e in sc.EPOCHS] + [(s, e) for s in (sc.SEEDS[0], sc.SEEDS[2]) for e in (0, (5 << 32) | 9)]


TRIPLET_CASES = [(g, s, e) for g in sc.GRAPHS for s, e in _stream_pairs(g)]


@pytest.mark.parametrize("name,seed,epoch", TRIPLET_CASES, ids=["%s-%x-%x" % c for c in TRIPLET_CASES])
def test_triplets_bitwise(name, seed, epoch):
    dev, I = _device_graph(name)
    want, rec = sc.model_triplets(name, seed, epoch)
    if (seed, epoch) == (2022, 0):
        sc.check_triplet_reach(name, want, rec)
    n_max = sc.graph_n(name)
    for n in sorted(set(min(n, n_max) for n in sc.NS)):
        got = _triplets(dev, I, n, seed, epoch)
        for what, g, w in zip(("users", "pos", "neg"), got, want):
            assert _same(g, w[:n]), (what, n, int((g != w[:n]).sum()), np.nonzero(g != w[:n])[0][:5])


def test_epochs_differ_in_the_model():
    """What the bitwise comparisons above then hold the kernel to: the epoch's word 2 and its bits 32 .. 55 reach the stream."""
    u = {e: sc.model_triplets("ordinary", 2022, e)[0][0] for e in (0, 2 ** 32, (5 << 32) | 9)}
    assert (u[0] != u[2 ** 32]).any() and (u[0] != u[(5 << 32) | 9]).any() and (u[2 ** 32] != u[(5 << 32) | 9]).any()


CAND_CASES = [(g, 2022, e) for g in sc.GRAPHS for e in sc.EPOCHS] + [("ordinary", s, 0) for s in (sc.SEEDS[0], sc.SEEDS[2])]


@pytest.mark.parametrize("name,seed,epoch", CAND_CASES, ids=["%s-%x-%x" % c for c in CAND_CASES])
def test_candidates_bitwise(name, seed, epoch):
    dev, I = _device_graph(name)
    (wu, wp, wc), rec = sc.model_candidates(name, seed, epoch)
    if epoch == 0:
        sc.check_candidate_reach(name, (wu, wp, wc), rec)
    n = sc.CAND_N[name]
    tu, tp, tq = _triplets(dev, I, n, seed, epoch)
    for M in sc.CAND_MS:
        u, p, c = _candidates(dev, I, n, seed, epoch, M)
        assert _same(u, wu) and _same(p, wp), M
        assert u.tobytes() == tu.tobytes() and p.tobytes() == tp.tobytes(), M       # the triplet run's bits
        assert c[:, 0].astype(np.int64).tobytes() == tq.tobytes(), M
        assert _same(c, wc[:, :M]), (M, np.argwhere(c != wc[:, :M])[:5])


def _negatives(ptr, excl, I, n_neg, seed):
    from elimrec_amd import ops
    buf, view = _between_canaries((len(ptr) - 1, n_neg), torch.int32)
    ops.sample_negatives(_t(ptr), _t(excl), I, n_neg, seed, view)
    return _result(buf, len(ptr) - 1)


@pytest.mark.parametrize("n_neg", sc.N_NEGS)
def test_negatives_bitwise(n_neg):
    for seed in sc.NEG_SEEDS:
        want, rec = sc.model_negatives("small", n_neg, seed)
        sc.check_negative_reach("small", n_neg, rec)
        got = _negatives(*sc.neg_case(n_neg), n_neg, seed)
        assert _same(got, want), (seed, np.argwhere(got != want)[:5])
    want, rec = sc.model_negatives("roomy", n_neg, sc.NEG_SEEDS[1])
    sc.check_negative_reach("roomy", n_neg, rec)
    assert _same(_negatives(*sc.roomy_case(), n_neg, sc.NEG_SEEDS[1]), want)


def test_negatives_bitwise_at_neg_max():
    I, n_neg = sc.WIDE
    want, rec = sc.model_negatives("wide", n_neg, sc.NEG_SEEDS[0])
    sc.check_negative_reach("wide", n_neg, rec)
    got = _negatives(*sc.wide_case(), n_neg, sc.NEG_SEEDS[0])
    assert _same(got, want), np.argwhere(got != want)[:5]


# ------------------------------------------------------------------------------------------------ through the classes
def _csr_of_train(ds):
    train = ds.get_user_train_dict()
    ids = np.fromiter(train.keys(), dtype=np.int32, count=len(train))
    ptr = np.concatenate([[0], np.cumsum([len(train[u]) for u in ids])]).astype(np.int64)
    items = np.concatenate([np.sort(np.asarray(train[u], dtype=np.int32)) for u in ids])
    return ids, ptr, items, sum(len(v) for v in train.values())


def _epoch(sampler):
    return [x.cpu().numpy() for x in sampler.sample_epoch()]


def test_pairwise_sampler_epochs_resume_and_shards():
    from elimrec_amd import PairwiseSamplerV2, SyntheticDataset
    ds = SyntheticDataset(120, 200, 2400, feat_dims=(4, 4, 4), seed=2)
    ids, ptr, items, n = _csr_of_train(ds)
    seed = 2 ** 63 + 5
    want = [sm.triplets(ids, ptr, items, ds.num_items, n, seed, e)[0] for e in range(3)]
    smp = PairwiseSamplerV2(ds, batch_size=512, device=DEV, seed=seed)
    assert smp.num_trainings == n
    for e in range(3):
        assert smp.epoch == e
        assert all(_same(g, w) for g, w in zip(_epoch(smp), want[e])), e
    resumed = PairwiseSamplerV2(ds, batch_size=512, device=DEV, seed=seed)
    resumed.epoch = 2
    assert all(_same(g, w) for g, w in zip(_epoch(resumed), want[2]))
    batches = list(PairwiseSamplerV2(ds, batch_size=512, device=DEV, seed=seed))         # the batches are views of epoch 0, in order
    assert all(_same(np.concatenate([b[k].cpu().numpy() for b in batches]), want[0][k]) for k in range(3))
    W = 5
    share = -(-n // W)
    assert share * W != n                                                                # the share is rounded up
    for r in range(W):
        shard = PairwiseSamplerV2(ds, batch_size=512, device=DEV, seed=2022 + r, shard=(r, W))
        assert shard.num_trainings == share
        w = sm.triplets(ids, ptr, items, ds.num_items, share, 2022 + r, 0)[0]
        assert all(_same(g, x) for g, x in zip(_epoch(shard), w)), r


def test_hard_sampler_without_tables_is_the_models_column_0():
    from helpers import FixtureDataset, build_model_from_fixture, load_golden
    from elimrec_amd import PairwiseSamplerV2
    g = load_golden("ml3")
    data = FixtureDataset(g)
    model, _ = build_model_from_fixture(g, DEV)
    assert not model.has_cached_tables()
    ids, ptr, items, n = _csr_of_train(data)
    hard = PairwiseSamplerV2(data, device=DEV, seed=5, neg_sampling="hard", neg_candidates=6, model=model)
    for e in (0, 1):
        (wu, wp, wc), _ = sm.candidates(ids, ptr, items, data.num_items, n, 5, e, 6)
        u, p, q = _epoch(hard)
        assert _same(u, wu) and _same(p, wp) and _same(q, wc[:, 0].astype(np.int64)), e
        assert hard.last_stats["hard"] is False
        (tu, tp, tq), _ = sm.triplets(ids, ptr, items, data.num_items, n, 5, e)
        assert _same(q, tq)


def test_dataset_evaluation_negatives():
    from elimrec_amd import SyntheticDataset
    ds = SyntheticDataset(120, 200, 2400, feat_dims=(4, 4, 4), seed=2)
    assert ds.neg_seed == 2024
    neg = ds.get_user_test_neg_dict(15)
    ptr, excl = ds.exclusion_csr()
    want, _ = sm.negatives(ptr, excl, ds.num_items, 15, ds.neg_seed)
    users = np.nonzero(np.diff(ptr) > 0)[0]
    assert sorted(neg) == users.tolist() and len(users) == 120
    for u in users:
        assert neg[int(u)] == sorted(want[u].tolist()), u
