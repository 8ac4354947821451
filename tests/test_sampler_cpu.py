"""tests/sampler_model.py, the numpy model of csrc/sampler.hip's three Philox streams, and the inputs of test_sampler_gpu.py
(tests/sampler_cases.py): the model's draws satisfy the distributional contract, its rank -> id mapping equals a brute-force set
difference, and the inputs reach every branch according to the model's own records. No GPU."""
import numpy as np
import pytest

import sampler_cases as sc
import sampler_model as sm


def _members(ids, ptr, items, I):
    held = np.zeros((int(ids.max()) + 1, I), dtype=bool)
    for slot, uid in enumerate(ids):
        held[uid, items[ptr[slot]:ptr[slot + 1]]] = True
    return held


@pytest.mark.parametrize("name", sc.GRAPHS)
def test_triplets_contract_and_reach(name):
    ids, ptr, items, I = sc.graph(name)
    held = _members(ids, ptr, items, I)
    for seed, epoch in ((2022, 0), (sc.SEEDS[2], sc.EPOCHS[4])):
        (u, p, q), rec = sc.model_triplets(name, seed, epoch)
        assert u.dtype == p.dtype == q.dtype == np.int64 and len(u) == len(p) == len(q) == sc.graph_n(name)
        assert np.isin(u, ids).all() and held[u, p].all()
        assert (q >= 0).all() and (q < I).all() and not held[u, q].any()
        assert ((rec.round == sm.FALLBACK) == (rec.half == -1)).all() and rec.round.max() <= sm.LAST_ROUND
        sc.check_triplet_reach(name, (u, p, q), rec)


def test_triplets_users_are_roughly_uniform():
    """A sanity check of the model, not a pin: 4096 draws over 150 users, chi-square at 5 sigma."""
    ids = sc.graph("ordinary")[0]
    u = sc.model_triplets("ordinary", 2022, 1)[0][0]
    counts = np.array([(u == uid).sum() for uid in ids])
    exp = len(u) / len(ids)
    assert abs(((counts - exp) ** 2 / exp).sum() - (len(ids) - 1)) < 5 * np.sqrt(2 * (len(ids) - 1))


def test_epoch_and_seed_words_reach_the_stream():
    """Epochs 0, 2^32 and (5 << 32) | 9 differ in counter word 3 or 2; bits 56 .. 63 of the epoch are dropped; seeds that differ
    in one key word give different streams; a shorter run is the longer one's prefix."""
    ids, ptr, items, I = sc.graph("ordinary")
    runs = {e: sm.triplets(ids, ptr, items, I, 300, 2022, e)[0] for e in (0, 2 ** 32, (5 << 32) | 9, 3, (1 << 56) | 3, (1 << 55) | 3)}
    for a, b in ((0, 2 ** 32), (0, (5 << 32) | 9), (2 ** 32, (5 << 32) | 9), (3, (1 << 55) | 3)):
        assert all((x != y).any() for x, y in zip(runs[a], runs[b])), (a, b)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(runs[3], runs[(1 << 56) | 3]))
    seeds = {s: sm.triplets(ids, ptr, items, I, 300, s, 0)[0][0] for s in (5, 2 ** 32 + 5, 2 ** 63 + 5, 6)}
    assert all((seeds[5] != seeds[s]).any() for s in (2 ** 32 + 5, 2 ** 63 + 5, 6))
    short = sm.triplets(ids, ptr, items, I, 257, 2022, 0)[0]
    assert all(x.tobytes() == y[:257].tobytes() for x, y in zip(short, runs[0]))


@pytest.mark.parametrize("name", sc.GRAPHS)
def test_candidates_contract_and_reach(name):
    ids, ptr, items, I = sc.graph(name)
    held = _members(ids, ptr, items, I)
    n = sc.CAND_N[name]
    (u, p, c), rec = sc.model_candidates(name, 2022, 0)
    assert c.dtype == np.int32 and c.shape == (n, 64) and rec.round.shape == (n, 64)
    (u0, p0, q0), rec0 = sc.model_triplets(name, 2022, 0)
    assert u.tobytes() == u0[:n].tobytes() and p.tobytes() == p0[:n].tobytes() and c[:, 0].astype(np.int64).tobytes() == q0[:n].tobytes()
    assert (rec.round[:, 0] == rec0.round[:n]).all() and (rec.half[:, 0] == rec0.half[:n]).all()
    assert (c >= 0).all() and (c < I).all() and not held[u[:, None], c].any()
    for j in range(1, 64):
        assert all((c[:, j] != c[:, k]).any() for k in range(j)), j          # no two columns share a counter at an epoch < 2^32
    sc.check_candidate_reach(name, (u, p, c), rec)
    narrow = sm.candidates(ids, ptr, items, I, 50, 2022, 0, 5)[0]
    assert narrow[2].tobytes() == np.ascontiguousarray(c[:50, :5]).tobytes() and narrow[0].tobytes() == u[:50].tobytes()


def test_candidate_columns_above_epoch_2_pow_32():
    """The documented limit: a triplet's own stream carries the epoch's bits 32 .. 55 where column j carries j, so at epoch
    (5 << 32) | 9 column 0 and column 5 are one stream (and no other pair is)."""
    c = sc.model_candidates("ordinary", 2022, (5 << 32) | 9)[0][2]
    same = [(j, k) for j in range(64) for k in range(j) if (c[:, j] == c[:, k]).all()]
    assert same == [(5, 0)]


@pytest.mark.parametrize("excl", [sc.LIST_AT_0, sc.LIST_AT_END, sc.LIST_RUNS], ids=["at_0", "at_end", "runs"])
def test_rank_to_id_by_brute_force(excl):
    allowed = np.setdiff1d(np.arange(sc.NEG_I), excl)
    ranks = np.arange(len(allowed))
    assert np.array_equal(sm.rank_to_id(excl, ranks), allowed[ranks])
    assert np.array_equal(sm.rank_to_id([], ranks), ranks)


def _check_negatives(ptr, excl, I, n_neg, out):
    assert out.dtype == np.int32 and out.shape == (len(ptr) - 1, n_neg)
    for u, row in enumerate(out):
        assert len(set(row.tolist())) == n_neg and row.min() >= 0 and row.max() < I
        assert not np.isin(row, excl[ptr[u]:ptr[u + 1]]).any()


@pytest.mark.parametrize("n_neg", sc.N_NEGS)
def test_negatives_contract_and_reach(n_neg):
    ptr, excl, I = sc.neg_case(n_neg)
    assert len(excl[ptr[0]:ptr[1]]) == 0 and I - (ptr[5] - ptr[4]) == n_neg + 1
    outs = []
    for seed in sc.NEG_SEEDS:
        out, rec = sc.model_negatives("small", n_neg, seed)
        _check_negatives(ptr, excl, I, n_neg, out)
        sc.check_negative_reach("small", n_neg, rec)
        outs.append(out)
    assert (outs[0] != outs[1]).any()                                          # the seed's high word is a key word
    ptr, excl, I = sc.roomy_case()
    out, rec = sc.model_negatives("roomy", n_neg, sc.NEG_SEEDS[0])
    _check_negatives(ptr, excl, I, n_neg, out)
    sc.check_negative_reach("roomy", n_neg, rec)


def test_negatives_records_over_all_counts():
    """Across the n_neg values every kind of drop occurs: against earlier rounds, within a round, surplus."""
    recs = [r for n_neg in sc.N_NEGS for r in sc.model_negatives("small", n_neg, sc.NEG_SEEDS[0])[1]]
    assert any(r.dup_prev for r in recs) and any(r.dup_round for r in recs) and any(r.surplus for r in recs)
    assert any(r.rounds == 1 for r in recs) and any(r.rounds > 10 for r in recs)


def test_negatives_wide_case():
    ptr, excl, I = sc.wide_case()
    out, rec = sc.model_negatives("wide", sc.WIDE[1], sc.NEG_SEEDS[0])
    _check_negatives(ptr, excl, I, sc.WIDE[1], out)
    sc.check_negative_reach("wide", sc.WIDE[1], rec)
    assert max(r.rounds for r in rec) < 1 << 12                                # far from the 2^16 rounds of the closing fallback


def test_negatives_small_rounds_per_call_is_the_same_stream():
    ptr, excl, I = sc.neg_case(65)
    a = sm.negatives(ptr, excl, I, 65, 9, rounds_per_call=1)
    b = sm.negatives(ptr, excl, I, 65, 9)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]
