"""The inputs shared by test_sampler_cpu.py and test_sampler_gpu.py, and the conditions that say they reach every branch of the
three contracts -- computed by tests/sampler_model.py's records alone, asserted in both files."""
import functools

import numpy as np

import sampler_model as sm

SEEDS = (0, 2022, 2 ** 63 + 5)                                               # both key words matter
EPOCHS = (0, 1, 2 ** 32 - 1, 2 ** 32, (5 << 32) | 9, (1 << 56) | 3)          # bits 32 .. 55 reach counter word 3, 56 .. 63 are dropped
NS = (1, 255, 256, 257, 4096)                                                # the kernel's block is 256 threads
N_DENSE = 400
CAND_MS = (1, 2, 5, 64)
N_NEGS = (1, 63, 64, 65, 700)
NEG_SEEDS = (77, 77 + (9 << 32))                                             # differ in the high word only
I_DENSE = 4096


def _graph(user_ids, slices, I):
    slices = [np.sort(np.asarray(s, dtype=np.int32)) for s in slices]
    assert len(user_ids) == len(slices) and len(set(user_ids)) == len(user_ids)
    assert all(0 < len(s) < I and len(np.unique(s)) == len(s) and s[0] >= 0 and s[-1] < I for s in slices)
    ptr = np.concatenate([[0], np.cumsum([len(s) for s in slices])]).astype(np.int64)
    return np.asarray(user_ids, dtype=np.int32), ptr, np.concatenate(slices), I


def _all_but(missing):
    return np.setdiff1d(np.arange(I_DENSE), missing)


ORD_USERS, ORD_ITEMS = 150, 301


@functools.lru_cache(maxsize=None)
def graph(name):
    """-> (user_ids int32, ptr int64, items int32, I).
    ordinary: 150 users whose ids are a permutation with gaps, I = 301. Slot 0 (ptr = 0) holds 3 items with item 0, slot 1 one item,
        slot 2 items 0 and I - 1, slot 3 every even id, slot 4 all but 5 ids, the last slot 2 items with I - 1.
    dense: ONE user holding all but ids 1234 and 4000 of 4096 (two missing ids: the fallback gives 1234, the rejection loop either).
    dense_edges: two users holding all but {0, 4095} and all but {0, 1} (the fallback's k = 0 exit, the ends of the slice)."""
    if name == "dense":
        return _graph([5], [_all_but([1234, 4000])], I_DENSE)
    if name == "dense_edges":
        return _graph([7, 3], [_all_but([0, 4095]), _all_but([0, 1])], I_DENSE)
    assert name == "ordinary"
    rng = np.random.default_rng(20221)
    I = ORD_ITEMS
    ids = rng.permutation(4 * ORD_USERS)[:ORD_USERS] + 11
    slices = [rng.permutation(I)[:rng.integers(1, 40)] for _ in range(ORD_USERS)]
    slices[0] = [0, 17, 150]
    slices[1] = [123]
    slices[2] = [0, 5, 6, 7, 200, I - 1]
    slices[3] = np.arange(0, I, 2)
    slices[4] = np.setdiff1d(np.arange(I), [3, 99, 100, 250, I - 1])
    slices[-1] = [44, I - 1]
    return _graph(ids, slices, I)


GRAPHS = ("ordinary", "dense", "dense_edges")


def graph_n(name):
    return NS[-1] if name == "ordinary" else N_DENSE


@functools.lru_cache(maxsize=None)
def model_triplets(name, seed, epoch):
    """The model's longest run on a graph; triplet i depends on (seed, epoch, i) alone, so a shorter run is its prefix."""
    ids, ptr, items, I = graph(name)
    (u, p, q), rec = sm.triplets(ids, ptr, items, I, graph_n(name), seed, epoch)
    for a in (u, p, q, rec.round, rec.half):
        a.setflags(write=False)
    return (u, p, q), rec


CAND_N = {"ordinary": 1025, "dense": 70, "dense_edges": 70}                  # x 64 columns: more than one block each


@functools.lru_cache(maxsize=None)
def model_candidates(name, seed, epoch):
    """The model's widest draw (64 columns); column j depends on (seed, epoch, i, j) alone, so a narrower draw is its prefix."""
    ids, ptr, items, I = graph(name)
    (u, p, c), rec = sm.candidates(ids, ptr, items, I, CAND_N[name], seed, epoch, CAND_MS[-1])
    for a in (u, p, c, rec.round, rec.half):
        a.setflags(write=False)
    return (u, p, c), rec


def check_triplet_reach(name, out, rec):
    """The conditions of a graph on one model run of graph_n(name) triplets."""
    ids, ptr, items, I = graph(name)
    users, pos, neg = out
    fell = rec.round == sm.FALLBACK
    if name == "ordinary":
        assert not fell.any()
        assert {int(ids[0]), int(ids[1]), int(ids[2]), int(ids[-1])} <= set(users.tolist())     # ptr = 0, one item, the last user
        assert not set(users.tolist()) & set(range(len(ids))) - set(ids.tolist())               # ids, not slots
        assert (rec.round >= 3).any() and (rec.half == 1).any() and (rec.half == 0).any()
        assert (neg == 0).any() and (neg == I - 1).any() and (pos == 0).any() and (pos == I - 1).any()
        return
    for slot, uid in enumerate(ids):
        mine = users == uid
        s = items[ptr[slot]:ptr[slot + 1]]
        missing = np.setdiff1d(np.arange(I), s)
        assert len(missing) == 2
        need = 20 if name == "dense" else 10
        assert (mine & fell).sum() >= need and (mine & ~fell).sum() >= need, (name, uid)
        assert (neg[mine & fell] == missing[0]).all()                          # always the smaller missing id
        assert set(neg[mine & ~fell].tolist()) == set(missing.tolist())       # either: fallback and rejection can be told apart
        assert (rec.round[mine] > 128).any() and (rec.half[mine] == 1).any() and (rec.half[mine] == 0).any()


def check_candidate_reach(name, out, rec):
    """Columns j > 0 of the dense users take the fallback and the rejection loop; every column of an ordinary user is drawn."""
    fell = rec.round[:, 1:] == sm.FALLBACK
    if name == "ordinary":
        assert not fell.any() and (rec.round[:, 1:] >= 3).any() and (rec.half[:, 1:] == 1).any()
    else:
        assert fell.any(axis=0).all() and (~fell).any(axis=0).sum() >= 32 and (rec.round[:, 1:] > 128).any()


# ------------------------------------------------------------------------------------------------ exclusion lists
NEG_I = 1000
LIST_AT_0 = np.array([0, 1, 2, 10, 11, 500, 998])                             # starts at 0
LIST_AT_END = np.array([3, 400, 401, 997, 998, 999])                          # ends at I - 1
LIST_RUNS = np.concatenate([np.arange(5, 25), np.arange(26, 30), [31, 33], np.arange(600, 700), np.arange(990, 999)])
ROOMY_I = 1 << 20


def _csr_of(lists):
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return ptr, np.concatenate([np.asarray(x, dtype=np.int32) for x in lists]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def neg_case(n_neg):
    """-> (ptr, excl, I = 1000): user 0 nothing excluded, 1 .. 3 the three lists above, 4 a random list leaving M = n_neg + 1
    ids, 5 one leaving M = n_neg + 40, 6 every id but the last n_neg + 1, 7 every id but the first n_neg + 1."""
    rng = np.random.default_rng(500 + n_neg)
    lists = [[], LIST_AT_0, LIST_AT_END, LIST_RUNS,
             np.sort(rng.permutation(NEG_I)[:NEG_I - n_neg - 1]), np.sort(rng.permutation(NEG_I)[:NEG_I - n_neg - 40]),
             np.arange(NEG_I - n_neg - 1), np.arange(n_neg + 1, NEG_I)]
    return _csr_of(lists) + (NEG_I,)


@functools.lru_cache(maxsize=None)
def roomy_case():
    """-> (ptr, excl, I = 2^20): ranks so many that a round of 64 completes without a drop. Users: nothing excluded, LIST_AT_0, and
    a list ending at I - 1."""
    return _csr_of([[], LIST_AT_0, [5, ROOMY_I - 2, ROOMY_I - 1]]) + (ROOMY_I,)


WIDE = (20000, 16000)                                                         # I, n_neg = NEG_MAX: the ABI's edge


@functools.lru_cache(maxsize=None)
def wide_case():
    rng = np.random.default_rng(16000)
    return _csr_of([np.sort(rng.permutation(WIDE[0])[:1500]), [0, WIDE[0] - 1]]) + (WIDE[0],)


@functools.lru_cache(maxsize=None)
def model_negatives(case, n_neg, seed):
    ptr, excl, I = neg_case(n_neg) if case == "small" else roomy_case() if case == "roomy" else wide_case()
    out, rec = sm.negatives(ptr, excl, I, n_neg, seed)
    out.setflags(write=False)
    return out, rec


def check_negative_reach(case, n_neg, rec):
    rounds, dup_prev, dup_round, surplus = (np.array(x) for x in zip(*rec))
    if case == "roomy":
        if n_neg <= sm.LANES:                                                  # one round, nothing dropped but the surplus
            assert (rounds == 1).all() and not dup_prev.any() and not dup_round.any() and (surplus == sm.LANES - n_neg).all()
        else:
            assert (rounds >= -(-n_neg // sm.LANES)).all() and (rounds <= -(-n_neg // sm.LANES) + 1).all()
        return
    if case == "wide":
        assert (rounds > 250).all() and dup_prev.all() and dup_round.all()
        return
    assert dup_round.all()                                                     # 64 draws over <= 1000 ranks
    assert surplus.any()
    assert dup_round[4] >= 10                                                  # M = n_neg + 1
    if n_neg >= sm.LANES:
        assert (rounds >= 2).all() and dup_prev.all()
    if n_neg == 1:
        assert (rounds[:4] == 1).all() and (surplus[:4] >= 50).all()
