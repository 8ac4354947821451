"""A numpy model of the three sampler contracts (include/elimrec_hip.h: elimrec_sample_triplets, elimrec_sample_triplet_candidates,
elimrec_sample_negatives; csrc/sampler.hip), written from their comments: which Philox4x32-10 counter makes which draw, the `%`
reductions, the rejection rounds and the fallback. Bitwise: the tests compare tobytes(). Philox itself is bootstrap_model.philox4x32
(checked against Random123's known answers in test_bootstrap_cpu.py). Calls no project code.

Each function also returns a record of the branches it took, so that a test can assert that its inputs reach them:
  triplets / candidates -> Draws(round, half): per triplet (per triplet and column) the round 1 .. 255 and the half 0 / 1 of that
      round's four words that gave the negative; round = FALLBACK (0), half = -1 where all 255 rounds were rejected;
  negatives -> NegRecord per user: rounds, dup_prev (draws dropped as kept by an earlier round), dup_round (dropped as drawn by an
      earlier lane of the same round), surplus (fresh ranks beyond n_neg in the last round)."""
import collections

import numpy as np

from bootstrap_model import philox4x32

U64 = np.uint64
M32 = U64(0xFFFFFFFF)
S32 = U64(32)
FALLBACK = 0                 # Draws.round of a negative that came from the fallback
LAST_ROUND = 255
LANES = 64

Draws = collections.namedtuple("Draws", "round half")
NegRecord = collections.namedtuple("NegRecord", "rounds dup_prev dup_round surplus")


def _key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def _u64(hi, lo):
    return (hi << S32) | lo


def _csr(user_ids, ptr, items):
    return np.asarray(user_ids, dtype=np.int64), np.asarray(ptr, dtype=np.int64), np.asarray(items, dtype=np.int64)


def _user_pos(user_ids, ptr, items, n, seed, epoch):
    """Round 0 of every triplet's stream -> (ui, users, pos): counter (i lo, i hi, epoch lo, epoch bits 32 .. 55)."""
    epoch = int(epoch) & 0xFFFFFFFFFFFFFFFF
    i = np.arange(n, dtype=U64)
    r = philox4x32((i & M32, i >> S32, epoch & 0xFFFFFFFF, (epoch >> 32) & 0xFFFFFF), _key(seed))
    ui = (_u64(r[:, 0], r[:, 1]) % U64(len(user_ids))).astype(np.int64)
    beg, cnt = ptr[ui], ptr[ui + 1] - ptr[ui]
    off = (_u64(r[:, 2], r[:, 3]) % cnt.astype(U64)).astype(np.int64)
    return ui, user_ids[ui], items[beg + off]


def _first_missing(ptr, items):
    """Per user the smallest k with items[beg + k] != k (the slice's length if there is none): the fallback's answer."""
    out = np.empty(len(ptr) - 1, dtype=np.int64)
    for u in range(len(out)):
        s = items[ptr[u]:ptr[u + 1]]
        off = np.nonzero(s != np.arange(len(s)))[0]
        out[u] = off[0] if len(off) else len(s)
    return out


def _outside(i, ui, low24, ptr, items, I, seed, epoch):
    """One negative per entry of the flat arrays (i, ui, low24): rounds 1 .. 255 of the stream whose counter word 3 is
    low24 | round << 24, two 64-bit draws % I per round, the first draw not among the user's items; then the fallback."""
    key, e_lo = _key(seed), int(epoch) & 0xFFFFFFFF
    member = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr)) * I + items        # ascending: slices are sorted
    neg = np.full(len(i), -1, dtype=np.int64)
    rnd = np.full(len(i), FALLBACK, dtype=np.int64)
    half = np.full(len(i), -1, dtype=np.int64)
    live = np.arange(len(i))
    for k in range(1, LAST_ROUND + 1):
        if not len(live):
            break
        ii = i[live].astype(U64)
        r = philox4x32((ii & M32, ii >> S32, e_lo, low24[live].astype(U64) | U64(k << 24)), key)
        for t in (0, 1):
            a = (_u64(r[:, 2 * t], r[:, 2 * t + 1]) % U64(I)).astype(np.int64)
            q = ui[live] * I + a
            at = np.searchsorted(member, q)
            held = member[np.minimum(at, len(member) - 1)] == q
            take = ~held & (neg[live] < 0)
            neg[live[take]], rnd[live[take]], half[live[take]] = a[take], k, t
        live = live[neg[live] < 0]
    neg[live] = _first_missing(ptr, items)[ui[live]]
    return neg, Draws(rnd, half)


def triplets(user_ids, ptr, items, I, n, seed, epoch):
    """-> (users int64 [n], pos int64 [n], neg int64 [n]), Draws with [n] records."""
    user_ids, ptr, items = _csr(user_ids, ptr, items)
    ui, users, pos = _user_pos(user_ids, ptr, items, n, seed, epoch)
    low24 = np.full(n, (int(epoch) >> 32) & 0xFFFFFF, dtype=np.int64)
    neg, rec = _outside(np.arange(n, dtype=np.int64), ui, low24, ptr, items, int(I), seed, epoch)
    return (users, pos, neg), rec


def candidates(user_ids, ptr, items, I, n, seed, epoch, M):
    """-> (users int64 [n], pos int64 [n], cands int32 [n x M]), Draws with [n x M] records. Column 0: the triplet's own stream;
    column j >= 1: the low 24 bits of counter word 3 carry j."""
    user_ids, ptr, items = _csr(user_ids, ptr, items)
    ui, users, pos = _user_pos(user_ids, ptr, items, n, seed, epoch)
    low24 = np.tile(np.arange(M, dtype=np.int64), (n, 1))
    low24[:, 0] = (int(epoch) >> 32) & 0xFFFFFF
    neg, rec = _outside(np.repeat(np.arange(n, dtype=np.int64), M), np.repeat(ui, M), low24.reshape(-1), ptr, items, int(I), seed,
                        epoch)
    return (users, pos, neg.reshape(n, M).astype(np.int32)), Draws(rec.round.reshape(n, M), rec.half.reshape(n, M))


def rank_to_id(excl, rank):
    """The rank-th id (from 0) not in the sorted unique list excl: rank + #{j : excl[j] - j <= rank}."""
    excl = np.asarray(excl, dtype=np.int64)
    rank = np.asarray(rank, dtype=np.int64)
    return rank + np.searchsorted(excl - np.arange(len(excl)), rank, side="right")


def negatives(ptr, excl, I, n_neg, seed, rounds_per_call=64):
    """-> int32 [n_users x n_neg] in draw order, [NegRecord per user]. Key = the seed, counter (u lo, u hi, round, lane); the
    rank of (round, lane) is the 64-bit draw of words 0, 1 % (I - |excl_u|); a round's 64 lanes are taken in lane order."""
    ptr, excl = np.asarray(ptr, dtype=np.int64), np.asarray(excl, dtype=np.int64)
    key, n_users = _key(seed), len(ptr) - 1
    out = np.empty((n_users, n_neg), dtype=np.int32)
    records = []
    lane = np.arange(LANES, dtype=U64)
    for u in range(n_users):
        e = excl[ptr[u]:ptr[u + 1]]
        M = int(I) - len(e)
        assert M > n_neg, "the caller rejects I - |exclusion| <= n_neg"
        kept, n_acc = np.empty(n_neg, dtype=np.int64), 0
        seen = np.zeros(M, dtype=bool) if M <= 1 << 26 else None
        rnd = dup_prev = dup_round = surplus = 0
        while n_acc < n_neg:
            rs = np.arange(rnd, rnd + rounds_per_call, dtype=U64)[:, None]
            r = philox4x32((u & 0xFFFFFFFF, u >> 32, rs, lane[None, :]), key)
            ranks = (_u64(r[..., 0], r[..., 1]) % U64(M)).astype(np.int64)
            for c in ranks:
                old = seen[c] if seen is not None else np.isin(c, kept[:n_acc])
                first = np.zeros(LANES, dtype=bool)
                first[np.unique(c, return_index=True)[1]] = True
                ok = ~old & first
                fresh = c[ok]                                                         # in lane order
                take = min(len(fresh), n_neg - n_acc)
                kept[n_acc:n_acc + take] = fresh[:take]
                if seen is not None:
                    seen[fresh[:take]] = True
                n_acc += take
                rnd, dup_prev, dup_round, surplus = rnd + 1, dup_prev + int(old.sum()), dup_round + int((~old & ~first).sum()), \
                    surplus + len(fresh) - take
                if n_acc == n_neg:
                    break
        assert rnd <= 1 << 16, "the kernel's closing fallback is not modelled (unreachable for n_neg <= 16000)"
        out[u] = rank_to_id(e, kept)
        records.append(NegRecord(rnd, dup_prev, dup_round, surplus))
    return out, records
