"""Epoch-level pairwise sampler with the interface of the reference's `PairwiseSamplerV2`
(data/sampler.py:297-351): iterate -> (users, pos_items, neg_items) batches, `len()` = number of
batches. Sampling itself runs on the GPU (csrc/sampler.hip): the whole epoch of
`num_trainings` triplets is drawn in one launch and the batches are device-tensor views, so the
training loop does no per-batch host->device copy.

Contract (tests/test_hip_parity.py::test_sampler_contract_on_device): users uniform with replacement over users that have >= 1
training item; positives uniform over that user's training items; negatives uniform over the
catalogue minus the user's training items. The draws are i.i.d., so the reference's extra
`shuffle` pass is a distributional no-op and is not repeated. The random stream is Philox, a function
of (seed, epoch) -- the reference's libc rand() stream cannot be reproduced on a GPU and is
never seeded there either (random_choice.pyx:8).

The stream itself is pinned too (tests/test_sampler_gpu.py, bit for bit against tests/sampler_model.py, the executable form of
include/elimrec_hip.h's comment), which is what lets a resumed run replay epoch e of its seed. Triplet i of epoch e takes the output
words r0 .. r3 of Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (i & 0xffffffff, i >> 32, e & 0xffffffff,
low24 | round << 24), low24 = (e >> 32) & 0xffffff (bits 56 .. 63 of the epoch are dropped):
  round 0: the user is the ((r0 << 32 | r1) % n_train_users)-th key of the training dict, the positive the ((r2 << 32 | r3) % count)-th
    of its items in ascending order;
  rounds 1 .. 255: the candidates (r0 << 32 | r1) % num_items and (r2 << 32 | r3) % num_items; the first one, in that order, outside
    the user's training items is the negative;
  after 510 rejected candidates: the smallest id the user does not hold. This fallback is biased (always the smallest missing id)
    and reached only by users who hold nearly the whole catalogue: with probability (1 - f)^510 when the fraction f is missing.
The `%` reductions carry a relative bias of at most m / 2^64. With shard=(rank, world) the process draws the first
ceil(num_trainings / world) triplets of its own seed's stream. Candidate column j >= 1 of neg_sampling="hard" is the same rejection
loop and fallback with low24 = j.

neg_sampling="hard" (dynamic negative sampling, not in the reference): M = neg_candidates uniform candidates are drawn per triplet
-- column 0 is the uniform sampler's negative -- and the epoch trains on the one the model's cached tables score highest
(EliMRec.hard_negatives_device, csrc/hardneg.hip). The tables are those of the last training forward, so an epoch's negatives are
picked by the model as it stood at the end of the epoch before; while no forward has cached tables (the first epoch of a run, the
first one after a resume) the epoch is the uniform one, bit for bit.
"""
import numpy as np
import torch

from . import ops


class PairwiseSamplerV2(object):
    def __init__(self, dataset, neg_num=1, batch_size=1024, shuffle=True, drop_last=False, device=None, seed=2022,
                 shard=None, neg_sampling="uniform", neg_candidates=8, neg_space="fused", model=None):
        """shard = (rank, world): this process draws its 1/world share of the epoch's `num_trainings` triplets (rounded
        up, so every rank runs the same number of batches); give every rank its own seed.
        neg_sampling: "uniform" (one uniform negative) or "hard" (the best of neg_candidates uniform candidates under `model`'s
        cached tables, scored in neg_space: "fused", "loss" or a head letter -- EliMRec.hard_negatives_device)."""
        if neg_num <= 0:
            raise ValueError("'neg_num' must be a positive integer.")
        if neg_num != 1:
            raise NotImplementedError("neg_num > 1 is not used by the EliMRec driver (main.py:59)")
        if neg_sampling not in ("uniform", "hard"):
            raise ValueError("neg_sampling must be 'uniform' or 'hard', got %r" % (neg_sampling,))
        if isinstance(neg_candidates, bool) or int(neg_candidates) != neg_candidates \
                or not 1 <= int(neg_candidates) <= ops.HARD_NEG_MAX_CANDIDATES:
            raise ValueError("neg_candidates must be an integer in [1, %d], got %r" % (ops.HARD_NEG_MAX_CANDIDATES, neg_candidates))
        if neg_sampling == "hard":
            if model is None:
                raise ValueError("neg_sampling='hard' needs the model whose cached tables score the candidates (model=...)")
            model.hard_negative_weights(neg_space)             # ValueError for a space the model does not have
        self.neg_sampling, self.neg_candidates, self.neg_space, self.model = neg_sampling, int(neg_candidates), neg_space, model
        self.last_stats = None                                 # of the last hard epoch: hard, moved, score_picked, score_first
        self.batch_size, self.drop_last, self.shuffle, self.neg_num = batch_size, drop_last, shuffle, neg_num
        self.item_num = dataset.num_items
        user_pos = dataset.get_user_train_dict()
        if not isinstance(user_pos, dict):
            raise TypeError("'user_pos_dict' must be a dict.")
        if not user_pos:
            raise ValueError("'user_pos_dict' cannot be empty.")
        self.num_trainings = sum(len(v) for v in user_pos.values())
        if shard is not None:
            rank, world = int(shard[0]), int(shard[1])
            if not (0 <= rank < world):
                raise ValueError("shard=(rank, world) with 0 <= rank < world")
            self.num_trainings = (self.num_trainings + world - 1) // world
        users = np.fromiter(user_pos.keys(), dtype=np.int32, count=len(user_pos))
        counts = np.fromiter((len(user_pos[u]) for u in users), dtype=np.int64, count=len(users))
        if int(counts.max()) >= self.item_num:
            raise ValueError("The number of 'exclusion' is greater than 'high'.")
        self._users = users
        self._ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self._items = np.concatenate([np.sort(np.asarray(user_pos[u], dtype=np.int32)) for u in users])
        self.device = device
        self.seed = int(seed)
        self.epoch = 0
        self._dev = None

    def __len__(self):
        n = self.num_trainings
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def _to_device(self):
        device = self.device if self.device is not None else torch.device("cuda:0")
        if torch.device(device).type != "cuda":
            raise RuntimeError("PairwiseSamplerV2 samples on the GPU; device '%s' has no implementation" % device)
        if self._dev is None:
            self._dev = (torch.from_numpy(self._users).to(device), torch.from_numpy(self._ptr).to(device),
                         torch.from_numpy(self._items).to(device))
        return device

    def sample_epoch(self):
        """One epoch of triplets as three device int64 tensors of length num_trainings."""
        device = self._to_device()
        n = self.num_trainings
        u = torch.empty(n, dtype=torch.int64, device=device)
        p = torch.empty_like(u)
        if self.neg_sampling == "hard":
            return u, p, self._hard_negatives(u, p, device)
        q = torch.empty_like(u)
        ops.sample_triplets(self._dev[0], self._dev[1], self._dev[2], self.item_num, n, self.seed, self.epoch, u, p, q)
        self.epoch += 1
        return u, p, q

    def _hard_negatives(self, u, p, device):
        """Draws users, positives (into u, p) and [n x M] candidates, and picks per triplet the candidate the model's cached
        tables score highest; candidate 0 -- the uniform negative -- while the model has no cached tables. Fills last_stats."""
        n, M = self.num_trainings, self.neg_candidates
        cands = torch.empty(n, M, dtype=torch.int32, device=device)
        ops.sample_triplet_candidates(self._dev[0], self._dev[1], self._dev[2], self.item_num, n, self.seed, self.epoch, M, u, p, cands)
        self.epoch += 1
        if not self.model.has_cached_tables():
            self.last_stats = dict(hard=False, moved=0.0, score_picked=float("nan"), score_first=float("nan"))
            return cands[:, 0].long()
        neg, pos, score = self.model.hard_negatives_device(u, cands, space=self.neg_space)
        first = self.model.hard_negatives_device(u, cands[:, :1].contiguous(), space=self.neg_space)[2]
        self.last_stats = dict(hard=True, moved=float((pos != 0).float().mean().item()) if n else 0.0,
                               score_picked=float(score.mean().item()) if n else float("nan"),
                               score_first=float(first.mean().item()) if n else float("nan"))
        return neg

    def __iter__(self):
        u, p, q = self.sample_epoch()
        n, bs = self.num_trainings, self.batch_size
        for start in range(0, n, bs):
            stop = min(start + bs, n)
            if stop - start < bs and self.drop_last:
                return
            yield u[start:stop], p[start:stop], q[start:stop]
