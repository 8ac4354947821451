"""Full-catalogue top-K evaluation with the reference's facade (evaluator/proxy_evaluator.py:40-108,
evaluator/backend/cpp/uni_evaluator.py:37-203): `ProxyEvaluator(...).evaluate(model)` ->
(float32 ndarray over metrics x top_show, tab-joined "%.8f" string); with `group_view` the same per user group
(GroupedEvaluator below: one scoring pass, the group means reduced on the device).

What changed underneath: for a model that exposes `predict_device`, scoring, train-item masking,
top-K and the metric curves all run on the GPU (csrc/eval.hip) and only the per-user metric rows
([users x metrics*K] floats) come back to the host for the final mean -- the reference instead
copies a [128 x I] score matrix to the host per batch and ranks it on 8 CPU threads.

Tie rule: the reference's std::partial_sort_copy breaks ties in the C++ library's heap order
(SURVEY quirk 6). tie_order = "reference" (the default) gives exactly those lists: the library
algorithm is replayed on the device, one wave per user, inside the scoring call (csrc/eval.hip
ref_order_kernel) -- same cost as tie_order = "id", the device's own rule (score descending, item
id ascending). The two agree on every row without tied scores at or across the K boundary.
"""
import collections

import numpy as np
import torch

from . import ops
from .data_iterator import DataIterator

metric_dict = {"Precision": 1, "Recall": 2, "MAP": 3, "NDCG": 4, "MRR": 5}
re_metric_dict = {v: k for k, v in metric_dict.items()}


class CandidateScoringError(ValueError):
    """A candidate-list (sampled-negative) evaluation or scoring call this package does not run: item-sharded / lean tables,
    or a top-K beyond the shortest candidate list."""


class UniEvaluator(object):
    def __init__(self, dataset, user_train_dict, user_test_dict, user_neg_test=None, metric=None, top_k=50,
                 batch_size=1024, num_thread=8):
        if not isinstance(user_train_dict, dict):
            raise TypeError("user_train_dict must be a dict")
        if user_test_dict is not None and not isinstance(user_test_dict, dict):
            raise TypeError("user_test_dict must be a dict or None")
        if metric is None:
            metric = ["Precision", "Recall", "MAP", "NDCG", "MRR"]
        elif isinstance(metric, str):
            metric = [metric]
        elif not isinstance(metric, (set, tuple, list)):
            raise TypeError("The type of 'metric' (%s) is invalid!" % metric.__class__.__name__)
        for m in metric:
            if m not in metric_dict:
                raise ValueError("There is not the metric named '%s'!" % metric)
        if user_neg_test is not None and not isinstance(user_neg_test, dict):
            raise TypeError("user_neg_test must be a dict or None")
        self.dataset = dataset
        self.user_pos_train = user_train_dict
        self.user_pos_test = user_test_dict
        self.user_neg_test = user_neg_test
        self.metrics_num = len(metric)
        self.metrics = [metric_dict[m] for m in metric]
        self.num_thread = num_thread          # kept for interface parity; ranking runs on the GPU
        self.batch_size = batch_size
        # users scored per launch. The reference's test_batch_size (128) bounds the [batch x I] host matrix it ranks on the
        # CPU; on the device the per-user results do not depend on the grouping, and a larger block lets eight workgroups
        # share every item tile through L2 and amortises the launches and the users' operand loads of every catalogue chunk
        # (128: 0.048 s, 1024: 0.036 s, 2048: 0.0335 s per validation pass at the Tiktok shape with EXACT math; with the default
        # math 2048: 0.0271, 4096: 0.0258, 8192: 0.0253, 32768: 0.0250 -- 8192 users x 16384 items is a 537 MB score block)
        self.block_users = max(int(batch_size), 8192)
        self.workspace_gib = 8.0                # the scorer's workspace budget: users per launch are halved until it fits
        self.max_top = top_k if isinstance(top_k, int) else max(top_k)
        self.top_show = np.arange(top_k) + 1 if isinstance(top_k, int) else np.sort(top_k)
        self._dev_cache = {}
        self._default_users = None
        # ties among equal scores: "reference" (default) = the reference's lists (evaluate.h:26-33's partial_sort_copy replayed on
        # the device, every row); "id" = the device's own rule (score descending, item id ascending) (--tie_order)
        self.tie_order = "reference"
        self.tie_rows_replayed = 0
        # the default scorer (dot products as six bf16 piece products, csrc/eval.hip score_t16b_kernel) returned a wrong score once
        # in round 3 on one device and never again in 49 000 replays: every evaluation re-scores its first
        # users with the fp32-MFMA scorer and compares the K returned scores -- a difference beyond the two forms' round-off is
        # counted, logged, and the rest of the evaluation runs on the fp32 scorer (scorer_check_users = 0: no check)
        self.scorer_check_users = 1024
        # ... in the first evaluation of a run and in every 16th after it: the check re-scores 1024 users with the slower scorer,
        # 0.8 ms of a 13 ms pass at the Tiktok shape
        self.scorer_check_every = 16
        self._evaluations = 0
        self.scorer_checked_rows = self.scorer_mismatch_rows = 0
        self.range_violations = 0          # scorer waves that saw a score outside their launch's range invariant, over all passes
        if user_neg_test is not None:
            # sampled negatives: every user's list holds its test items and at least n_neg negatives, so K <= n_neg + 1 keeps K real
            # candidates in every row with a test item; beyond it the reference's zero-filled topk_rank tail (evaluate.h counts
            # position 0 again) would be reproduced. Decided over the whole dict: the same for any grouping of the users into blocks
            n_neg = min((len(v) for v in user_neg_test.values()), default=0)
            if self.max_top > n_neg + 1:
                raise CandidateScoringError("sampled-negative evaluation ranks 1 test item + %d negatives: top-K %d exceeds "
                                            "rec.evaluate.neg + 1 = %d" % (n_neg, self.max_top, n_neg + 1))

    def _cross_check_scorer(self, model, users, cache_key=None):
        """Top-K of the first `scorer_check_users` users by the default (bf16 x 3) scorer and by the fp32-MFMA scorer, compared ON THE
        DEVICE: the number of rows whose returned scores differ by more than 1e-6 (the forms agree to 2.4e-7) stays a device scalar,
        which _cross_check_verdict reads once the pass's own launches are enqueued -- the check costs its two scorer calls, not a host
        round trip in front of the pass. Returns (count tensor, users checked) or None when there is nothing to check."""
        from . import _lib
        lib = _lib.load()
        if (not users or self.scorer_check_users <= 0 or int(lib.elimrec_score_get_math()) == 0 or int(lib.elimrec_score_get_bf16x3()) == 0
                or model.latent_dim not in (32, 64) or getattr(model, "_eval_shard", None) is not None
                or self.max_top > min(128, model.num_items)):
            return None
        device = model._require_gpu()
        key = (str(device), "check", cache_key, self.scorer_check_users) if cache_key is not None else None
        hit = self._dev_cache.get(key) if key is not None else None
        if hit is None:
            users = list(users[:self.scorer_check_users])
            train_ptr, train_items = self._batch_csr(users, self.user_pos_train, device, unique=False)
            users_t = torch.as_tensor(np.asarray(users, dtype=np.int64)).to(device)
            hit = (users_t, train_ptr, train_items)
            if key is not None:
                self._dev_cache[key] = hit
        users_t, train_ptr, train_items = hit
        _, val_a = model.predict_device(users_t, top_k=self.max_top, train_ptr=train_ptr, train_items=train_items)
        lib.elimrec_score_set_bf16x3(0)
        try:
            _, val_b = model.predict_device(users_t, top_k=self.max_top, train_ptr=train_ptr, train_items=train_items)
        finally:
            lib.elimrec_score_set_bf16x3(1)
        diff = (val_a - val_b).abs()
        bad = (torch.where(torch.isfinite(val_a) & torch.isfinite(val_b), diff, (val_a != val_b).float()) > 1e-6).any(1).sum()
        return bad, int(users_t.numel())

    def _range_verdict(self, model, first, act=True):
        """Reads (and clears) the scorers' range-invariant counter behind the pass's launches. Violations under the default
        (bf16 x 3) scorer switch the process to the fp32 scorer and the pass is scored again; under the fp32 scorer they are an
        error: the cached tables themselves must hold non-finite values. act = False (several ranks: a rank must not leave the
        collectives of the pass on its own): counted and logged only."""
        from . import _lib
        n = ops.score_range_violations(reset=True)
        self.range_violations += n
        if not n:
            return 0
        if not act:
            from .logger import Logger
            Logger.info("[evaluator] %d scorer waves of this rank saw a score outside the range of predict type %s / fusion %s"
                        % (n, model.predict_type, model.fusion_mode))
            return 0
        lib = _lib.load()
        from .logger import Logger
        if first and int(lib.elimrec_score_get_bf16x3()) and int(lib.elimrec_score_get_math()) == 1 and model.latent_dim in (32, 64):
            Logger.info("[evaluator] %d scorer waves saw a score outside the range of predict type %s / fusion %s: the fp32 scorer is "
                        "used from here on, this pass is scored again" % (n, model.predict_type, model.fusion_mode))
            lib.elimrec_score_set_bf16x3(0)
            return n
        raise FloatingPointError("the evaluator's scores left the range of predict type %s / fusion %s in %d scorer waves (fp32 scorer): "
                                 "the cached tables hold non-finite or corrupted values" % (model.predict_type, model.fusion_mode, n))

    def _cross_check_verdict(self, pending):
        """Reads the cross-check's count (a host synchronisation: call it behind the pass's launches). On any differing row the
        process keeps the fp32 scorer from here on; returns the number of such rows."""
        if pending is None:
            return 0
        from . import _lib
        bad, n = int(pending[0]), pending[1]
        self.scorer_checked_rows += n
        self.scorer_mismatch_rows += bad
        if bad:
            from .logger import Logger
            Logger.info("[evaluator] %d of %d cross-checked users got different top-%d scores from the bf16x3 scorer and the fp32-MFMA "
                        "scorer (> 1e-6): the fp32 scorer is used from here on, this pass is scored again" % (bad, n, self.max_top))
            _lib.load().elimrec_score_set_bf16x3(0)
        return bad

    def metrics_info(self):
        cols = ["\t".join(("%s@" % re_metric_dict[m] + str(k)).ljust(12) for k in self.top_show) for m in self.metrics]
        return "metrics:\t%s" % "\t".join(cols)

    def _batch_csr(self, users, table, device, unique):
        lists = [sorted(set(table.get(u, []))) if unique else table.get(u, []) for u in users]
        ptr = np.zeros(len(users) + 1, dtype=np.int64)
        np.cumsum([len(x) for x in lists], out=ptr[1:])
        flat = np.fromiter((i for x in lists for i in x), dtype=np.int32, count=int(ptr[-1]))
        return torch.from_numpy(ptr).to(device), torch.from_numpy(flat).to(device)

    def evaluate(self, model, test_users=None, shard=None):
        """shard = (rank, world): this process scores a contiguous 1/world slice of the users and the per-user metric rows
        are summed across the ranks (all_reduce of the zero-filled [users x metrics*K] matrix), so every rank ends with
        the same rows -- and, the final mean being taken over the same matrix, the same bits -- as a single process.
        Default: the ranks of an initialised torch.distributed job (the cached tables are replicated on every rank)."""
        if test_users is None:
            test_users = self.default_users()
        all_dev = self._rows_of(model, test_users, shard)
        return self._summary(all_dev.cpu().numpy())                       # [users, metrics*K]

    def _rows_of(self, model, test_users, shard):
        """evaluate()'s argument checks and its metric_rows call; the default users' index tensors are the cached ones."""
        cached = test_users is self._default_users
        if not isinstance(test_users, (list, tuple, set, np.ndarray)):
            raise TypeError("'test_user' must be a list, tuple, set or numpy array!")
        if not hasattr(model, "predict_device"):
            raise TypeError("model must expose predict_device(); host-side ranking is not part of this package")
        return self.metric_rows(model, list(test_users), shard=shard, cached=cached)

    def default_users(self):
        """The test users in evaluate()'s default order (the list whose index tensors stay cached on the device)."""
        if getattr(self, "_default_users", None) is None:
            self._default_users = list(self.user_pos_test.keys())
        return self._default_users

    def _summary(self, all_rows):
        """Host rows [users, metrics*K] -> (float32 means at the shown K, their tab-joined "%.8f" string)."""
        final = np.mean(all_rows, axis=0).reshape(self.metrics_num, self.max_top)[:, self.top_show - 1].reshape(-1)
        buf = "\t".join(("%.8f" % x).ljust(12) for x in final)
        return final, buf

    def metric_rows(self, model, test_users, shard=None, cached=False, reduce=True):
        """Per-user metric rows of `test_users` on the device, [len(test_users), metrics*K]; with shard = (rank, world)
        only this rank's slice is computed (the rest zero) and `reduce` sums the matrix over the ranks."""
        import torch.distributed as dist
        if shard is None and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            shard = (dist.get_rank(), dist.get_world_size())
        if self.user_neg_test is not None:
            return self._sampled_metric_rows(model, test_users, shard, cached, reduce)
        n = len(test_users)
        sharded = shard is not None and shard[1] > 1
        if hasattr(model, "_ensure_tables") and getattr(model, "_cache", None) is not None and not sharded:
            model._ensure_tables()       # (lean tables on one rank: the item-shard scorer exists once the tables are built)
        if sharded and hasattr(model, "_ensure_tables"):
            # every rank, before any rank can run out of users: materialising the cached tables of a multi-rank job is a
            # collective (ColumnShardEngine.materialize_tables), and a rank with an empty slice would otherwise skip it
            model._ensure_tables()
        if getattr(model, "_eval_shard", None) is not None:
            # the cached tables are ITEM-sharded (row-sharded constants, shard_eval.py): every rank scores every user
            # against its items and the merged lists -- hence the metric rows -- are identical on all ranks
            sharded = False
        lo, hi = (n * shard[0] // shard[1], n * (shard[0] + 1) // shard[1]) if sharded else (0, n)
        alloc = torch.zeros if sharded else torch.empty
        all_dev = alloc(n, self.metrics_num * self.max_top, dtype=torch.float32, device=model._require_gpu())
        at = lo
        mine = test_users[lo:hi]
        block = self._users_per_launch(model)
        check = self._evaluations % self.scorer_check_every == 0
        self._evaluations += 1
        pending = self._cross_check_scorer(model, mine, cache_key=(lo, hi) if cached else None) if check else None
        for attempt in (0, 1):
            at = lo
            for k, batch_users in enumerate(DataIterator(mine, batch_size=block, shuffle=False, drop_last=False)):
                key = (k, lo, hi, block) if cached else None
                self.evaluate_batch(model, batch_users, cache_key=key, out=all_dev[at:at + len(batch_users)])
                at += len(batch_users)
            # the scorer's cross-check of this pass's first users, read behind the pass's launches; a mismatch switches the process to
            # the fp32 scorer and the pass is scored once more with it. Likewise the range invariant EVERY scorer launch of the pass
            # checked in its epilogue (every score is a sigmoid of a bounded argument: csrc/eval.hip ScoreArgs::lo / hi)
            out_of_range = self._range_verdict(model, first=attempt == 0, act=not sharded and getattr(model, "_eval_shard", None) is None)
            if attempt == 1 or not (self._cross_check_verdict(pending) or out_of_range):
                break
        if sharded and reduce:
            dist.all_reduce(all_dev, op=dist.ReduceOp.SUM)
        return all_dev

    def _sampled_metric_rows(self, model, test_users, shard, cached, reduce):
        """The reference's candidate branch (cpp/uni_evaluator.py:132-140) on the device: per user block the candidate lists
        list(user_pos_test[u]) + user_neg_test[u] as CSR, their scores (-inf padded rows, csrc/eval.hip score_cand_kernel), the
        top-K positions -- tie_order "reference": evaluate.h's partial_sort_copy replayed on the device over the padded rows;
        "id": (score desc, position asc) -- and the metric curves with truth = positions 0 .. npos - 1. No train-item masking."""
        import torch.distributed as dist
        n = len(test_users)
        sharded = shard is not None and shard[1] > 1
        if hasattr(model, "_ensure_tables"):
            model._ensure_tables()
        if getattr(model, "_eval_shard", None) is not None:
            raise CandidateScoringError("sampled-negative evaluation needs the whole cached item table on every rank; the tables are "
                                        "item-sharded (lean / multi-rank evaluation): evaluate with --eval_candidates=full")
        device = model._require_gpu()
        lo, hi = (n * shard[0] // shard[1], n * (shard[0] + 1) // shard[1]) if sharded else (0, n)
        alloc = torch.zeros if sharded else torch.empty
        all_dev = alloc(n, self.metrics_num * self.max_top, dtype=torch.float32, device=device)
        K = self.max_top
        at = lo
        for k, batch_users in enumerate(DataIterator(test_users[lo:hi], batch_size=self.block_users, shuffle=False, drop_last=False)):
            key = (str(device), "sampled", k, lo, hi, self.block_users) if cached else None
            hit = self._dev_cache.get(key) if key is not None else None
            if hit is None:
                lists = [list(self.user_pos_test[u]) + list(self.user_neg_test[u]) for u in batch_users]
                npos = [len(self.user_pos_test[u]) for u in batch_users]
                lens = np.fromiter((len(x) for x in lists), dtype=np.int64, count=len(lists))
                ptr = np.zeros(len(lists) + 1, dtype=np.int64)
                np.cumsum(lens, out=ptr[1:])
                flat = np.fromiter((i for x in lists for i in x), dtype=np.int32, count=int(ptr[-1]))
                tptr = np.zeros(len(lists) + 1, dtype=np.int64)
                np.cumsum(npos, out=tptr[1:])
                titems = np.concatenate([np.arange(p, dtype=np.int32) for p in npos]) if tptr[-1] else np.zeros(1, dtype=np.int32)
                width = int(lens.max())
                users_t = torch.as_tensor(np.asarray(batch_users, dtype=np.int64)).to(device)
                pos_t = torch.arange(width, dtype=torch.int32, device=device).expand(len(lists), width).contiguous() \
                    if self.tie_order != "reference" else None
                hit = (users_t, torch.from_numpy(ptr).to(device), torch.from_numpy(flat).to(device), torch.from_numpy(tptr).to(device),
                       torch.from_numpy(titems).to(device), width, pos_t)
                if key is not None:
                    self._dev_cache[key] = hit
            users_t, cand_ptr, cand_items, truth_ptr, truth_items, width, pos_t = hit
            B = users_t.numel()
            scores = torch.empty(B, width, dtype=torch.float32, device=device)
            model.predict_candidates_device(users_t, cand_ptr, cand_items, scores)
            idx = torch.empty(B, K, dtype=torch.int32, device=device)
            val = torch.empty(B, K, dtype=torch.float32, device=device)
            if self.tie_order == "reference":
                ops.topk_reference_order(scores, K, idx, val)
            else:
                if pos_t is None:
                    pos_t = torch.arange(width, dtype=torch.int32, device=device).expand(B, width).contiguous()
                ops.topk_merge(scores, pos_t, K, idx, val)
            ops.score_range_check(val, idx, model.predict_type, model.fusion_mode)
            ops.rank_metrics(idx, truth_ptr, truth_items, self.metrics, all_dev[at:at + B])
            at += B
        self._evaluations += 1
        self._range_verdict(model, first=False, act=not sharded)
        if sharded and reduce:
            dist.all_reduce(all_dev, op=dist.ReduceOp.SUM)
        return all_dev

    def _users_per_launch(self, model):
        """block_users, halved until the scorer's workspace for this catalogue (or this rank's item shard) fits the budget
        (workspace_gib, default 8): a recdim outside the chunked scorer's set needs a [users x items] score block, which
        at 12.5 M items per rank is 50 MB per user."""
        block = self.block_users
        sh = getattr(model, "_eval_shard", None)
        # (item shards differ by one item between ranks when I % W != 0, and the sharded scorer's collectives run once per user
        # block: the block size must come out the same on every rank, so it is sized from the LARGEST shard)
        bounds = getattr(sh, "bounds", None)
        n_items = (max(b - a for a, b in zip(bounds[:-1], bounds[1:])) if bounds else sh.i1 - sh.i0) if sh is not None else model.num_items
        budget = float(self.workspace_gib) * 2 ** 30
        while block > 16 and ops.score_workspace(block, model.num_users, n_items, model.S, self.max_top, topk_only=True,
                                                 d=model.latent_dim) > budget:
            block //= 2
        return block

    def _topk_in_reference_order(self, model, users_t, train_ptr, train_items):
        """tie_order = "reference": the lists evaluate.h:26-33 makes of these users' masked score rows -- std::partial_sort_copy's
        heap order among equal scores -- computed ON THE DEVICE inside the scoring call (csrc/eval.hip ref_order_kernel: one wave
        per user replays the library algorithm operation for operation on the scores the scorer has just produced, the heap carried
        from catalogue chunk to chunk). Every row, tied or not; no score row is materialised or copied, nothing synchronises with
        the host, and the pass costs what the "id" order costs whatever the state of training.
        Item-sharded tables (several ranks, shard_eval.py): a rank sees only its items, and the algorithm is sequential over the
        catalogue -- the merged (score, id) lists are the reference's on every row without a tie at or across K; the rows that
        have one get their whole score rows (all-gathered, as predict() returns them) ranked by the same device kernel."""
        K = self.max_top
        if getattr(model, "_eval_shard", None) is None:
            return model.predict_device(users_t, top_k=K, train_ptr=train_ptr, train_items=train_items, tie_order="reference")
        if K + 1 > min(256, model.num_items):
            raise ValueError("tie_order=reference over item-sharded tables needs the merged top-(K + 1) list: K + 1 = %d exceeds "
                             "min(256, num_items = %d); evaluate with --tie_order=id" % (K + 1, model.num_items))
        idx1, val1 = model.predict_device(users_t, top_k=K + 1, train_ptr=train_ptr, train_items=train_items)
        idx, val = idx1[:, :K].contiguous(), val1[:, :K].contiguous()
        tied = torch.nonzero((val1[:, :-1] == val1[:, 1:]).any(1)).flatten()       # (every rank holds the same merged lists)
        self.tie_rows_replayed += int(tied.numel())
        # <= 1 GiB of score rows at a time (a row of configs[4]'s catalogue is 400 MB); every rank holds the same merged lists, hence
        # the same `tied` and the same number of (collective) score-row calls
        step = max(1, (1 << 28) // max(1, model.num_items))
        for a in range(0, int(tied.numel()), step):
            part = tied[a:a + step]
            lo_t, hi_t = train_ptr[part], train_ptr[part + 1]
            sub_ptr = torch.zeros(part.numel() + 1, dtype=torch.int64, device=users_t.device)
            torch.cumsum(hi_t - lo_t, 0, out=sub_ptr[1:])
            take = torch.repeat_interleave(lo_t - sub_ptr[:-1], hi_t - lo_t) + torch.arange(int(sub_ptr[-1]), device=users_t.device)
            it = train_items[take] if take.numel() else torch.zeros(1, dtype=torch.int32, device=users_t.device)
            sc = torch.empty(part.numel(), model.num_items, dtype=torch.float32, device=users_t.device)
            model.predict_device(users_t[part], scores=sc, train_ptr=sub_ptr, train_items=it.contiguous())
            ti = torch.empty(part.numel(), K, dtype=torch.int32, device=users_t.device)
            tv = torch.empty(part.numel(), K, dtype=torch.float32, device=users_t.device)
            ops.topk_reference_order(sc, K, ti, tv)
            idx[part], val[part] = ti, tv
        return idx, val

    def evaluate_batch(self, model, batch_users, return_topk=False, cache_key=None, out=None):
        """Per-user metric rows [len(batch_users), metrics*K] (device tensor) for one user block.
        cache_key: the user blocks of the default evaluation order are the same every time, so their
        index tensors (user ids, train-mask CSR, truth CSR) are built once and stay on the device."""
        device = model._require_gpu()
        key = (str(device), cache_key) if cache_key is not None else None
        hit = self._dev_cache.get(key) if key is not None else None
        if hit is None:
            train_ptr, train_items = self._batch_csr(batch_users, self.user_pos_train, device, unique=False)
            truth_ptr, truth_items = self._batch_csr(batch_users, self.user_pos_test, device, unique=True)
            users_t = torch.as_tensor(np.asarray(batch_users, dtype=np.int64)).to(device)
            hit = (users_t, train_ptr, train_items, truth_ptr, truth_items)
            if key is not None:
                self._dev_cache[key] = hit
        users_t, train_ptr, train_items, truth_ptr, truth_items = hit
        if self.tie_order == "reference":
            idx, val = self._topk_in_reference_order(model, users_t, train_ptr, train_items)
        else:
            idx, val = model.predict_device(users_t, top_k=self.max_top, train_ptr=train_ptr, train_items=train_items)
        if out is None:
            out = torch.empty(len(batch_users), self.metrics_num * self.max_top, dtype=torch.float32, device=device)
        ops.rank_metrics(idx, truth_ptr, truth_items, self.metrics, out)
        return (out, idx, val) if return_topk else out


def assign_user_groups(test_users, user_train_dict, group_view):
    """The reference's user groups (evaluator/grouped_evaluator.py:63-80) without pandas: bounds [0] + group_view, a test user's
    group is np.searchsorted(group_view, n_train) -- n_train in (lo, hi], so a user without training items lands in the first
    group -- users beyond the last bound are discarded, groups without users are omitted; groups in ascending order of their
    bounds, a group's users in the order of `test_users`.
    -> (labels ["(lo,hi]:".ljust(12)], positions [int64 arrays of indices into test_users], number of discarded users)."""
    if not isinstance(group_view, list):
        raise TypeError("The type of 'group_view' must be `list`!")
    for b in group_view:
        if isinstance(b, bool) or not isinstance(b, (int, np.integer)) or b <= 0:
            raise ValueError("group_view must hold strictly ascending positive integers, got %r" % (group_view,))
    if any(hi <= lo for lo, hi in zip(group_view[:-1], group_view[1:])):
        raise ValueError("group_view must hold strictly ascending positive integers, got %r" % (group_view,))
    bounds = [0] + [int(b) for b in group_view]
    n_train = np.fromiter((len(user_train_dict.get(u, [])) for u in test_users), dtype=np.int64, count=len(test_users))
    group = np.searchsorted(np.asarray(bounds[1:], dtype=np.int64), n_train)
    labels, positions = [], []
    for g in range(len(group_view)):
        at = np.flatnonzero(group == g)
        if at.size:
            labels.append(("(%d,%d]:" % (bounds[g], bounds[g + 1])).ljust(12))
            positions.append(at.astype(np.int64))
    if not labels:
        raise ValueError("The splitting of user groups is not suitable!")
    return labels, positions, int((group >= len(group_view)).sum())


class GroupedEvaluator(object):
    """Ranking quality per user group, the users bucketed by their number of TRAINING interactions (the reference's
    evaluator/grouped_evaluator.py:12-112; group_view = [10, 30, 50, 100] -> (0,10], (10,30], (30,50], (50,100], heavier users
    discarded). The reference runs one evaluator pass per group; here every test user is scored ONCE -- the inner UniEvaluator's
    metric_rows over its default user order, so the full-catalogue, the sampled-negative, the user-sliced and the item-sharded
    forms all apply -- and one launch pair (ops.group_metric_means, csrc/eval.hip) turns the [users x metrics*K] block into
    [groups x metrics*K] float64-accumulated means on the device; only those cross to the host."""

    def __init__(self, dataset, user_train_dict, user_test_dict, user_neg_test=None, metric=None, group_view=None, top_k=50,
                 batch_size=1024, num_thread=8):
        if not isinstance(group_view, list):
            raise TypeError("The type of 'group_view' must be `list`!")
        self.evaluator = UniEvaluator(dataset, user_train_dict, user_test_dict, user_neg_test, metric=metric, top_k=top_k,
                                      batch_size=batch_size, num_thread=num_thread)
        self.user_pos_train = user_train_dict
        self.user_pos_test = user_test_dict
        self.group_view = list(group_view)
        users = self.evaluator.default_users()
        self.group_labels, self._positions, self.num_discarded = assign_user_groups(users, user_train_dict, group_view)
        self.group_sizes = [int(p.size) for p in self._positions]
        self.grouped_user = {label: [users[i] for i in at] for label, at in zip(self.group_labels, self._positions)}
        self._index = {}                   # device -> ops.GroupIndex: the groups as CSR over the rows of the default user order

    # (BasicModel's --tie_order plumbing sets `.evaluator.tie_order` of the facade: it reaches the evaluator that ranks)
    @property
    def tie_order(self):
        return self.evaluator.tie_order

    @tie_order.setter
    def tie_order(self, value):
        self.evaluator.tie_order = value

    def metrics_info(self):
        return self.evaluator.metrics_info()

    def _group_index(self, device):
        hit = self._index.get(str(device))
        if hit is None:
            ptr = np.zeros(len(self._positions) + 1, dtype=np.int64)
            np.cumsum(self.group_sizes, out=ptr[1:])
            hit = ops.GroupIndex(ptr, np.concatenate(self._positions).astype(np.int32), len(self.evaluator.default_users()), device)
            self._index[str(device)] = hit
        return hit

    def group_means(self, rows):
        """Device rows [default users x metrics*K] (UniEvaluator.metric_rows) -> host float32 [groups x metrics*K]."""
        out = torch.empty(len(self.group_labels), rows.shape[1], dtype=torch.float32, device=rows.device)
        return ops.group_metric_means(rows, self._group_index(rows.device), None, out).cpu().numpy()

    def format_groups(self, final):
        """[groups x shown columns] -> the reference's multi-line string (grouped_evaluator.py:107-112)."""
        return "".join("\n%s\t%s" % (label, "\t".join(("%.8f" % x).ljust(12) for x in row))
                       for label, row in zip(self.group_labels, final))

    def evaluate_rows(self, rows):
        """(final [groups x metrics*len(top_show)] float32, buf) from the metric rows of the default users."""
        ev = self.evaluator
        means = self.group_means(rows)
        final = means.reshape(len(self.group_labels), ev.metrics_num, ev.max_top)[:, :, ev.top_show - 1].reshape(len(self.group_labels), -1)
        return final, self.format_groups(final)

    def evaluate(self, model, shard=None):
        ev = self.evaluator
        return self.evaluate_rows(ev._rows_of(model, ev.default_users(), shard))

    def evaluate_with_overall(self, model, shard=None):
        """(overall final, overall buf, group final, group buf) from ONE scoring pass: the overall pair is UniEvaluator.evaluate's
        own expression over the same rows -- the bits an evaluation without group_view has."""
        ev = self.evaluator
        rows = ev._rows_of(model, ev.default_users(), shard)
        group_final, group_buf = self.evaluate_rows(rows)
        final, buf = ev._summary(rows.cpu().numpy())
        return final, buf, group_final, group_buf


class EffectReport(object):
    """What the test users' top-K lists are made of (--effect_report=K): per (user, rank <= K) pair the effect breakdown of
    EliMRec.effects_device -- ui, its catalogue mean, te, nde, the TE / TIE scores, the heads' cosines -- and its column means
    over all pairs and, with group_view, per user group (assign_user_groups). The lists are the model's top-K under its current
    predict type with train items masked, in user blocks as metric_rows takes them; the means are ops.group_metric_means over
    the [users*K x C] block (float64 sums, the segments = rows of that block): only [1 + groups x C] floats reach the host."""

    def __init__(self, dataset, user_train_dict, user_test_dict, top_k, group_view=None):
        if not isinstance(user_train_dict, dict) or not isinstance(user_test_dict, dict):
            raise TypeError("user_train_dict and user_test_dict must be dicts")
        if isinstance(top_k, bool) or not isinstance(top_k, (int, np.integer)) or top_k < 1:
            raise ValueError("top_k must be a positive integer, got %r" % (top_k,))
        self.dataset = dataset
        self.user_pos_train = user_train_dict
        self.user_pos_test = user_test_dict
        self.top_k = int(top_k)
        self.users = list(user_test_dict.keys())
        self.block_users = 8192
        self.tie_order = "id"
        self.group_labels, self._positions = ["all:".ljust(12)], [np.arange(len(self.users), dtype=np.int64)]
        if group_view is not None:
            labels, positions, self.num_discarded = assign_user_groups(self.users, user_train_dict, group_view)
            self.group_labels += labels
            self._positions += positions
        self._index = {}                   # device -> ops.GroupIndex over the rows of the [users*K x C] block

    def _group_index(self, device):
        hit = self._index.get(str(device))
        if hit is None:
            K = self.top_k
            rows = [(p[:, None] * K + np.arange(K, dtype=np.int64)[None, :]).reshape(-1) for p in self._positions]
            ptr = np.zeros(len(rows) + 1, dtype=np.int64)
            np.cumsum([r.size for r in rows], out=ptr[1:])
            hit = ops.GroupIndex(ptr, np.concatenate(rows).astype(np.int32), len(self.users) * K, device)
            self._index[str(device)] = hit
        return hit

    def effect_rows(self, model):
        """The breakdown of every test user's top-K list on the device: ([users*K x C] float32, column names)."""
        if not hasattr(model, "effects_device"):
            raise TypeError("model must expose effects_device()")
        if hasattr(model, "_ensure_tables") and getattr(model, "_cache", None) is not None:
            model._ensure_tables()
        if getattr(model, "_eval_shard", None) is not None:
            raise CandidateScoringError("the effect report needs the whole cached item table on this rank; the tables are "
                                        "item-sharded (lean / multi-rank evaluation): run without --effect_report")
        if self.top_k > model.num_items:
            raise CandidateScoringError("effect report of the top-%d lists: the catalogue has %d items" % (self.top_k, model.num_items))
        device = model._require_gpu()
        columns = ops.effect_columns(model._mods)
        K, C = self.top_k, len(columns)
        rows = torch.empty(len(self.users) * K, C, dtype=torch.float32, device=device)
        at = 0
        for batch_users in DataIterator(self.users, batch_size=self.block_users, shuffle=False, drop_last=False):
            B = len(batch_users)
            lists = [self.user_pos_train.get(u, []) for u in batch_users]
            ptr = np.zeros(B + 1, dtype=np.int64)
            np.cumsum([len(x) for x in lists], out=ptr[1:])
            flat = np.fromiter((i for x in lists for i in x), dtype=np.int32, count=int(ptr[-1]))
            users_t = torch.as_tensor(np.asarray(batch_users, dtype=np.int64)).to(device)
            idx, _ = model.predict_device(users_t, top_k=K, train_ptr=torch.from_numpy(ptr).to(device),
                                          train_items=torch.from_numpy(flat).to(device), tie_order=self.tie_order)
            cand_ptr = torch.arange(B + 1, dtype=torch.int64, device=device) * K
            model.effects_device(users_t, cand_ptr, idx.reshape(-1), rows[at * K:(at + B) * K].view(B, K, C))
            at += B
        return rows, columns

    def columns_info(self, columns):
        return "columns:\t%s" % "\t".join(str(c).ljust(12) for c in columns)

    def evaluate(self, model):
        """(final [1 + groups x C] float32: row 0 = all pairs, then one row per user group; buf: a header of column names and
        one line per row in the grouped evaluator's format)."""
        rows, columns = self.effect_rows(model)
        out = torch.empty(len(self.group_labels), rows.shape[1], dtype=torch.float32, device=rows.device)
        final = ops.group_metric_means(rows, self._group_index(rows.device), None, out).cpu().numpy()
        buf = self.columns_info(columns) + "".join("\n%s\t%s" % (label, "\t".join(("%.8f" % x).ljust(12) for x in row))
                                                    for label, row in zip(self.group_labels, final))
        return final, buf


def assign_item_groups(item_ids, train_item_counts, item_group_view):
    """Items bucketed by popularity, the counterpart of assign_user_groups: item_group_view = [b1..bn] (strictly ascending
    positive integers) gives `cold` (0 training interactions), (0,b1], ..., (b(n-1),bn] and the open (bn,inf); an entry of
    item_ids lands in the bucket of train_item_counts[its id]. Groups without entries are omitted; groups in that order, a
    group's entries in the order of item_ids.
    -> (labels ["cold:" / "(lo,hi]:" / "(bn,inf):", each .ljust(12)], positions [int64 arrays of indices into item_ids])."""
    if not isinstance(item_group_view, list) or not item_group_view:
        raise TypeError("The type of 'item_group_view' must be a non-empty `list`!")
    for b in item_group_view:
        if isinstance(b, bool) or not isinstance(b, (int, np.integer)) or b <= 0:
            raise ValueError("item_group_view must hold strictly ascending positive integers, got %r" % (item_group_view,))
    if any(hi <= lo for lo, hi in zip(item_group_view[:-1], item_group_view[1:])):
        raise ValueError("item_group_view must hold strictly ascending positive integers, got %r" % (item_group_view,))
    bounds = [int(b) for b in item_group_view]
    ids = np.asarray(item_ids, dtype=np.int64).reshape(-1)
    counts = np.asarray(train_item_counts, dtype=np.int64).reshape(-1)
    if ids.size and (ids.min() < 0 or ids.max() >= counts.size):
        raise IndexError("item ids must lie in [0, %d)" % counts.size)
    n = counts[ids]
    # 0 = cold, 1 + g = (bounds[g - 1], bounds[g]] (count in (lo, hi], as the user groups), 1 + len(bounds) = beyond the last bound
    group = np.where(n == 0, 0, 1 + np.searchsorted(np.asarray(bounds, dtype=np.int64), n))
    names = ["cold:"] + ["(%d,%d]:" % (lo, hi) for lo, hi in zip([0] + bounds[:-1], bounds)] + ["(%d,inf):" % bounds[-1]]
    labels, positions = [], []
    for g, name in enumerate(names):
        at = np.flatnonzero(group == g)
        if at.size:
            labels.append(name.ljust(12))
            positions.append(at.astype(np.int64))
    return labels, positions


RankTables = collections.namedtuple("RankTables", ("pair_columns", "pair_labels", "pairs", "user_columns", "user_labels", "users"))


class RankReport(object):
    """Where the held-out items stand in the FULL ranking (--rank_report=1): every (test user, test item) pair's exact catalogue
    rank under the model's current predict type with the train items masked (EliMRec.rank_items_device: the evaluator's scoring
    call into a score block, then csrc/rank.hip's count over it), and from the ranks
      per pair: rank, rr = 1 / (rank + 1), pct = rank / (candidates - 1), hit@K for every K of top_k;
      per user: auc, mrr_full = 1 / (first_rank + 1), first_rank = the best rank among the user's test items
    as means over all pairs / users, per user group (group_view, assign_user_groups) and -- pair columns -- per item popularity
    group (item_group_view, assign_item_groups over the items' training interactions). The pair means are MICRO-averages: every
    pair weighs the same, so a user with many test items weighs more, and hit@K here is NOT the evaluator's per-user recall
    (a mean of per-user ratios). Ranks order equal scores by item id whatever the evaluator's tie_order is.
    Pairs are all (user, item) of user_test_dict in dict order; a pair whose item is also in the user's train list is dropped
    (num_dropped), then a user without a pair or without a candidate besides its test items (num_skipped_users). Users go in
    blocks whose [users x items] score block stays within block_bytes; the row and mean kernels leave only the tables to the host."""

    def __init__(self, dataset, user_train_dict, user_test_dict, top_k, group_view=None, item_group_view=None):
        if not isinstance(user_train_dict, dict) or not isinstance(user_test_dict, dict):
            raise TypeError("user_train_dict and user_test_dict must be dicts")
        ks = [top_k] if isinstance(top_k, (int, np.integer)) and not isinstance(top_k, bool) else list(top_k)
        if not ks or any(isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1 for k in ks):
            raise ValueError("top_k must be a positive integer or a list of them, got %r" % (top_k,))
        self.dataset = dataset
        self.num_items = I = int(dataset.num_items)
        self.user_pos_train = user_train_dict
        self.user_pos_test = user_test_dict
        self.ks = [int(k) for k in ks]
        self.block_bytes = 2 << 30
        self.num_dropped = self.num_skipped_users = 0
        self.users, pair_items, lens, n_cand = [], [], [], []
        for u, test_items in user_test_dict.items():
            seen = set(int(i) for i in user_train_dict.get(u, []))
            kept = [int(i) for i in test_items if int(i) not in seen]
            self.num_dropped += len(test_items) - len(kept)
            if not kept or I - len(seen) - len(kept) <= 0:
                self.num_skipped_users += 1
                continue
            self.users.append(u)
            pair_items.append(kept)
            lens.append(len(kept))
            n_cand.append(I - len(seen))
        if not self.users:
            raise ValueError("the rank report has no (test user, test item) pair left to rank")
        self.pair_ptr = np.zeros(len(self.users) + 1, dtype=np.int64)
        np.cumsum(lens, out=self.pair_ptr[1:])
        self.pair_items = np.fromiter((i for x in pair_items for i in x), dtype=np.int32, count=int(self.pair_ptr[-1]))
        if self.pair_items.min() < 0 or self.pair_items.max() >= I:
            raise IndexError("test item ids must lie in [0, %d)" % I)
        self.pair_user = np.repeat(np.arange(len(self.users), dtype=np.int64), lens)       # position in self.users
        self.user_n_cand = np.asarray(n_cand, dtype=np.int32)
        self.pair_n_cand = self.user_n_cand[self.pair_user]
        self.num_pairs = int(self.pair_items.size)
        # groups: rows of the user block / of the pair block
        self.user_labels, user_pos = ["all:".ljust(12)], [np.arange(len(self.users), dtype=np.int64)]
        self.pair_labels, pair_pos = ["all:".ljust(12)], [np.arange(self.num_pairs, dtype=np.int64)]
        if group_view is not None:
            labels, positions, self.num_discarded = assign_user_groups(self.users, user_train_dict, group_view)
            self.user_labels += labels
            user_pos += positions
            self.pair_labels += labels
            pair_pos += [np.flatnonzero(np.isin(self.pair_user, p)) for p in positions]
        if item_group_view is not None:
            counts = np.zeros(I, dtype=np.int64)
            for items in user_train_dict.values():
                np.add.at(counts, np.asarray(list(items), dtype=np.int64), 1)
            labels, positions = assign_item_groups(self.pair_items, counts, item_group_view)
            self.pair_labels += [("item " + x.strip()).ljust(12) for x in labels]
            pair_pos += positions
        self._user_pos, self._pair_pos = user_pos, pair_pos
        self._device = {}                  # device -> the CSRs, candidate counts and group indices resident there

    @property
    def block_users(self):
        """Users per scoring call: as many as keep the [users x items] float32 block (rows padded to 16 bytes) within block_bytes."""
        return max(1, int(self.block_bytes) // ((self.num_items + 3) // 4 * 16))

    def _resident(self, device):
        hit = self._device.get(str(device))
        if hit is None:
            def index(positions, n_rows):
                ptr = np.zeros(len(positions) + 1, dtype=np.int64)
                np.cumsum([p.size for p in positions], out=ptr[1:])
                return ops.GroupIndex(ptr, np.concatenate(positions).astype(np.int32), n_rows, device)
            hit = dict(pair_ptr=torch.from_numpy(self.pair_ptr).to(device), user_n_cand=torch.from_numpy(self.user_n_cand).to(device),
                       pair_n_cand=torch.from_numpy(np.ascontiguousarray(self.pair_n_cand)).to(device),
                       user_groups=index(self._user_pos, len(self.users)), pair_groups=index(self._pair_pos, self.num_pairs), blocks={})
            self._device[str(device)] = hit
        return hit

    def _block(self, res, a, b, device):
        """Users [a, b) of self.users as one scoring call's inputs, kept on the device: (users, TargetIndex, train_ptr, train_items)."""
        hit = res["blocks"].get((a, b))
        if hit is None:
            ptr = self.pair_ptr[a:b + 1] - self.pair_ptr[a]
            target = ops.TargetIndex(ptr, self.pair_items[self.pair_ptr[a]:self.pair_ptr[b]], b - a, self.num_items, device)
            lists = [self.user_pos_train.get(u, []) for u in self.users[a:b]]
            tptr = np.zeros(b - a + 1, dtype=np.int64)
            np.cumsum([len(x) for x in lists], out=tptr[1:])
            flat = np.fromiter((int(i) for x in lists for i in x), dtype=np.int32, count=int(tptr[-1]))
            train = (torch.from_numpy(tptr).to(device), torch.from_numpy(flat).to(device)) if flat.size else (None, None)
            hit = (torch.as_tensor(np.asarray(self.users[a:b], dtype=np.int64)).to(device), target) + train
            res["blocks"][(a, b)] = hit
        return hit

    def pair_ranks(self, model):
        """The exact catalogue rank of every pair under the model's current predict type: int32 [num_pairs] on the device."""
        if not hasattr(model, "rank_items_device"):
            raise TypeError("model must expose rank_items_device()")
        if hasattr(model, "_ensure_tables") and getattr(model, "_cache", None) is not None:
            model._ensure_tables()
        if getattr(model, "_eval_shard", None) is not None:
            raise CandidateScoringError("the rank report needs the whole cached item table on this rank; the tables are "
                                        "item-sharded (lean / multi-rank evaluation): run without --rank_report")
        if model.num_items != self.num_items:
            raise ValueError("the report was built for %d items, the model has %d" % (self.num_items, model.num_items))
        device = model._require_gpu()
        res = self._resident(device)
        ranks = torch.empty(self.num_pairs, dtype=torch.int32, device=device)
        step = self.block_users
        for a in range(0, len(self.users), step):
            b = min(a + step, len(self.users))
            users, target, tptr, titems = self._block(res, a, b, device)
            ranks[self.pair_ptr[a]:self.pair_ptr[b]] = model.rank_items_device(users, target, tptr, titems)[0]
        return ranks

    def _tables(self, pair_rows, pair_columns, user_rows, user_columns, res):
        pairs = torch.empty(len(self.pair_labels), pair_rows.shape[1], dtype=torch.float32, device=pair_rows.device)
        ops.group_metric_means(pair_rows, res["pair_groups"], None, pairs)
        users = None
        if user_rows is not None:
            users = torch.empty(len(self.user_labels), user_rows.shape[1], dtype=torch.float32, device=user_rows.device)
            users = ops.group_metric_means(user_rows, res["user_groups"], None, users).cpu().numpy()
        final = RankTables(tuple(pair_columns), list(self.pair_labels), pairs.cpu().numpy(), tuple(user_columns),
                           list(self.user_labels) if users is not None else [], users)
        buf = self._format(final.pair_columns, final.pair_labels, final.pairs)
        if users is not None:
            buf += "\n" + self._format(final.user_columns, final.user_labels, final.users)
        return final, buf

    @staticmethod
    def _format(columns, labels, table):
        return "columns:\t%s" % "\t".join(str(c).ljust(12) for c in columns) + "".join(
            "\n%s\t%s" % (label, "\t".join(("%.8f" % x).ljust(12) for x in row)) for label, row in zip(labels, table))

    def evaluate(self, model, ranks=None):
        """(final, buf). final = RankTables: pairs [1 + user groups + item groups x (3 + len(ks))] float32 -- row 0 = all pairs --
        the means of rank, rr, pct, hit@K; users [1 + user groups x 3] the means of auc, mrr_full, first_rank. The pair means are
        micro-averages (see the class). buf: per table a header of column names and one "%.8f" line per row, in the grouped
        evaluator's format. ranks: pair_ranks(model) if the caller already holds it."""
        if ranks is None:
            ranks = self.pair_ranks(model)
        res = self._resident(ranks.device)
        pair_rows = torch.empty(self.num_pairs, 3 + len(self.ks), dtype=torch.float32, device=ranks.device)
        ops.rank_pair_rows(ranks, res["pair_n_cand"], self.ks, pair_rows)
        user_rows = torch.empty(len(self.users), 3, dtype=torch.float32, device=ranks.device)
        ops.rank_user_rows(ranks, res["pair_ptr"], res["user_n_cand"], user_rows)
        return self._tables(pair_rows, ops.rank_pair_columns(self.ks), user_rows, ops.RANK_USER_COLUMNS, res)

    def shift(self, ranks_a, ranks_b):
        """How far the pairs move from ranking a to ranking b (e.g. TE -> TIE): (final, buf) in evaluate()'s pair grouping over
        delta = a - b (positive: b ranks the test item higher), improved = (b < a), worsened = (b > a)."""
        if ranks_a.shape != (self.num_pairs,) or ranks_b.shape != (self.num_pairs,) or ranks_a.device != ranks_b.device:
            raise ValueError("shift() takes two pair_ranks() results of this report on one device")
        rows = torch.stack(((ranks_a - ranks_b).float(), (ranks_b < ranks_a).float(), (ranks_b > ranks_a).float()), dim=1)
        return self._tables(rows, ("delta", "improved", "worsened"), None, (), self._resident(ranks_a.device))


class NeighbourReport(object):
    """Whose neighbourhood the fused space copies (--neighbour_report=K): for EVERY item its top-k neighbour lists by cosine in the
    fused space and in each single-modal head's space (EliMRec.neighbours_device, csrc/knn.hip), items in blocks of block_items,
    and per item the columns of ops.neighbour_columns(mods):
      overlap_<m> = |fused list & head m's list| / k (ops.list_overlap); cos_fused, cos_<m> = the mean score of the list;
      pop_fused, pop_<m> = the mean training-interaction count of the listed neighbours
    (fillers skipped; a column of a row without neighbours is NaN). Their means over all items and -- item_group_view -- per item
    popularity group (assign_item_groups over the items' training interactions) are ops.group_metric_means over the
    [items x C] block: only the [1 + groups x C] table reaches the host. The lists do not depend on the predict type."""

    def __init__(self, dataset, user_train_dict, k, item_group_view=None):
        if not isinstance(user_train_dict, dict):
            raise TypeError("user_train_dict must be a dict")
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1 or k > ops.KNN_MAX_K:
            raise ValueError("k must be an integer in [1, %d], got %r" % (ops.KNN_MAX_K, k))
        self.dataset = dataset
        self.num_items = I = int(dataset.num_items)
        self.k = int(k)
        self.block_items = 8192
        self.item_counts = np.zeros(I, dtype=np.int64)
        for items in user_train_dict.values():
            np.add.at(self.item_counts, np.asarray(list(items), dtype=np.int64), 1)
        self.group_labels, self._positions = ["all:".ljust(12)], [np.arange(I, dtype=np.int64)]
        if item_group_view is not None:
            labels, positions = assign_item_groups(np.arange(I, dtype=np.int64), self.item_counts, item_group_view)
            self.group_labels += labels
            self._positions += positions
        self._device = {}                  # device -> the group index, the counts and the blocks' checked queries resident there

    def _resident(self, device):
        hit = self._device.get(str(device))
        if hit is None:
            ptr = np.zeros(len(self._positions) + 1, dtype=np.int64)
            np.cumsum([p.size for p in self._positions], out=ptr[1:])
            hit = dict(groups=ops.GroupIndex(ptr, np.concatenate(self._positions).astype(np.int32), self.num_items, device),
                       counts=torch.from_numpy(self.item_counts.astype(np.float64)).to(device), queries={})
            self._device[str(device)] = hit
        return hit

    def neighbour_rows(self, model):
        """Every item's row of the report on the device: ([items x C] float32, column names)."""
        if not hasattr(model, "neighbours_device"):
            raise TypeError("model must expose neighbours_device()")
        if hasattr(model, "_ensure_tables") and getattr(model, "_cache", None) is not None:
            model._ensure_tables()
        if getattr(model, "_eval_shard", None) is not None:
            raise CandidateScoringError("the neighbour report needs the whole cached item table on this rank; the tables are "
                                        "item-sharded (lean / multi-rank evaluation): run without --neighbour_report")
        if model.num_items != self.num_items:
            raise ValueError("the report was built for %d items, the model has %d" % (self.num_items, model.num_items))
        device = model._require_gpu()
        res = self._resident(device)
        mods = tuple(model._mods)
        columns = ops.neighbour_columns(mods)
        S, k, I = len(mods), self.k, self.num_items
        rows = torch.empty(I, len(columns), dtype=torch.float32, device=device)
        step = max(1, int(self.block_items))
        idx = torch.empty(1 + S, min(step, I), k, dtype=torch.int32, device=device)
        val = torch.empty(1 + S, min(step, I), k, dtype=torch.float32, device=device)
        cnt = torch.empty(min(step, I), dtype=torch.int32, device=device)
        nan = torch.full((), float("nan"), dtype=torch.float64, device=device)
        for a in range(0, I, step):
            b = min(a + step, I)
            query = res["queries"].get((a, b))
            if query is None:
                query = res["queries"][(a, b)] = ops.NeighbourQuery(np.arange(a, b, dtype=np.int32), I, device)
            for h, space in enumerate(("fused",) + mods):
                model.neighbours_device("item", None, k, space, idx[h, :b - a], val[h, :b - a], query=query)
            listed = idx[:, :b - a] >= 0                                           # [1 + S x B x k]
            n = listed.sum(dim=2).double()
            out = rows[a:b]
            for h in range(S):
                ops.list_overlap(idx[0, :b - a], idx[1 + h, :b - a], cnt)
                out[:, h] = torch.where(n[0] > 0, cnt[:b - a].double() / k, nan).float()
            out[:, S:2 * S + 1] = (torch.where(listed, val[:, :b - a].double(), 0.0).sum(dim=2) / n).t().float()
            pop = res["counts"][idx[:, :b - a].clamp(min=0).long()]
            out[:, 2 * S + 1:] = (torch.where(listed, pop, 0.0).sum(dim=2) / n).t().float()
        return rows, columns

    def evaluate(self, model):
        """(final [1 + item groups x C] float32: row 0 = all items, then one row per item popularity group; buf: a header of column
        names and one "%.8f" line per row, in the effect report's format)."""
        rows, columns = self.neighbour_rows(model)
        out = torch.empty(len(self.group_labels), rows.shape[1], dtype=torch.float32, device=rows.device)
        final = ops.group_metric_means(rows, self._resident(rows.device)["groups"], None, out).cpu().numpy()
        buf = "columns:\t%s" % "\t".join(str(c).ljust(12) for c in columns) + "".join(
            "\n%s\t%s" % (label, "\t".join(("%.8f" % x).ljust(12) for x in row)) for label, row in zip(self.group_labels, final))
        return final, buf


EXPOSURE_COLUMNS = ("items", "coverage", "gini", "entropy", "slot_share")


def exposure_summary(counts, positions):
    """How the list slots spread over the catalogue: float64 [len(positions) x 5], per group of item positions (index arrays into
    counts) the columns EXPOSURE_COLUMNS:
      items = the group's size; coverage = the share of its items with count > 0;
      gini = the Gini coefficient of its counts, sum_i (2 i - n - 1) c_(i) / (n sum c) over the ascending counts c_(1..n)
             (0 = every item listed equally often, (n - 1) / n = one item takes every slot; 0 for an empty or all-zero group);
      entropy = -sum p log2 p in bits over p = c / sum c of the group (0 for an empty or all-zero group);
      slot_share = the group's counts over ALL counts (0 when nothing is listed at all).
    counts: how often each item is listed (ops.list_exposure). Pure numpy, float64."""
    c_all = np.asarray(counts, dtype=np.float64).reshape(-1)
    total = c_all.sum()
    out = np.zeros((len(positions), len(EXPOSURE_COLUMNS)), dtype=np.float64)
    for g, at in enumerate(positions):
        c = np.sort(c_all[np.asarray(at, dtype=np.int64).reshape(-1)])
        n, s = c.size, c.sum()
        out[g, 0] = n
        if n:
            out[g, 1] = np.count_nonzero(c > 0) / float(n)
        if n and s > 0:
            out[g, 2] = ((2.0 * np.arange(1, n + 1) - n - 1.0) * c).sum() / (n * s)
            p = c[c > 0] / s
            out[g, 3] = 0.0 - (p * np.log2(p)).sum()
        if total > 0:
            out[g, 4] = s / total
    return out


ListTables = collections.namedtuple("ListTables", ("user_columns", "user_labels", "users", "item_columns", "item_labels", "items"))


class ListReport(object):
    """The recommendation lists themselves (--list_report=K): every test user's top-K list under the model's current predict
    type with the train items masked (predict_device, users in blocks of block_users as EffectReport takes them), and
      per user the columns of ops.list_columns(mods): ils_fused, ils_<m> = the mean pairwise cosine of the K listed items in the
        fused space and in each head's space (EliMRec.list_similarity_device, csrc/lists.hip: one launch per block for all
        spaces), pop = the mean training-interaction count of the listed items (float64 quotient; NaN for an empty list);
      per item how often it is listed (ops.list_exposure, int32 counters filled block after block).
    The user table is ops.group_metric_means over the rows: all users, then the group_view groups (assign_user_groups). The
    item table is exposure_summary of the counters over all items, then the item_group_view groups (assign_item_groups over the
    items' training interactions); the counters come to the host once per evaluate(): num_items int32 values."""

    def __init__(self, dataset, user_train_dict, user_test_dict, top_k, group_view=None, item_group_view=None):
        if not isinstance(user_train_dict, dict) or not isinstance(user_test_dict, dict):
            raise TypeError("user_train_dict and user_test_dict must be dicts")
        if isinstance(top_k, bool) or not isinstance(top_k, (int, np.integer)) or top_k < 2 or top_k > ops.LIST_MAX_K:
            raise ValueError("top_k must be an integer in [2, %d], got %r" % (ops.LIST_MAX_K, top_k))
        self.dataset = dataset
        self.num_items = I = int(dataset.num_items)
        self.user_pos_train = user_train_dict
        self.user_pos_test = user_test_dict
        self.top_k = int(top_k)
        self.users = list(user_test_dict.keys())
        self.block_users = 8192
        self.tie_order = "id"
        self.item_counts = np.zeros(I, dtype=np.int64)
        for items in user_train_dict.values():
            np.add.at(self.item_counts, np.asarray(list(items), dtype=np.int64), 1)
        self.group_labels, self._positions = ["all:".ljust(12)], [np.arange(len(self.users), dtype=np.int64)]
        if group_view is not None:
            labels, positions, self.num_discarded = assign_user_groups(self.users, user_train_dict, group_view)
            self.group_labels += labels
            self._positions += positions
        self.item_labels, self._item_positions = ["all:".ljust(12)], [np.arange(I, dtype=np.int64)]
        if item_group_view is not None:
            labels, positions = assign_item_groups(np.arange(I, dtype=np.int64), self.item_counts, item_group_view)
            self.item_labels += [("item " + x.strip()).ljust(12) for x in labels]
            self._item_positions += positions
        self.columns = self.shift_columns = None   # ops.list_columns of the model list_rows() last saw; ("overlap", "d_<column>"...)
        self._device = {}                  # device -> the user group index and the items' training counts resident there

    def _resident(self, device):
        hit = self._device.get(str(device))
        if hit is None:
            ptr = np.zeros(len(self._positions) + 1, dtype=np.int64)
            np.cumsum([p.size for p in self._positions], out=ptr[1:])
            hit = dict(groups=ops.GroupIndex(ptr, np.concatenate(self._positions).astype(np.int32), len(self.users), device),
                       counts=torch.from_numpy(self.item_counts.astype(np.float64)).to(device))
            self._device[str(device)] = hit
        return hit

    def list_rows(self, model):
        """Every test user's row, list and the catalogue's exposure on the device: ([users x C] float32, column names,
        lists int32 [users x K], counts int32 [num_items])."""
        if not hasattr(model, "list_similarity_device"):
            raise TypeError("model must expose list_similarity_device()")
        if hasattr(model, "_ensure_tables") and getattr(model, "_cache", None) is not None:
            model._ensure_tables()
        if getattr(model, "_eval_shard", None) is not None:
            raise CandidateScoringError("the list report needs the whole cached item table on this rank; the tables are "
                                        "item-sharded (lean / multi-rank evaluation): run without --list_report")
        if model.num_items != self.num_items:
            raise ValueError("the report was built for %d items, the model has %d" % (self.num_items, model.num_items))
        if self.top_k > model.num_items:
            raise CandidateScoringError("list report of the top-%d lists: the catalogue has %d items" % (self.top_k, model.num_items))
        device = model._require_gpu()
        res = self._resident(device)
        columns = self.columns = ops.list_columns(model._mods)
        K, nb, n_users = self.top_k, len(columns) - 1, len(self.users)
        rows = torch.empty(n_users, len(columns), dtype=torch.float32, device=device)
        ils = torch.empty(n_users, nb, dtype=torch.float32, device=device)
        lists = torch.empty(n_users, K, dtype=torch.int32, device=device)
        counts = torch.zeros(self.num_items, dtype=torch.int32, device=device)
        at = 0
        for batch_users in DataIterator(self.users, batch_size=self.block_users, shuffle=False, drop_last=False):
            B = len(batch_users)
            train = [self.user_pos_train.get(u, []) for u in batch_users]
            ptr = np.zeros(B + 1, dtype=np.int64)
            np.cumsum([len(x) for x in train], out=ptr[1:])
            flat = np.fromiter((i for x in train for i in x), dtype=np.int32, count=int(ptr[-1]))
            users_t = torch.as_tensor(np.asarray(batch_users, dtype=np.int64)).to(device)
            idx, _ = model.predict_device(users_t, top_k=K, train_ptr=torch.from_numpy(ptr).to(device),
                                          train_items=torch.from_numpy(flat).to(device), tie_order=self.tie_order)
            lists[at:at + B] = idx
            model.list_similarity_device(lists[at:at + B], ils[at:at + B], side="item")
            ops.list_exposure(lists[at:at + B], counts)
            at += B
        listed = lists >= 0
        pop = torch.where(listed, res["counts"][lists.clamp(min=0).long()], 0.0).sum(dim=1) / listed.sum(dim=1).double()
        rows[:, :nb] = ils
        rows[:, nb] = pop.float()
        return rows, columns, lists, counts

    def _user_table(self, rows):
        out = torch.empty(len(self.group_labels), rows.shape[1], dtype=torch.float32, device=rows.device)
        return ops.group_metric_means(rows, self._resident(rows.device)["groups"], None, out).cpu().numpy()

    @staticmethod
    def _format(columns, labels, table):
        return "columns:\t%s" % "\t".join(str(c).ljust(12) for c in columns) + "".join(
            "\n%s\t%s" % (label, "\t".join(("%.8f" % x).ljust(12) for x in row)) for label, row in zip(labels, table))

    def evaluate(self, model, rows=None):
        """(final, buf). final = ListTables: users [1 + user groups x C] float32 -- row 0 = all test users -- the means of
        ops.list_columns; items [1 + item groups x 5] float64 -- row 0 = the whole catalogue -- exposure_summary of the counters,
        columns EXPOSURE_COLUMNS. buf: per table a header of column names and one "%.8f" line per row, in the grouped evaluator's
        format. rows: list_rows(model) if the caller already holds it."""
        rows, columns, _, counts = self.list_rows(model) if rows is None else rows
        items = exposure_summary(counts.cpu().numpy(), self._item_positions)
        final = ListTables(tuple(columns), list(self.group_labels), self._user_table(rows), EXPOSURE_COLUMNS, list(self.item_labels), items)
        buf = self._format(final.user_columns, final.user_labels, final.users) + "\n" + self._format(
            final.item_columns, final.item_labels, final.items)
        return final, buf

    def shift(self, rows_a, lists_a, rows_b, lists_b):
        """How the lists change from a to b (e.g. TE -> TIE): (final [1 + user groups x 1 + C] float32, buf) in evaluate()'s user
        grouping over the columns self.shift_columns: overlap = |list a & list b| / K (ops.list_overlap) and d_<column> = b - a for
        every user column."""
        n, K = len(self.users), self.top_k
        if (tuple(lists_a.shape) != (n, K) or lists_a.shape != lists_b.shape or rows_a.shape != rows_b.shape or rows_a.shape[0] != n
                or len({t.device for t in (rows_a, rows_b, lists_a, lists_b)}) != 1):
            raise ValueError("shift() takes the rows and lists of two list_rows() results of this report on one device")
        cnt = torch.empty(n, dtype=torch.int32, device=lists_a.device)
        ops.list_overlap(lists_a, lists_b, cnt)
        rows = torch.cat(((cnt.double() / K).float()[:, None], rows_b - rows_a), dim=1)
        if self.columns is None or len(self.columns) != rows_a.shape[1]:
            raise ValueError("shift() takes rows of this report's list_rows()")
        self.shift_columns = ("overlap",) + tuple("d_" + c for c in self.columns)
        final = self._user_table(rows)
        return final, self._format(self.shift_columns, self.group_labels, final)


class ProxyEvaluator(object):
    def __init__(self, dataset, user_train_dict, user_test_dict, user_neg_test=None, metric=None, group_view=None,
                 top_k=50, batch_size=1024, num_thread=8):
        if group_view is not None:
            self.evaluator = GroupedEvaluator(dataset, user_train_dict, user_test_dict, user_neg_test, metric=metric,
                                              group_view=group_view, top_k=top_k, batch_size=batch_size, num_thread=num_thread)
        else:
            self.evaluator = UniEvaluator(dataset, user_train_dict, user_test_dict, user_neg_test, metric=metric,
                                          top_k=top_k, batch_size=batch_size, num_thread=num_thread)

    def metrics_info(self):
        return self.evaluator.metrics_info()

    def evaluate(self, model):
        return self.evaluator.evaluate(model)

    def evaluate_with_overall(self, model):
        """(overall final, overall buf, group final, group buf); without group_view the group pair is (None, None)."""
        if isinstance(self.evaluator, GroupedEvaluator):
            return self.evaluator.evaluate_with_overall(model)
        return self.evaluator.evaluate(model) + (None, None)
