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
import numpy as np
import torch

from . import ops
from .data_iterator import DataIterator
from .ops import CandidateScoringError                                                                      # noqa: F401
# (the reports and their pure functions live in reports.py; they stay importable from here)
from .reports import CalibrationReport, CalibrationTables, calibration_columns, item_classes                 # noqa: F401
from .reports import CLUSTER_COLUMNS, CLUSTER_USER_COLUMNS, ClusterReport, ClusterShift, ClusterTables, cluster_rows, cluster_user_rows   # noqa: F401
from .reports import CoNeighbourReport, co_neighbour_columns   # noqa: F401
from .reports import COLDSTART_VARIANTS, ColdStartReport, cold_test_items, coldstart_columns, coldstart_row, isolated_row_scale   # noqa: F401
from .reports import NEWUSER_VARIANTS, NewUserReport, fold_in_weights, format_newuser, newuser_columns, newuser_overall_metrics   # noqa: F401
from .reports import BASELINE_LIST_COLUMNS, BaselineReport, BaselineTables   # noqa: F401
from .reports import GEOMETRY_COLUMNS, GeometryReport, GeometryTables, spectrum_summary   # noqa: F401
from .reports import (AUDIENCE_COLUMNS, AUDIENCE_EXPOSURE_COLUMNS, AudienceReport, AudienceTables, DIVERSIFY_COLUMNS, EXPOSURE_COLUMNS, DiversifyReport, DiversifyTables, EffectReport, HistoryReport, ListReport,   # noqa: F401
                      ListTables, NeighbourReport, RankReport, RankTables, SignificanceReport, SignificanceTables, assign_item_groups, assign_user_groups, bootstrap_summary, exposure_summary, format_rows, group_index, group_table, lists_csr)

metric_dict = {"Precision": 1, "Recall": 2, "MAP": 3, "NDCG": 4, "MRR": 5}
re_metric_dict = {v: k for k, v in metric_dict.items()}


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
        return lists_csr(users, table, device, unique=unique)

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
                ptr, flat, lens = ops.ragged(lists, dtype=np.int32)
                tptr, titems, _ = ops.ragged([np.arange(p, dtype=np.int32) for p in npos], dtype=np.int32)
                titems = titems if titems.size else np.zeros(1, dtype=np.int32)
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
        if str(device) not in self._index:
            self._index[str(device)] = group_index(self._positions, len(self.evaluator.default_users()), device)
        return self._index[str(device)]

    def group_means(self, rows):
        """Device rows [default users x metrics*K] (UniEvaluator.metric_rows) -> host float32 [groups x metrics*K]."""
        return group_table(rows, self._group_index(rows.device), len(self.group_labels))

    def format_groups(self, final):
        """[groups x shown columns] -> the reference's multi-line string (grouped_evaluator.py:107-112)."""
        return format_rows(self.group_labels, final)

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
