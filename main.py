#!/usr/bin/env python3
"""NeuRec-style driver with the reference's command line (reference main.py:27-175):

    python main.py --recommender=EliMRec --data.input.dataset=<name> --alpha=0.5 --loss=bpr_loss [--key=value ...]

Behaviour kept from the reference's `Net.run`: one pass of the pairwise sampler per epoch, validation every
`test_step` epochs with predict_type TIE, a checkpoint + TE/TIE test pass whenever validation recall improves
(not on epoch 0), early stop after `stop_cnt` epochs without improvement, the same log lines (`--group_view=[10,30,50,100]` adds
the per-user-group table under each test line, `--effect_report=K` the effect breakdown of the top-K lists, `--rank_report=1` the test items' exact catalogue ranks, `--neighbour_report=K` the items' cosine neighbourhoods, fused against single-modal, `--list_report=K` the top-K lists' intra-list similarity and catalogue exposure, `--audience_report=K` the test items' top-K audiences (the users the model ranks highest per item), `--diversify_report=K` the top-N pools re-ranked to K items by greedy MMR per lambda, `--history_report=K` which items of the users' training histories back the top-K lists (`--history_top=T` named per pair), `--significance_report=R` bootstrap intervals of the test metrics over the test users and the paired TE->TIE difference with its p-value, `--neg_sampling=hard` trains on the best of `--neg_candidates=M` uniform negatives per triplet under the last forward's tables; validation and model selection stay on the overall metrics). The per-batch work,
the sampler and the evaluator run on the GPU (elimrec_amd). `--data.input.dataset=synthetic` uses the seeded
Tiktok-shape generator instead of reading files.

`--loss=<method>` names the model method that computes the loss, as in the reference (main.py:98), and the epoch loop is the
reference's: loss method -> zero_grad -> backward(retain_graph=True) -> optimizer step. With `bpr_loss` (EliMRec's own loss)
those four lines run the column-shard engine's fused step (elimrec_amd/plugin.py); any other method of the model (`infonce`,
`fast_loss`, the base class's generic losses) goes through the differentiable table build.
`--resume=<checkpoint>` (not in the reference, which only saves): restores the parameters from a reference-format
checkpoint and, when the side file `<checkpoint>.resume` written next to it exists, the Adam moments, step counts,
epoch counter and best metrics.

Multi-GPU: `--gpus=N` (starts N ranks itself) or a torch.distributed.run launch, one process per GPU. Every rank owns recdim/world columns of the
embedding tables (elimrec_amd/shard.py); an epoch is split over the ranks -- each draws 1/world of the epoch's
triplets in batches of batch_size/world, so the global batch, the number of optimizer steps per epoch and the
learning-rate schedule are those of the single-GPU (and the reference's) configuration; the logged loss is the mean
over ranks.
"""
import os
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "3")      # before the HIP runtime initialises (elimrec_amd/__init__.py has the measurements)

import torch

from elimrec_amd import (Configurator, Dataset, EliMRec, FusedAdam, Logger, Meter, PairwiseSamplerV2,
                         SyntheticDataset, set_seed)
from elimrec_amd import ColumnShardEngine, ColumnShardTrainer
from elimrec_amd.dist import DataParallelTrainer

EFFECTS = ("TE", "TIE")


def count_parameters(module):
    sizes = [(p.numel(), p.requires_grad) for p in module.parameters()]
    return {"Total": sum(n for n, _ in sizes), "Trainable": sum(n for n, g in sizes if g)}


def open_device(cfg):
    """This process's GPU (LOCAL_RANK under torch.distributed.run) and its rank / world size."""
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if cfg.no_cuda or not torch.cuda.is_available():
        print("use cpu")
        raise SystemExit("elimrec_amd has no CPU path for training: an MI355X is required (no_cuda must be FALSE)")
    same_gpu = os.environ.get("ELIMREC_SAME_GPU") == "1"   # every rank on device 0 (one-GPU staging of the multi-rank job, as in
    if same_gpu:                                           # bench.py: RCCL refuses duplicate devices, so the group is gloo and
        local_rank = 0                                     # the collectives are staged through the host)
    print("use", "cuda:%d" % local_rank)
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if same_gpu:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
    return device, rank, world


def open_dataset(cfg):
    if cfg["data.input.dataset"] != "synthetic":
        return Dataset(cfg)
    users, items, interactions = cfg["synthetic_shape"] if "synthetic_shape" in cfg else (36656, 76085, 720829)
    dims = tuple(cfg["synthetic_dims"]) if "synthetic_dims" in cfg else (128, 128, 128)
    data = SyntheticDataset(users, items, interactions, feat_dims=dims, seed=0)
    data.evaluate_neg = int(cfg["rec.evaluate.neg"]) if "rec.evaluate.neg" in cfg else 0
    return data


class Net(object):
    def __init__(self, args):
        self.config = cfg = args
        Logger.logger = Logger(name="_".join([cfg.recommender, cfg["data.input.dataset"], cfg.loss, cfg.suffix]),
                               show_in_console=cfg.verbose != 0, is_creat_log_file=cfg.create_log_file, path=cfg.log_path)
        Logger.info(cfg.params_str())
        cfg.device, self.rank, self.world = open_device(cfg)
        self.dataset = open_dataset(cfg)
        if cfg.recommender != "EliMRec":
            raise ValueError("unknown recommender '%s'" % cfg.recommender)
        self.recommender = EliMRec(cfg, self.dataset).to(cfg.device)
        self.cf_mode = cfg["cf_mode"] if "cf_mode" in cfg else True
        # --group_view=[10,30,50,100]: metrics per user group (users bucketed by their number of training items) beside the overall
        # ones, from the same scoring pass. Validation and model selection keep the overall metrics -- the bits of a run without it
        self.grouped = cfg["group_view"] is not None
        # --effect_report=K (default 0: off): under each [TEST] line the effect breakdown of the test users' top-K lists
        self.effect_report = int(cfg["effect_report"]) if "effect_report" in cfg else 0
        if self.effect_report and self.world > 1:
            raise ValueError("--effect_report needs the whole cached item table on one rank: it is single-GPU")
        # --rank_report=1 (default 0: off): under each [TEST] line where the test items stand in the FULL ranking (rank, rr, pct,
        # hit@K per pair; auc, mrr_full, first_rank per user), after both effects how far TIE moves them relative to TE
        self.rank_report = int(cfg["rank_report"]) if "rank_report" in cfg else 0
        if self.rank_report and self.world > 1:
            raise ValueError("--rank_report needs the whole cached item table on one rank: it is single-GPU")
        # --neighbour_report=K (default 0: off): once per [TEST], after both effects' lines, how much of every item's top-K cosine
        # neighbourhood in the fused space each single-modal head's neighbourhood repeats (the lists do not depend on the predict type)
        self.neighbour_report = int(cfg["neighbour_report"]) if "neighbour_report" in cfg else 0
        if self.neighbour_report and self.world > 1:
            raise ValueError("--neighbour_report needs the whole cached item table on one rank: it is single-GPU")
        # --geometry_report=1 (default 0: off): once per [TEST], after both effects' lines, what the cosine spaces look like --
        # uniformity (--geometry_t), effective rank and centre of the user and item rows, alignment of the training and test pairs,
        # in the fused space and in each head's (the spaces do not depend on the predict type)
        self.geometry_report = int(cfg["geometry_report"]) if "geometry_report" in cfg else 0
        if self.geometry_report and self.world > 1:
            raise ValueError("--geometry_report needs the whole cached tables on one rank: it is single-GPU")
        # --co_report=K (default 0: off), --co_measure=count|cosine|jaccard: once per [TEST], after both effects' lines, how much of
        # every item's top-K co-interaction list ("users who took this also took ...") its top-K cosine lists hold, in the fused space
        # and in each head's (the lists do not depend on the predict type)
        self.co_report = int(cfg["co_report"]) if "co_report" in cfg else 0
        if self.co_report and self.world > 1:
            raise ValueError("--co_report needs the whole cached item table on one rank: it is single-GPU")
        # --list_report=K (default 0: off): under each [TEST] line the top-K lists' intra-list similarity, popularity and catalogue
        # exposure, after both effects how the lists change from TE to TIE
        self.list_report = int(cfg["list_report"]) if "list_report" in cfg else 0
        if self.list_report and self.world > 1:
            raise ValueError("--list_report needs the whole cached item table on one rank: it is single-GPU")
        # --audience_report=K (default 0: off): under each [TEST] line the test items' top-K audiences (whom the item would be pushed
        # to, its training users left out), after both effects how the audiences change from TE to TIE
        self.audience_report = int(cfg["audience_report"]) if "audience_report" in cfg else 0
        if self.audience_report and self.world > 1:
            raise ValueError("--audience_report needs the whole cached tables on one rank: it is single-GPU")
        # --diversify_report=K (default 0: off): under each [TEST] line the top-N pools (--diversify_pool) re-ranked to K items by
        # greedy MMR at every --diversify_lambda: recall / NDCG against intra-list similarity, popularity and exposure
        self.diversify_report = int(cfg["diversify_report"]) if "diversify_report" in cfg else 0
        if self.diversify_report and self.world > 1:
            raise ValueError("--diversify_report needs the whole cached item table on one rank: it is single-GPU")
        # --calibrate_report=K (default 0: off): under each [TEST] line the top-N pools (--calibrate_pool) re-ranked to K items towards
        # each user's own mix of item popularity classes (--item_group_view) at every --calibrate_lambda: miscalibration and class
        # shares against recall / NDCG; the lambda = 1 rows under TE and TIE say whether TIE calibrates the lists by itself
        self.calibrate_report = int(cfg["calibrate_report"]) if "calibrate_report" in cfg else 0
        if self.calibrate_report and self.world > 1:
            raise ValueError("--calibrate_report needs the whole cached item table on one rank: it is single-GPU")
        # --cluster_report=K (default 0: off): under each [TEST] line the top-K lists read per content cluster (--cluster_count
        # spherical k-means clusters of the item rows in --cluster_space), and after both effects the TE -> TIE shift of the clusters'
        # exposure: does TIE move exposure between kinds of content
        self.cluster_report = int(cfg["cluster_report"]) if "cluster_report" in cfg else 0
        if self.cluster_report and self.world > 1:
            raise ValueError("--cluster_report needs the whole cached item table on one rank: it is single-GPU")
        # --neg_sampling=hard (default uniform): every epoch trains on the best of --neg_candidates=M (8) uniform candidates per
        # triplet under the tables of the last training forward, scored in --neg_space=fused|loss|<head> (fused); the first epoch
        # of a run -- no tables yet -- is the uniform one
        self.neg_sampling = str(cfg["neg_sampling"]) if "neg_sampling" in cfg else "uniform"
        if self.neg_sampling not in ("uniform", "hard"):
            raise ValueError("--neg_sampling must be uniform or hard, got %r" % self.neg_sampling)
        if self.neg_sampling == "hard" and self.world > 1:
            raise ValueError("--neg_sampling=hard needs the whole cached item table on one rank: it is single-GPU")
        # --history_report=K (default 0: off): under each [TEST] line the support the users' own training histories give their top-K
        # lists -- largest / mean cosine to the history and the unexpectedness 1 - max, per space -- and the TE -> TIE shift after both
        self.history_report = int(cfg["history_report"]) if "history_report" in cfg else 0
        if self.history_report and self.world > 1:
            raise ValueError("--history_report needs the whole cached item table on one rank: it is single-GPU")
        # --significance_report=R (default 0: off): under each [TEST] line the bootstrap standard error and percentile interval
        # (--significance_level) of every shown metric over R resamples of the test users, overall and per user group; after both
        # effects the paired TE -> TIE difference with its two-sided p-value. It needs metric rows only (run on one GPU only so far)
        self.significance_report = int(cfg["significance_report"]) if "significance_report" in cfg else 0
        # --baseline_report=K (default 0: off), --baseline_sources=[co,rp3,ials,ease,fused,v,...], --baseline_l2=500.0 (EASE's one
        # hyper-parameter, source ease), --baseline_neighbours=50, --baseline_measure,
        # --baseline_alpha=1.0, --baseline_beta=0.6 (RP3beta's exponents, source rp3): under each [TEST] line a [baselines] table --
        # neighbour-vote recommenders (ItemKNN and RP3beta over the training graph, content-KNN in a space of the tables; under the
        # table one "rp3:" line with the exponents, the lists' power-of-two scale and the share of votes the fixed point loses) on the same split; only `overlap` (with the model's own lists) differs between the effects. With
        # --significance_report also the paired model - baseline metric difference per source
        self.baseline_report = int(cfg["baseline_report"]) if "baseline_report" in cfg else 0
        if self.baseline_report and self.world > 1:
            raise ValueError("--baseline_report needs the whole cached item table on one rank: it is single-GPU")
        # --coldstart_report=K (default 0: off): under each [TEST] line how the cold test items rank as trained, folded in from their
        # content and folded in with the mean id row; after both effects the TE -> TIE difference of the means
        self.coldstart_report = int(cfg["coldstart_report"]) if "coldstart_report" in cfg else 0
        if self.coldstart_report and self.world > 1:
            raise ValueError("--coldstart_report needs the whole cached item table on one rank: it is single-GPU")
        # --newuser_report=K (default 0: off): under each [TEST] line the test users as trained, folded in from their training items and
        # folded in with the mean id row; after both effects the TE -> TIE difference of the means
        self.newuser_report = int(cfg["newuser_report"]) if "newuser_report" in cfg else 0
        if self.newuser_report and self.world > 1:
            raise ValueError("--newuser_report needs the whole cached tables on one rank: it is single-GPU")
        Logger.info(count_parameters(self.recommender))
        self.opt = FusedAdam(self.recommender.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
        self.loss_name = str(cfg.loss)
        if not callable(getattr(self.recommender, self.loss_name, None)):
            raise AttributeError("'%s' has no loss method '%s' (--loss)" % (cfg.recommender, self.loss_name))
        self.engine = self.trainer = None
        rec = self.recommender
        if self.loss_name != "bpr_loss":
            if self.world > 1:
                raise ValueError("--loss=%s runs through the generic autograd path, which is single-GPU" % self.loss_name)
        elif getattr(rec, "_lazy", False) and rec.latent_dim % (4 * self.world) != 0:
            # (the replicated-table trainer below no longer carries the folded forms a lazy model needs: fail here, by name, instead
            # of at the first step)
            ok = [w for w in range(1, 9) if rec.latent_dim % (4 * w) == 0]
            raise ValueError("recdim %d does not split into 4-float column groups over %d ranks: the column-shard engine needs "
                             "recdim %% (4 x world) == 0 -- launch on %s GPUs (or pad recdim)" % (rec.latent_dim, self.world, ok))
        elif getattr(rec, "_lazy", False):
            # the column-shard engine with this job's world / rank. It attaches itself to the model (elimrec_amd/plugin.py): the
            # epoch loop below is the reference's own four lines (main.py:98-101) and runs on it
            self.engine = ColumnShardEngine(rec)
            self.trainer = ColumnShardTrainer(self.engine, self.opt, world_size=self.world, rank=self.rank)
        else:       # adjacencies with a diagonal (norm / mean+I) without --propagation=folded, layer_num < 2: replicated tables
            self.trainer = DataParallelTrainer(rec, self.opt, world_size=self.world, rank=self.rank)
        self.start_epoch, self.resume_state = 0, None
        if "resume" in cfg and cfg["resume"]:
            self.load_checkpoint(str(cfg["resume"]))

    # ------------------------------------------------------------------ checkpoint / resume
    def save_checkpoint(self, path, epoch, extra):
        """The reference's checkpoint (state_dict, main.py:131-133) + a side file with what a resume needs on top."""
        rec = self.recommender
        if self.engine is not None:
            self.engine.sync_to_model()                       # all ranks (collective when world > 1)
            emb = self.engine.optimizer_state()
        else:
            emb = None
        if self.rank != 0:
            return
        torch.save(rec.state_dict(), path)
        torch.save(dict(epoch=epoch, embedding_adam=emb, adam=self.opt.export_state(rec.named_parameters()), extra=extra),
                   path + ".resume")

    def load_checkpoint(self, path):
        rec = self.recommender
        state = torch.load(path, map_location="cpu")
        rec.load_state_dict(state, strict=True)
        if self.engine is not None:
            self.engine.load_from_model()
        side = path + ".resume"
        if os.path.exists(side):
            extra = torch.load(side, map_location="cpu", weights_only=True)     # tensors, numbers, strings, dicts only
            rec._workspace(1)                                  # parameters move into the flat buffers before the moments
            self.opt.import_state(rec.named_parameters(), extra["adam"])
            if self.engine is not None and extra.get("embedding_adam") is not None:
                self.engine.load_optimizer_state(extra["embedding_adam"])
            self.start_epoch = int(extra["epoch"]) + 1
            self.resume_state = extra.get("extra")
            Logger.info("[resumed] %s at epoch %d (optimizer state restored)" % (path, self.start_epoch))
        else:
            Logger.info("[resumed] %s (parameters only: no %s)" % (path, side))

    # ------------------------------------------------------------------ pieces of an epoch
    def generic_step(self, users, pos, neg):
        """main.py:98-101 as written: loss method -> zero_grad -> backward -> optimizer step."""
        loss = getattr(self.recommender, self.loss_name)(users, pos, neg)
        self.opt.zero_grad()
        loss.backward(retain_graph=True)
        self.opt.step()
        return loss

    def train_epoch(self, batches):
        """One pass over the sampler; the mean loss of the epoch. One rank: the reference's line 102 verbatim --
        `loss.cpu().item()` after every batch (the engine publishes each step's loss to the host from the launch that sums it,
        elimrec_amd/plugin.py: the read does not wait for the step). Several ranks: the losses stay on the device and are
        all-reduced once per epoch."""
        self.recommender.train()
        tracker = Meter(name="MultiLoss(bpr)")
        tracker.reset()
        # the reference's loop body; only the replicated-table fallback (no engine) has a step call of its own
        step = self.generic_step if (self.trainer is None or self.engine is not None) else self.trainer.step
        # the column-shard engine returns views into a ring of loss slots: an epoch longer than the ring keeps copies
        ring = getattr(self.engine, "loss_ring_len", 0) if self.engine is not None else 0
        keep = (lambda t: t.clone()) if ring and len(batches) >= ring else (lambda t: t)
        shard_trainer = self.trainer if self.engine is not None else None
        if shard_trainer is not None:
            batches = list(batches)                   # the epoch's triplets, sampled on the device in one launch (data/sampler.py)
            shard_trainer.prestage(batches)           # ... complete before the first step: every step's planner may run ahead
            if getattr(shard_trainer, "lookup", False) and getattr(shard_trainer, "multi", False):
                shard_trainer.plan_lookup(batches)    # row-sharded constants: this epoch's lookup split sizes, planned ahead
        if self.world == 1:
            for users, pos, neg in batches:
                loss = step(users, pos, neg)
                tracker.update(val=loss.cpu().item())                               # main.py:102
        else:
            import torch.distributed as dist
            on_device = torch.stack([keep(step(users, pos, neg).detach()) for users, pos, neg in batches])
            dist.all_reduce(on_device, op=dist.ReduceOp.SUM)
            on_device /= self.world
            for value in on_device.cpu().tolist():
                tracker.update(val=value)
        if self.world > 1:       # every rank sees a bad index of any rank: all raise together, none is left in a collective
            import torch.distributed as dist
            dist.all_reduce(self.recommender._index_err(), op=dist.ReduceOp.MAX)
        self.recommender.check_indices()
        return tracker.avg

    def validate(self, epoch, meters):
        """TIE validation metrics of this epoch -> the meters; returns the (precision, recall, ndcg) triple or None."""
        rec = self.recommender
        rec.eval()
        Logger.info("[VALID]")
        Logger.info("[CF Mode]")
        for m in meters.values():
            m.reset_time()
        rec.predict_type = "TIE"
        result = rec.evaluate_with_overall()[0] if self.grouped else rec.evaluate()[0]
        if result is not None:
            for key, value in zip(("precision", "recall", "ndcg"), result):
                meters[key].update(val=value, epoch=epoch)
            Logger.info("[{}]\t{}\t{}\t{}".format("TIE", meters["recall"], meters["ndcg"], meters["precision"]))
        return result

    def test_all_effects(self):
        """TE and TIE metrics on the test split, formatted as the reference prints them."""
        rec, lines, ranks, shown, backed, sure, reached, grouped, cold, fresh = self.recommender, {}, {}, {}, {}, {}, {}, {}, {}, {}
        if self.grouped:
            Logger.info(rec.test_evaluator.metrics_info())
        for effect in EFFECTS:
            rec.predict_type = effect
            result, _, _, group_table = rec.test_with_overall() if self.grouped else rec.test() + (None, None)
            assert result is not None
            lines[effect] = "  [{}]\t{}\t{}\t{}".format(effect, result[1], result[0], result[2])
            Logger.info(lines[effect])
            if self.grouped:               # one line per user group: "(lo,hi]:" and the metrics in the header's order
                Logger.info("  [{}] by training interactions:{}".format(effect, group_table))
            if self.effect_report:         # what the top-K lists under this effect are made of: column means, overall and per group
                Logger.info("  [{}] effect breakdown of the top-{} lists:\n{}".format(effect, self.effect_report, rec.effect_report()[1]))
            if self.rank_report:           # where the test items stand in the full ranking under this effect
                ranks[effect] = rec.rank_reporter.pair_ranks(rec)
                Logger.info("  [{}] catalogue rank of the test items:\n{}".format(effect, rec.rank_reporter.evaluate(rec, ranks[effect])[1]))
            if self.coldstart_report:      # the cold test items as trained / from content / with the mean id row under this effect
                cold[effect], buf = rec.coldstart_reporter.evaluate(rec)
                Logger.info("  [{}] cold test items (no training interaction):\n{}".format(effect, buf))
            if self.newuser_report:        # the test users as trained / folded in from their histories / with the mean id row
                fresh[effect], buf = rec.newuser_reporter.evaluate(rec)
                Logger.info("  [{}] [new users] test users folded in from their training histories:\n{}".format(effect, buf))
            if self.list_report:           # the lists themselves under this effect: how alike, how popular, how much of the catalogue
                shown[effect] = rec.list_reporter.list_rows(rec)
                Logger.info("  [{}] top-{} lists: similarity, popularity, exposure:\n{}".format(
                    effect, self.list_report, rec.list_reporter.evaluate(rec, shown[effect])[1]))
            if self.audience_report:       # the reverse lists under this effect: whom each test item reaches
                reached[effect] = rec.audience_reporter.audience_rows(rec)
                Logger.info("  [{}] top-{} audiences of the test items: reach, activity, exposure over the users:\n{}".format(
                    effect, self.audience_report, rec.audience_reporter.evaluate(rec, reached[effect])[1]))
            if self.diversify_report:      # the top-N pools under this effect re-ranked to K by greedy MMR, one row per lambda
                reporter = rec.diversify_reporter
                Logger.info("  [{}] top-{} of the top-{} pools by MMR, per lambda:\n{}".format(
                    effect, reporter.top_k, reporter.pool, reporter.evaluate(rec)[1]))
            if self.calibrate_report:      # the top-N pools under this effect re-ranked to K towards the users' own popularity mix
                reporter = rec.calibrate_reporter
                Logger.info("  [{}] top-{} of the top-{} pools calibrated to the users' popularity mix, per lambda:\n{}".format(
                    effect, reporter.top_k, reporter.pool, reporter.evaluate(rec)[1]))
            if self.cluster_report:        # the lists under this effect read per content cluster of the items
                reporter = rec.cluster_reporter
                grouped[effect] = reporter.evaluate(rec)
                Logger.info("  [{}] top-{} lists over the {} content clusters ({} space):\n{}".format(
                    effect, reporter.top_k, reporter.num_classes, reporter.space, grouped[effect][1]))
            if self.history_report:        # how close the users' training histories sit to the lists under this effect, per space
                backed[effect] = rec.history_reporter.history_rows(rec)
                Logger.info("  [{}] support of the top-{} lists in the users' histories:\n{}".format(
                    effect, self.history_report, rec.history_reporter.evaluate(rec, backed[effect])[1]))
            if self.significance_report:   # how far the metrics of this effect move under resampling of the test users
                reporter = rec.significance_reporter
                sure[effect] = reporter.metric_rows(rec)
                Logger.info("  [{}] metric intervals ({} replicates, {:g} %):\n{}".format(
                    effect, reporter.replicates, 100.0 * reporter.level, reporter.evaluate(rec, sure[effect])[1]))
            if self.baseline_report:       # neighbourhood baselines on the same split; only `overlap` depends on the effect
                reporter = rec.baseline_reporter
                Logger.info("  [{}] [baselines] top-{} neighbour-vote lists ({} neighbours, {}):\n{}".format(
                    effect, reporter.k, reporter.neighbours, reporter.measure, reporter.evaluate(rec)[1]))
                if self.significance_report:   # model - baseline per user, the users resampled as pairs
                    for source in reporter.sources:
                        Logger.info("  [{} - {}] metric difference, paired bootstrap:\n{}".format(
                            effect, source, rec.significance_reporter.shift(reporter.metric_rows(rec, source), sure[effect])[1]))
        if self.coldstart_report:          # d_<column>: TIE - TE
            Logger.info("  [TE->TIE] cold test items:\n{}".format(rec.coldstart_reporter.shift(cold["TE"], cold["TIE"])[1]))
        if self.newuser_report:            # d_<column>: TIE - TE
            Logger.info("  [TE->TIE] [new users]:\n{}".format(rec.newuser_reporter.shift(fresh["TE"], fresh["TIE"])[1]))
        if self.rank_report:               # positive delta: TIE ranks the test item higher than TE does
            Logger.info("  [TE->TIE] rank shift of the test items:\n{}".format(rec.rank_reporter.shift(ranks["TE"], ranks["TIE"])[1]))
        if self.list_report:               # overlap: the share of the TE list that TIE keeps; d_<column>: TIE - TE
            a, b = shown["TE"], shown["TIE"]
            Logger.info("  [TE->TIE] list shift:\n{}".format(rec.list_reporter.shift(a[0], a[2], b[0], b[2])[1]))
        if self.audience_report:           # overlap: the share of an item's TE audience that TIE keeps; d_<column>: TIE - TE
            Logger.info("  [TE->TIE] audience shift:\n{}".format(rec.audience_reporter.shift(reached["TE"], reached["TIE"])[1]))
        if self.cluster_report:            # d_slot_share: the share of the list slots a cluster gains under TIE; d_<column>: TIE - TE
            Logger.info("  [TE->TIE] content clusters, exposure shift:\n{}".format(
                rec.cluster_reporter.shift(grouped["TE"][0], grouped["TIE"][0])[1]))
        if self.history_report:            # d_<column>: TIE - TE; a positive d_unexpected_<space>: TIE strays further from the history
            Logger.info("  [TE->TIE] history support shift:\n{}".format(rec.history_reporter.shift(backed["TE"], backed["TIE"])[1]))
        if self.significance_report:       # TIE - TE per user, the users resampled as pairs; p: two-sided, "no difference"
            Logger.info("  [TE->TIE] metric difference, paired bootstrap:\n{}".format(
                rec.significance_reporter.shift(sure["TE"], sure["TIE"])[1]))
        if self.neighbour_report:
            Logger.info("  [neighbours] top-{} cosine neighbours of every item, fused space against the heads:\n{}".format(
                self.neighbour_report, rec.neighbour_reporter.evaluate(rec)[1]))
        if self.geometry_report:
            Logger.info("  [geometry] uniformity (t = {:g}), spectrum and alignment of the cosine spaces:\n{}".format(
                rec.geometry_reporter.t, rec.geometry_reporter.evaluate(rec)[1]))
        if self.co_report:
            Logger.info("  [co-neighbours] top-{} co-interaction neighbours ({}) of every item against its cosine neighbours:\n{}".format(
                self.co_report, rec.co_reporter.measure, rec.co_reporter.evaluate(rec)[1]))
        return lines

    # ------------------------------------------------------------------ the run
    def run(self):
        cfg, rec = self.config, self.recommender
        k = str(cfg["topks"][0])
        stamp = int(time.time())
        loss_meter = Meter("loss", id=stamp)
        meters = {"recall": Meter("R@" + k, id=stamp), "precision": Meter("P@" + k, id=stamp), "ndcg": Meter("N@" + k, id=stamp)}
        if cfg.batch_size % self.world != 0:
            raise ValueError("batch_size %d is not a multiple of the %d ranks" % (cfg.batch_size, self.world))
        hard = {}
        if self.neg_sampling == "hard":
            hard = dict(neg_sampling="hard", neg_candidates=cfg["neg_candidates"] if "neg_candidates" in cfg else 8,
                        neg_space=str(cfg["neg_space"]) if "neg_space" in cfg else "fused", model=rec)
        batches = PairwiseSamplerV2(self.dataset, neg_num=1, batch_size=cfg.batch_size // self.world, shuffle=True,
                                    device=cfg.device, seed=cfg.seed + self.rank,
                                    shard=(self.rank, self.world) if self.world > 1 else None, **hard)
        batches.epoch = self.start_epoch
        best_recall = dict.fromkeys(EFFECTS, 0)
        best_epoch = dict.fromkeys(EFFECTS, 0)
        best_valid_line, test_lines = "", dict.fromkeys(EFFECTS, "")
        checkpoint = rec.getFileName()
        if self.resume_state:
            best_recall, best_epoch = dict(self.resume_state["best_recall"]), dict(self.resume_state["best_epoch"])
            best_valid_line, test_lines = self.resume_state["best_valid_line"], dict(self.resume_state["test_lines"])
        for epoch in range(self.start_epoch, cfg.num_epoch):
            Logger.info("======================")
            Logger.info("EPOCH[%d/%d]" % (epoch, cfg.num_epoch))
            loss_meter.reset_time()
            epoch_loss = self.train_epoch(batches)
            if hard:
                st = batches.last_stats
                Logger.info("[hard negatives] " + ("best of %d in '%s': %.4f of the triplets moved off the uniform negative, mean score "
                                                   "%.4f against %.4f" % (batches.neg_candidates, batches.neg_space, st["moved"],
                                                                          st["score_picked"], st["score_first"])
                                                   if st["hard"] else "uniform (no tables yet)"))
            if (epoch + 1) % cfg["test_step"] == 0:
                result = self.validate(epoch, meters)
                if meters["recall"].val > best_recall["TIE"] and epoch != 0:
                    best_valid_line = "[EPOCH {}]\n{}\t{}\t{}".format(epoch, meters["recall"], meters["ndcg"], meters["precision"])
                    Logger.info("[Better Result]")
                    Logger.info("[TEST]")
                    for effect in EFFECTS:
                        best_recall[effect], best_epoch[effect] = float(result[1]), epoch
                    test_lines = self.test_all_effects()
                    if cfg["save_flag"]:
                        Logger.info("[saved][EPOCH %d]" % epoch)
                        self.save_checkpoint(checkpoint, epoch, dict(best_recall=best_recall, best_epoch=best_epoch,
                                                                     best_valid_line=best_valid_line, test_lines=test_lines))
                if epoch - best_epoch["TIE"] > cfg.stop_cnt:
                    break
            loss_meter.update(val=epoch_loss, epoch=epoch)
            Logger.info("%s" % loss_meter)
        Logger.info("=>[{}] best_valid_result:\n{}".format("TIE", best_valid_line))
        for effect in EFFECTS:
            Logger.info("=>[{}] test_result:\n{}".format(effect, test_lines[effect]))
        return best_recall, test_lines


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    os.chdir(here)
    config = Configurator(os.path.join(here, "NeuRec.properties"), default_section="hyperparameters")
    if "gpus" in config and int(config["gpus"]) > 1 and "WORLD_SIZE" not in os.environ:
        # --gpus=N from a bare shell: start one rank per GPU as child processes (this parent has not touched the GPU)
        import socket
        import subprocess
        import sys
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        raise SystemExit(subprocess.call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node",
                                          str(int(config["gpus"])), "--master-addr", "127.0.0.1", "--master-port", str(port),
                                          os.path.abspath(__file__)] + sys.argv[1:], env=env))
    set_seed(config["seed"])
    Net(config).run()
