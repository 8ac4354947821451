"""Plugin base class with the reference's method set (models/BasicModel.py:9-113): builds the
valid/test evaluators from the config, names checkpoints, exposes evaluate()/test()."""
import os

import torch
import torch.nn.functional as F
from torch import nn

from . import ops
from .evaluator import ProxyEvaluator, UniEvaluator
from .reports import AudienceReport, BaselineReport, CalibrationReport, ClusterReport, ColdStartReport, CoNeighbourReport, DiversifyReport, EffectReport, GeometryReport, HistoryReport, ListReport, NeighbourReport, NewUserReport, RankReport, SignificanceReport



def baseline_sources(value):
    """--baseline_sources as a tuple of names: a list / tuple of strings, or the switch's text "[co,fused,v]" (names unquoted)."""
    if isinstance(value, str):
        text = value.strip()
        if not (text.startswith("[") and text.endswith("]")):
            raise ValueError("baseline_sources is a list like [co,fused,v], got %r" % (value,))
        value = [x.strip().strip("'\"") for x in text[1:-1].split(",")]
    if not isinstance(value, (list, tuple)) or not value or any(not isinstance(x, str) or not x for x in value) or len(set(value)) != len(value):
        raise ValueError("baseline_sources is a list of distinct names like [co,fused,v], got %r" % (value,))
    return tuple(value)


class BasicModel(nn.Module):
    def __init__(self, dataset, config):
        super(BasicModel, self).__init__()
        self.config = config
        self.dataset = dataset
        train = dataset.get_user_train_dict()
        common = dict(metric=config["metric"], group_view=config["group_view"], top_k=config["topks"],
                      batch_size=config["test_batch_size"], num_thread=config["num_thread"])
        # --eval_candidates=full|sampled (CLI-only, default full): "sampled" ranks each user's test items among the data set's
        # rec.evaluate.neg sampled negatives (cpp/uni_evaluator.py:132-140); "full" ranks the whole catalogue even when
        # rec.evaluate.neg > 0, as the reference's driver does (models/BasicModel.py:14-31 passes None)
        mode = str(config["eval_candidates"]) if "eval_candidates" in config else "full"
        if mode not in ("full", "sampled"):
            raise ValueError("eval_candidates must be full or sampled")
        valid_neg = test_neg = None
        if mode == "sampled":
            n_neg = int(config["rec.evaluate.neg"]) if "rec.evaluate.neg" in config else 0
            if n_neg <= 0:
                raise ValueError("--eval_candidates=sampled needs rec.evaluate.neg > 0 (negatives per user)")
            valid_neg, test_neg = dataset.get_user_valid_neg_dict(n_neg), dataset.get_user_test_neg_dict(n_neg)
        self.valid_evaluator = ProxyEvaluator(dataset, train, dataset.get_user_valid_dict(), valid_neg, **common)
        self.test_evaluator = ProxyEvaluator(dataset, train, dataset.get_user_test_dict(), test_neg, **common)
        if "tie_order" in config:        # --tie_order=reference (CLI-only): the reference's lists among equal scores too (evaluator.py)
            if str(config["tie_order"]) not in ("id", "reference"):
                raise ValueError("tie_order must be id or reference")
            for ev in (self.valid_evaluator, self.test_evaluator):
                ev.evaluator.tie_order = str(config["tie_order"])
        # --effect_report=K (CLI-only, default 0 = off): the effect breakdown of the test users' top-K lists, its column means
        # overall and per user group (reports.EffectReport)
        k_report = int(config["effect_report"]) if "effect_report" in config else 0
        if k_report < 0:
            raise ValueError("effect_report must be 0 (off) or the K of the lists to break down")
        self.effect_reporter = EffectReport(dataset, train, dataset.get_user_test_dict(), k_report,
                                            group_view=config["group_view"]) if k_report else None
        # --rank_report=1 (CLI-only, default 0 = off): the exact catalogue rank of every (test user, test item) pair and its means
        # overall, per user group and -- with --item_group_view=[...] -- per item popularity group (reports.RankReport)
        item_view = config["item_group_view"] if "item_group_view" in config else None
        if "rank_report" in config and int(config["rank_report"]) not in (0, 1):
            raise ValueError("rank_report must be 0 (off) or 1")
        self.rank_reporter = RankReport(dataset, train, dataset.get_user_test_dict(), config["topks"], group_view=config["group_view"],
                                        item_group_view=item_view) if "rank_report" in config and int(config["rank_report"]) else None
        # --neighbour_report=K (CLI-only, default 0 = off): every item's top-K cosine neighbours in the fused space and in each head's
        # space -- how much of the fused list a head's list repeats, the lists' mean cosine and popularity -- as means overall and,
        # with --item_group_view=[...], per item popularity group (reports.NeighbourReport)
        k_near = int(config["neighbour_report"]) if "neighbour_report" in config else 0
        if k_near < 0:
            raise ValueError("neighbour_report must be 0 (off) or the K of the neighbour lists")
        self.neighbour_reporter = NeighbourReport(dataset, train, k_near, item_group_view=item_view) if k_near else None
        # --list_report=K (CLI-only, default 0 = off): the test users' top-K lists themselves -- intra-list similarity in the fused
        # space and in each head's space, popularity of the listed items, catalogue coverage / Gini / entropy of the exposure --
        # overall, per user group (--group_view) and per item popularity group (--item_group_view) (reports.ListReport)
        k_list = int(config["list_report"]) if "list_report" in config else 0
        if k_list and not 2 <= k_list <= min(ops.LIST_MAX_K, int(dataset.num_items)):
            raise ValueError("list_report must be 0 (off) or the K of the lists, 2 <= K <= min(%d, the catalogue's %d items), got %d"
                             % (ops.LIST_MAX_K, int(dataset.num_items), k_list))
        self.list_reporter = ListReport(dataset, train, dataset.get_user_test_dict(), k_list, group_view=config["group_view"],
                                        item_group_view=item_view) if k_list else None
        # --audience_report=K (CLI-only, default 0 = off): for every item with a test interaction the K users the model ranks highest
        # for it, the item's training users left out -- how many of its test users it reaches, how active and how highly scored the
        # listed users are, how the list slots spread over the users -- overall and per item popularity group (--item_group_view)
        # (reports.AudienceReport)
        k_aud = int(config["audience_report"]) if "audience_report" in config else 0
        if k_aud and not 1 <= k_aud <= ops.AUDIENCE_MAX_K:
            raise ValueError("audience_report must be 0 (off) or the K of the audience lists, 1 <= K <= %d, got %d" % (ops.AUDIENCE_MAX_K, k_aud))
        self.audience_reporter = AudienceReport(dataset, train, dataset.get_user_test_dict(), k_aud, item_group_view=item_view) if k_aud else None
        # --diversify_report=K (CLI-only, default 0 = off): the test users' top-N pools (--diversify_pool=N, default min(4K, 256,
        # the catalogue)) re-ranked to K items by greedy MMR at every --diversify_lambda (default [1.0,0.9,0.7,0.5]): what the trade
        # costs in recall / NDCG and buys in intra-list similarity and catalogue exposure, overall and per user group
        # (reports.DiversifyReport)
        k_div = int(config["diversify_report"]) if "diversify_report" in config else 0
        self.diversify_reporter = None
        if k_div:
            pool = config["diversify_pool"] if "diversify_pool" in config else None
            lambdas = config["diversify_lambda"] if "diversify_lambda" in config else [1.0, 0.9, 0.7, 0.5]
            self.diversify_reporter = DiversifyReport(dataset, train, dataset.get_user_test_dict(), k_div, pool=pool, lambdas=lambdas,
                                                      group_view=config["group_view"])
        # --calibrate_report=K (CLI-only, default 0 = off): the test users' top-N pools (--calibrate_pool=N, default min(4K, 256, the
        # catalogue)) re-ranked to K items towards each user's own mix of item popularity classes (--item_group_view, required) at
        # every --calibrate_lambda (default [1.0,0.9,0.7,0.5]): the lists' miscalibration and class shares against recall / NDCG,
        # overall and per user group (reports.CalibrationReport)
        k_cal = int(config["calibrate_report"]) if "calibrate_report" in config else 0
        self.calibrate_reporter = None
        if k_cal:
            if item_view is None:
                raise ValueError("--calibrate_report needs --item_group_view=[...]: the item classes are its popularity buckets")
            pool = config["calibrate_pool"] if "calibrate_pool" in config else None
            lambdas = config["calibrate_lambda"] if "calibrate_lambda" in config else [1.0, 0.9, 0.7, 0.5]
            self.calibrate_reporter = CalibrationReport(dataset, train, dataset.get_user_test_dict(), k_cal, item_view, pool=pool,
                                                        lambdas=lambdas, group_view=config["group_view"])
        # --cluster_report=K (CLI-only, default 0 = off): the items grouped into --cluster_count=C (default 8, 2 <= C <= 16) content
        # clusters by spherical k-means of their rows in --cluster_space=fused|<head> (default fused), once per table version; the
        # test users' top-K lists read per cluster: size, pop, cohesion, train / test / slot share, and per user the clusters in a
        # list and its miscalibration against the user's own cluster mix, overall and per user group (reports.ClusterReport)
        k_clu = int(config["cluster_report"]) if "cluster_report" in config else 0
        self.cluster_reporter = None
        if k_clu:
            n_clu = int(config["cluster_count"]) if "cluster_count" in config else 8
            space = str(config["cluster_space"]) if "cluster_space" in config else "fused"
            self.cluster_reporter = ClusterReport(dataset, train, dataset.get_user_test_dict(), k_clu, n_clusters=n_clu, space=space,
                                                  group_view=config["group_view"])
        # --history_report=K (CLI-only, default 0 = off): which items of the test users' training histories back their top-K lists
        # (--history_top=T entries named per pair, default 3): the largest and the mean cosine of the history to each listed item
        # and the unexpectedness 1 - max, in the fused space and in each head's, overall and per user group (reports.HistoryReport)
        k_hist = int(config["history_report"]) if "history_report" in config else 0
        self.history_reporter = None
        if k_hist:
            t_hist = config["history_top"] if "history_top" in config else 3
            self.history_reporter = HistoryReport(dataset, train, dataset.get_user_test_dict(), k_hist, top=t_hist,
                                                  group_view=config["group_view"])
        # --significance_report=R (CLI-only, default 0 = off): R bootstrap replicates over the test users of the evaluator's own metric
        # rows: standard error and percentile interval (--significance_level, default 0.95; --significance_seed, default 2022) of
        # every shown metric, overall and per user group, and the paired TE -> TIE difference with its p-value
        # (reports.SignificanceReport). Its evaluator is one of its own -- the test pass's arguments, not its state
        n_rep = config["significance_report"] if "significance_report" in config else 0
        if isinstance(n_rep, bool) or not isinstance(n_rep, int) or n_rep < 0:
            raise ValueError("significance_report must be 0 (off) or the number of bootstrap replicates, got %r" % (n_rep,))
        self.significance_reporter = None
        if n_rep:
            ev = UniEvaluator(dataset, train, dataset.get_user_test_dict(), test_neg, metric=config["metric"], top_k=config["topks"],
                              batch_size=config["test_batch_size"], num_thread=config["num_thread"])
            ev.tie_order = self.test_evaluator.evaluator.tie_order
            self.significance_reporter = SignificanceReport(
                dataset, train, dataset.get_user_test_dict(), config["topks"], metric=config["metric"], group_view=config["group_view"],
                replicates=n_rep, level=config["significance_level"] if "significance_level" in config else 0.95,
                seed=config["significance_seed"] if "significance_seed" in config else 2022, evaluator=ev)
        # --geometry_report=1 (CLI-only, default 0 = off): what the learned cosine spaces look like -- uniformity at --geometry_t
        # (default 2.0), effective rank, top1, rank99 and centre of the user and the item rows of the fused space and of each head's,
        # per user group (--group_view) and item popularity group (--item_group_view), and the alignment of the training and the test
        # pairs -- once per table version (reports.GeometryReport)
        if "geometry_report" in config and int(config["geometry_report"]) not in (0, 1):
            raise ValueError("geometry_report must be 0 (off) or 1")
        self.geometry_reporter = None
        if "geometry_report" in config and int(config["geometry_report"]):
            self.geometry_reporter = GeometryReport(dataset, train, dataset.get_user_test_dict(), group_view=config["group_view"],
                                                    item_group_view=item_view, t=config["geometry_t"] if "geometry_t" in config else 2.0)
        # --co_report=K (CLI-only, default 0 = off): every item's top-K co-interaction neighbours ("users who took this also took
        # ...", --co_measure=count|cosine|jaccard, default cosine) beside its top-K cosine neighbours in the fused space and in each
        # head's: how much of the behavioural list the learned lists hold, overall and per --item_group_view popularity group
        # (reports.CoNeighbourReport)
        k_co = int(config["co_report"]) if "co_report" in config else 0
        if k_co < 0:
            raise ValueError("co_report must be 0 (off) or the K of the co-interaction lists")
        co_measure = str(config["co_measure"]) if "co_measure" in config else "cosine"
        if co_measure not in ops.COOCCUR_MEASURES:
            raise ValueError("co_measure is one of %s, got %r" % (", ".join(sorted(ops.COOCCUR_MEASURES)), co_measure))
        self.co_reporter = CoNeighbourReport(dataset, train, k_co, measure=co_measure, item_group_view=item_view) if k_co else None
        # --baseline_report=K (CLI-only, default 0 = off): baselines beside the model -- per --baseline_sources entry (default [co]:
        # ItemKNN over the training graph under --baseline_measure=count|cosine|jaccard, default cosine; fused / a head letter:
        # content-KNN in that space; rp3: RP3beta over the training graph under --baseline_alpha / --baseline_beta; ials: the iALS
        # factor model, no vote; ease: the closed-form EASE^R item-item model under --baseline_l2, no vote) the test users' top-K
        # lists, voted for by the --baseline_neighbours (default 50) nearest items of every train item: the evaluator's metrics,
        # how full and how popular the lists are, how much of the model's own list they hold and their catalogue exposure, overall
        # and per user group (reports.BaselineReport)
        k_base = config["baseline_report"] if "baseline_report" in config else 0
        if isinstance(k_base, bool) or not isinstance(k_base, int) or k_base < 0:
            raise ValueError("baseline_report must be 0 (off) or the K of the baseline lists, got %r" % (k_base,))
        sources = baseline_sources(config["baseline_sources"]) if "baseline_sources" in config else ("co",)
        n_near = config["baseline_neighbours"] if "baseline_neighbours" in config else 50
        if isinstance(n_near, bool) or not isinstance(n_near, int) or not 1 <= n_near <= ops.VOTE_MAX_K:
            raise ValueError("baseline_neighbours must be an integer in [1, %d], got %r" % (ops.VOTE_MAX_K, n_near))
        base_measure = str(config["baseline_measure"]) if "baseline_measure" in config else "cosine"
        if base_measure not in ops.COOCCUR_MEASURES:
            raise ValueError("baseline_measure is one of %s, got %r" % (", ".join(sorted(ops.COOCCUR_MEASURES)), base_measure))
        # --baseline_alpha=1.0 / --baseline_beta=0.6 (CLI-only): RP3beta's exponents for the source rp3 -- the transition
        # probabilities' power and the popularity penalty on the target item; finite numbers in [0, 4], the commonly used defaults
        base_alpha, base_beta = ops._rp3_params("baseline_alpha / baseline_beta", config["baseline_alpha"] if "baseline_alpha" in config else 1.0,
                                                config["baseline_beta"] if "baseline_beta" in config else 0.6)
        # --baseline_factors=64 / --baseline_iters=15 / --baseline_conf=1.0 / --baseline_reg=0.01 / --baseline_reg_scale=0.0 (CLI-only):
        # the source ials -- implicit-feedback ALS over the training graph (EliMRec.fit_ials): factors in {16, 32, 48, 64}, 1 <= iters
        # <= 100, conf >= 0, reg > 0, 0 <= reg_scale <= 1 (0: the constant ridge; > 0: scaled by (degree + 1) ** reg_scale); not tuned
        ials = ops._ials_params("baseline_factors / _iters / _conf / _reg / _reg_scale",
                                *[config["baseline_" + k] if ("baseline_" + k) in config else v for k, v in (
                                    ("factors", 64), ("iters", 15), ("conf", 1.0), ("reg", 0.01), ("reg_scale", 0.0))])
        # --baseline_l2=500.0 (CLI-only): the source ease -- EASE^R over the training graph (EliMRec.fit_ease), its one
        # hyper-parameter, finite and > 0; 500 is the commonly quoted value, not tuned
        base_l2 = ops._ease_params("baseline_l2", config["baseline_l2"] if "baseline_l2" in config else 500.0)
        self.baseline_reporter = None
        if k_base:
            for x in sources:        # (the model checks a head letter against its own heads at the first list)
                if x not in ("co", "rp3", "ials", "ease", "fused", "v", "a", "t"):
                    raise ValueError("baseline_sources names 'co', 'rp3', 'ials', 'ease', 'fused' or a head letter (v, a, t), got %r" % (x,))
            self.baseline_reporter = BaselineReport(dataset, train, dataset.get_user_test_dict(), config["topks"], metric=config["metric"],
                                                    sources=sources, neighbours=n_near, measure=base_measure,
                                                    group_view=config["group_view"], list_k=k_base, alpha=base_alpha, beta=base_beta,
                                                    factors=ials[0], iters=ials[1], conf=ials[2], reg=ials[3], reg_scale=ials[4], l2=base_l2)
        # --coldstart_report=K (CLI-only, default 0 = off): the cold test items (no training interaction, a test interaction) as
        # trained, folded in from their content and folded in with the mean id row -- pair means of rank, pct, rr and hit@K for the
        # topks and K, overall and per user group (reports.ColdStartReport)
        k_cold = int(config["coldstart_report"]) if "coldstart_report" in config else 0
        if k_cold < 0:
            raise ValueError("coldstart_report must be 0 (off) or a K for hit@K")
        self.coldstart_reporter = None
        if k_cold:
            ks = [int(k) for k in config["topks"]]
            self.coldstart_reporter = ColdStartReport(dataset, train, dataset.get_user_test_dict(), ks + [k_cold] * (k_cold not in ks),
                                                      group_view=config["group_view"])
        # --newuser_report=K (CLI-only, default 0 = off): the test users with a training history as trained, folded in from their
        # training items and folded in with the mean id row -- the evaluator's metrics at the topks and K, the share of the trained
        # top-K list each variant keeps and the cosine to the trained row, overall and per user group (reports.NewUserReport)
        k_new = config["newuser_report"] if "newuser_report" in config else 0
        if isinstance(k_new, bool) or not isinstance(k_new, int) or not 0 <= k_new <= 256:
            raise ValueError("newuser_report must be 0 (off) or the K of the lists, 1 <= K <= 256, got %r" % (k_new,))
        self.newuser_reporter = None
        if k_new:
            ks = [int(k) for k in config["topks"]]
            self.newuser_reporter = NewUserReport(dataset, train, dataset.get_user_test_dict(), ks + [k_new] * (k_new not in ks),
                                                  group_view=config["group_view"], metric=config["metric"], k=k_new)
            self.newuser_reporter.tie_order = self.test_evaluator.evaluator.tie_order
        self.infonce_criterion = nn.CrossEntropyLoss()          # BasicModel.py:32

    def getFileName(self):
        """`{path}/{recommender}-{dataset}-{loss}-{suffix}.pth.tar` (BasicModel.py:34-40)."""
        cfg = self.config
        os.makedirs(cfg["path"], exist_ok=True)          # (several ranks of one job arrive here together)
        name = "%s-%s-%s-%s.pth.tar" % (cfg["recommender"], cfg["data.input.dataset"], cfg["loss"], cfg["suffix"])
        return os.path.join(cfg["path"], name)

    def predict(self, user_ids, candidate_items=None):
        raise NotImplementedError

    def compute(self):
        raise NotImplementedError

    def getEmbedding(self, users, pos_items, neg_items):
        raise NotImplementedError

    def evaluate(self):
        return self.valid_evaluator.evaluate(self)

    def test(self):
        return self.test_evaluator.evaluate(self)

    # (overall final, overall buf, group final, group buf) from one pass; the overall pair is what evaluate() / test() return
    # without group_view, the group pair is (None, None) then
    def evaluate_with_overall(self):
        return self.valid_evaluator.evaluate_with_overall(self)

    def test_with_overall(self):
        return self.test_evaluator.evaluate_with_overall(self)

    def effect_report(self):
        """(final, buf) of reports.EffectReport over the test users under the current predict type; None when --effect_report is off."""
        return self.effect_reporter.evaluate(self) if self.effect_reporter is not None else None

    # ---- generic losses on top of getEmbedding (BasicModel.py:59-113). EliMRec overrides bpr_loss; these are the
    # reference's base-class versions, differentiable through EliMRec.compute()'s autograd bridge.
    def bpr_loss(self, users, pos, neg):
        """BasicModel.py:59-79: softplus(neg - pos) on un-normalised embedding rows."""
        users_emb, pos_emb, neg_emb, _, _, _ = self.getEmbedding(users.long(), pos.long(), neg.long())
        pos_scores = torch.sum(torch.mul(users_emb, pos_emb), dim=1)
        neg_scores = torch.sum(torch.mul(users_emb, neg_emb), dim=1)
        return torch.mean(F.softplus(neg_scores - pos_scores))

    def infonce(self, users, pos, neg=None):
        """BasicModel.py:81-95 (in-batch negatives; `neg` accepted and ignored so the driver's three-argument call works)."""
        users_emb, pos_emb, _, _, _, _ = self.getEmbedding(users.long(), pos.long(), None)
        users_emb = F.normalize(users_emb, dim=1)
        pos_emb = F.normalize(pos_emb, dim=1)
        logits = torch.mm(users_emb, pos_emb.T) / self.temp
        labels = torch.arange(users.shape[0], device=logits.device)
        return self.infonce_criterion(logits, labels)

    def fast_loss(self, users, pos, neg=None):
        """BasicModel.py:97-113."""
        users_emb, pos_emb, _, _, _, _ = self.getEmbedding(users.long(), pos.long(), None)
        alpha = self.config["alpha"]
        users_emb = F.normalize(users_emb, dim=1)
        pos_emb = F.normalize(pos_emb, dim=1)
        all_users, all_items = self._last_tables          # the tables of THIS forward, with their autograd graph
        all_users = F.normalize(all_users, dim=1)
        all_items = F.normalize(all_items, dim=1)
        pos_scores = torch.sum(torch.mul(users_emb, pos_emb), dim=1)
        pos_loss = torch.sum((alpha - 1) * torch.pow(pos_scores, 2) - 2 * alpha * pos_scores)
        all_loss = torch.trace(torch.matmul(torch.matmul(all_users.T, all_users), torch.matmul(all_items.T, all_items)))
        return pos_loss + all_loss
