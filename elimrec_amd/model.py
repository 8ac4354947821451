"""EliMRec on MI355X: the reference's plugin class (models/EliMRec.py:31-407) with the same
constructor, parameter names, state_dict keys and methods, whose per-batch work runs entirely
in libelimrec_hip.so.

Data layout in HBM (fp32, row-major; N = U + I nodes, users first):
  X0/Out [N x C], C = M*d   every propagated table side by side: column block 0 = id table,
                            1.. = projected V/A/T features. One 1-KiB row (Tiktok shape) serves
                            all M LightGCN graphs, so the CSR structure is read once per hop.
  Y      [N x Cy], Cy=(1+S)d block 0 = fused embedding (all_users / all_items), block 1+h =
                            single-modal head h (pre_fusion_{user,item}_{v,a,t}). The BPR head
                            gathers one contiguous row per index; predict() reads only Y.
What the reference does with 12+12 torch.sparse.mm calls, 8 addmm and autograd per batch is here:
  default (bipartite adjacency, or --propagation=folded on one with a diagonal; layer_num >= 2): the constant feature tables
      folded into GEMM operands, only the d-column id table through the graph, everything after the graph at the batch's
      active rows -- the column-shard engine (shard.py: slab-major tables, wave-tile hops, fused head, Adam as the last
      adjoint hop's epilogue). bpr_loss -> backward -> optimizer.step completes a request the engine runs as ONE enqueue
      (plugin.py). The full cached tables predict() reads are materialised on first use (_ensure_tables).
  the unfolded forms (any adjacency: --propagation=full | bipartite, --head_rows=all, layer_num < 2), row-major, every row
      every step: assemble_x0 + 3 linear_fwd -> propagate -> 5 linear_fwd -> bpr_head, and back: segment plan/apply ->
      head_bwd_input / linear_bwd_w -> propagate (A^T) -> embed_grad / linear_bwd_w. Also what compute() and the generic
      BasicModel losses differentiate through, and bench.py's "reference-equivalent work" line.
Propagation is linear, so nothing of the forward pass is kept for backward except Out (or its active rows) and Y.
"""
import collections
import math
import os

import numpy as np
import scipy.sparse as sp
import torch
from torch import nn
from torch.nn import functional as F

from . import _lib, ops
from .basic_model import BasicModel
from .evaluator import CandidateScoringError
from .logger import Logger
from .plugin import EmbeddingParameter, LazyGradParameter, StepController


# EliMRec.explain's result: column names, item ids CPU int32 [B x W] (-1 = padding), values CPU fp32 [B x W x C]
Effects = collections.namedtuple("Effects", ("columns", "items", "values"))
Neighbours = collections.namedtuple("Neighbours", ("ids", "scores"))
Audience = collections.namedtuple("Audience", ("users", "scores"))
Clusters = collections.namedtuple("Clusters", ("assign", "cos", "centroids", "counts", "n_iter", "converged"))
Geometry = collections.namedtuple("Geometry", ("columns", "labels", "values"))


def classes_from_clusters(assign, n_clusters):
    """The `classes` argument of recommend_calibrated from a cluster assignment (Clusters.assign, n_clusters <= 15 when a row has no
    cluster, <= 16 otherwise): int32 [I] with the rows of no cluster (-1: a zero or non-finite norm) in a class of their own, the
    LAST one (n_clusters); without such a row the assignment itself."""
    a = np.asarray(assign.cpu() if isinstance(assign, torch.Tensor) else assign).astype(np.int32)
    return np.where(a < 0, np.int32(n_clusters), a).astype(np.int32)


class NewItems(object):
    """Items folded in from content (EliMRec.fold_in_items), on the device: rows [Q x Cy] -- the rows the cached item table would
    hold for them --, table [U + Q x Cy] = the cached user rows, then the new rows (a catalogue of Q items to the scorers), sqn its
    block norms [U + Q x 1 + S], and version = the model's table version the rows were computed against: a handle used after the
    cached tables changed raises. New item q carries id num_items + q wherever ids are merged with the catalogue's."""

    def __init__(self, rows, table, sqn, version, num_users):
        self.rows, self.table, self.sqn, self.version, self.num_users = rows, table, sqn, int(version), int(num_users)
        self.n_items = int(rows.shape[0])

    def __len__(self):
        return self.n_items


class NewUsers(object):
    """Users folded in from their histories (EliMRec.fold_in_users), on the device: rows [Q x Cy] -- the rows the cached user table
    would hold for them --, table [Q + I x Cy] = the new rows, then the cached item rows (Q users and the catalogue to the
    scorers: new user q is user q), sqn its block norms [Q + I x 1 + S], layer_mean [Q x C] the rows of the layer-mean table the
    projections read, hist_ptr int64 [Q + 1] / hist_items int32 the histories resident on the device (the scorer's mask), with
    their host copies hist_ptr_host / hist_flat, and version = the model's table version the rows were computed against: a handle
    used after the cached tables changed raises."""

    def __init__(self, rows, table, sqn, version, num_users, num_items, hist_ptr_host, hist_flat, hist_ptr, hist_items, layer_mean=None):
        self.rows, self.table, self.sqn, self.version = rows, table, sqn, int(version)
        self.num_users, self.num_items = int(num_users), int(num_items)
        self.hist_ptr_host, self.hist_flat, self.hist_ptr, self.hist_items, self.layer_mean = hist_ptr_host, hist_flat, hist_ptr, hist_items, layer_mean
        self.n_users = int(rows.shape[0])

    def __len__(self):
        return self.n_users


KNN_LIST_BLOCK = 4096                    # items per launch when neighbour_lists builds the lists of the whole catalogue
KnnLists = collections.namedtuple("KnnLists", ("ids", "scores", "votes"))
IalsFactors = collections.namedtuple("IalsFactors", ("users", "items", "params", "objective"))
EaseModel = collections.namedtuple("EaseModel", ("P", "l2", "pivot_min", "bytes"))
HistorySupport = collections.namedtuple("HistorySupport", ("items", "history", "scores", "count", "mean"))


def create_adj_mat(train_users, train_items, num_users, num_items, adj_type):
    """models/EliMRec.py:309-354. Returns a scipy CSR [N, N] in fp32 (values rounded as scipy does)."""
    u = np.asarray(train_users, dtype=np.int32)
    i = np.asarray(train_items, dtype=np.int32)
    n = num_users + num_items
    half = sp.csr_matrix((np.ones_like(u, dtype=np.float32), (u, i + num_users)), shape=(n, n))
    adj = half + half.T

    def row_normalised(a):
        deg = np.asarray(a.sum(1)).flatten()
        with np.errstate(divide="ignore"):
            inv = np.power(deg, -1.0)
        inv[np.isinf(inv)] = 0.0
        return sp.diags(inv).dot(a)

    if adj_type == "plain":
        out = adj
    elif adj_type == "norm":
        out = row_normalised(adj + sp.eye(n))
    elif adj_type == "gcmc":
        out = row_normalised(adj)
    elif adj_type == "pre":
        deg = np.asarray(adj.sum(1))
        with np.errstate(divide="ignore"):
            inv = np.power(deg, -0.5).flatten()
        inv[np.isinf(inv)] = 0.0
        dm = sp.diags(inv)
        out = dm.dot(adj).dot(dm)
    else:
        out = row_normalised(adj) + sp.eye(n)
    out = sp.csr_matrix(out).astype(np.float32)
    out.sort_indices()
    return out


class _BprLossFn(torch.autograd.Function):
    """Glue between torch's autograd/optimizer API (main.py:98-101) and the HIP path: forward enqueues the forward
    kernels and returns the 0-dim loss; backward enqueues the backward kernels and leaves every parameter's gradient in
    `.grad` (nothing for parameters the loss does not reach: the set the reference leaves without .grad -- with ONE
    stated exception, `word_embedding.weight` on the tiktok data set: the reference builds t_feat once from it and keeps
    that graph alive with retain_graph=True (main.py:99), so the dead parameter keeps receiving a gradient and an Adam /
    weight-decay update every step; here t_feat is a constant and word_embedding a checkpoint key that stays at its
    initial value -- losses and scores are unaffected, the saved tensor differs from a reference run's).
    The gradients live in one flat buffer laid out like the parameters; backward assigns its views to `.grad` itself
    instead of returning them to autograd, whose AccumulateGrad would copy each of the 18 tensors (the views are not
    "stealable") -- 18 clones per step, and an optimizer that no longer sees adjacent gradients. A `.grad` that already
    holds something else is accumulated into, as autograd would; a `.grad` that already IS the flat view is overwritten
    (two backward passes without zero_grad do not accumulate -- the reference's loop zeroes every step, main.py:98).
    The forward's state lives in the model's workspace, not in the autograd context: backward must follow ITS forward.
    Each forward takes a generation number; backward raises if another forward (or compute()) ran in between."""

    @staticmethod
    def forward(ctx, model, users, pos, neg, *params):
        ctx.model = model
        ctx.params = params
        ctx.names = model._param_names
        loss = model._forward_hip(users, pos, neg, need_grad=True)
        ctx.gen = model._fwd_gen
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        model = ctx.model
        if ctx.gen != model._fwd_gen:
            raise RuntimeError("backward of a stale loss: another forward ran on this model since (the forward's state "
                               "lives in the model's workspace; call backward before the next bpr_loss / compute)")
        # upstream gradient into a fixed buffer: the backward regions are recorded against stable addresses
        gscale = model._ws.setdefault("gscale", torch.ones(1, dtype=torch.float32, device=grad_out.device))
        gscale.copy_(grad_out.reshape(1))
        grads = model._backward_hip(gscale)
        for name, p in zip(ctx.names, ctx.params):
            g = grads.get(name)
            if g is None or not p.requires_grad:
                continue
            if p.grad is None:
                p.grad = g
            elif p.grad.data_ptr() != g.data_ptr():
                p.grad.add_(g)
        return (None,) * (4 + len(ctx.params))


class _TablesFn(torch.autograd.Function):
    """compute() (models/EliMRec.py:228-272) as a differentiable op for losses written against the tables themselves
    (BasicModel.bpr_loss / infonce / fast_loss on top of getEmbedding, models/BasicModel.py:59-113): forward runs the
    HIP table build and returns copies of all_users / all_items; backward takes DENSE table gradients, treats every node
    as an active row of the fused head block and runs the same HIP backward as the training step. Parameter gradients
    land in `.grad` (the flat gradient views) as with _BprLossFn."""

    @staticmethod
    def forward(ctx, model, *params):
        ctx.model, ctx.params, ctx.names = model, params, model._param_names
        ws = model._workspace(model._ws_key[1] if model._ws_key else 1, parity=model._ws_key[3] if model._ws_key else 0)
        model._slab_fwd = False
        model._fwd_gen = getattr(model, "_fwd_gen", 0) + 1
        ctx.gen = model._fwd_gen
        model._compute_tables(ws)
        U, d = model.num_users, model.latent_dim
        return ws["Y"][:U, :d].clone(), ws["Y"][U:, :d].clone()

    @staticmethod
    def backward(ctx, g_users, g_items):
        model = ctx.model
        if ctx.gen != model._fwd_gen:
            raise RuntimeError("backward of stale tables: another forward ran on this model since compute()")
        grads = model._backward_tables(g_users, g_items)
        for name, p in zip(ctx.names, ctx.params):
            g = grads.get(name)
            if g is None or not p.requires_grad:
                continue
            if p.grad is None:
                p.grad = g
            elif p.grad.data_ptr() != g.data_ptr():
                p.grad.add_(g)
        return (None,) * (1 + len(ctx.params))


class EliMRec(BasicModel):
    def __init__(self, config, dataset):
        super(EliMRec, self).__init__(dataset, config)
        self.__init_weight()

    # ------------------------------------------------------------------ construction
    def __init_weight(self):
        cfg = self.config
        self.num_users = self.dataset.num_users
        self.num_items = self.dataset.num_items
        self.latent_dim = cfg["recdim"]
        self.n_layers = cfg["layer_num"]
        self.temp = cfg["temp"]
        self.logits = cfg["logits"]
        opt = lambda key, default: cfg[key] if key in cfg else default
        self.predict_type = opt("predict_type", "TIE")
        Logger.info("predict type: " + self.predict_type)
        self.mm_fusion_mode = opt("mm_fusion_mode", "concat")
        Logger.info("mm fusion mode: " + self.mm_fusion_mode)
        self.is_u_s = opt("is_u_s", False)
        Logger.info("cf in single modal preference: " + str(self.is_u_s))
        self.fusion_mode = opt("s_fusion_mode", "rubi")
        Logger.info("score fusion mode: " + self.fusion_mode)
        Logger.info("alpha: " + str(cfg["alpha"]))          # KeyError if missing, as in the reference (:66)
        self.modified_ui_loss = opt("modified_ui_loss", True)
        Logger.info("modified_ui_loss: " + str(self.modified_ui_loss))
        self.modality = opt("modality", "vat")
        Logger.info("Modality Ablation: " + str(self.modality))
        # --lean_tables=1 (CLI-only; BASELINE.json configs[4]): nothing of size N lives on the device outside the
        # column-sharded engine -- the embedding PARAMETERS and the raw feature tables stay on the host (the engine uploads
        # its column slice / its item block), no device CSR copies of the graph, no [N x C] tables in the workspace. Training
        # and evaluation run through ColumnShardTrainer / the item-sharded evaluator only.
        self._lean = str(opt("lean_tables", "0")) in ("1", "True", "true")
        if self.latent_dim % 4 != 0:
            raise ValueError("recdim must be a multiple of 4 for the HIP kernels (got %d)" % self.latent_dim)
        if self.mm_fusion_mode not in ("concat", "mean"):
            raise ValueError("mm_fusion_mode must be 'concat' or 'mean'")
        self.dataset_name = cfg["data.input.dataset"]
        self.is_kwai = self.dataset_name == "kwai"
        # tables after the id table. The reference keys this on the data set name only (kwai -> V, else V,A,T:
        # EliMRec.py:148,234,254,261); `--feature_modalities=vt` (CLI-only, not in the reference) selects any
        # subset whose features the data set provides, e.g. BASELINE.json's Kwai-shape "V+T" configuration.
        self._mods = ["v"] if self.is_kwai else ["v", "a", "t"]
        if "feature_modalities" in cfg:
            self._mods = [m for m in "vat" if m in str(cfg["feature_modalities"])]
            if not self._mods or any(not hasattr(self.dataset, m + "_feat") for m in self._mods):
                raise ValueError("feature_modalities=%r needs the matching <m>_feat tensors on the data set"
                                 % cfg["feature_modalities"])
        self.M = 1 + len(self._mods)
        self.C = self.M * self.latent_dim
        self.S = len(self._mods)                                       # single-modal heads
        self.Cy = (1 + self.S) * self.latent_dim

        self._create_u_embeding_i()
        self._cache = None                     # (all_users, all_items, all_s_embs) views into Y
        self._tables_dirty = False

        tu, ti = self.dataset.get_train_interactions()
        if str(opt("adj_build", "host")) == "device":     # CLI-only: degree count, normalisation and sort on the GPU (adjacency.py)
            from .adjacency import build_adj_device
            rp, cl, vl = build_adj_device(tu, ti, self.num_users, self.num_items, cfg["adj_type"], torch.device("cuda", torch.cuda.current_device()))
            n_nodes = self.num_users + self.num_items
            adj = sp.csr_matrix((vl.cpu().numpy(), cl.cpu().numpy(), rp.cpu().numpy()), shape=(n_nodes, n_nodes))
        else:
            adj = create_adj_mat(tu, ti, self.num_users, self.num_items, cfg["adj_type"])
        self._adj_host = adj                      # the engine's plan is built from this (host) matrix ...
        self._plan_build = str(opt("plan_build", "host"))      # ... or, --plan_build=device (CLI-only), from the device CSR by csrc/plan.hip
        if self._plan_build not in ("host", "device"):
            raise ValueError("plan_build must be host or device")
        if not self._lean:
            self._register_csr("adj", adj)
        adj_t = adj.T.tocsr()
        adj_t.sort_indices()
        self._adj_symmetric = (abs(adj - adj_t)).nnz == 0
        if not self._adj_symmetric and not self._lean:
            self._register_csr("adjT", adj_t)
        # Bipartite fast path (csrc/spmm.hip): no user-user / item-item entries (true for 'pre', 'plain', 'gcmc')
        U = self.num_users
        mode = opt("propagation", "auto")        # CLI-only: auto | folded | bipartite | full
        if mode not in ("auto", "folded", "bipartite", "full"):
            raise ValueError("propagation must be auto, folded, bipartite or full")
        self._bipartite = (self.n_layers >= 1 and adj[:U, :U].nnz == 0 and adj[U:, U:].nnz == 0 and mode != "full")
        # "folded": the propagated FEATURE tables are linear in the projection weights with constant factors,
        # mean_k A^k [0 ; F_m W_m^T + 1 b_m^T] = (mean_k A^k [0 ; F_m]) W_m^T + (mean_k A^k [0 ; 1]) b_m^T,
        # so the constant matrices S_m = mean_k A^k [0 ; F_m] ([N x D_m]) and c = mean_k A^k [0 ; 1] are
        # propagated ONCE at start-up; per step only the id table and the shared user part go through the
        # graph (d columns instead of M*d) and the feature blocks of Out come from one GEMM each.
        self._folded = self._bipartite and mode in ("auto", "folded")
        # an adjacency WITH a diagonal (adj_type norm / mean + I) and --propagation=folded asked for explicitly: the folded
        # algebra holds for any A-hat, only the one-table parity trick does not -- the column-sharded engine then carries the
        # E_u-borne and the E_i-borne part side by side ("wide" tables, csrc/wide.hip, shard.py). The model's own training path
        # (bpr_loss through autograd) has no such form: train with ColumnShardTrainer (main.py does), evaluate as ever.
        no_cross = adj[:U, :U].nnz == 0 and adj[U:, U:].nnz == 0
        self._wide = (not no_cross) and mode == "folded" and self.n_layers >= 2
        if self._wide:
            self._folded = True
        # "batch" head rows (CLI-only: --head_rows=batch|all): the projections AFTER the graph (feature blocks of
        # Out, embedding_*_after_GCN, s_dense_*) are row-wise, and the loss reads them at the batch's 3B rows only,
        # so a training step evaluates them there; the full cached tables predict() reads (:98-99) are filled in on
        # first use from the graph tables of that same forward and a copy of the (pre-update) projection weights.
        self._lazy = self._folded and self.n_layers >= 2 and str(opt("head_rows", "batch")) != "all"
        if self._lean and not self._lazy:
            raise ValueError("--lean_tables=1 needs the folded propagation with batch head rows (bipartite adjacency, layer_num >= 2)")
        if self._bipartite and not self._lean:
            P, Q = adj[:U, U:].tocsr(), adj[U:, :U].tocsr()
            self._register_csr("bipP", P)
            self._register_csr("bipQ", Q)
            if not self._adj_symmetric:
                self._register_csr("bipPT", P.T.tocsr())
                self._register_csr("bipQT", Q.T.tocsr())

        # same construction order as the reference (:88-93) so a seeded run draws the same init
        d = self.latent_dim
        self.s_dense_v = nn.Linear(d, d)
        self.s_dense_a = nn.Linear(d, d)
        self.s_dense_t = nn.Linear(d, d)
        nn.init.xavier_uniform_(self.s_dense_v.weight)
        nn.init.xavier_uniform_(self.s_dense_a.weight)
        nn.init.xavier_uniform_(self.s_dense_t.weight)
        # the same tensors as parameter classes that know about the deferred training step (plugin.py): `.grad` of every
        # parameter and the VALUE of the two embedding tables become real on first read
        self._plugin = StepController(self)
        for mod in self.modules():
            for pname, prm in list(mod._parameters.items()):
                if prm is not None:
                    cls = EmbeddingParameter if mod in (self.embedding_user, self.embedding_item) else LazyGradParameter
                    mod._parameters[pname] = cls(prm.data, prm.requires_grad)
        self._plugin.adopt(self.parameters())
        self._param_names = [n for n, _ in self.named_parameters()]
        # step regions: recorded C-ABI call lists (see _region)
        self._use_replay = os.environ.get("ELIMREC_REPLAY", "1") != "0"
        self._regions = {}
        self._ws = None
        self._ws_key = None

    def __setattr__(self, name, value):
        # per-step bookkeeping (plan sizes, cache markers, ...) skips nn.Module's parameter / buffer / submodule checks
        if name[0] == "_" and not isinstance(value, (torch.Tensor, torch.nn.Module)) and name not in self.__dict__.get("_buffers", ()):
            object.__setattr__(self, name, value)
        else:
            super().__setattr__(name, value)

    # cached tables of the last forward (models/EliMRec.py:121-122); materialised on first use in "batch" mode
    def _cached(self, k):
        self._plugin.realise_forward()         # a bpr_loss whose step has not run yet IS the last training forward
        if self._cache is None:
            return None
        self._ensure_tables()
        if self.__dict__.get("_eval_shard") is not None and k != 0:
            raise RuntimeError("the cached item tables are sharded over the ranks (--feature_shard=row): all_items / all_s_embs "
                               "exist per item block only; use predict() / evaluate(), which gather what they need")
        if self._cache is True:                 # published by a training step: the views are built on first use
            Y, U, d = self._cache_src, self.num_users, self.latent_dim
            s_embs = {}
            for h, m in enumerate(self._mods):
                blk = Y[:, (h + 1) * d:(h + 2) * d]
                s_embs["pre_fusion_user_" + m] = blk[:U]
                s_embs["pre_fusion_item_" + m] = blk[U:]
            self._cache = (Y[:U, :d], Y[U:, :d], s_embs)
        return self._cache[k]

    all_users = property(lambda self: self._cached(0))
    all_items = property(lambda self: self._cached(1))
    all_s_embs = property(lambda self: self._cached(2))

    def _register_csr(self, name, m):
        m = m.tocsr()
        m.sort_indices()
        if m.nnz >= 2 ** 31 or m.shape[0] >= 2 ** 31 - 1:
            raise ValueError("graph too large for int32 CSR")
        self.register_buffer(name + "_rowptr", torch.from_numpy(m.indptr.astype(np.int32)), persistent=False)
        self.register_buffer(name + "_col", torch.from_numpy(m.indices.astype(np.int32)), persistent=False)
        self.register_buffer(name + "_val", torch.from_numpy(m.data.astype(np.float32)), persistent=False)

    def _scipy_adj(self):
        """The propagation matrix as scipy CSR (the host matrix it was built as)."""
        if self.__dict__.get("_adj_host") is not None:
            return self._adj_host
        n = self.num_users + self.num_items
        return sp.csr_matrix((self.adj_val.cpu().numpy(), self.adj_col.cpu().numpy(), self.adj_rowptr.cpu().numpy()),
                             shape=(n, n))

    def _csr(self, name):
        """Device CSR + its row-split plan (built on first use on the current device)."""
        rowptr = getattr(self, name + "_rowptr")
        cache = self.__dict__.setdefault("_csr_cache", {})
        hit = cache.get(name)
        if hit is None or hit.rowptr.data_ptr() != rowptr.data_ptr():
            hit = ops.Csr(rowptr, getattr(self, name + "_col"), getattr(self, name + "_val"), rowptr.numel() - 1)
            if rowptr.is_cuda:
                hit.build_split(self.C)
            cache[name] = hit
        return hit

    def _create_u_embeding_i(self):
        """models/EliMRec.py:356-407, same RNG draw order."""
        d = self.latent_dim
        self.embedding_user = nn.Embedding(self.num_users, d)
        self.embedding_item = nn.Embedding(self.num_items, d)
        nn.init.xavier_uniform_(self.embedding_user.weight)
        nn.init.xavier_uniform_(self.embedding_item.weight)
        Logger.info("[use Xavier initilizer]")
        ds = self.dataset
        custom = "feature_modalities" in self.config
        if self._lean:
            # host tensors (not buffers: .to(device) leaves them where they are); the engine's distributed fold uploads the
            # rank's item block of each (shard.py)
            if self.dataset_name == "tiktok" and not custom:
                raise ValueError("--lean_tables=1 does not cover the tiktok word-bag text features")
            # --feature_load=block: not even that -- a reader that serves normalised row blocks (dataset.FeatureBlocks); the
            # distributed fold asks it for the rank's item block and for nothing else
            block = str(self.config["feature_load"]) == "block" if "feature_load" in self.config else False
            for m in self._mods:
                object.__setattr__(self, m + "_feat", ds.feature_blocks(m) if block else
                                   F.normalize(getattr(ds, m + "_feat").float(), dim=1).contiguous())
        elif "feature_load" in self.config and str(self.config["feature_load"]) == "block":
            raise ValueError("--feature_load=block needs --lean_tables=1 (and --feature_shard=row): the other forms keep whole feature tables")
        elif "v" in self._mods:
            self.register_buffer("v_feat", F.normalize(ds.v_feat.float(), dim=1).contiguous(), persistent=False)
        if self._lean:
            pass
        elif custom:
            for m in self._mods:
                if m != "v":
                    self.register_buffer(m + "_feat", F.normalize(getattr(ds, m + "_feat").float(), dim=1).contiguous(),
                                         persistent=False)
        elif not self.is_kwai:
            self.register_buffer("a_feat", F.normalize(ds.a_feat.float(), dim=1).contiguous(), persistent=False)
            if self.dataset_name == "tiktok":
                # :371-378: t_feat is the scatter-mean of word embeddings, built ONCE at init and
                # never recomputed -> a constant, un-normalised [I x 128] table.
                self.word_embedding = nn.Embedding(11574, 128)
                nn.init.xavier_normal_(self.word_embedding.weight)
                self.register_buffer("t_feat", self._word_bag_t_feat(), persistent=False)
            else:
                self.register_buffer("t_feat", F.normalize(ds.t_feat.float(), dim=1).contiguous(), persistent=False)
        for m in self._mods:
            feat = getattr(self, m + "_feat")
            if feat.shape[0] != self.num_items:
                raise ValueError("%s_feat has %d rows, expected num_items=%d" % (m, feat.shape[0], self.num_items))
            if feat.shape[1] % 4 != 0:
                raise ValueError("feature width of '%s' must be a multiple of 4 (got %d)" % (m, feat.shape[1]))
        for m in self._mods:                      # v_dense, a_dense, t_dense in the reference's order (:384-389)
            setattr(self, m + "_dense", nn.Linear(getattr(self, m + "_feat").shape[1], d))
        self.item_feat_dim = d * self.M if self.mm_fusion_mode == "concat" else d
        for m in self._mods:                      # :397-400
            nn.init.xavier_uniform_(getattr(self, m + "_dense").weight)
        self.embedding_user_after_GCN = nn.Linear(self.item_feat_dim, d)
        nn.init.xavier_uniform_(self.embedding_user_after_GCN.weight)
        self.embedding_item_after_GCN = nn.Linear(self.item_feat_dim, d)
        nn.init.xavier_uniform_(self.embedding_item_after_GCN.weight)

    @torch.no_grad()
    def _word_bag_t_feat(self):
        """:371-378: scatter-mean of the word embeddings of every item's words -- [I x 128], not normalised."""
        words = self.dataset.words_tensor
        w = self.word_embedding.weight.detach()
        idx0, idx1 = words[0].to(w.device), words[1].to(w.device)
        rows = int(words[0].max()) + 1
        tot = torch.zeros(rows, 128, device=w.device).index_add_(0, idx0, w[idx1])
        cnt = torch.zeros(rows, device=w.device).index_add_(0, idx0, torch.ones(words.shape[1], device=w.device)).clamp_(min=1)
        return (tot / cnt[:, None]).contiguous()

    def load_state_dict(self, state_dict, strict=True, **kw):
        """nn.Module.load_state_dict + what depends on the loaded tensors without being a checkpoint key: on the tiktok
        data set t_feat is built from word_embedding (:371-378) and the folded constant S_t from t_feat, so both are
        rebuilt from the LOADED word_embedding -- a resume under another seed scores with the features its weights were
        trained with."""
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        self._plugin.params_changed()
        if self.dataset_name == "tiktok" and hasattr(self, "word_embedding") and "feature_modalities" not in self.config:
            self.t_feat.copy_(self._word_bag_t_feat().to(self.t_feat.device))
            if self._ws is not None and self._ws.get("fold") is not None:
                self._fold_constants(self._ws)
                self._regions = {}            # recorded launches hold the old constants' addresses
                eng = self.__dict__.get("_slab_engine")
                if eng is not None and getattr(eng, "_on_constants_changed", None):
                    eng._on_constants_changed()
        return out

    # ------------------------------------------------------------------ device workspace
    def _device(self):
        return self.embedding_user_after_GCN.weight.device

    def _apply(self, fn, *args, **kwargs):
        """Lean tables: .to(device) / .cuda() move everything EXCEPT the two embedding tables, which stay host parameters
        (state_dict keys as ever); the engine uploads the column slice its rank owns."""
        if not self.__dict__.get("_lean"):
            return super()._apply(fn, *args, **kwargs)
        keep = {k: self._modules[k] for k in ("embedding_user", "embedding_item")}
        order = list(self._modules.keys())
        for k in keep:
            del self._modules[k]
        try:
            return super()._apply(fn, *args, **kwargs)
        finally:
            mods = dict(self._modules)
            mods.update(keep)
            self._modules.clear()
            for k in order:
                self._modules[k] = mods[k]

    def _require_gpu(self):
        dev = self._device()
        if dev.type != "cuda":
            raise RuntimeError("EliMRec (elimrec_amd): the model is on '%s'. The hot path exists only as HIP kernels "
                               "for MI355X; move the model to a GPU (`.to('cuda:0')`). There is no CPU fallback." % dev)
        return dev

    def _workspace(self, B, bwd_rows=None, parity=0):
        """Device buffers for batch size B. bwd_rows = number of gradient rows the backward pass
        will be fed (3*B locally; 3*B*world_size when row gradients are all-gathered). parity: the column-shard engine keeps TWO
        sets of the batch-dependent buffers per batch size and alternates them step by step, so that the planner of step
        t + 1 never writes what a kernel of step t still reads (shard.py: cs_plan)."""
        dev = self._require_gpu()
        bwd_rows = 3 * int(B) if bwd_rows is None else int(bwd_rows)
        parity = int(parity)
        if (self._ws is not None and self._ws_key[:2] == (str(dev), int(B)) and self._ws_key[2] >= bwd_rows
                and self._ws_key[3] == parity):
            return self._ws
        # the batch-dependent buffers of every batch size seen so far are kept (an epoch ends with a ragged batch: B ->
        # tail -> B would otherwise reallocate twice per epoch and invalidate every recorded region)
        sets = self.__dict__.setdefault("_ws_sets", {})
        hit = sets.get((str(dev), int(B), parity))
        if hit is not None and self._ws is not None and self._ws_key[0] == str(dev) and hit[0] >= bwd_rows:
            self._ws.update(hit[2])
            self._ws_key, self._ws_gen = (str(dev), int(B), hit[0], parity), hit[1]
            return self._ws
        key = (str(dev), int(B), bwd_rows, parity)
        self._ws_new = getattr(self, "_ws_new", 0) + 1           # a set allocated (and zero-filled on the CURRENT stream) just now
        N, C, Cy, d = self.num_users + self.num_items, self.C, self.Cy, self.latent_dim
        f32 = dict(dtype=torch.float32, device=dev)
        ws = self._ws if (self._ws is not None and self._ws_key[0] == key[0]) else {}
        self._ws_gen_counter = getattr(self, "_ws_gen_counter", 0) + 1
        self._ws_gen = self._ws_gen_counter                  # recorded regions hold these buffers' addresses
        if "flat_param" not in ws and self._lean:
            # lean tables: the projection weights only (the embeddings are host parameters; the engine holds its column slice
            # of them, of their gradient and of their moments), no table of N rows at all
            self._flatten_parameters(ws)
            ws["fold"] = None
            ws["Y"] = None
        elif "flat_param" not in ws:                        # everything that does not depend on the batch size
            self._flatten_parameters(ws)
            names = ("Out",) if self._folded else (("X0", "Out") if self._bipartite else ("X0", "T0", "T1", "Out", "G"))
            for name in names:
                ws[name] = torch.empty(N, C, **f32)
            if self._wide:
                # the engine's wide form: its own fold (hop kernels), its own tables; here only the parameter views it loads from
                ws["fold"] = None
                ws["X0d"] = ws["flat_param"][:N * d].view(N, d)
                ws["gX0d"] = ws["flat_grad"][:N * d].view(N, d)
            if self._bipartite:
                if not self._folded:
                    ws["H"] = torch.empty(N, d, **f32)
                    ws["bip_ws"] = torch.empty(ops.bipartite_workspace(self.num_users, self.num_items, d, self.M),
                                               dtype=torch.uint8, device=dev)
                if self._folded:
                    ws["Narrow"] = torch.empty(N, d, **f32)        # the part of Out every table shares
                    ws["SrcA"] = torch.empty(N, d, **f32)          # adjoint source tables (active rows only)
                    ws["SrcB"] = torch.empty(N, d, **f32)
                    ws["fold_ws"] = torch.empty(ops.folded_workspace(N, d), dtype=torch.uint8, device=dev)
                    if self.__dict__.get("_skip_fold"):    # the column-sharded engine folds the constants itself, row-sharded
                        ws["fold"] = None
                    else:
                        self._fold_constants(ws)
                    # [E_u ; E_i] and its gradient as ONE [N x d] table: the two embeddings are the first two
                    # tensors of the flat parameter / gradient buffers, back to back
                    eu, ei = self.embedding_user.weight, self.embedding_item.weight
                    gv = ws["grad_views"]
                    adjacent = (ei.data_ptr() == eu.data_ptr() + eu.numel() * 4 and
                                gv["embedding_item.weight"].data_ptr() == gv["embedding_user.weight"].data_ptr() + eu.numel() * 4)
                    if not adjacent:
                        raise RuntimeError("folded propagation expects embedding_user/embedding_item adjacent in the flat buffers")
                    ws["X0d"] = ws["flat_param"][:N * d].view(N, d)
                    ws["gX0d"] = ws["flat_grad"][:N * d].view(N, d)
                else:
                    ws["gXI"] = torch.empty(self.num_items, C, **f32)
            ws["Y"] = torch.zeros(N, Cy, **f32)
            shapes = [(self.num_items, d, getattr(self, m + "_feat").shape[1]) for m in self._mods]
            ws["bwd_w_items"] = torch.empty(max(ops.linear_bwd_w_batched_workspace(shapes), 1), dtype=torch.uint8,
                                            device=dev)
        n3 = bwd_rows
        ws["loss_rows"] = torch.empty(B, **f32)
        ws["grad_rows"] = torch.empty(3 * B, Cy, **f32)
        ws["keys"] = torch.empty(3 * B, dtype=torch.int32, device=dev)          # node id of every local triplet slot
        ws["keys_scratch"] = torch.empty(3 * B, dtype=torch.int32, device=dev)
        ws["slot_seg"] = torch.empty(n3, dtype=torch.int32, device=dev)        # active-row index of every (global) slot
        if self._lazy:
            ws["OutAct"] = torch.empty(n3, C, **f32)               # Out / Y rows of the batch's active nodes
            ws["YAct"] = torch.empty(n3, Cy, **f32)
        ws["active_rows"] = torch.empty(n3, dtype=torch.int32, device=dev)
        ws["dY"] = torch.empty(n3, Cy, **f32)
        ws["seg_info"] = torch.zeros(8, dtype=torch.int32, device=dev)
        ws["plan_ws"] = torch.empty(max(ops.segment_plan_workspace(n3), 1), dtype=torch.uint8, device=dev)
        shapes = [(n3, d, C), (n3, d, C)] + [(n3, d, d)] * self.S
        if self._folded:    # the folded feature projections' weight gradients ride in the same launch
            ws["dOutR"] = torch.empty(n3, C, **f32)                # dLoss/dOut rows in slot order
            shapes += [(n3, d, getattr(self, m + "_feat").shape[1]) for m in self._mods]
        ws["bwd_w_rows"] = torch.empty(max(ops.linear_bwd_w_batched_workspace(shapes), 1), dtype=torch.uint8, device=dev)
        self._ws, self._ws_key = ws, key
        batch_keys_ = ("loss_rows", "grad_rows", "keys", "keys_scratch", "slot_seg", "OutAct", "YAct", "active_rows", "dY",
                       "seg_info", "plan_ws", "dOutR", "bwd_w_rows")
        self.__dict__.setdefault("_ws_sets", {})[(key[0], key[1], parity)] = (bwd_rows, self._ws_gen, {k: ws[k] for k in batch_keys_ if k in ws})
        return ws

    @torch.no_grad()
    def _fold_constants(self, ws):
        """S_m = mean_k A^k [0 ; F_m]  ([N x D_m]) and c = mean_k A^k [0 ; 1]  ([N]), computed once per device
        with the same propagation kernels (narrow part = 0, one table of width D_m)."""
        U, I, L, dev = self.num_users, self.num_items, self.n_layers, self._device()
        P, Q = self._csr("bipP"), self._csr("bipQ")
        fold = {}
        widths = [getattr(self, m + "_feat").shape[1] for m in self._mods] + [4]
        wmax = max(widths)
        for csr in (P, Q):
            csr.build_split(max(wmax, self.C))              # the row-split scratch must cover the widest table
        tmp_ws = torch.empty(ops.bipartite_workspace(U, I, wmax, 1), dtype=torch.uint8, device=dev)
        zeros_u = torch.zeros(U, wmax, dtype=torch.float32, device=dev)
        for m in self._mods:
            feat = getattr(self, m + "_feat")
            D = feat.shape[1]
            out = torch.empty(U + I, D, dtype=torch.float32, device=dev)
            ops.propagate_bipartite(P, Q, U, I, D, 1, L, zeros_u[:, :D].contiguous(), feat, out, tmp_ws)
            fold[m] = out
        ones = torch.ones(I, 4, dtype=torch.float32, device=dev)
        cpad = torch.empty(U + I, 4, dtype=torch.float32, device=dev)
        ops.propagate_bipartite(P, Q, U, I, 4, 1, L, zeros_u[:, :4].contiguous(), ones, cpad, tmp_ws)
        cpad[:, 1:] = 0.0                                   # column 0 = c; the rest pads the bias-gradient GEMM
        fold["c_pad"] = cpad
        fold["c"] = cpad[:, 0].contiguous()
        ws["fold"] = fold

    def _flatten_parameters(self, ws):
        """Re-point every parameter into ONE contiguous fp32 buffer (same Parameter objects, so an
        optimizer created earlier stays valid) and lay the gradients out the same way: the dense Adam
        update over all 18 tensors then becomes a single launch (optim.FusedAdam merges adjacent
        tensors)."""
        params = list(self.named_parameters())
        if self._lean:
            params = [(n_, p) for n_, p in params if not n_.startswith(("embedding_user.", "embedding_item."))]
        dev = self._device()
        sizes = [(p.numel() + 3) // 4 * 4 for _, p in params]          # keep every tensor 16-B aligned
        flat = torch.zeros(sum(sizes), dtype=torch.float32, device=dev)
        flat_grad = torch.zeros_like(flat)
        views, off = {}, 0
        with torch.no_grad():
            for (name, p), n in zip(params, sizes):
                dst = flat[off:off + p.numel()].view_as(p)
                dst.copy_(p.data)
                p.data = dst
                views[name] = flat_grad[off:off + p.numel()].view_as(p)
                off += n
        ws["flat_param"], ws["flat_grad"], ws["grad_views"] = flat, flat_grad, views
        offs, o = {}, 0
        for (name, p), n in zip(params, sizes):
            offs[name] = (o, p.numel())
            o += n
        ws["param_off"] = offs                   # name -> (offset in the flat buffers, numel)
        # every non-embedding parameter, live and as the copy a training forward takes (predict() after an
        # optimizer step must still see the weights its cached tables were computed with)
        tail = 0 if self._lean else sizes[0] + sizes[1]
        ws["tail_off"] = tail
        ws["snap"] = torch.zeros(flat.numel() - tail, dtype=torch.float32, device=dev)
        live, snap, off = {}, {}, 0
        for (name, p), n in zip(params, sizes):
            if off >= tail:
                live[name] = p.data
                snap[name] = ws["snap"][off - tail:off - tail + p.numel()].view_as(p)
            off += n
        ws["live_views"], ws["snap_views"] = live, snap

    def _fusion_weights(self, W=None):
        """[d x C] fusion weights as the kernels consume them. 'mean' fusion (mean over the M
        tables, then a [d x d] Linear; :224-225) is the same map as a [d x C] Linear whose M
        column blocks are all W/M."""
        if W is None:
            wu, wi = self.embedding_user_after_GCN.weight, self.embedding_item_after_GCN.weight
        else:
            wu, wi = W["embedding_user_after_GCN.weight"], W["embedding_item_after_GCN.weight"]
        if self.mm_fusion_mode == "concat":
            return wu, wi
        return (wu.detach() / self.M).repeat(1, self.M).contiguous(), (wi.detach() / self.M).repeat(1, self.M).contiguous()

    def _block_weights(self):
        """Per head block loss weights: fused head 1; single-modal heads alpha if the modality is
        active (:125-126,133-142)."""
        modality = "v" if self.is_kwai else self.modality
        key = (self.predict_type, modality)
        hit = self.__dict__.get("_bw_cache")
        if hit is not None and hit[0] == key:
            return list(hit[1])
        alpha = float(self.config["alpha"])
        w = [1.0]
        for m in self._mods:
            on = (self.predict_type != "normal") and (m in modality)
            w.append(alpha * modality.count(m) if on else 0.0)
        self._bw_cache = (key, tuple(w))
        return w

    # ------------------------------------------------------------------ forward / backward (HIP)
    def _fold_problems(self, ws, W, out, rows=None, rng=None):
        """Out_m = S_m W_m^T + c b_m^T + Narrow for every feature table m -- over all rows into `out`, or gathered
        at `rows` (int32 node ids; slots `rng` = device (begin, end)) into the compact `out`."""
        d, fold = self.latent_dim, ws["fold"]
        fr = self.__dict__.get("_fold_rows") if self.__dict__.get("_slab_fwd") else None
        if rows is not None and fr is not None:
            # the column-sharded engine looked the constants' rows up for this batch (row-sharded / 16-bit storage,
            # lookup.py): compact [R x D_m] rows in active-row order, c and the shared part compact too -- row r, not rows[r]
            n = out.shape[0]
            return [(fr["S"][m][:n], W[m + "_dense.weight"], W[m + "_dense.bias"], out[:, (k + 1) * d:(k + 2) * d], fr["c"][:n],
                     fr["narrow"][:n], None, rng) for k, m in enumerate(self._mods)]
        extra = () if rows is None else (rows, rng)
        return [(fold[m], W[m + "_dense.weight"], W[m + "_dense.bias"], out[:, (k + 1) * d:(k + 2) * d], fold["c"],
                 ws["Narrow"]) + extra for k, m in enumerate(self._mods)]

    @torch.no_grad()
    def _full_tables(self, ws, W):
        """Folded mode: everything after the graph, over all N rows, with the projection weights W."""
        ops.linear_fwd_batched(self._fold_problems(ws, W, ws["Out"]))
        self._head_forward(ws, W)

    @torch.no_grad()
    def _ensure_tables(self):
        """Batch-row mode: the full cached tables of the last training forward, built when somebody reads them."""
        if self._tables_dirty:
            self._tables_dirty = False
            self.__dict__["_slab_engine"].materialize_tables(self._ws)

    @torch.no_grad()
    def _compute_tables(self, ws):
        """compute() + gcn_cf() (:228-272,144-153): fills ws['Out'] and ws['Y'] over all rows."""
        U, I, d, M, C = self.num_users, self.num_items, self.latent_dim, self.M, self.C
        Out, Y = ws["Out"], ws["Y"]
        X0 = ws.get("X0")
        if self._folded:
            # id table + shared user part through the graph at d columns; feature blocks from the folded constants
            self._timed(lambda: ops.propagate_folded(self._csr("adj"), U, I, d, self.n_layers, ws["X0d"], Out[:, :d],
                                                     ws["Narrow"], ws["fold_ws"]))
            self._tables_dirty = False
            self._full_tables(ws, ws["live_views"])
            return
        if self._bipartite:
            ops.copy_cols(self.embedding_item.weight, X0[U:, :d])          # XI block 0 = item id table
        else:
            ops.assemble_x0(self.embedding_user.weight, self.embedding_item.weight, X0, M)
        ops.linear_fwd_batched([(getattr(self, m + "_feat"), getattr(self, m + "_dense").weight,
                                 getattr(self, m + "_dense").bias, X0[U:, (k + 1) * d:(k + 2) * d])
                                for k, m in enumerate(self._mods)])
        if self._bipartite:
            self._timed(lambda: ops.propagate_bipartite(self._csr("bipP"), self._csr("bipQ"), U, I, d, M, self.n_layers,
                                                        self.embedding_user.weight, X0[U:], Out, ws["bip_ws"]))
        else:
            self._propagate(self._csr("adj"), X0, ws["T0"], ws["T1"], Out)
        self._head_forward(ws)

    def _head_forward(self, ws, W=None):
        U, d = self.num_users, self.latent_dim
        Out, Y = ws["Out"], ws["Y"]
        W = ws["live_views"] if W is None else W
        wu, wi = self._fusion_weights(W)
        head = [(Out[:U], wu, W["embedding_user_after_GCN.bias"], Y[:U, :d]),
                (Out[U:], wi, W["embedding_item_after_GCN.bias"], Y[U:, :d])]
        for h, m in enumerate(self._mods):
            blk = slice((h + 1) * d, (h + 2) * d)
            head.append((Out[:, blk], W["s_dense_%s.weight" % m], W["s_dense_%s.bias" % m], Y[:, blk]))
        ops.linear_fwd_batched(head)
        self._table_W = W                         # the weights these tables were built with (fold_in_items reads the same ones)
        self._publish_cache(Y, dirty=self._tables_dirty)

    def _propagate(self, csr, X0, t0, t1, out):
        self._timed(lambda: ops.propagate(csr, X0, self.n_layers, t0, t1, out))

    def _timed(self, fn, hops=None):
        """Run `hops` (default L) full propagation hops; optionally bracketed by HIP events on the launch stream
        (bench.py)."""
        prof = getattr(self, "_kernel_events", None)
        if prof is None:
            fn()
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        prof.append((e0, e1, self.n_layers if hops is None else hops))

    def _publish_cache(self, Y, dirty=False):
        """The tables of this forward are the ones predict() / all_users / all_items / all_s_embs read (views into Y, built
        on first use: a training step only notes where they are)."""
        self._table_version = getattr(self, "_table_version", 0) + 1
        self._cache_src = Y
        self._cache = True
        self._tables_dirty = dirty
        if dirty:
            self._eval_shard = None          # an item-sharded scorer of an older forward (shard.py) is stale now

    # ------------------------------------------------------------------ recorded regions
    def _region(self, name, key, fn):
        """Run fn() -- a fixed sequence of launches on workspace buffers. The first run records the C-ABI calls it
        makes (function + converted arguments); later runs with the same `key` re-issue that list without the
        Python that built it: the step is some 25 launches of 5-50 us each, and issued one by one through the
        tensor-level wrappers the host side costs as much as the GPU side. `key` names everything the launches
        depend on besides buffer contents (sizes, pointers of caller-owned tensors, mode flags, the stream).
        (Capturing the regions as hipGraphs instead was measured in round 2 -- + 12 us per graph launch on this stack -- and
        removed in round 4; a whole step is one host call through csrc/program.hip, elimrec_amd/program.py.)"""
        if self.mm_fusion_mode != "concat" or not self._use_replay:   # 'mean' fusion mixes torch ops into the regions
            return fn()
        key = key + (ops._stream(),)
        name = "%s@%d" % (name, self._ws_gen)       # one entry per batch-size buffer set
        ent = self._regions.get(name)
        if ent is None or ent[0] != key:
            ent = self._regions[name] = [key, 0, None, None]
        if ent[2] is not None:
            _lib.replay(ent[2], name)
            return ent[3]
        calls = []
        _lib.record(calls)
        try:
            out = fn()
        finally:
            _lib.record(None)
        ent[2], ent[3] = calls, out
        return out

    def _fwd_head(self, ws, all_keys, n, B, rank, grad_rows):
        """Everything after the graph at the batch's active rows, generic shapes (the column-shard engine's head when its
        fused 16-row kernels do not cover the shape; the layer means are in ws['OutAct'][:, :d] / the compact shared part
        already): feature blocks, fused Linear and single-modal heads, loss rows and their gradient rows. One recorded region."""
        U, I, d, L = self.num_users, self.num_items, self.latent_dim, self.n_layers
        act, seg = ws["active_rows"][:n], ws["seg_info"]
        bw = self._last_block_weights

        def head():
            OutAct, YAct = ws["OutAct"][:n], ws["YAct"][:n]
            W = ws["live_views"]
            ops.linear_fwd_batched(self._fold_problems(ws, W, OutAct, act, seg[6:8]))
            wu, wi = self._fusion_weights(W)
            bu, bi = W["embedding_user_after_GCN.bias"], W["embedding_item_after_GCN.bias"]
            none3 = (None, None, None)
            problems = [(OutAct, wu, bu, YAct[:, :d]) + none3 + (seg[2:4],), (OutAct, wi, bi, YAct[:, :d]) + none3 + (seg[4:6],)]
            for h, m in enumerate(self._mods):
                blk = slice((h + 1) * d, (h + 2) * d)
                problems.append((OutAct[:, blk], W["s_dense_%s.weight" % m], W["s_dense_%s.bias" % m], YAct[:, blk]) + none3
                                + (seg[6:8],))
            ops.linear_fwd_batched(problems)
            ops.bpr_head_rows(YAct, ws["slot_seg"][3 * B * rank:3 * B * (rank + 1)], d, bw, ws["loss_rows"], grad_rows)

        self._region("fwd_head", (self._ws_gen, all_keys.data_ptr(), n, B, rank, tuple(bw), grad_rows is not None), head)
        self._publish_cache(ws["Y"], dirty=True)

    def _index_tensors(self, *ts):
        """int64, contiguous, on the model's device (no-ops for tensors that already are)."""
        dev = self._device()
        return tuple(t if (t.dtype == torch.int64 and t.device == dev and t.is_contiguous())
                     else t.to(device=dev, dtype=torch.int64).contiguous() for t in ts)

    @torch.no_grad()
    def batch_keys(self, users, pos, neg):
        """int32 [3B] node ids of the triplet slots (3b: user, 3b+1: U + pos, 3b+2: U + neg) -- the rows the loss
        reads (getEmbedding's gathers, :274-289) and the keys of the head-gradient rows."""
        B = int(users.numel())
        ws = self._workspace(B, getattr(self, "_bwd_rows_hint", None))
        users, pos, neg = self._index_tensors(users, pos, neg)
        return ops.triplet_rows(users, pos, neg, self.num_users, ws["keys"][:3 * B], I=self.num_items, err=self._index_err())

    def _index_err(self):
        e = self.__dict__.get("_index_err_word")
        if e is None or e.device != self._device():
            e = self.__dict__["_index_err_word"] = torch.zeros(1, dtype=torch.int32, device=self._device())
        return e

    def check_indices(self):
        """Raise IndexError if any batch since the last call held a user / item id outside the tables (the reference
        fails at the gather, models/EliMRec.py:277-281; here the kernels flag it, keep running in bounds, and the host
        looks at the flag when it synchronises anyway -- once per epoch in main.py)."""
        e = self.__dict__.get("_index_err_word")
        if e is None:
            return
        bits = int(e.item())
        if bits:
            e.zero_()
            what = [n for b, n in enumerate(("user", "positive item", "negative item")) if bits >> b & 1]
            raise IndexError("EliMRec: %s index out of range in a training batch" % " / ".join(what))

    @torch.no_grad()
    def _forward_hip(self, users, pos, neg, need_grad, all_keys=None, rank=0):
        """Forward on this rank's triplets. all_keys: the node ids of every rank's slots in rank order (default:
        this rank's own). The segment plan of those keys (unique active nodes, slot -> active row) is made FIRST:
        it depends on the indices only, the forward evaluates the head at the active rows, and the backward
        reduces the gathered gradient rows with it."""
        B = int(users.numel())
        self._fwd_gen = getattr(self, "_fwd_gen", 0) + 1
        users, pos, neg = self._index_tensors(users, pos, neg)
        keys = self.batch_keys(users, pos, neg)
        ws = self._ws
        all_keys = keys if all_keys is None else all_keys
        n = int(all_keys.numel())
        if n > ws["slot_seg"].numel():
            raise RuntimeError("workspace holds %d gradient rows, the gathered batch has %d" % (ws["slot_seg"].numel(), n))
        self._plan_n = n
        self._last_block_weights = self._block_weights()
        grad_rows = ws["grad_rows"] if need_grad else None
        ops.segment_plan(all_keys, self.num_users, self.num_users + self.num_items, ws["active_rows"][:n], ws["seg_info"],
                         ws["slot_seg"][:n], ws["plan_ws"])
        self._compute_tables(ws)
        # the tables were built with the live weights, which the optimizer step that follows replaces: keep a copy of the projection
        # weights for fold_in_items, as the column-shard engine's update does (one device copy of the non-embedding parameters)
        if "snap" in ws:
            ws["snap"].copy_(ws["flat_param"][ws["tail_off"]:])
            self._table_W = ws["snap_views"]
        ops.bpr_head(ws["Y"], self.num_users, self.num_items, users, pos, neg, self.latent_dim,
                     self._last_block_weights, ws["loss_rows"], grad_rows, ws["keys_scratch"] if need_grad else None)
        loss = torch.empty((), dtype=torch.float32, device=self._device())
        ops.fixed_order_sum(ws["loss_rows"], loss)
        return loss

    @torch.no_grad()
    def _backward_batch_rows(self, ws, gscale, grad_rows, n, head_only=True, pack_bwd=None, merge=None,
                             defer_reduce=False, sources=None):
        """The head's backward at the batch's active rows (the column-shard engine's cs_backward_local): gradient rows ->
        active rows (the forward's plan) -> dOut rows, head and projection weight gradients from the compact Out / dY rows.
        Two recorded regions; the adjoint propagation is the engine's."""
        U, I, d, M, C, S = self.num_users, self.num_items, self.latent_dim, self.M, self.C, self.S
        dY, seg, act = ws["dY"][:n], ws["seg_info"], ws["active_rows"][:n]
        dOutR, OutAct, gv, fold = ws["dOutR"][:n], ws["OutAct"][:n], ws["grad_views"], ws["fold"]
        bw = self._last_block_weights
        heads_on = [h for h in range(S) if bw[1 + h] != 0.0]     # heads switched off carry an all-zero gradient block
        concat = self.mm_fusion_mode == "concat"
        f32 = dict(dtype=torch.float32, device=self._device())
        grads = {}

        def head_input():
            wu, wi = self._fusion_weights()
            head_ws = [getattr(self, "s_dense_" + m).weight for m in self._mods]
            ops.segment_apply_head_bwd(grad_rows, act, seg, dY, ws["plan_ws"], U, d, C, [h + 1 for h in range(S)], wu, wi,
                                       head_ws, dOutR, scale=gscale, pack_bwd=pack_bwd, sources=sources)

        def head_weights():
            # fusion Linears: dW = dY_f^T . Out[active rows], user slots / item slots separately
            problems, fused_tmp = [], {}
            for name, rng in (("embedding_user_after_GCN", seg[2:4]), ("embedding_item_after_GCN", seg[4:6])):
                gw = gv[name + ".weight"] if concat else torch.empty(d, C, **f32)
                fused_tmp[name] = gw
                problems.append(dict(A=dY[:, :d], B=OutAct, out=gw, rng=rng, colsum=gv[name + ".bias"]))
                grads[name + ".weight"], grads[name + ".bias"] = gv[name + ".weight"], gv[name + ".bias"]
            for h in heads_on:
                name, blk = "s_dense_" + self._mods[h], slice((h + 1) * d, (h + 2) * d)
                problems.append(dict(A=dY[:, blk], B=OutAct[:, blk], out=gv[name + ".weight"], rng=seg[6:8],
                                     colsum=gv[name + ".bias"]))
                grads[name + ".weight"], grads[name + ".bias"] = gv[name + ".weight"], gv[name + ".bias"]
            # feature projections: Out_m = S_m W_m^T + c b_m^T + (shared part)  =>  dW_m = dOut_m^T S_m over the
            # active rows only, db_m = dOut_m^T c
            fr = self.__dict__.get("_fold_rows") if self.__dict__.get("_slab_fwd") else None
            for k, m in enumerate(self._mods):
                if fr is not None:      # the constants' rows of this batch, compact (looked up by the engine): row r itself
                    problems.append(dict(A=dOutR[:, (k + 1) * d:(k + 2) * d], B=fr["S"][m][:n], out=gv[m + "_dense.weight"],
                                         rng=seg[6:8], colsum=gv[m + "_dense.bias"], colsum_weight=fr["c"]))
                else:
                    problems.append(dict(A=dOutR[:, (k + 1) * d:(k + 2) * d], B=fold[m], out=gv[m + "_dense.weight"],
                                         row_index=act, rng=seg[6:8], colsum=gv[m + "_dense.bias"], colsum_weight=fold["c"]))
                grads[m + "_dense.weight"], grads[m + "_dense.bias"] = gv[m + "_dense.weight"], gv[m + "_dense.bias"]
            handle = ops.linear_bwd_w_batched(problems, ws["bwd_w_rows"], merge=merge, defer_reduce=bool(defer_reduce) and concat,
                                              defer_all=defer_reduce == "all" and concat)
            if not concat:  # 'mean' fusion: fold the M replicated column blocks back into the [d x d] weight
                for name, gw in fused_tmp.items():
                    gv[name + ".weight"].copy_(gw.view(d, M, d).sum(1) / M)
            return dict(grads), handle

        key = (self._ws_gen, grad_rows.data_ptr(), gscale.data_ptr(), n, tuple(bw))
        self._region("bwd_head_in", key + (0 if pack_bwd is None else pack_bwd.data_ptr(),
                                           0 if sources is None else (sources[1] if sources[0] == "split" else sources[0].data).data_ptr()),
                     head_input)
        mkey = (str(defer_reduce),) + (() if merge is None else (merge["rows"].data_ptr(), merge["keys"].data_ptr(),
                                                                 merge["mask"].data_ptr()))
        grads, self._bwd_w_reduce = self._region("bwd_head_w", key + mkey, head_weights)
        return dict(grads)

    @torch.no_grad()
    def _backward_hip(self, gscale, grad_rows=None):
        """Returns {parameter name: gradient tensor}. gscale: device fp32[1] (d loss_total / d loss).
        grad_rows default to the rows the last local forward produced; a data-parallel driver passes the rows
        gathered from every rank (in the order of the keys the forward planned)."""
        ws = self._ws
        dev = self._device()
        U, I, d, M, C, S = self.num_users, self.num_items, self.latent_dim, self.M, self.C, self.S
        grad_rows = ws["grad_rows"] if grad_rows is None else grad_rows
        n_rows = grad_rows.shape[0]
        if n_rows != self._plan_n:
            raise RuntimeError("backward got %d gradient rows, the forward planned %d" % (n_rows, self._plan_n))
        dY, seg, act = ws["dY"][:n_rows], ws["seg_info"], ws["active_rows"][:n_rows]
        ops.segment_apply(grad_rows, seg, dY, ws["plan_ws"], scale=gscale)
        bw = self._last_block_weights
        heads_on = [h for h in range(S) if bw[1 + h] != 0.0]
        wu, wi = self._fusion_weights()
        G0 = ws.get("X0")
        if not self._bipartite:
            G0.zero_()      # the bipartite path masks inactive rows instead of reading zeros
        # heads switched off by the modality ablation carry an all-zero gradient block
        head_ws = [getattr(self, "s_dense_" + m).weight for m in self._mods]
        if self._folded:    # dLoss/dOut rows of the active nodes, in slot order
            dOutR = ws["dOutR"][:n_rows]
            ops.head_bwd_input(dY, act, seg, U, d, C, [h + 1 for h in range(S)], wu, wi, head_ws, 1.0, None, compact=dOutR)
        else:
            ops.head_bwd_input(dY, act, seg, U, d, C, [h + 1 for h in range(S)], wu, wi, head_ws, 1.0, G0)
        grads = {}
        f32 = dict(dtype=torch.float32, device=dev)
        out_rows, out_index = ws["Out"], act
        # fusion Linears: dW = dY_f^T . Out[active rows], user slots / item slots separately
        gv = ws["grad_views"]
        concat = self.mm_fusion_mode == "concat"
        problems, fused_tmp = [], {}
        for name, rng in (("embedding_user_after_GCN", seg[2:4]), ("embedding_item_after_GCN", seg[4:6])):
            gw = gv[name + ".weight"] if concat else torch.empty(d, C, **f32)
            fused_tmp[name] = gw
            problems.append(dict(A=dY[:, :d], B=out_rows, out=gw, row_index=out_index, rng=rng, colsum=gv[name + ".bias"]))
            grads[name + ".weight"], grads[name + ".bias"] = gv[name + ".weight"], gv[name + ".bias"]
        for h in heads_on:
            name = "s_dense_" + self._mods[h]
            problems.append(dict(A=dY[:, (h + 1) * d:(h + 2) * d], B=out_rows[:, (h + 1) * d:(h + 2) * d],
                                 out=gv[name + ".weight"], row_index=out_index, rng=seg[6:8], colsum=gv[name + ".bias"]))
            grads[name + ".weight"], grads[name + ".bias"] = gv[name + ".weight"], gv[name + ".bias"]
        if self._folded:
            # feature projections: Out_m = S_m W_m^T + c b_m^T + (shared part)  =>  dW_m = dOut_m^T S_m over the
            # active rows only, db_m = dOut_m^T c  (the dense I-row contraction of the unfolded path disappears)
            fold = ws["fold"]
            for k, m in enumerate(self._mods):
                problems.append(dict(A=dOutR[:, (k + 1) * d:(k + 2) * d], B=fold[m], out=gv[m + "_dense.weight"],
                                     row_index=act, rng=seg[6:8], colsum=gv[m + "_dense.bias"], colsum_weight=fold["c"]))
                grads[m + "_dense.weight"], grads[m + "_dense.bias"] = gv[m + "_dense.weight"], gv[m + "_dense.bias"]
        ops.linear_bwd_w_batched(problems, ws["bwd_w_rows"])
        if not concat:      # 'mean' fusion: fold the M replicated column blocks back into the [d x d] weight
            for name, gw in fused_tmp.items():
                gv[name + ".weight"].copy_(gw.view(d, M, d).sum(1) / M)
        # back through the propagation (A^T; A itself when symmetric), then the layer-0 pieces
        gu, gi = gv["embedding_user.weight"], gv["embedding_item.weight"]
        if self._folded:
            AT = self._csr("adj" if self._adj_symmetric else "adjT")
            self._timed(lambda: ops.propagate_folded_bwd(AT, U, I, d, M, self.n_layers, dOutR, act, seg, ws["SrcA"],
                                                         ws["SrcB"], ws["gX0d"], ws["fold_ws"]))
            grads["embedding_user.weight"], grads["embedding_item.weight"] = gu, gi
            return grads
        if self._bipartite:
            ops.blocksum_rows(G0, act, seg, d, M, ws["H"])
            sym = self._adj_symmetric
            PT, QT = self._csr("bipQ" if sym else "bipPT"), self._csr("bipP" if sym else "bipQT")
            gXI = ws["gXI"]
            self._timed(lambda: ops.propagate_bipartite_bwd(PT, QT, U, I, d, M, self.n_layers, G0, ws["H"], act, seg,
                                                            gXI, gu, ws["bip_ws"]))
            ops.copy_cols(gXI[:, :d], gi)
            g_items = gXI
        else:
            G = ws["G"]
            self._propagate(self._csr("adj" if self._adj_symmetric else "adjT"), G0, ws["T0"], ws["T1"], G)
            ops.embed_grad(G, U, I, d, M, gu, gi)
            g_items = G[U:]
        grads["embedding_user.weight"], grads["embedding_item.weight"] = gu, gi
        problems = []
        for k, m in enumerate(self._mods):
            problems.append(dict(A=g_items[:, (k + 1) * d:(k + 2) * d], B=getattr(self, m + "_feat"),
                                 out=gv[m + "_dense.weight"], colsum=gv[m + "_dense.bias"]))
            grads[m + "_dense.weight"], grads[m + "_dense.bias"] = gv[m + "_dense.weight"], gv[m + "_dense.bias"]
        ops.linear_bwd_w_batched(problems, ws["bwd_w_items"])
        return grads

    # ------------------------------------------------------------------ engine API (elimrec_amd/dist.py)
    def forward_local(self, users, pos, neg, all_keys=None, rank=0, world_size=1):
        """Forward on this rank's triplets; all_keys = batch_keys() of every rank, concatenated in rank order.
        Returns (loss, grad_rows [3B x Cy]): d(local mean loss)/dY rows of this rank's slots."""
        B = int(users.numel())
        if self._lazy:
            raise RuntimeError("forward_local / backward_global (elimrec_amd.dist.DataParallelTrainer) drive the unfolded row-major "
                               "forms only (--propagation=full|bipartite, --head_rows=all, layer_num < 2); this model trains on the "
                               "column-shard engine: model.bpr_loss -> backward -> FusedAdam.step, or ColumnShardTrainer.step")
        self._bwd_rows_hint = 3 * B * world_size
        self._workspace(B, 3 * B * world_size)
        loss = self._forward_hip(users, pos, neg, need_grad=True, all_keys=all_keys, rank=rank)
        return loss, self._ws["grad_rows"]

    def backward_global(self, grad_rows, scale):
        """Backward from the gradient rows of every rank (rank order); `scale` is a device fp32[1]."""
        return self._backward_hip(scale, grad_rows=grad_rows)

    # ------------------------------------------------------------------ reference API
    def bpr_loss(self, users, pos_items, neg_items):
        """models/EliMRec.py:115-142. int64 index tensors of shape [b] -> 0-dim loss supporting
        .backward(retain_graph=True) and .cpu().item() (main.py:98-102)."""
        self._require_gpu()
        if self.is_kwai:
            self.modality = "v"                        # :133-134
        if self._lazy:
            # the column-shard engine's step, run when the caller's optimizer steps (plugin.py): loss.backward() and
            # FusedAdam.step() complete the request; whatever is read in between is made real first
            return self._plugin.begin(users, pos_items, neg_items)
        return _BprLossFn.apply(self, users, pos_items, neg_items, *self._all_params())

    @property
    def plugin(self):
        """The controller behind bpr_loss -> backward -> optimizer.step (plugin.py): `.engine`, `.trainer` once a step ran."""
        return self._plugin

    def state_dict(self, *args, **kwargs):
        """nn.Module.state_dict with the embedding tables written back from the engine's master copy first."""
        self._plugin.sync_params()
        return super().state_dict(*args, **kwargs)

    def _all_params(self):
        params = self.__dict__.get("_param_list")
        if params is None:      # the Parameter objects are fixed after construction (they are re-pointed, never replaced)
            params = self.__dict__["_param_list"] = [p for _, p in self.named_parameters()]
        return params

    def _no_lean(self, what):
        if self.__dict__.get("_wide"):
            raise RuntimeError("--propagation=folded on an adjacency with a diagonal: %s is not available (the folded form of such "
                               "an adjacency exists on the column-sharded engine only); train with ColumnShardTrainer" % what)
        if self.__dict__.get("_lean"):
            raise RuntimeError("--lean_tables=1: %s is not available (no table of N rows lives outside the column-sharded "
                               "engine); train with ColumnShardTrainer, evaluate with evaluate() / predict()" % what)

    def compute(self):
        """:228-272. Returns (all_users [U x d], all_items [I x d]). Under torch.no_grad(): views into Y. With autograd
        enabled: differentiable copies (_TablesFn) -- what getEmbedding / the generic BasicModel losses build on."""
        self._require_gpu()
        self._no_lean("compute()")
        self._plugin.settle()
        self._plugin.sync_params()               # the table build below reads the parameters themselves
        if torch.is_grad_enabled():
            self._last_tables = _TablesFn.apply(self, *self._all_params())
            return self._last_tables
        self._slab_fwd = False
        ws = self._workspace(self._ws_key[1] if self._ws_key else 1, parity=self._ws_key[3] if self._ws_key else 0)
        self._compute_tables(ws)
        self._last_tables = (self.all_users, self.all_items)
        return self._last_tables

    @torch.no_grad()
    def _backward_tables(self, g_users, g_items):
        """HIP backward from dense gradients of all_users / all_items: every node is an active row whose head-gradient
        row holds its table gradient in the fused block and zeros in the single-modal blocks."""
        U, I, d, Cy = self.num_users, self.num_items, self.latent_dim, self.Cy
        N = U + I
        dev = self._device()
        ws = self._workspace(self._ws_key[1] if self._ws_key else 1, N, parity=self._ws_key[3] if self._ws_key else 0)
        rows = torch.zeros(N, Cy, dtype=torch.float32, device=dev)
        if g_users is not None:
            rows[:U, :d] = g_users
        if g_items is not None:
            rows[U:, :d] = g_items
        keys = torch.arange(N, dtype=torch.int32, device=dev)
        ops.segment_plan(keys, U, N, ws["active_rows"][:N], ws["seg_info"], ws["slot_seg"][:N], ws["plan_ws"])
        self._plan_n = N
        self._last_block_weights = [1.0] + [0.0] * self.S
        lazy, self._lazy = self._lazy, False          # the tables were built over all rows: the full-row backward
        try:
            return self._backward_hip(torch.ones(1, dtype=torch.float32, device=dev), grad_rows=rows)
        finally:
            self._lazy = lazy

    def gcn_cf(self, detach=False):
        """:144-153. The single-modal head tables computed by the last compute()."""
        return self.all_s_embs

    def getEmbedding(self, users, pos_items, neg_items):
        """:274-289: rows of the fused tables for users / positives / negatives + the raw ("ego") embedding rows. The
        table rows carry autograd (through compute()); the ego rows are returned detached -- no loss of the reference
        reads them (BasicModel.py:59-113 only unpacks them)."""
        all_users, all_items = self.compute()
        ego_u, ego_i = self.embedding_user.weight.detach(), self.embedding_item.weight.detach()
        neg = (all_items[neg_items], ego_i[neg_items]) if neg_items is not None else (None, None)
        return all_users[users], all_items[pos_items], neg[0], ego_u[users], ego_i[pos_items], neg[1]

    def forward(self, users, items):
        """:299-307."""
        all_users, all_items = self.compute()
        return torch.sum(all_users[users] * all_items[items], dim=1).detach()

    def _head_mask(self):
        modality = "v" if self.is_kwai else self.modality
        return sum(1 << h for h, m in enumerate(self._mods) if m in modality)

    def _cached_tables(self, what, sharded_msg=None):
        """The one way into the cached tables for everything that reads them: a GPU model, the pending step made real, tables
        cached by a training forward (`what`: the caller's words for the error) and materialised; sharded_msg: the refusal of
        item-sharded tables by a caller that needs them whole on this rank. -> the device."""
        dev = self._require_gpu()
        self._plugin.realise_forward()
        if self._ws is None or self._cache is None:
            raise RuntimeError("%s the tables cached by a training forward (call bpr_loss or compute first)" % what)
        self._ensure_tables()
        if sharded_msg is not None and self.__dict__.get("_eval_shard") is not None:
            raise CandidateScoringError(sharded_msg)
        return dev

    def _score_workspace(self, dev, B, top_k, topk_only):
        """The scorer's workspace for B users (grow-only, kept in the model's workspace)."""
        need = ops.score_workspace(B, self.num_users, self.num_items, self.S, top_k, topk_only=topk_only, d=self.latent_dim)
        if self._ws.get("score_ws") is None or self._ws["score_ws"].numel() < need:
            self._ws["score_ws"] = torch.empty(need, dtype=torch.uint8, device=dev)
        return self._ws["score_ws"]

    def _catalogue_row_sum(self, dev, users, predict_type, sqn):
        """The scorer's pass 1 only, the whole catalogue as the one shard: sum_i sigmoid(u . i) per user (one launch)."""
        I = self.num_items
        row_sum = torch.empty(users.numel(), dtype=torch.float32, device=dev)
        ops.score_topk_shard(self._ws["Y"], self.num_users, I, users, self.latent_dim, self.S, self._head_mask(), self.fusion_mode,
                             predict_type, self._score_workspace(dev, users.numel(), 1, True), 1, row_sum, I, 0, sqnorm=sqn)
        return row_sum

    def _side_rows(self, side):
        """(first row, number of rows) of the item rows (side "item") or the user rows ("user") in the cached Y."""
        if side not in ("item", "user"):
            raise ValueError("side must be 'item' or 'user', got %r" % (side,))
        return (self.num_users, self.num_items) if side == "item" else (0, self.num_users)

    @torch.no_grad()
    def predict_device(self, user_ids, scores=None, top_k=0, train_ptr=None, train_items=None, tie_order="id"):
        """Device-side predict (+ optional train-item masking and top-K). Uses the tables cached
        by the LAST training forward, like the reference (:98-99). tie_order: the lists' order among equal
        scores -- "id" (lowest item id first) or "reference" (evaluate.h:26-33's partial_sort_copy, replayed on the device)."""
        dev = self._cached_tables("predict() needs")
        users = torch.as_tensor(user_ids, device=dev).long().contiguous()
        B, I = users.numel(), self.num_items
        sh = self.__dict__.get("_eval_shard")
        if sh is not None:       # several ranks with row-sharded tables: this rank scores its block of the items (shard_eval.py)
            if scores is not None:
                scores.copy_(sh.scores(users, train_ptr, train_items))
            if top_k:
                if tie_order != "id":
                    raise ValueError("item-sharded tables rank by (score, id); the evaluator re-ranks tied rows in the reference's order")
                return sh.topk(users, top_k, train_ptr, train_items)
            return None, None
        # top-K only (the evaluator): no [B x I] score block in the workspace, the catalogue is scored in chunks
        score_ws = self._score_workspace(dev, B, max(top_k, 1), scores is None and top_k > 0)
        idx = val = None
        if top_k:
            idx = torch.empty(B, top_k, dtype=torch.int32, device=dev)
            val = torch.empty(B, top_k, dtype=torch.float32, device=dev)
        self._block_sqnorms(dev)
        ops.score_topk(self._ws["Y"], self.num_users, I, users, self.latent_dim, self.S, self._head_mask(),
                       self.fusion_mode, self.predict_type, score_ws, scores=scores, K=top_k,
                       topk_idx=idx, topk_val=val, train_ptr=train_ptr, train_items=train_items, sqnorm=self._ws["sqn"],
                       tie_order=tie_order)
        return idx, val

    def _block_sqnorms(self, dev):
        """Block norms of the cached tables: computed once per table version, reused by every user block."""
        if self._ws.get("sqn_version") != self._table_version:
            if self._ws.get("sqn") is None:
                self._ws["sqn"] = torch.empty(self.num_users + self.num_items, 1 + self.S, dtype=torch.float32, device=dev)
            ops.row_sqnorms(self._ws["Y"], self.latent_dim, 1 + self.S, self._ws["sqn"])
            self._ws["sqn_version"] = self._table_version
        return self._ws["sqn"]

    @torch.no_grad()
    def predict_candidates_device(self, user_ids, cand_ptr, cand_items, out):
        """Device form of predict_candidates: the lists as CSR (cand_ptr int64 [B + 1], cand_items int32, device tensors) ->
        out [B x width] (float32, rows contiguous) = each user's candidate scores in list order, then -inf (csrc/eval.hip
        score_cand_kernel). Score of candidate (u, i) = predict([u])[0, i]; TIE's catalogue mean comes from the scorer's pass 1
        over the whole catalogue (one launch per call)."""
        dev = self._cached_tables("predict_candidates() needs", "candidate scoring needs the whole cached item table on this rank; the "
                                  "tables are item-sharded (lean / multi-rank evaluation): score the full catalogue instead")
        users = torch.as_tensor(user_ids, device=dev).long().contiguous()
        I = self.num_items
        sqn = self._block_sqnorms(dev)
        row_sum = None
        if ops.PREDICT_TYPES.get(self.predict_type, 0) == 2 and users.numel():
            row_sum = self._catalogue_row_sum(dev, users, self.predict_type, sqn)
        ops.score_candidates(self._ws["Y"], self.num_users, I, users, self.latent_dim, self.S, self._head_mask(), self.fusion_mode,
                             self.predict_type, cand_ptr, cand_items, out, sqnorm=sqn, row_sum=row_sum, I_total=I)
        return out

    def _id_lists(self, lists, what, bound=None):
        """One list of ids per row as CSR on the host, every id checked against [0, bound) (default: the catalogue):
        (ptr int64, flat int64, lens) -- ops.ragged with this front's IndexError."""
        bound = self.num_items if bound is None else bound
        return ops.ragged(lists, check=(bound, "%s ids must lie in [0, %d)" % (what, bound)), cast=int)

    def _excluded(self, exclude, ids, what, bound=None):
        """`exclude` (dict id -> ids to leave out, or None) for the rows `ids`, checked: (ptr int64, flat int64)."""
        return self._id_lists([(exclude or {}).get(int(i), []) for i in ids], "excluded " + what, bound)[:2]

    def predict_candidates(self, user_ids, candidate_items):
        """Scores of given candidate lists: CPU fp32 [len(user_ids) x longest list], row b = predict([u_b])[0, candidate_items[b]]
        in list order, padded with -inf (the layout cpp/uni_evaluator.py:136-137 ranks: util/tool.py pad_sequences, post)."""
        dev = self._require_gpu()
        if len(candidate_items) != len(user_ids):
            raise ValueError("one candidate list per user: %d lists for %d users" % (len(candidate_items), len(user_ids)))
        ptr, flat, lens = self._id_lists(candidate_items, "candidate item")
        out = torch.empty(len(user_ids), int(lens.max()) if lens.size else 0, dtype=torch.float32, device=dev)
        self.predict_candidates_device(user_ids, torch.from_numpy(ptr).to(dev), torch.from_numpy(flat.astype(np.int32)).to(dev), out)
        return out.cpu()

    @torch.no_grad()
    def effects_device(self, user_ids, cand_ptr, cand_items, out):
        """The effect breakdown of candidate lists (CSR as predict_candidates_device takes them) -> out [B x width x (6 + S)]
        (float32, contiguous): per listed pair the columns of ops.effect_columns(self._mods) -- ui, the user's catalogue mean of it,
        te, nde, the TE and TIE scores (the bits predict_candidates gives under either type) and every head's cosine; NaN beyond a
        list's length (csrc/eval.hip score_cand_kernel, FX form). The catalogue mean comes from the scorer's pass 1 over the whole
        catalogue whatever self.predict_type is (one launch per call)."""
        dev = self._cached_tables("explain() needs", "the effect breakdown needs the whole cached item table on this rank; the tables "
                                  "are item-sharded (lean / multi-rank evaluation)")
        users = torch.as_tensor(user_ids, device=dev).long().contiguous()
        if not users.numel():
            return out
        sqn = self._block_sqnorms(dev)
        row_sum = self._catalogue_row_sum(dev, users, "TIE", sqn)
        ops.score_effects(self._ws["Y"], self.num_users, self.num_items, users, self.latent_dim, self.S, self._head_mask(),
                          self.fusion_mode, cand_ptr, cand_items, out, sqn, row_sum, self.num_items)
        return out

    def explain(self, user_ids, candidate_items=None, top_k=None, exclude=None, tie_order="id"):
        """Why items rank where they do: Effects(columns, items int32 [B x W] (-1 padded), values fp32 [B x W x C]) on the CPU,
        columns = ops.effect_columns(self._mods). candidate_items: one list of item ids per user -- the breakdown of those pairs.
        top_k: the breakdown of each user's top-K list under the model's current predict type and fusion mode (predict_device),
        `exclude` = dict user -> item ids left out of the ranking (the train items, masked as the evaluator masks them)."""
        if (candidate_items is None) == (top_k is None):
            raise ValueError("explain() takes exactly one of candidate_items and top_k")
        n = len(user_ids)
        columns = ops.effect_columns(self._mods)
        if candidate_items is not None:
            if exclude is not None:
                raise ValueError("exclude applies to top_k lists; candidate_items are taken as given")
            if len(candidate_items) != n:
                raise ValueError("one candidate list per user: %d lists for %d users" % (len(candidate_items), n))
            ptr, flat, lens = self._id_lists(candidate_items, "candidate item")
            items = ops.ragged_padded(flat, lens)
            dev = self._require_gpu()
            cand_ptr, cand_items = torch.from_numpy(ptr).to(dev), torch.from_numpy(flat.astype(np.int32)).to(dev)
        else:
            top_k = int(top_k)
            if top_k < 1 or top_k > self.num_items:
                raise ValueError("top_k must lie in [1, %d]" % self.num_items)
            tptr, tflat = self._excluded(exclude, user_ids, "item")
            dev = self._require_gpu()
            if n:
                idx, _ = self.predict_device(user_ids, top_k=top_k, train_ptr=torch.from_numpy(tptr).to(dev),
                                             train_items=torch.from_numpy(tflat.astype(np.int32)).to(dev), tie_order=tie_order)
            else:
                idx = torch.empty(0, top_k, dtype=torch.int32, device=dev)
            items = idx.cpu().numpy()
            cand_ptr = torch.arange(n + 1, dtype=torch.int64, device=dev) * top_k
            cand_items = idx.reshape(-1)
        out = torch.empty(n, items.shape[1], len(columns), dtype=torch.float32, device=dev)
        self.effects_device(user_ids, cand_ptr, cand_items, out)
        return Effects(columns, torch.from_numpy(np.ascontiguousarray(items)), out.cpu())

    @torch.no_grad()
    def rank_items_device(self, user_ids, tgt_index, train_ptr=None, train_items=None, top_k=0):
        """Where given items stand in each user's FULL ranking under the current predict type and fusion mode: (rank int32 [P], idx,
        val). tgt_index: ops.TargetIndex over (len(user_ids), num_items) -- one list of item ids per user, checked on the host when
        it was built; rank[p] = the 0-based position of target p by (score descending, id ascending) among the whole catalogue
        with the train items (train_ptr / train_items, CSR on the device) masked, -1 for a target that is itself masked. One
        predict_device call into a [B x I] block -- scored and masked as the evaluator's lists are -- then ops.rank_targets over
        that block (csrc/rank.hip). top_k > 0: idx / val [B x top_k] are the top-K lists selected from the same block by the same
        call (tie order "id"), so rank < top_k exactly for the listed targets; None otherwise."""
        self._require_gpu()
        if not isinstance(tgt_index, ops.TargetIndex):
            raise TypeError("rank_items_device takes the targets as an ops.TargetIndex (checked on the host once)")
        dev = self._cached_tables("rank_items() needs", "exact ranks need the whole cached item table on this rank; the tables are "
                                  "item-sharded (lean / multi-rank evaluation)")
        users = torch.as_tensor(user_ids, device=dev).long().contiguous()
        B, I = users.numel(), self.num_items
        if tgt_index.n_rows != B or tgt_index.n_items != I:
            raise ValueError("the TargetIndex was built for %d users of %d items, the call has %d users of %d items"
                             % (tgt_index.n_rows, tgt_index.n_items, B, I))
        rank = torch.empty(tgt_index.n_targets, dtype=torch.int32, device=dev)
        if not B:
            return rank, None, None
        lds = (I + 3) // 4 * 4                    # rows 16-byte aligned: the count takes its 16-byte loads
        block = torch.empty(B, lds, dtype=torch.float32, device=dev)[:, :I]
        idx, val = self.predict_device(users, scores=block, top_k=int(top_k), train_ptr=train_ptr, train_items=train_items,
                                       tie_order="id")
        ops.rank_targets(block, tgt_index, None, rank)
        return rank, idx, val

    def rank_items(self, user_ids, items, exclude=None):
        """The exact catalogue rank of given items: CPU int32 [len(user_ids) x longest list], row b = the 0-based positions of
        items[b] (one list of item ids per user) in user b's full ranking under the current predict type, padded with -1.
        `exclude` = dict user -> item ids masked out of the ranking (the train items, as explain() takes it); an item that is
        itself excluded gets -1."""
        n = len(user_ids)
        if len(items) != n:
            raise ValueError("one item list per user: %d lists for %d users" % (len(items), n))
        ptr, flat, lens = self._id_lists(items, "item")
        tptr, tflat = self._excluded(exclude, user_ids, "item")
        dev = self._require_gpu()
        rank = np.zeros(0, dtype=np.int32)
        if flat.size:
            index = ops.TargetIndex(ptr, flat.astype(np.int32), n, self.num_items, dev)
            masked = (torch.from_numpy(tptr).to(dev), torch.from_numpy(tflat.astype(np.int32)).to(dev)) if tflat.size else (None, None)
            rank = self.rank_items_device(user_ids, index, *masked)[0].cpu().numpy()
        return torch.from_numpy(ops.ragged_padded(rank, lens))

    def _neighbour_space(self, space):
        """Head block of the cached Y a neighbour space names: 0 = the fused rows predict() scores with, 1 + h = head h."""
        if space == "fused":
            return 0
        if isinstance(space, str) and space in self._mods:
            return 1 + list(self._mods).index(space)
        raise ValueError("space must be 'fused' or one of this model's heads %s, got %r" % ("/".join(self._mods) or "(none)", space))

    @torch.no_grad()
    def neighbours_device(self, side, rows, k, space, out_idx, out_val, query=None):
        """The k rows closest by cosine to each given row, among the item rows (side "item") or the user rows ("user") of one block
        of the cached tables: space "fused" (block 0, the rows predict() scores with) or a head letter of self._mods. out_idx int32 /
        out_val float32 (optional) [B x k] on the device, (score descending, id ascending), -1 / -inf where fewer than k rows exist
        (csrc/knn.hip). rows: the query ids (host array or tensor, checked on the host; the row itself is always left out) -- or
        query = an ops.NeighbourQuery over the side's rows, checked once, which may carry per-query exclusion lists. Tables as
        predict_device: those of the last training forward."""
        self._require_gpu()
        lo, n = self._side_rows(side)
        h = self._neighbour_space(space)
        dev = self._cached_tables("similar_items() / similar_users() need", "neighbour lists need the whole cached tables on this rank; "
                                  "the tables are item-sharded (lean / multi-rank evaluation)")
        d = self.latent_dim
        sqn = self._block_sqnorms(dev)
        if query is None:
            query = ops.NeighbourQuery(rows, n, dev)
        elif not isinstance(query, ops.NeighbourQuery) or query.n_rows != n:
            raise ValueError("query must be an ops.NeighbourQuery over the %d %s rows" % (n, side))
        need = ops.cosine_topk_workspace(query.n_queries, n, k)
        if self._ws.get("knn_ws") is None or self._ws["knn_ws"].numel() < need:
            self._ws["knn_ws"] = torch.empty(need, dtype=torch.uint8, device=dev)
        ops.cosine_topk(self._ws["Y"][lo:lo + n, h * d:(h + 1) * d], sqn[lo:lo + n, h], query, k, out_idx, out_val, exclude_self=True,
                        workspace=self._ws["knn_ws"])
        return out_idx, out_val

    def _similar(self, side, ids, k, space, exclude):
        n_rows = self.num_items if side == "item" else self.num_users
        k = int(k)
        if not 1 <= k <= ops.KNN_MAX_K:
            raise ValueError("k must lie in [1, %d]" % ops.KNN_MAX_K)
        self._neighbour_space(space)
        ids = self._id_lists([ids], side, n_rows)[1]
        ptr, flat = self._excluded(exclude, ids, side, n_rows)
        dev = self._require_gpu()
        idx = torch.empty(ids.size, k, dtype=torch.int32, device=dev)
        val = torch.empty(ids.size, k, dtype=torch.float32, device=dev)
        query = ops.NeighbourQuery(ids, n_rows, dev, ptr if flat.size else None, flat if flat.size else None)
        self.neighbours_device(side, None, k, space, idx, val, query=query)
        return Neighbours(idx.cpu(), val.cpu())

    def similar_items(self, item_ids, k, space="fused", exclude=None):
        """The k items closest to each given item by cosine: Neighbours(ids CPU int32 [B x k] (-1 padded), scores CPU fp32 [B x k]
        (-inf padded)), by (score descending, id ascending). space: "fused" -- the rows predict() scores with -- or one of the
        model's single-modal heads (a letter of self._mods: does the fused neighbourhood copy the visual one?). The item itself is
        always left out; `exclude` = dict item -> item ids to leave out as well. 1 <= k <= 256."""
        return self._similar("item", item_ids, k, space, exclude)

    def similar_users(self, user_ids, k, space="fused", exclude=None):
        """similar_items over the user rows: the k users closest to each given user."""
        return self._similar("user", user_ids, k, space, exclude)

    def cooccur_index(self, side):
        """The training graph as the ops.CooccurIndex of one side ("item": item -> its training users and back; "user": the
        transpose), built from the data set's train dict at the first call, checked on the host and kept on the model's device."""
        self._side_rows(side)
        dev = self._require_gpu()
        kept = self.__dict__.setdefault("_co_index", {})
        hit = kept.get(side)
        if hit is None or hit.device != dev:
            hit = kept[side] = ops.CooccurIndex.from_train(self.dataset.get_user_train_dict(), self.num_users, self.num_items, side, dev)
        return hit

    @torch.no_grad()
    def co_neighbours_device(self, side, rows, k, measure, out_idx, out_val, out_cnt=None):
        """The k co-interaction neighbours of each given row of the TRAINING GRAPH -- side "item": the items the same users took
        ("users who took this also took ..."), side "user": the users who took the same items -- as ops.cooccur_topk lists them:
        out_idx int32 / out_val float32 (optional) / out_cnt int32 (optional, the raw co-count) [B x k] on the device, by (score
        descending, id ascending), -1 / -inf / 0 where fewer than k rows share a neighbour; the row itself is never listed
        (csrc/cooccur.hip). measure: "count", "cosine" or "jaccard". rows: the query ids (host array or tensor, checked on the
        host). Nothing of the learned tables is read: this works on an untrained model, before the first step. Single-GPU."""
        who = "co_neighbours_device"
        k, _ = ops._form_k(who, k, ops.COOCCUR_MAX_K), ops._cooccur_measure(who, measure)
        index = self.cooccur_index(side)
        q = ops._cooccur_rows(who, index, rows)
        need = ops.cooccur_workspace(int((index.walk[q] > ops.COOCCUR_SLOTS // 2).sum()), index.n_query)
        ops.cooccur_topk(index, q, k, out_idx, out_val, out_cnt, measure=measure, workspace=self._kept_workspace(who, need, index.device))
        return out_idx, out_val

    def _kept_workspace(self, who, need, dev):
        """The model's ONE zeroed workspace for the dense form of the two-form calls (ops.cooccur_topk, walk_topk,
        neighbour_vote_topk): a uint8 tensor of at least `need` bytes on `dev`, None for need = 0. Re-made (and zeroed) when it is
        missing, too small or on another device; past ops.COOCCUR_WORKSPACE_BUDGET a ValueError that names the caller, before
        anything is allocated."""
        # One buffer is enough for the three families: each runs on the current stream, and every call leaves its workspace zero
        # (csrc/co_select.h), so the next call -- of whichever family -- finds it as the first one did.
        ws = self.__dict__.get("_form_ws")
        if need and (ws is None or ws.numel() < need or ws.device != torch.device(dev)):
            if need > ops.COOCCUR_WORKSPACE_BUDGET:
                raise ValueError("%s: the dense form's rows need %d bytes, the budget is %d" % (who, need, ops.COOCCUR_WORKSPACE_BUDGET))
            ws = self.__dict__["_form_ws"] = torch.zeros(need, dtype=torch.uint8, device=dev)
        return ws if need else None

    def _graph_neighbours(self, side, ids, k, lists_into):
        """The host half of co_items / rp3_items and their user twins: the ids checked against their side, lists_into(ids, idx, val)
        fills the two device tensors [B x k] -> Neighbours on the CPU."""
        ids = self._id_lists([ids], side, self.num_items if side == "item" else self.num_users)[1]
        dev = self._require_gpu()
        idx = torch.empty(ids.size, k, dtype=torch.int32, device=dev)
        val = torch.empty(ids.size, k, dtype=torch.float32, device=dev)
        lists_into(ids, idx, val)
        return Neighbours(idx.cpu(), val.cpu())

    def _co(self, side, ids, k, measure):
        k, _ = ops._form_k("co_%ss" % side, k, ops.COOCCUR_MAX_K), ops._cooccur_measure("co_%ss" % side, measure)
        return self._graph_neighbours(side, ids, k, lambda ids, idx, val: self.co_neighbours_device(side, ids, k, measure, idx, val))

    def co_items(self, item_ids, k, measure="cosine"):
        """The k items most often taken by the same training users as each given item -- "users who took this also took ...",
        ItemKNN's neighbour lists: Neighbours(ids CPU int32 [B x k] (-1 padded), scores CPU fp32 [B x k] (-inf padded)), the tuple
        similar_items returns, by (score descending, id ascending). With c = the users who took both, a and b the two items'
        training interactions: measure "count" scores c, "cosine" c / sqrt(a b), "jaccard" c / (a + b - c). The item itself is
        never listed, nor an item without a common user. 1 <= k <= 256 and a known measure, else ValueError; an id outside the
        catalogue is an IndexError -- both before anything touches the device. The lists are read off the training graph alone: no
        cached tables are needed, so this works on an untrained model."""
        return self._co("item", item_ids, k, measure)

    def co_users(self, user_ids, k, measure="cosine"):
        """co_items over the users: the k users who took the most items in common with each given user. Needs no cached tables: it
        works on an untrained model."""
        return self._co("user", user_ids, k, measure)

    def walk_weights(self, side, alpha, beta):
        """The ops.WalkWeights of RP3beta over one side of the training graph (ops.rp3_weights over cooccur_index(side)), kept per
        (side, alpha, beta) on the model's device."""
        index = self.cooccur_index(side)
        kept = self.__dict__.setdefault("_walk_weights", {})
        key = (side, float(alpha), float(beta))
        hit = kept.get(key)
        if hit is None or hit.device != index.device:
            hit = kept[key] = ops.rp3_weights(index, alpha, beta)
        return hit

    @torch.no_grad()
    def walk_neighbours_device(self, side, rows, k, alpha, beta, out_idx, out_val):
        """The k RP3beta neighbours of each given row of the TRAINING GRAPH -- side "item": the items a two-step random walk item
        -> user -> item reaches, each transition probability raised to `alpha`, the target's score divided by its popularity
        deg^beta; side "user": the same over users -- as ops.walk_topk lists them: out_idx int32 / out_val float32 [B x k] on the
        device, by (score descending, id ascending), -1 / -inf where fewer than k rows are reached; the row itself is never listed
        (csrc/walk.hip). rows: the query ids (host array or tensor, checked on the host). The dense form's workspace is kept (every
        call leaves it zero). Nothing of the learned tables is read: this works on an untrained model. Single-GPU."""
        who = "walk_neighbours_device"
        k = ops._form_k(who, k, ops.WALK_MAX_K)
        index = self.cooccur_index(side)
        weights = self.walk_weights(side, alpha, beta)
        q = ops._cooccur_rows(who, index, rows)
        need = ops.walk_workspace(int((index.walk[q] > ops.WALK_SLOTS // 2).sum()), index.n_query)
        ops.walk_topk(index, q, k, weights, out_idx, out_val, workspace=self._kept_workspace(who, need, index.device))
        return out_idx, out_val

    def _rp3(self, side, ids, k, alpha, beta):
        k = ops._form_k("rp3_%ss" % side, k, ops.WALK_MAX_K)
        alpha, beta = ops._rp3_params("rp3_%ss" % side, alpha, beta)
        return self._graph_neighbours(side, ids, k, lambda ids, idx, val: self.walk_neighbours_device(side, ids, k, alpha, beta, idx, val))

    def rp3_items(self, item_ids, k, alpha=1.0, beta=0.6):
        """The k items a two-step random walk over the training graph reaches from each given item, RP3beta's neighbour lists
        (Paudel et al. 2016; beta = 0 is P3alpha, Cooper et al. 2014): Neighbours(ids CPU int32 [B x k] (-1 padded), scores CPU
        fp32 [B x k] (-inf padded)), by (score descending, id ascending). score(q, j) = sum over the users u who took both of
        (1 / deg(q))^alpha (1 / deg(u))^alpha, divided by deg(j)^beta -- beta is the popularity penalty on the target item. The
        defaults alpha = 1.0, beta = 0.6 are those of the commonly used implementation and are NOT TUNED here. The item itself is
        never listed, nor an item without a common user. 1 <= k <= 256, alpha and beta finite in [0, 4], else ValueError; an id
        outside the catalogue is an IndexError -- both before anything touches the device. The lists are read off the training
        graph alone: no cached tables are needed, so this works on an untrained model."""
        return self._rp3("item", item_ids, k, alpha, beta)

    def rp3_users(self, user_ids, k, alpha=1.0, beta=0.6):
        """rp3_items over the users: the k users a walk user -> item -> user reaches from each given user. The defaults are those of
        the commonly used implementation and are not tuned here. Needs no cached tables: it works on an untrained model."""
        return self._rp3("user", user_ids, k, alpha, beta)

    def _knn_source(self, source, neighbours, measure, alpha=1.0, beta=0.6):
        """The checks neighbour_lists / recommend_knn / BaselineReport share, before anything touches the device: -> neighbours."""
        if isinstance(neighbours, bool) or not isinstance(neighbours, (int, np.integer)) or not 1 <= neighbours <= ops.VOTE_MAX_K:
            raise ValueError("neighbours must be an integer in [1, %d], got %r" % (ops.VOTE_MAX_K, neighbours))
        ops._cooccur_measure("neighbour_lists", measure)
        if source == "rp3":
            ops._rp3_params("neighbour_lists", alpha, beta)
        elif source != "co":
            if not (source == "fused" or (isinstance(source, str) and source in self._mods)):
                raise ValueError("source must be 'co', 'rp3', 'fused' or one of this model's heads %s, got %r"
                                 % ("/".join(self._mods) or "(none)", source))
        return int(neighbours)

    @staticmethod
    def _vote_scale(val):
        """(e, zero_votes) of a block of list values [n x Kn] (-inf fillers) whose magnitudes the vote's 2^-24 fixed point would lose:
        the power of two 2^e that puts the largest finite value into [0.5, 1) (0 without a positive one; at most 126), applied IN
        PLACE with torch.ldexp -- exact, and the order is kept --, and the share of the listed entries whose vote rint(double(val)
        * 2^24) is 0 all the same (0.0 without a listed entry)."""
        finite = torch.isfinite(val)
        top = float(torch.where(finite, val, torch.zeros_like(val)).max().item()) if val.numel() else 0.0
        e = min(126, -math.frexp(top)[1]) if top > 0.0 else 0
        if e:
            val.copy_(torch.ldexp(val, torch.tensor(e, dtype=torch.int32, device=val.device)))
        listed = int(finite.sum().item())
        lost = int((finite & (torch.round(val.double() * 2.0 ** ops.VOTE_FRAC_BITS) == 0)).sum().item())
        return e, (lost / listed if listed else 0.0)

    @torch.no_grad()
    def neighbour_lists(self, source="co", neighbours=50, measure="cosine", alpha=1.0, beta=0.6):
        """The `neighbours` nearest items of EVERY item as the ops.NeighbourLists [num_items x neighbours] neighbour_vote_topk
        takes, built in blocks of KNN_LIST_BLOCK items and kept on the device. source "co": the co-interaction neighbours of the
        training graph under `measure` (co_neighbours_device; no cached tables are needed, so this works on an untrained model),
        kept per (neighbours, measure); "rp3": the RP3beta neighbours of the training graph under `alpha` and `beta`
        (walk_neighbours_device; `measure` is not used; untrained models as well), kept per (neighbours, alpha, beta) -- their
        values, deg^-alpha deg^-alpha deg^-beta, are far below the 2^-24 a vote is quantised to, so the whole block is multiplied by
        ONE power of two 2^e that puts its largest value into [0.5, 1): the returned lists carry scale_exp = e and zero_votes = the
        share of the listed entries whose fixed-point vote is 0 all the same (that loss is the vote's, and it is reported, not
        hidden); "fused" or a head letter of self._mods: the cosine neighbours in that space of the cached tables
        (neighbours_device; `measure` is not used), kept per table version. alpha and beta are read by "rp3" alone. Errors as
        similar_items / co_items / rp3_items."""
        neighbours = self._knn_source(source, neighbours, measure, alpha, beta)
        dev = self._require_gpu()
        kept = self.__dict__.setdefault("_knn_lists", {})
        if source == "co":
            key, version = ("co", neighbours, measure), 0
        elif source == "rp3":
            key, version = ("rp3", neighbours, float(alpha), float(beta)), 0
        else:
            self._cached_tables("similar_items() / similar_users() need", "neighbour lists need the whole cached tables on this rank; "
                                "the tables are item-sharded (lean / multi-rank evaluation)")
            key, version = (source, neighbours), getattr(self, "_table_version", 0)
        hit = kept.get(key)
        if hit is not None and hit[0] == version and hit[1].device == dev:
            return hit[1]
        I = self.num_items
        idx = torch.empty(I, neighbours, dtype=torch.int32, device=dev)
        val = torch.empty(I, neighbours, dtype=torch.float32, device=dev)
        for lo in range(0, I, KNN_LIST_BLOCK):
            rows = np.arange(lo, min(I, lo + KNN_LIST_BLOCK), dtype=np.int64)
            if source == "co":
                self.co_neighbours_device("item", rows, neighbours, measure, idx[lo:lo + rows.size], val[lo:lo + rows.size])
            elif source == "rp3":
                self.walk_neighbours_device("item", rows, neighbours, alpha, beta, idx[lo:lo + rows.size], val[lo:lo + rows.size])
            else:
                self.neighbours_device("item", rows, neighbours, source, idx[lo:lo + rows.size], val[lo:lo + rows.size])
        scale = self._vote_scale(val) if source == "rp3" else None
        lists = ops.NeighbourLists(idx, val, dev)
        if scale is not None:
            lists.scale_exp, lists.zero_votes = scale
        kept[key] = (version, lists)
        return lists

    @torch.no_grad()
    def knn_recommend_device(self, users, lists, hist, k, excl=None, out_idx=None, out_val=None, out_cnt=None):
        """The k items the neighbour lists of each user's history vote for (ops.neighbour_vote_topk, csrc/vote.hip): out_idx int32,
        out_val float32, out_cnt int32 [B x k] on the device (allocated here when None), by (score descending, id ascending), -1 /
        -inf / 0 where fewer are voted for. users: segment ids of hist (host array or tensor, checked on the host); lists: an
        ops.NeighbourLists (neighbour_lists); hist: an ops.HistoryIndex whose own ids are left out; excl: a second HistoryIndex of
        the same segments to leave out as well. The dense form's workspace is kept (every call leaves it zero). Single-GPU."""
        dev = self._require_gpu()
        who = "knn_recommend_device"
        k = ops._form_k(who, k, ops.VOTE_MAX_K)
        ops._vote_indexes(who, lists, hist, excl)
        u = ops._checked_ids(users, hist.n_rows, who, "users", "users span [%d, %d], the histories have %d segments")
        B = int(u.size)
        out_idx = torch.empty(B, k, dtype=torch.int32, device=dev) if out_idx is None else out_idx
        out_val = torch.empty(B, k, dtype=torch.float32, device=dev) if out_val is None else out_val
        out_cnt = torch.empty(B, k, dtype=torch.int32, device=dev) if out_cnt is None else out_cnt
        need = ops.vote_workspace(int((ops.vote_votes(lists, hist, excl)[u] > ops.VOTE_SLOTS // 2).sum()), lists.n)
        ops.neighbour_vote_topk(lists, hist, u, k, out_idx, out_val, out_cnt, excl=excl, workspace=self._kept_workspace(who, need, dev))
        return out_idx, out_val, out_cnt

    def recommend_knn(self, user_ids, k, neighbours=50, source="co", measure="cosine", history=None, exclude=None, alpha=1.0, beta=0.6):
        """A neighbourhood recommender beside the model's own lists: per user the k items the `neighbours` nearest items of every
        item of the user's history vote for -- KnnLists(ids CPU int32 [B x k] (-1 padded), scores CPU fp32 [B x k] (-inf padded: the
        sum of the neighbour scores behind the item, in 2^-24 fixed point), votes CPU int32 [B x k] (their number)), by (score
        descending, id ascending). source "co" is ItemKNN over the training graph under `measure` ("count", "cosine", "jaccard");
        "fused" or a head letter of self._mods is content-KNN in that space ("v": recommend what looks like what you took);
        "rp3" is RP3beta over the training graph under `alpha` and `beta` (rp3_items; the two are ignored by the other sources; the
        defaults are the commonly used ones, not tuned here), its scores in units of 2^-e, e = neighbour_lists(...).scale_exp.
        history: dict user -> item ids (default: the data set's train dict, as explain_history takes it); the history's own items
        are never listed; `exclude` = dict user -> item ids left out on top, as explain() takes it. k or neighbours outside
        [1, 256], an unknown source or measure: ValueError; an id outside its side: IndexError -- both before anything touches the
        device. An empty user_ids returns [0 x k] without a launch."""
        k = ops._form_k("recommend_knn", k, ops.VOTE_MAX_K)
        neighbours = self._knn_source(source, neighbours, measure, alpha, beta)
        users = self._id_lists([user_ids], "user", self.num_users)[1]
        if history is None:
            history = self.dataset.get_user_train_dict()
        elif not isinstance(history, dict):
            raise TypeError("history must be a dict user -> item ids")
        hptr, hflat, _ = self._id_lists([history.get(int(u), []) for u in users], "history item")
        tptr, tflat = self._excluded(exclude, users, "item")
        n = int(users.size)
        if not n:
            return KnnLists(torch.empty(0, k, dtype=torch.int32), torch.empty(0, k, dtype=torch.float32), torch.empty(0, k, dtype=torch.int32))
        dev = self._require_gpu()
        lists = self.neighbour_lists(source, neighbours, measure, alpha, beta)
        hist = ops.HistoryIndex(hptr, hflat, dev, n_items=self.num_items)
        excl = ops.HistoryIndex(tptr, tflat, dev, n_items=self.num_items) if tflat.size else None
        idx, val, cnt = self.knn_recommend_device(np.arange(n, dtype=np.int64), lists, hist, k, excl)     # row b's history is segment b
        return KnnLists(idx.cpu(), val.cpu(), cnt.cpu())

    @staticmethod
    def _ials_params(factors=64, iters=15, conf=1.0, reg=0.01, reg_scale=0.0, seed=2022):
        """The checks fit_ials / recommend_ials / BaselineReport share (ops._ials_params), before anything touches the device: -> the
        parameter tuple the fit is kept under."""
        return ops._ials_params("fit_ials", factors, iters, conf, reg, reg_scale, seed)

    def _ials_graph(self, dev):
        """The training graph as the two ops.AlsIndex of the fit -- every user's list de-duplicated and sorted, the transpose
        likewise --, checked once and kept on the device: (users' index, items' index)."""
        hit = self.__dict__.get("_ials_index")
        if hit is None or hit[0].device != dev:
            U, I = self.num_users, self.num_items
            train = self.dataset.get_user_train_dict()
            none = np.zeros(0, dtype=np.int64)
            up, ui, _ = self._id_lists([np.unique(np.asarray(train.get(u, none), dtype=np.int64)) for u in range(U)], "train item")
            order = np.argsort(ui, kind="stable")
            ip = np.zeros(I + 1, dtype=np.int64)
            np.cumsum(np.bincount(ui, minlength=I), out=ip[1:])
            iu = np.repeat(np.arange(U, dtype=np.int64), np.diff(up))[order]
            hit = self.__dict__["_ials_index"] = (ops.AlsIndex(up, ui, U, I, dev), ops.AlsIndex(ip, iu, I, U, dev))
        return hit

    @torch.no_grad()
    def fit_ials(self, factors=64, iters=15, conf=1.0, reg=0.01, reg_scale=0.0, seed=2022):
        """The implicit-feedback ALS baseline (Hu, Koren, Volinsky, ICDM 2008) over the TRAINING GRAPH alone: IalsFactors(users
        float32 [U x factors], items float32 [I x factors] -- device tensors --, params, objective), kept per parameter tuple (a
        second call returns the kept handle). A pure-ID factor model of the model's own dimension: what the content and the graph
        convolution buy is the difference to it. Nothing of the learned tables is read, so this works on an untrained model.
        Items start at float32(0.01 * default_rng(seed).standard_normal((I, factors))), users at zero; every iteration solves the
        users from the items, then the items from the users, each half-sweep one ops.als_solve (csrc/als.hip) over the float64
        Gram of the fixed side (ops.row_gram). reg[r] = reg * (deg(r) + 1) ** reg_scale: reg_scale = 0 is the classical constant
        ridge, reg_scale > 0 the frequency-scaled ridge of Rendle et al. (RecSys 2022) without its second constant. objective:
        float64 [2 iters], the iALS loss after every half-sweep,
            <G_X, G_Y>_F + sum_obs [(1 + conf)(1 - s)^2 - s^2] + sum_r reg[r] |x_r|^2,
        the Grams from ops.row_gram, the observed term a float64 torch composition (a log line, not the hot path). The defaults
        are not tuned here. factors in {16, 32, 48, 64}, 1 <= iters <= 100, conf >= 0, reg > 0, 0 <= reg_scale <= 1, all finite:
        else ValueError before anything touches the device. Single-GPU."""
        params = self._ials_params(factors, iters, conf, reg, reg_scale, seed)
        factors, iters, conf, reg, reg_scale, seed = params
        dev = self._require_gpu()
        kept = self.__dict__.setdefault("_ials", {})
        hit = kept.get(params)
        if hit is not None and hit.users.device == dev:
            return hit
        U, I = self.num_users, self.num_items
        by_user, by_item = self._ials_graph(dev)
        # the ridges stay host arrays for als_solve: checked there without a read back (a device tensor would be read back per half-sweep)
        host_u = reg * (by_user.deg.astype(np.float64) + 1.0) ** reg_scale
        host_i = reg * (by_item.deg.astype(np.float64) + 1.0) ** reg_scale
        reg_u, reg_i = torch.from_numpy(host_u).to(dev), torch.from_numpy(host_i).to(dev)
        Y = torch.from_numpy((0.01 * np.random.default_rng(seed).standard_normal((I, factors))).astype(np.float32)).to(dev)
        X = torch.zeros(U, factors, dtype=torch.float32, device=dev)
        ones = torch.ones(max(U, I), dtype=torch.float32, device=dev)
        every = torch.arange(max(U, I), dtype=torch.int32, device=dev)
        G = {s: torch.empty(factors, factors, dtype=torch.float64, device=dev) for s in "XY"}
        ws = torch.empty(max(16, ops.row_gram_workspace(max(U, I), factors)), dtype=torch.uint8, device=dev)
        edge_u = torch.repeat_interleave(torch.arange(U, device=dev), torch.from_numpy(by_user.deg).to(dev))
        edge_i = by_user.nbr[:by_user.n_edges].long()
        objective = torch.empty(2 * iters, dtype=torch.float64, device=dev)

        def gram(T, side, n):
            return ops.row_gram_device(T, ones[:n], every[:n], out_gram=G[side], workspace=ws)[0]

        def loss(at):
            s = (X[edge_u].double() * Y[edge_i].double()).sum(1)
            objective[at] = ((gram(X, "X", U) * gram(Y, "Y", I)).sum() + ((1.0 + conf) * (1.0 - s) ** 2 - s * s).sum()
                             + (reg_u * X.double().pow(2).sum(1)).sum() + (reg_i * Y.double().pow(2).sum(1)).sum())

        for it in range(iters):
            ops.als_solve(by_user, Y, gram(Y, "Y", I), host_u, conf, X)
            loss(2 * it)
            ops.als_solve(by_item, X, gram(X, "X", U), host_i, conf, Y)
            loss(2 * it + 1)
        hit = kept[params] = IalsFactors(X, Y, params, objective.cpu().numpy())
        return hit

    @torch.no_grad()
    def ials_recommend_device(self, users, factors, k, excl=None, out_idx=None, out_val=None):
        """The k items with the largest x_u . y_i of an IalsFactors (fit_ials), over ops.cross_topk: out_idx int32 / out_val
        float32 [B x k] on the device (allocated here when None), by (score descending, id ascending), -1 / -inf where fewer than
        k items are left. users: user ids (host array or tensor, checked on the host) or an ops.CrossQuery that carries its
        exclusions; excl: (ptr, item ids) to leave out per user, as CSR on the host. 1 <= k <= 256. Single-GPU."""
        dev = self._require_gpu()
        if not isinstance(factors, IalsFactors):
            raise TypeError("factors must be the IalsFactors fit_ials returns")
        k = ops._form_k("ials_recommend_device", k, ops.COOCCUR_MAX_K)
        if isinstance(users, ops.CrossQuery):
            query = users
        else:
            query = ops.CrossQuery(users, self.num_users, self.num_items, dev, *(excl if excl is not None else (None, None)))
        B = query.n_queries
        out_idx = torch.empty(B, k, dtype=torch.int32, device=dev) if out_idx is None else out_idx
        out_val = torch.empty(B, k, dtype=torch.float32, device=dev) if out_val is None else out_val
        ops.cross_topk(factors.users, None, factors.items, None, query, k, out_idx, out_val)
        return out_idx, out_val

    def recommend_ials(self, user_ids, k, exclude=None, **fit):
        """The iALS baseline's lists: per user the k items with the largest x_u . y_i under fit_ials(**fit) -- Neighbours(ids CPU
        int32 [B x k] (-1 padded), scores CPU fp32 [B x k] (-inf padded)), by (score descending, id ascending). exclude: dict user
        -> item ids left out, as recommend_knn takes it; default: the data set's train dict. A user without history has the zero
        vector: every item scores 0 and the lowest ids are listed. k outside [1, 256] or a fit parameter out of range: ValueError;
        an id outside its side: IndexError -- both before anything touches the device. An empty user_ids returns [0 x k] without
        a launch or a fit."""
        k = ops._form_k("recommend_ials", k, ops.COOCCUR_MAX_K)
        params = self._ials_params(**fit)
        users = self._id_lists([user_ids], "user", self.num_users)[1]
        tptr, tflat = self._excluded(self.dataset.get_user_train_dict() if exclude is None else exclude, users, "item")
        if not users.size:
            return Neighbours(torch.empty(0, k, dtype=torch.int32), torch.empty(0, k, dtype=torch.float32))
        self._require_gpu()
        idx, val = self.ials_recommend_device(users, self.fit_ials(*params), k, (tptr, tflat))
        return Neighbours(idx.cpu(), val.cpu())

    @torch.no_grad()
    def fit_ease(self, l2=500.0):
        """The EASE^R baseline (Steck, WWW 2019) over the TRAINING GRAPH alone: with X the binary user x item matrix (every
        user's list de-duplicated, as _ials_graph builds it), G = X^T X + l2 I and P = G^-1 -- EaseModel(P float64 [I x I] on the
        device, l2, pivot_min, bytes), kept per l2 (a second call returns the kept handle). The item-item weights are B_ij =
        -P_ij / P_jj off the diagonal; they are never formed: ease_recommend_device ranks from P. ops.gram_counts builds G (exact
        integer counts), ops.spd_inverse inverts it in place in float64 (csrc/ease.hip); pivot_min is the smallest pivot of the
        sweep (>= l2 up to rounding: how far G is from singular), bytes what P and the sweep's workspace took. Nothing of the
        learned tables is read, so this works on an untrained model. l2 is the model's one hyper-parameter, an explicit
        popularity damping; the default 500 is the commonly quoted value, not tuned here. l2 finite and > 0 and num_items <=
        ops.EASE_MAX_ITEMS: else ValueError before anything touches the device. Single-GPU; lean tables are refused.
        Every kept fit holds 8 I^2 bytes of device memory (46 GB at the Tiktok shape) until drop_ease releases it."""
        l2 = ops._ease_params("fit_ease", l2, self.num_items)
        self._no_lean("fit_ease()")
        dev = self._require_gpu()
        kept = self.__dict__.setdefault("_ease", {})
        hit = kept.get(l2)
        if hit is not None and hit.P.device == dev:
            return hit
        U, I = self.num_users, self.num_items
        train = self.dataset.get_user_train_dict()
        index = ops.CooccurIndex.from_train({u: np.unique(np.asarray(v, dtype=np.int64)) for u, v in train.items()}, U, I, "item", dev)
        P = torch.empty(I, I, dtype=torch.float64, device=dev)
        ops.gram_counts(index, l2, P)
        ws = torch.empty(ops.spd_inverse_workspace(I), dtype=torch.uint8, device=dev)
        pivot_min = ops.spd_inverse(P, ws)
        hit = kept[l2] = EaseModel(P, l2, pivot_min, P.numel() * 8 + ws.numel())
        return hit

    def drop_ease(self, l2=None):
        """Release the kept EASE fit of `l2` (None: every kept fit) -- 8 I^2 bytes of device memory each; a handle the caller
        still holds keeps its tensor alive. -> the number of fits dropped."""
        kept = self.__dict__.get("_ease", {})
        gone = list(kept) if l2 is None else [k for k in kept if k == float(l2)]
        for k in gone:
            del kept[k]
        return len(gone)

    @torch.no_grad()
    def ease_recommend_device(self, users, ease, k, hist, excl=None, out_idx=None, out_val=None):
        """The k items with the largest EASE score -(sum_{i in H, i != j} P_ij) / P_jj of an EaseModel (fit_ease), over
        ops.ease_topk: out_idx int32 / out_val float32 [B x k] on the device (allocated here when None), by (score descending, id
        ascending), -1 / -inf where fewer than k items are left. users: segment ids of hist (host array or tensor, checked on the
        host); hist: an ops.HistoryIndex with n_items = num_items, the histories; excl: a second HistoryIndex over the same
        segments, the ids left out instead of the history (default: the history itself). 1 <= k <= 256. Single-GPU."""
        dev = self._require_gpu()
        if not isinstance(ease, EaseModel):
            raise TypeError("ease must be the EaseModel fit_ease returns")
        k = ops._form_k("ease_recommend_device", k, ops.EASE_MAX_K)
        B = int(np.asarray(ops._host(users)).size)
        out_idx = torch.empty(B, k, dtype=torch.int32, device=dev) if out_idx is None else out_idx
        out_val = torch.empty(B, k, dtype=torch.float32, device=dev) if out_val is None else out_val
        ops.ease_topk(ease.P, hist, users, k, out_idx, out_val, excl=excl)
        return out_idx, out_val

    def recommend_ease(self, user_ids, k, exclude=None, history=None, l2=500.0):
        """The EASE baseline's lists: per user the k items with the largest score under fit_ease(l2) -- Neighbours(ids CPU int32
        [B x k] (-1 padded), scores CPU fp32 [B x k] (-inf padded)), by (score descending, id ascending). history: dict user ->
        item ids (default: the data set's train dict, as recommend_knn takes it); the history's own items are never listed;
        exclude: dict user -> item ids left out on top. A user without history scores 0 everywhere: the lowest ids are listed.
        k outside [1, 256], l2 not finite and positive or a catalogue beyond ops.EASE_MAX_ITEMS: ValueError; an id outside its
        side: IndexError -- both before anything touches the device. An empty user_ids returns [0 x k] without a launch or a fit."""
        k = ops._form_k("recommend_ease", k, ops.EASE_MAX_K)
        l2 = ops._ease_params("recommend_ease", l2, self.num_items)
        users = self._id_lists([user_ids], "user", self.num_users)[1]
        if history is None:
            history = self.dataset.get_user_train_dict()
        elif not isinstance(history, dict):
            raise TypeError("history must be a dict user -> item ids")
        lists = [list(history.get(int(u), [])) for u in users]
        hptr, hflat, _ = self._id_lists(lists, "history item")
        tptr, tflat = self._excluded(exclude, users, "item")
        n = int(users.size)
        if not n:
            return Neighbours(torch.empty(0, k, dtype=torch.int32), torch.empty(0, k, dtype=torch.float32))
        dev = self._require_gpu()
        hist = ops.HistoryIndex(hptr, hflat, dev, n_items=self.num_items)
        excl = None
        if tflat.size:                   # what is left out replaces the history in ease_topk: the history and the extra ids
            eptr, eflat, _ = self._id_lists([h + list((exclude or {}).get(int(u), [])) for h, u in zip(lists, users)], "excluded item")
            excl = ops.HistoryIndex(eptr, eflat, dev, n_items=self.num_items)
        idx, val = self.ease_recommend_device(np.arange(n, dtype=np.int64), self.fit_ease(l2), k, hist, excl)    # row b is segment b
        return Neighbours(idx.cpu(), val.cpu())

    @torch.no_grad()
    def clusters_device(self, side, n_clusters, space="fused", iters=25, seed=2022, init=None):
        """Spherical k-means of the item rows (side "item") or the user rows ("user") of one block of the cached tables -- space
        "fused" or a head letter of self._mods, as neighbours_device takes it -- into n_clusters content clusters by cosine:
        ops.KMeans(assign, cos, centroids, counts -- device tensors --, n_iter, converged, cohesion), Lloyd's loop on the device
        (ops.spherical_kmeans, csrc/kmeans.hip: one assign and one update launch per iteration). 1 <= n_clusters <= 256,
        iters >= 1; init: n_clusters row indices (default: drawn on the host from `seed`). Tables as predict_device: those of the
        last training forward."""
        n_clusters, iters = ops._kmeans_params("clusters_device", n_clusters, iters)
        lo, n = self._side_rows(side)
        h = self._neighbour_space(space)
        dev = self._cached_tables("cluster_items() / cluster_users() need", "content clusters need the whole cached tables on this rank; "
                                  "the tables are item-sharded (lean / multi-rank evaluation)")
        d = self.latent_dim
        sqn = self._block_sqnorms(dev)
        return ops.spherical_kmeans(self._ws["Y"][lo:lo + n, h * d:(h + 1) * d], sqn[lo:lo + n, h], n_clusters, iters=iters, seed=seed,
                                    init=init)

    def _clusters(self, side, n_clusters, space, iters, seed):
        km = self.clusters_device(side, n_clusters, space, iters, seed)
        return Clusters(km.assign.cpu(), km.cos.cpu(), km.centroids.cpu(), km.counts.cpu(), km.n_iter, km.converged)

    def cluster_items(self, n_clusters, space="fused", iters=25, seed=2022):
        """Content clusters of the items: Clusters(assign CPU int32 [I] (-1: an item whose row has no norm), cos CPU fp32 [I] the
        cosine to its centroid (-inf there), centroids CPU fp32 [n_clusters x d] unit rows, counts CPU int32 [n_clusters], n_iter,
        converged) -- spherical k-means in the "fused" space predict() scores with, or in one single-modal head's (a letter of
        self._mods: the visual clusters). Not converged after `iters` iterations: assign / cos were formed against the centroids'
        predecessors (ops.spherical_kmeans). With n_clusters <= 16, classes_from_clusters(assign, n_clusters) -- the -1 entries, if
        any, moved to a class of their own, n_clusters, which then has to stay <= 15 -- is a valid `classes` argument of
        recommend_calibrated: lists calibrated to the user's own mix of content."""
        return self._clusters("item", n_clusters, space, iters, seed)

    def cluster_users(self, n_clusters, space="fused", iters=25, seed=2022):
        """cluster_items over the user rows."""
        return self._clusters("user", n_clusters, space, iters, seed)

    def _geometry_spaces(self, space):
        """The spaces a geometry call covers: every one (space None: "fused", then the heads) or the one named."""
        if space is None:
            return ("fused",) + tuple(self._mods)
        self._neighbour_space(space)
        return (space,)

    @torch.no_grad()
    def geometry_device(self, side, space="fused", rows=None, t=2.0):
        """The raw geometry of one cosine space over the item rows (side "item") or the user rows ("user") of the cached tables:
        (S float64 [1], pairs int64 [1], n_valid int64 [1], G float64 [d x d], m float64 [d]) on the device, nothing read back --
        the all-pairs uniformity sum at temperature t (ops.uniformity_sum: uniformity = log(S / pairs)) and the float64 Gram matrix
        and sum of the unit rows (ops.row_gram; reports.spectrum_summary reads the spectrum), two launches each (csrc/geometry.hip).
        space: "fused" (block 0, the rows predict() scores with) or a head letter of self._mods. rows: the ids within the side --
        None: all of them; a host array or list, checked on the host (IndexError); or an int32 tensor on the device, which the
        kernels check entry by entry (an id outside the side is skipped). A repeated id is an entry of its own; a row without a
        norm takes part in nothing. 0 < t <= 8. Tables as predict_device: those of the last training forward."""
        lo, n = self._side_rows(side)
        h = self._neighbour_space(space)
        t = ops._geometry_t("geometry_device", t)
        if rows is not None and not (isinstance(rows, torch.Tensor) and rows.is_cuda):
            rows = np.ascontiguousarray(self._id_lists([rows], side, n)[1], dtype=np.int32)
        self._require_gpu()
        dev = self._cached_tables("embedding_geometry() needs", "the embedding geometry needs the whole cached tables on this rank; "
                                  "the tables are item-sharded (lean / multi-rank evaluation)")
        d = self.latent_dim
        sqn = self._block_sqnorms(dev)
        if rows is None:
            rows = self._ws.get("geo_all_" + side)
            if rows is None:
                rows = self._ws["geo_all_" + side] = torch.arange(n, dtype=torch.int32, device=dev)
        elif not isinstance(rows, torch.Tensor):
            rows = torch.from_numpy(rows).to(dev)
        need = max(ops.uniformity_workspace(rows.numel(), d), ops.row_gram_workspace(rows.numel(), d))
        if self._ws.get("geo_ws") is None or self._ws["geo_ws"].numel() < need:
            self._ws["geo_ws"] = torch.empty(need, dtype=torch.uint8, device=dev)
        table, sq = self._ws["Y"][lo:lo + n, h * d:(h + 1) * d], sqn[lo:lo + n, h]
        S, counts = ops.uniformity_sum_device(table, sq, rows, t, workspace=self._ws["geo_ws"])
        G, m, _ = ops.row_gram_device(table, sq, rows, workspace=self._ws["geo_ws"])
        return S, counts[0:1], counts[1:2], G, m

    def embedding_geometry(self, side="item", space=None, rows=None, t=2.0):
        """What a learned space looks like: Geometry(columns, labels, values CPU float64 [spaces x 6]), one row per space --
        space None: "fused" and every single-modal head of self._mods; or the one space named -- over the item rows (side "item")
        or the user rows ("user"), all of them or the ids `rows`. Columns (reports.GEOMETRY_COLUMNS):
          n           the rows that took part (a row without a norm does not);
          uniformity  log of the mean of exp(-t |x^ - y^|^2) = exp(2 t (cos - 1)) over all pairs of them (Wang & Isola, ICML'20):
                      0 for fully collapsed rows, more negative for rows spread over the sphere; NaN with fewer than two rows;
          erank       exp of the entropy of the covariance spectrum of the unit rows (Roy & Vetterli), between 1 and d;
          top1        the share of the variance along the first principal direction;
          rank99      the number of leading directions that hold 99 % of the variance (dimensional collapse, Jing et al., ICLR'22);
          centre      the norm of the mean unit row: 0 for rows spread evenly round the sphere, 1 for fully collapsed rows.
        The all-pairs sum and the Gram matrix are formed on the device (geometry_device), the d x d spectrum on the host in
        float64. Tables as predict(): those of the last training forward."""
        from . import reports
        spaces = self._geometry_spaces(space)
        self._side_rows(side)
        ops._geometry_t("embedding_geometry", t)
        raw = [self.geometry_device(side, s, rows, t) for s in spaces]
        values = np.stack([reports.geometry_row(*[x.cpu().numpy() for x in r]) for r in raw])
        return Geometry(reports.GEOMETRY_COLUMNS, tuple(spaces), torch.from_numpy(values))

    @torch.no_grad()
    def alignment_device(self, users, items, out=None):
        """2 - 2 cos(user row, item row) of every pair in every space: out float32 [n x (1 + S)] on the device, column 0 the fused
        space, column 1 + h head h. users int64 [n] / items int32 [n] on the device. One hard_negatives_device launch per space with
        the item as the pair's only candidate: the cosine is its score, bit for bit. A pair with a row that has no norm has cosine
        0 there and so the value 2; a user or an item outside its range gives +inf."""
        n = users.numel()
        dev = self._require_gpu()
        spaces = ("fused",) + tuple(self._mods)
        if out is None:
            out = torch.empty(n, len(spaces), dtype=torch.float32, device=dev)
        neg = torch.empty(n, dtype=torch.int64, device=dev)
        pos = torch.empty(n, dtype=torch.int32, device=dev)
        score = torch.empty(n, dtype=torch.float32, device=dev)
        cands = items.reshape(n, 1)
        for h, s in enumerate(spaces):
            self.hard_negatives_device(users, cands, s, neg, pos, score)
            out[:, h] = 2.0 - 2.0 * score
        return out

    def alignment(self, user_ids, item_ids, space=None):
        """The alignment term of Wang & Isola / DirectAU per (user, item) pair: |u^ - i^|^2 = 2 - 2 cos(u, i) between the user's
        and the item's unit rows -- CPU fp32 [n x (1 + S)], column 0 the fused space and column 1 + h head h (space None), or [n]
        for the one space named. user_ids / item_ids: one id each per pair, checked on the host (IndexError). A pair with a row
        that has no norm has cosine 0 in that space, so its value is 2; such pairs are not special-cased."""
        if space is not None:
            self._neighbour_space(space)
        users = self._id_lists([user_ids], "user", self.num_users)[1]
        items = self._id_lists([item_ids], "item", self.num_items)[1]
        if users.size != items.size:
            raise ValueError("one item per user: %d users for %d items" % (users.size, items.size))
        dev = self._require_gpu()
        out = self.alignment_device(torch.from_numpy(users.astype(np.int64)).to(dev), torch.from_numpy(items.astype(np.int32)).to(dev)).cpu()
        return out if space is None else out[:, self._neighbour_space(space)].contiguous()

    def _audience_row_sum(self, dev, sqn):
        """TIE's sum_i sigmoid(u . i) of EVERY user: the scorer's pass 1 in user blocks of at most 8192, computed once per table
        version and kept in the workspace (as _block_sqnorms keeps the norms)."""
        if self._ws.get("aud_row_sum_version") != self._table_version or self._ws.get("aud_row_sum") is None:
            U = self.num_users
            row_sum = torch.empty(U, dtype=torch.float32, device=dev)
            for lo in range(0, U, 8192):
                users = torch.arange(lo, min(U, lo + 8192), dtype=torch.int64, device=dev)
                row_sum[lo:lo + users.numel()] = self._catalogue_row_sum(dev, users, "TIE", sqn)
            self._ws["aud_row_sum"] = row_sum
            self._ws["aud_row_sum_version"] = self._table_version
        return self._ws["aud_row_sum"]

    @torch.no_grad()
    def audience_device(self, query, k, out_idx=None, out_val=None):
        """The k users the model ranks highest for each query item -- predict() read from the item's side -- under the current
        predict_type, fusion_mode and head mask: (idx int32 [Q x k], val float32 [Q x k]) on the device, (score descending, user id
        ascending), -1 / -inf where fewer than k users are eligible (csrc/audience.hip; no [U x Q] score block is written). query:
        an ops.AudienceQuery over this model's items and users (checked once; it may carry per-item lists of users to leave out),
        or item ids (host array or tensor, checked on the host). Tables as predict_device: those of the last training forward."""
        dev = self._cached_tables("audience() needs", "audience lists need the whole cached tables on this rank; the tables are "
                                  "item-sharded (lean / multi-rank evaluation)")
        k = int(k)
        if not 1 <= k <= ops.AUDIENCE_MAX_K:
            raise ValueError("k must lie in [1, %d]" % ops.AUDIENCE_MAX_K)
        U, I = self.num_users, self.num_items
        if not isinstance(query, ops.AudienceQuery):
            query = ops.AudienceQuery(query, I, U, dev)
        elif query.n_items != I or query.n_users != U:
            raise ValueError("query must be an ops.AudienceQuery over the %d items and %d users" % (I, U))
        Q = query.n_queries
        if out_idx is None:
            out_idx = torch.empty(Q, k, dtype=torch.int32, device=dev)
        if out_val is None:
            out_val = torch.empty(Q, k, dtype=torch.float32, device=dev)
        if Q == 0:
            return out_idx, out_val
        sqn = self._block_sqnorms(dev)
        row_sum = self._audience_row_sum(dev, sqn) if ops.PREDICT_TYPES.get(self.predict_type, 0) == 2 else None
        need = ops.audience_topk_workspace(Q, U, k)
        if self._ws.get("aud_ws") is None or self._ws["aud_ws"].numel() < need:
            self._ws["aud_ws"] = torch.empty(need, dtype=torch.uint8, device=dev)
        ops.audience_topk(self._ws["Y"], U, I, query, self.latent_dim, self.S, self._head_mask(), self.fusion_mode, self.predict_type, k,
                          out_idx, out_val, sqnorm=sqn, row_sum=row_sum, I_total=I, workspace=self._ws["aud_ws"])
        return out_idx, out_val

    def audience(self, item_ids, k, exclude=None):
        """The k users the model ranks highest for each given item: Audience(users CPU int32 [B x k] (-1 padded), scores CPU fp32
        [B x k] (-inf padded)), by (score descending, user id ascending), under the current predict type -- whom would this item be
        pushed to, and does TIE send it to other users than TE? `exclude` = dict item -> user ids to leave out (typically the
        item's training users). 1 <= k <= 256."""
        k = int(k)
        if not 1 <= k <= ops.AUDIENCE_MAX_K:
            raise ValueError("k must lie in [1, %d]" % ops.AUDIENCE_MAX_K)
        ids = self._id_lists([item_ids], "item")[1]
        ptr, flat = self._excluded(exclude, ids, "user", self.num_users)
        dev = self._require_gpu()
        if not ids.size:
            return Audience(torch.empty(0, k, dtype=torch.int32), torch.empty(0, k, dtype=torch.float32))
        query = ops.AudienceQuery(ids, self.num_items, self.num_users, dev, ptr if flat.size else None, flat if flat.size else None)
        idx, val = self.audience_device(query, k)
        return Audience(idx.cpu(), val.cpu())

    @torch.no_grad()
    def list_similarity_device(self, lists, out, side="item"):
        """Intra-list similarity: per list of item ids (side "item") or user ids ("user") the mean pairwise cosine of the listed
        rows in the fused space and in every head's space, from ONE launch over the side's rows of the cached Y (csrc/lists.hip).
        lists int32 [B x K] on the device, 1 <= K <= ops.LIST_MAX_K; an entry outside the side's rows (-1 fillers) is not listed,
        duplicates are pairs. out float32 [B x (1 + S)] on the device: column 0 = the fused rows predict() scores with, column
        1 + h = head self._mods[h]; NaN where fewer than two entries are listed. Tables as neighbours_device."""
        self._require_gpu()
        lo, n = self._side_rows(side)
        dev = self._cached_tables("list_similarity() needs", "list similarity needs the whole cached tables on this rank; the tables "
                                  "are item-sharded (lean / multi-rank evaluation)")
        d, nb = self.latent_dim, 1 + self.S
        sqn = self._block_sqnorms(dev)
        ops.list_pair_cosine(self._ws["Y"][lo:lo + n, :nb * d], sqn[lo:lo + n], lists, out, blocks=nb)
        return out

    def list_similarity(self, item_lists, space=None):
        """How alike the items of each list are: CPU fp32 [B x (1 + S)] -- column 0 the fused space, column 1 + h head
        self._mods[h] -- or [B] for one named space ("fused" or a head letter, as similar_items). item_lists: one sequence of item
        ids per list, of any lengths up to ops.LIST_MAX_K (shorter ones are padded, the padding is not listed); an id outside the
        catalogue raises IndexError. The value is the mean cosine over the list's position pairs; NaN below two items."""
        h = None if space is None else self._neighbour_space(space)
        lists = [[int(i) for i in x] for x in item_lists]
        K = max([len(x) for x in lists] + [1])
        if K > ops.LIST_MAX_K:
            raise ValueError("a list may hold at most %d items, got %d" % (ops.LIST_MAX_K, K))
        _, flat, lens = ops.ragged(lists, dtype=np.int32, check=(self.num_items, "item ids must lie in [0, %d)" % self.num_items))
        dev = self._require_gpu()
        out = torch.empty(len(lists), 1 + self.S, dtype=torch.float32, device=dev)
        self.list_similarity_device(torch.from_numpy(ops.ragged_padded(flat, lens, K)).to(dev), out, side="item")
        out = out.cpu()
        return out if h is None else out[:, h].contiguous()

    @torch.no_grad()
    def rerank_device(self, lists_idx, lists_val, k, lam, space="fused", out_idx=None, out_pos=None, out_val=None):
        """Diversified re-ranking of top-N pools: greedy maximal marginal relevance over the item rows of one block of the cached
        tables, ONE launch (csrc/rerank.hip). lists_idx int32 / lists_val float32 [B x N] on the device: per user a pool of items
        with their scores (predict_device(top_k=N) gives both), 1 <= k <= N <= ops.MMR_MAX_POOL; an entry outside the catalogue or
        with a score that is not finite (the -1 / -inf fillers) is never picked. With the pool's scores scaled to rel in [0, 1],
        step t takes the item with the largest lam * rel - (1 - lam) * (its largest cosine to the items taken so far), the lowest
        pool position among equals; lam = 1 keeps the pool's order. space: "fused" or a head letter, as neighbours_device.
        -> (out_idx int32 [B x k] the picked items, out_pos int32 their pool positions, out_val float32 their objectives), -1 / -1
        / -inf once no listed item is left; allocated here unless given. Tables as neighbours_device."""
        self._require_gpu()
        lo, n = self._side_rows("item")
        h = self._neighbour_space(space)
        dev = self._cached_tables("rerank_device() / recommend_diverse() need", "re-ranking needs the whole cached item table on this "
                                  "rank; the tables are item-sharded (lean / multi-rank evaluation)")
        d = self.latent_dim
        sqn = self._block_sqnorms(dev)
        B, k = lists_idx.shape[0], int(k)
        if out_idx is None:
            out_idx = torch.empty(B, k, dtype=torch.int32, device=dev)
        if out_pos is None:
            out_pos = torch.empty(B, k, dtype=torch.int32, device=dev)
        if out_val is None:
            out_val = torch.empty(B, k, dtype=torch.float32, device=dev)
        ops.mmr_rerank(self._ws["Y"][lo:lo + n, h * d:(h + 1) * d], sqn[lo:lo + n, h], lists_idx, lists_val, k, lam, out_idx, out_pos,
                       out_val)
        return out_idx, out_pos, out_val

    def has_cached_tables(self):
        """Whether a training forward has cached tables -- what predict() and every reader of the cached Y need (a bpr_loss whose
        step is still pending counts: _cached_tables makes it real). Never raises."""
        if getattr(self._plugin, "pending", None) is not None:
            return True
        return self._ws is not None and self._cache is not None

    def hard_negative_weights(self, space):
        """Per block of the cached Y the weight a hard-negative space puts on its cosine: "fused" / a head letter: that block
        alone; "loss": the logits of the training loss (:125-142) -- 1 on the fused block, alpha on every active head
        (_block_weights; under predict_type "normal" there are no single-modal terms and "loss" is "fused")."""
        if space == "loss":
            return [float(w) for w in self._block_weights()]
        h = self._neighbour_space(space)
        return [1.0 if b == h else 0.0 for b in range(1 + self.S)]

    @torch.no_grad()
    def hard_negatives_device(self, users, cands, space="fused", out_neg=None, out_pos=None, out_score=None):
        """Dynamic negative sampling's pick: per triplet the candidate item the cached tables score highest, ONE launch
        (csrc/hardneg.hip). users int64 [n], cands int32 [n x M] on the device, 1 <= M <= ops.HARD_NEG_MAX_CANDIDATES; a candidate
        outside the catalogue is never picked. The score of (u, i) is the weighted sum of the blocks' cosines between user row u
        and item row i of the cached Y; space: "fused" (block 0, the rows predict() scores with), a head letter of self._mods
        (that block alone), or "loss" (the training loss's logits: the fused block plus alpha times every active head).
        -> (out_neg int64 [n] the picked ids, out_pos int32 [n] their columns, out_score float32 [n] their scores), the lowest
        column among equal scores, -1 / -1 / -inf for a row without a listed candidate; allocated here unless given. Tables as
        predict_device: those of the last training forward."""
        w = self.hard_negative_weights(space)
        self._require_gpu()
        dev = self._cached_tables("hard_negatives_device() needs", "hard-negative sampling needs the whole cached item table on this "
                                  "rank; the tables are item-sharded (lean / multi-rank evaluation)")
        U, I, d, nb = self.num_users, self.num_items, self.latent_dim, 1 + self.S
        sqn = self._block_sqnorms(dev)
        n = users.numel()
        if out_neg is None:
            out_neg = torch.empty(n, dtype=torch.int64, device=dev)
        if out_pos is None:
            out_pos = torch.empty(n, dtype=torch.int32, device=dev)
        if out_score is None:
            out_score = torch.empty(n, dtype=torch.float32, device=dev)
        Y = self._ws["Y"]
        ops.pick_hard_negatives(Y[:U, :nb * d], sqn[:U], Y[U:U + I, :nb * d], sqn[U:U + I], w, users, cands, out_neg, out_pos, out_score)
        return out_neg, out_pos, out_score

    @torch.no_grad()
    def history_support_device(self, users, lists, hist, top=3, space="fused", exclude_self=True, out_idx=None, out_val=None,
                               out_cnt=None, out_mean=None):
        """"Because you interacted with what?": per (row b, target lists[b, k]) the entries of a history that sit closest to the
        target, ONE launch (csrc/history.hip). users int64 [B] / lists int32 [B x K] on the device, 1 <= K <= ops.LIST_MAX_K; hist:
        an ops.HistoryIndex on the device, users[b] names its segment (for the train dict laid out by user id that is the user id).
        The score of a history item against the target is the weighted sum of the blocks' cosines between the two item rows of the
        cached Y; space as hard_negative_weights: "fused", a head letter, or "loss". A target outside the catalogue, or a row whose
        user is outside the index, is not listed; nor is a history id outside the catalogue or -- with exclude_self -- equal to the
        target. -> (idx int32 [B x K x top] the history items' ids, best first, the earlier history position among equal scores;
        val float32 [B x K x top] their scores; cnt int32 [B x K] the listed history entries; mean float32 [B x K] their mean
        score), -1 / -inf / 0 / NaN where there is nothing; allocated here unless given. 1 - val[..., 0] is the pair's
        unexpectedness. Tables as similar_items: those of the last training forward, whole on this rank."""
        w = self.hard_negative_weights(space)
        self._require_gpu()
        lo, n = self._side_rows("item")
        dev = self._cached_tables("history_support_device() / explain_history() need", "history support needs the whole cached item "
                                  "table on this rank; the tables are item-sharded (lean / multi-rank evaluation)")
        d, nb = self.latent_dim, 1 + self.S
        sqn = self._block_sqnorms(dev)
        B, K = lists.shape
        top = int(top)
        if out_idx is None:
            out_idx = torch.empty(B, K, top, dtype=torch.int32, device=dev)
        if out_val is None:
            out_val = torch.empty(B, K, top, dtype=torch.float32, device=dev)
        if out_cnt is None:
            out_cnt = torch.empty(B, K, dtype=torch.int32, device=dev)
        if out_mean is None:
            out_mean = torch.empty(B, K, dtype=torch.float32, device=dev)
        ops.history_support(self._ws["Y"][lo:lo + n, :nb * d], sqn[lo:lo + n], w, users, lists, hist, top, out_idx, out_val, out_cnt,
                            out_mean, exclude_self=exclude_self)
        return out_idx, out_val, out_cnt, out_mean

    def explain_history(self, user_ids, items=None, top_k=None, top=3, space="fused", history=None, exclude=None):
        """Which items of each user's history back a recommendation: HistorySupport(items int32 [B x W] (-1 padded), history int32
        [B x W x top] -- per listed item the `top` history items closest to it, best first, -1 padded --, scores fp32 [B x W x top]
        (-inf padded), count int32 [B x W] the history entries compared, mean fp32 [B x W] their mean score (NaN without one)) on
        the CPU. items: one list of item ids per user, of any lengths up to ops.LIST_MAX_K -- those pairs; top_k: each user's top-K
        list under the current predict type, `exclude` = dict user -> item ids left out of the ranking, as explain() takes it.
        history: dict user -> item ids (default: the data set's train dict; a user absent from it has an empty history); the
        listed item itself is never its own support. space as history_support_device; 1 <= top <= ops.HISTORY_MAX_TOP. An id
        outside the catalogue raises IndexError."""
        if (items is None) == (top_k is None):
            raise ValueError("explain_history() takes exactly one of items and top_k")
        if isinstance(top, bool) or not isinstance(top, (int, np.integer)) or not 1 <= top <= 16:
            raise ValueError("top must be an integer in [1, 16], got %r" % (top,))
        self.hard_negative_weights(space)
        n = len(user_ids)
        if history is None:
            history = self.dataset.get_user_train_dict()
        elif not isinstance(history, dict):
            raise TypeError("history must be a dict user -> item ids")
        hptr, hflat, _ = self._id_lists([history.get(int(u), []) for u in user_ids], "history item")
        if items is not None:
            if exclude is not None:
                raise ValueError("exclude applies to top_k lists; items are taken as given")
            if len(items) != n:
                raise ValueError("one item list per user: %d lists for %d users" % (len(items), n))
            K = max([len(x) for x in items] + [1])
            if K > ops.LIST_MAX_K:
                raise ValueError("a list may hold at most %d items, got %d" % (ops.LIST_MAX_K, K))
            _, flat, lens = self._id_lists(items, "item")
            dev = self._require_gpu()
            lists = torch.from_numpy(ops.ragged_padded(flat, lens, K)).to(dev)
        else:
            top_k = int(top_k)
            if not 1 <= top_k <= min(ops.LIST_MAX_K, self.num_items):
                raise ValueError("top_k must lie in [1, min(%d, num_items = %d)], got %d" % (ops.LIST_MAX_K, self.num_items, top_k))
            tptr, tflat = self._excluded(exclude, user_ids, "item")
            dev = self._cached_tables("history_support_device() / explain_history() need", "history support needs the whole cached "
                                      "item table on this rank; the tables are item-sharded (lean / multi-rank evaluation)")
            if n:
                lists, _ = self.predict_device(user_ids, top_k=top_k, train_ptr=torch.from_numpy(tptr).to(dev),
                                               train_items=torch.from_numpy(tflat.astype(np.int32)).to(dev))
            else:
                lists = torch.empty(0, top_k, dtype=torch.int32, device=dev)
        hist = ops.HistoryIndex(hptr if n else np.zeros(2, dtype=np.int64), hflat, dev, n_items=self.num_items)
        rows = torch.arange(n, dtype=torch.int64, device=dev)                  # row b's history is segment b
        idx, val, cnt, mean = self.history_support_device(rows, lists, hist, top=int(top), space=space)
        return HistorySupport(lists.cpu(), idx.cpu(), val.cpu(), cnt.cpu(), mean.cpu())

    def recommend_diverse(self, user_ids, k, pool=None, lam=0.7, space="fused", exclude=None):
        """k items per user from the user's top-`pool` list, trading relevance against similarity to what is already picked
        (greedy MMR, rerank_device): CPU (ids int32 [B x k], scores fp32 [B x k]) in pick order -- scores are the model's scores
        of the picked items under the current predict type. One predict_device(top_k=pool) call and one re-rank launch. pool
        defaults to min(4 k, 256, num_items); lam in [0, 1]: 1 = the plain top-k, 0 = similarity alone; space as similar_items;
        `exclude` = dict user -> item ids left out of the ranking, as explain() takes it. -1 / -inf where a user has fewer than k
        items left."""
        k = int(k)
        pool = min(4 * k, ops.MMR_MAX_POOL, self.num_items) if pool is None else int(pool)
        if not 1 <= k <= pool <= min(ops.MMR_MAX_POOL, self.num_items):
            raise ValueError("need 1 <= k <= pool <= min(%d, num_items = %d), got k %d, pool %d"
                             % (ops.MMR_MAX_POOL, self.num_items, k, pool))
        lam = float(lam)
        if not 0.0 <= lam <= 1.0:
            raise ValueError("lam must lie in [0, 1], got %r" % lam)
        self._neighbour_space(space)
        tptr, tflat = self._excluded(exclude, user_ids, "item")
        dev = self._cached_tables("rerank_device() / recommend_diverse() need", "re-ranking needs the whole cached item table on this "
                                  "rank; the tables are item-sharded (lean / multi-rank evaluation)")
        n = len(user_ids)
        if not n:
            return torch.empty(0, k, dtype=torch.int32), torch.empty(0, k, dtype=torch.float32)
        masked = (torch.from_numpy(tptr).to(dev), torch.from_numpy(tflat.astype(np.int32)).to(dev)) if tflat.size else (None, None)
        idx, val = self.predict_device(user_ids, top_k=pool, train_ptr=masked[0], train_items=masked[1])
        out_idx, out_pos, _ = self.rerank_device(idx, val, k, lam, space=space)
        scores = torch.gather(val, 1, out_pos.clamp(min=0).long()).masked_fill_(out_pos < 0, float("-inf"))
        return out_idx.cpu(), scores.cpu()

    @torch.no_grad()
    def calibrate_device(self, lists_idx, lists_val, k, lam, class_of, targets, smooth=0.01, out_idx=None, out_pos=None, out_val=None):
        """Calibrated re-ranking of top-N pools (Steck, "Calibrated recommendations", RecSys 2018): k items per pool whose mix of
        item classes follows the row's target mix, ONE launch (csrc/calibrate.hip). lists_idx int32 / lists_val float32 [B x N] on
        the device (predict_device(top_k=N) gives both), 1 <= k <= N <= ops.MMR_MAX_POOL; class_of int32 [num_items] on the device:
        every item's class in [0, C), C <= ops.CALIBRATE_MAX_CLASSES; targets float32 [B x C]: the class shares to aim at. An entry
        outside the catalogue, with a score that is not finite (the -1 / -inf fillers) or with a class outside [0, C) is never
        picked. With the pool's scores scaled to rel in [0, 1], step t takes the item with the largest
        lam * rel - (1 - lam) * KL(targets || smoothed class shares of the picks so far plus the item), in float64, the lowest pool
        position among equals. lam weighs the RELEVANCE, as in rerank_device -- Steck's lambda weighs the calibration term --:
        lam = 1 keeps the pool's order, lam = 0 follows the targets alone. -> (out_idx int32 [B x k] the picked items, out_pos int32
        their pool positions, out_val float32 their objectives), -1 / -1 / -inf once no listed item is left; allocated here unless
        given. It reads no cached table itself."""
        dev = self._require_gpu()
        B, k = lists_idx.shape[0], int(k)
        if out_idx is None:
            out_idx = torch.empty(B, k, dtype=torch.int32, device=dev)
        if out_pos is None:
            out_pos = torch.empty(B, k, dtype=torch.int32, device=dev)
        if out_val is None:
            out_val = torch.empty(B, k, dtype=torch.float32, device=dev)
        ops.calibrate_rerank(lists_idx, lists_val, class_of, targets, k, lam, out_idx, out_pos, out_val, smooth=smooth)
        return out_idx, out_pos, out_val

    def recommend_calibrated(self, user_ids, k, classes, pool=None, lam=0.5, targets=None, smooth=0.01, exclude=None):
        """k items per user from the user's top-`pool` list whose mix of item classes follows the user's own (greedy calibrated
        re-ranking, calibrate_device): CPU (ids int32 [B x k], scores fp32 [B x k], kl fp32 [B]) -- ids in pick order, scores the
        model's scores of the picked items under the current predict type, kl the returned list's miscalibration C_KL against the
        user's target (ops.list_calibration). One predict_device(top_k=pool) call, one re-rank launch. classes: int array
        [num_items] with values in [0, C), C <= ops.CALIBRATE_MAX_CLASSES (reports.item_classes gives the popularity buckets);
        targets: float array [B x C], default the class shares of each user's training items (one ops.class_shares launch); pool
        defaults to min(4 k, 256, num_items); lam in [0, 1] weighs the RELEVANCE (1 = the plain top-k, 0 = the targets alone;
        Steck's lambda weighs the calibration term); 0 < smooth < 1; `exclude` = dict user -> item ids left out of the ranking, as
        explain() takes it. -1 / -inf where a user has fewer than k items left."""
        k = int(k)
        pool = min(4 * k, ops.MMR_MAX_POOL, self.num_items) if pool is None else int(pool)
        if not 1 <= k <= pool <= min(ops.MMR_MAX_POOL, self.num_items):
            raise ValueError("need 1 <= k <= pool <= min(%d, num_items = %d), got k %d, pool %d"
                             % (ops.MMR_MAX_POOL, self.num_items, k, pool))
        lam, smooth = float(lam), float(smooth)
        if not 0.0 <= lam <= 1.0:
            raise ValueError("lam must lie in [0, 1], got %r" % lam)
        if not 0.0 < smooth < 1.0:
            raise ValueError("smooth must lie in (0, 1), got %r" % smooth)
        classes = np.asarray(classes)
        if classes.ndim != 1 or classes.shape[0] != self.num_items or classes.dtype.kind not in "iu":
            raise ValueError("classes must be an integer array with one class per item (%d)" % self.num_items)
        max_c = ops.CALIBRATE_MAX_CLASSES
        if classes.size and not 0 <= int(classes.min()) <= int(classes.max()) < max_c:
            raise ValueError("classes must lie in [0, C) with C <= %d, got [%d, %d]" % (max_c, int(classes.min()), int(classes.max())))
        C = int(classes.max()) + 1 if classes.size else 1
        n = len(user_ids)
        if targets is not None:
            targets = np.asarray(targets, dtype=np.float32)
            if targets.ndim != 2 or targets.shape[0] != n or not C <= targets.shape[1] <= max_c:
                raise ValueError("targets must be [%d users x C], %d <= C <= %d, got %s" % (n, C, max_c, tuple(targets.shape)))
            C = targets.shape[1]
        tptr, tflat = self._excluded(exclude, user_ids, "item")
        if targets is None:
            train = self.dataset.get_user_train_dict()
            hptr, hflat, _ = self._id_lists([train.get(int(u), []) for u in user_ids], "training item")
        dev = self._cached_tables("calibrate_device() / recommend_calibrated() need", "calibrated re-ranking needs the whole cached item "
                                  "table on this rank; the tables are item-sharded (lean / multi-rank evaluation)")
        if not n:
            return torch.empty(0, k, dtype=torch.int32), torch.empty(0, k, dtype=torch.float32), torch.empty(0, dtype=torch.float32)
        class_of = torch.from_numpy(classes.astype(np.int32)).to(dev)
        if targets is None:
            targets_t = ops.class_shares(torch.from_numpy(hptr).to(dev), torch.from_numpy(hflat.astype(np.int32)).to(dev), class_of, C,
                                         torch.empty(n, C, dtype=torch.float32, device=dev))
        else:
            targets_t = torch.from_numpy(np.ascontiguousarray(targets)).to(dev)
        masked = (torch.from_numpy(tptr).to(dev), torch.from_numpy(tflat.astype(np.int32)).to(dev)) if tflat.size else (None, None)
        idx, val = self.predict_device(user_ids, top_k=pool, train_ptr=masked[0], train_items=masked[1])
        out_idx, out_pos, _ = self.calibrate_device(idx, val, k, lam, class_of, targets_t, smooth=smooth)
        scores = torch.gather(val, 1, out_pos.clamp(min=0).long()).masked_fill_(out_pos < 0, float("-inf"))
        kl = torch.empty(n, dtype=torch.float32, device=dev)
        ops.list_calibration(out_idx, class_of, C, torch.empty(n, C, dtype=torch.float32, device=dev), target=targets_t, smooth=smooth,
                             out_kl=kl)
        return out_idx.cpu(), scores.cpu(), kl.cpu()

    # ------------------------------------------------------------------ cold start: items folded in from content
    def _new_item_inputs(self, features, id_rows, normalized):
        """The host checks of fold_in_items, all before anything touches the device: ({letter: float32 [Q x D_m] host tensor,
        normalised as the model's own buffer is}, id rows float32 [Q x d], Q)."""
        if not isinstance(features, dict) or set(features) != set(self._mods):
            raise ValueError("features must be a dict with exactly the heads %s, got %s"
                             % ("/".join(self._mods), sorted(features) if isinstance(features, dict) else type(features).__name__))

        def host(x, what, width):
            t = x.detach().cpu() if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))
            if not t.is_floating_point() or t.dim() != 2 or t.shape[1] != width:
                raise ValueError("%s must be a float array [Q x %d], got %s %s" % (what, width, t.dtype, tuple(t.shape)))
            t = t.float().contiguous()
            if not bool(torch.isfinite(t).all()):
                raise ValueError("%s holds an entry that is not finite" % what)
            return t

        feats, Q = {}, None
        for m in self._mods:
            t = host(features[m], "features[%r]" % m, getattr(self, m + "_dense").weight.shape[1])
            if Q is not None and t.shape[0] != Q:
                raise ValueError("features[%r] has %d rows, the other heads have %d" % (m, t.shape[0], Q))
            Q = t.shape[0]
            word_bag = m == "t" and self.dataset_name == "tiktok" and "feature_modalities" not in self.config
            feats[m] = t if normalized or word_bag else F.normalize(t, dim=1).contiguous()     # (:377-378: the word bag stays as it is)
        ids = torch.zeros(Q, self.latent_dim) if id_rows is None else host(id_rows, "id_rows", self.latent_dim)
        if ids.shape[0] != Q:
            raise ValueError("id_rows has %d rows, the features have %d" % (ids.shape[0], Q))
        return feats, ids, Q

    def _whole_tables(self, what):
        """_cached_tables for the cold-start readers: single GPU, whole tables -- lean and item-sharded tables are refused."""
        msg = self._refuse_partial_tables(what)
        return self._cached_tables(what + " needs", msg)

    def _refuse_partial_tables(self, what):
        """The refusal of lean / wide / item-sharded tables alone (no table is built or read) -> the refusal's words."""
        msg = "%s needs the whole cached tables on this rank; the tables are item-sharded or lean" % what
        if self.__dict__.get("_lean") or self.__dict__.get("_wide") or self.__dict__.get("_eval_shard") is not None:
            raise CandidateScoringError(msg)
        return msg

    def _check_new(self, new):
        if not isinstance(new, NewItems) or new.num_users != self.num_users:
            raise TypeError("`new` must be the NewItems handle of this model's fold_in_items()")
        if new.n_items and new.version != getattr(self, "_table_version", 0):
            raise RuntimeError("the cached tables changed since these items were folded in (table version %d, now %d): "
                               "call fold_in_items() again" % (new.version, getattr(self, "_table_version", 0)))

    @torch.no_grad()
    def fold_in_items(self, features, id_rows=None, normalized=False):
        """Items that arrived after the graph was built, from their content alone -> NewItems (rows the cached item table would
        hold for them, on the device). features: dict head letter -> float [Q x D_m], exactly the letters of self._mods;
        normalized=False row-normalises them as the model normalises its own buffers (F.normalize, eps 1e-12; tiktok's word-bag
        t_feat is left alone), True takes every row as given. id_rows [Q x d] or None = zeros: a new item has no trained id row.
        A node without edges has the closed-form layer mean kappa x0 (reports.isolated_row_scale), so Out_m = (kappa F_m) W_m^T +
        kappa b_m and the id block = kappa id_rows; Y_new = the item fusion Linear on Out, plus the s_dense heads on its blocks --
        two ops.linear_fwd_batched calls with the weights the cached tables were built with (after a training step: the copy
        taken before the update). A row depends on its own inputs only. The checks and the normalisation run on the host, as the
        model's own buffers are normalised there: device inputs come down for them and go up again (one round trip of Q rows). ValueError for a missing / extra head, a wrong width or a non-finite entry, before anything touches the device;
        Q = 0 gives an empty handle without a launch."""
        from .reports import isolated_row_scale
        feats, ids, Q = self._new_item_inputs(features, id_rows, normalized)
        U, d, Cy = self.num_users, self.latent_dim, self.Cy
        if Q == 0:
            dev = self._require_gpu()
            return NewItems(torch.empty(0, Cy, dtype=torch.float32, device=dev), None, None, getattr(self, "_table_version", 0), U)
        dev = self._whole_tables("fold_in_items()")
        W = self.__dict__.get("_table_W")
        if W is None:                 # (tables put there by hand, not by a forward of this model)
            raise RuntimeError("fold_in_items() needs the weights the cached tables were built with: call bpr_loss or compute() first")
        kappa = isolated_row_scale(str(self.config["adj_type"]), self.n_layers)
        f32 = dict(dtype=torch.float32, device=dev)
        out = torch.empty(Q, self.C, **f32)
        out[:, :d] = ids.to(dev) * kappa
        scale = torch.full((Q,), kappa, **f32)
        zero = torch.zeros(Q, d, **f32)
        ops.linear_fwd_batched([((feats[m].to(dev) * kappa).contiguous(), W[m + "_dense.weight"], W[m + "_dense.bias"],
                                 out[:, (k + 1) * d:(k + 2) * d], scale, zero) for k, m in enumerate(self._mods)])
        Y = self._ws["Y"]
        table = torch.empty(U + Q, Cy, **f32)
        table[:U] = Y[:U]
        rows = table[U:]
        wi = self._fusion_weights(W)[1]
        head = [(out, wi, W["embedding_item_after_GCN.bias"], rows[:, :d])]
        for h, m in enumerate(self._mods):
            blk = slice((h + 1) * d, (h + 2) * d)
            head.append((out[:, blk], W["s_dense_%s.weight" % m], W["s_dense_%s.bias" % m], rows[:, blk]))
        ops.linear_fwd_batched(head)
        sqn = ops.row_sqnorms(table, d, 1 + self.S, torch.empty(U + Q, 1 + self.S, **f32))
        return NewItems(rows, table, sqn, self._table_version, U)

    @torch.no_grad()
    def predict_new_items_device(self, users, new, out):
        """out [B x Q] (float32, unit column stride, on the device) <- every user's score of every new item under the current
        predict type and fusion mode. The scorer predict_device runs, over the handle's table ([the users' rows ; the new rows]) as
        ONE item shard of Q items (ops.score_topk_shard, phase 2): a folded copy of a catalogue item scores bit for bit what
        predict() holds in the item's column. TIE's catalogue mean comes from the scorer's pass 1 over the TRAINED catalogue of
        num_items items: the new items are not in it."""
        self._check_new(new)
        dev = self._whole_tables("predict_new_items()")
        users = torch.as_tensor(users, device=dev).long().contiguous()
        B, Q = users.numel(), new.n_items
        if not B or not Q:
            return out
        if tuple(out.shape) != (B, Q):
            raise ValueError("out must be [%d x %d]" % (B, Q))
        if ops.PREDICT_TYPES.get(self.predict_type, 0) == 2:
            row_sum = self._catalogue_row_sum(dev, users, self.predict_type, self._block_sqnorms(dev))
        else:
            row_sum = torch.zeros(B, dtype=torch.float32, device=dev)
        need = ops.score_workspace(B, self.num_users, Q, self.S, 1, topk_only=False, d=self.latent_dim)
        if self._ws.get("new_score_ws") is None or self._ws["new_score_ws"].numel() < need:
            self._ws["new_score_ws"] = torch.empty(need, dtype=torch.uint8, device=dev)
        ops.score_topk_shard(new.table, self.num_users, Q, users, self.latent_dim, self.S, self._head_mask(), self.fusion_mode,
                             self.predict_type, self._ws["new_score_ws"], 2, row_sum, self.num_items, 0, scores=out, sqnorm=new.sqn)
        return out

    def predict_new_items(self, user_ids, new):
        """Scores of the new items: CPU fp32 [len(user_ids) x Q] -- what predict() would hold in the items' columns had they been
        in the catalogue without an edge."""
        dev = self._require_gpu()
        ids = self._id_lists([user_ids], "user", self.num_users)[1]
        out = torch.empty(ids.size, len(new), dtype=torch.float32, device=dev)
        return self.predict_new_items_device(torch.from_numpy(ids).to(dev), new, out).cpu()

    def audience_new_items(self, new, k, exclude=None):
        """audience() of the new items: Audience(users CPU int32 [Q x k], scores CPU fp32 [Q x k]) by (score descending, user id
        ascending) under the current predict type; `exclude` = dict new item q -> user ids to leave out. 1 <= k <= 256."""
        k = int(k)
        if not 1 <= k <= ops.AUDIENCE_MAX_K:
            raise ValueError("k must lie in [1, %d]" % ops.AUDIENCE_MAX_K)
        self._check_new(new)
        Q, U = new.n_items, self.num_users
        ptr, flat = self._excluded(exclude, range(Q), "user", U)
        if not Q:
            return Audience(torch.empty(0, k, dtype=torch.int32), torch.empty(0, k, dtype=torch.float32))
        dev = self._whole_tables("audience_new_items()")
        query = ops.AudienceQuery(np.arange(Q, dtype=np.int64), Q, U, dev, ptr if flat.size else None, flat if flat.size else None)
        idx = torch.empty(Q, k, dtype=torch.int32, device=dev)
        val = torch.empty(Q, k, dtype=torch.float32, device=dev)
        tie = ops.PREDICT_TYPES.get(self.predict_type, 0) == 2
        row_sum = self._audience_row_sum(dev, self._block_sqnorms(dev)) if tie else None
        ops.audience_topk(new.table, U, Q, query, self.latent_dim, self.S, self._head_mask(), self.fusion_mode, self.predict_type, k,
                          idx, val, sqnorm=new.sqn, row_sum=row_sum, I_total=self.num_items)
        return Audience(idx.cpu(), val.cpu())

    NEW_ITEM_QUERY_BLOCK = 64                # new rows per cosine_topk call of similar_to_new_items

    def similar_to_new_items(self, new, k, space="fused"):
        """The k CATALOGUE items closest to each new item by cosine: Neighbours(ids CPU int32 [Q x k], scores CPU fp32 [Q x k]) by
        (score descending, id ascending); space as similar_items. ops.cosine_topk over [the catalogue's block ; a block of new rows]
        with the new rows as the queries, each leaving out every new row of its block."""
        k = int(k)
        if not 1 <= k <= ops.KNN_MAX_K:
            raise ValueError("k must lie in [1, %d]" % ops.KNN_MAX_K)
        h = self._neighbour_space(space)
        self._check_new(new)
        Q, U, I, d = new.n_items, self.num_users, self.num_items, self.latent_dim
        if not Q:
            return Neighbours(torch.empty(0, k, dtype=torch.int32), torch.empty(0, k, dtype=torch.float32))
        dev = self._whole_tables("similar_to_new_items()")
        sqn = self._block_sqnorms(dev)
        nb = self.NEW_ITEM_QUERY_BLOCK
        table = torch.empty(I + nb, d, dtype=torch.float32, device=dev)
        norms = torch.empty(I + nb, dtype=torch.float32, device=dev)
        table[:I] = self._ws["Y"][U:, h * d:(h + 1) * d]
        norms[:I] = sqn[U:, h]
        idx = torch.empty(Q, k, dtype=torch.int32, device=dev)
        val = torch.empty(Q, k, dtype=torch.float32, device=dev)
        for a in range(0, Q, nb):
            n = min(nb, Q - a)
            table[I:I + n] = new.rows[a:a + n, h * d:(h + 1) * d]
            norms[I:I + n] = new.sqn[U + a:U + a + n, h]
            block = np.arange(I, I + n, dtype=np.int64)
            query = ops.NeighbourQuery(block, I + n, dev, np.arange(n + 1, dtype=np.int64) * n, np.tile(block, n))
            ops.cosine_topk(table[:I + n], norms[:I + n], query, k, idx[a:a + n], val[a:a + n], exclude_self=True)
        return Neighbours(idx.cpu(), val.cpu())

    def _train_mask(self, exclude, user_ids, dev):
        tptr, tflat = self._excluded(exclude, user_ids, "item")
        return (torch.from_numpy(tptr).to(dev), torch.from_numpy(tflat.astype(np.int32)).to(dev)) if tflat.size else (None, None)

    RECOMMEND_MAX_K = 256                    # the longest list recommend_with_new merges (2 k candidates per row in topk_merge's LDS)

    def recommend_with_new(self, user_ids, new, k, exclude=None):
        """Each user's top-k over the catalogue AND the new items: CPU (ids int32 [B x k], scores fp32 [B x k]) by (score
        descending, id ascending), new item q under id num_items + q; `exclude` = dict user -> catalogue item ids left out, as
        explain() takes it. The user's catalogue top-k (predict_device) merged with its best min(k, Q) new items (a stable sort
        of predict_new_items_device's block) by ops.topk_merge. 1 <= k <= min(RECOMMEND_MAX_K = 256, num_items). A user whose
        unmasked catalogue is shorter than k gets masked items at -inf from predict_device: they are no candidates of the merge,
        so new items take those places, and -1 / -inf remain only where catalogue and new items together are fewer than k."""
        k = int(k)
        if not 1 <= k <= min(self.RECOMMEND_MAX_K, self.num_items):
            raise ValueError("k must lie in [1, %d]" % min(self.RECOMMEND_MAX_K, self.num_items))
        self._check_new(new)
        ids = self._id_lists([user_ids], "user", self.num_users)[1]
        dev = self._require_gpu()
        masked = self._train_mask(exclude, ids, dev)
        B, Q = ids.size, new.n_items
        if not B:
            return torch.empty(0, k, dtype=torch.int32), torch.empty(0, k, dtype=torch.float32)
        self._whole_tables("recommend_with_new()")
        users = torch.from_numpy(ids).to(dev)
        idx, val = self.predict_device(users, top_k=k, train_ptr=masked[0], train_items=masked[1])
        idx = idx.masked_fill(val == float("-inf"), -1)          # a masked item behind a short catalogue is no candidate
        if not Q:
            return idx.cpu(), val.cpu()
        block = self.predict_new_items_device(users, new, torch.empty(B, Q, dtype=torch.float32, device=dev))
        kq = min(k, Q)
        nval, nidx = torch.sort(block, dim=1, descending=True, stable=True)     # equal scores keep q ascending
        cand_val = torch.cat((val, nval[:, :kq]), dim=1).contiguous()
        cand_idx = torch.cat((idx, (nidx[:, :kq] + self.num_items).int()), dim=1).contiguous()
        out_idx = torch.empty(B, k, dtype=torch.int32, device=dev)
        out_val = torch.empty(B, k, dtype=torch.float32, device=dev)
        ops.topk_merge(cand_val, cand_idx, k, out_idx, out_val)
        return out_idx.cpu(), out_val.cpu()

    RANK_BLOCK_BYTES = 2 << 30               # the [users x items] score block of rank_new_items stays within it (RankReport.block_bytes)

    @torch.no_grad()
    def rank_new_items_device(self, users, new, train_ptr=None, train_items=None, skip=None, among=False):
        """Where every new item would land in each user's FULL ranking: int32 [B x Q] on the device, rank[b, q] = the number of
        catalogue items user b scores at least as high as new item q (the new item goes behind equal scores: its id is the larger
        one), the train items (CSR on the device) masked. One predict_device call into a [B x I] block, predict_new_items_device,
        then ops.rank_values (csrc/coldstart.hip). skip: int [Q] (host), per new item a catalogue column that is not counted (its
        own entry when a catalogue item was folded in again; -1: none). among: add the number of OTHER new items that beat q by
        (score descending, q ascending)."""
        self._check_new(new)
        dev = self._whole_tables("rank_new_items()")
        users = torch.as_tensor(users, device=dev).long().contiguous()
        B, Q, I = users.numel(), new.n_items, self.num_items
        rank = torch.empty(B, Q, dtype=torch.int32, device=dev)
        if skip is not None:
            skip = np.asarray(skip).reshape(-1)
            if skip.size != Q or skip.dtype.kind not in "iu" or (skip.size and (skip.min() < -1 or skip.max() >= I)):
                raise IndexError("skip needs one catalogue column in [0, %d) or -1 per new item (%d)" % (I, Q))
        if not B or not Q:
            return rank
        lds = (I + 3) // 4 * 4                    # rows 16-byte aligned: the count takes its 16-byte loads
        block = torch.empty(B, lds, dtype=torch.float32, device=dev)[:, :I]
        self.predict_device(users, scores=block, train_ptr=train_ptr, train_items=train_items)
        vals = self.predict_new_items_device(users, new, torch.empty(B, Q, dtype=torch.float32, device=dev))
        val_ptr = np.arange(B + 1, dtype=np.int64) * Q
        ops.rank_values(block, val_ptr, vals.view(-1), rank.view(-1), skip=None if skip is None else np.tile(skip.astype(np.int32), B))
        if among:
            order = torch.sort(vals, dim=1, descending=True, stable=True)[1]
            place = torch.empty_like(order)
            place.scatter_(1, order, torch.arange(Q, device=dev).expand(B, Q).contiguous())
            rank += torch.where(rank >= 0, place.int(), torch.zeros_like(rank))
        return rank

    def rank_new_items(self, user_ids, new, exclude=None, among=False):
        """The catalogue rank every new item would take: CPU int32 [len(user_ids) x Q], 0-based, under the current predict type;
        `exclude` = dict user -> item ids masked out of the ranking (the train items, as rank_items takes it). Users go in blocks
        whose score block stays within RANK_BLOCK_BYTES. among=True counts the other new items ranked above it as well."""
        self._check_new(new)
        ids = self._id_lists([user_ids], "user", self.num_users)[1]
        tptr, tflat = self._excluded(exclude, ids, "item")
        dev = self._require_gpu()
        out = torch.empty(ids.size, len(new), dtype=torch.int32)
        step = max(1, int(self.RANK_BLOCK_BYTES) // ((self.num_items + 3) // 4 * 16))
        for a in range(0, ids.size, step):
            b = min(a + step, ids.size)
            masked = (None, None)
            if tptr[b] > tptr[a]:
                masked = (torch.from_numpy(tptr[a:b + 1] - tptr[a]).to(dev),
                          torch.from_numpy(tflat[tptr[a]:tptr[b]].astype(np.int32)).to(dev))
            out[a:b] = self.rank_new_items_device(torch.from_numpy(ids[a:b]).to(dev), new, masked[0], masked[1], among=among).cpu()
        return out

    # ------------------------------------------------------------------ cold start: users folded in from their histories
    def _item_degree(self):
        """Training interactions per item (int64 [num_items], host): the degree the frozen adjacency gives an item."""
        deg = self.__dict__.get("_item_train_degree")
        if deg is None:
            from .reports import item_train_counts
            deg = self._item_train_degree = item_train_counts(self.dataset.get_user_train_dict(), self.num_items)
        return deg

    def _new_user_inputs(self, histories, id_rows):
        """The host checks of fold_in_users, all before anything touches the device: (hist_ptr int64, hist_items int64, the id rows
        as a float32 [Q x d] host tensor, None (no id term) or "mean")."""
        if isinstance(histories, (str, bytes, dict)) or not hasattr(histories, "__len__"):
            raise TypeError("histories must be a list of item id lists, got %s" % type(histories).__name__)
        ptr, flat, _ = self._id_lists(list(histories), "history item")
        Q = len(histories)
        if id_rows is None or (isinstance(id_rows, str) and id_rows == "mean"):
            return ptr, flat, id_rows
        if isinstance(id_rows, str):
            raise ValueError("id_rows must be None, 'mean' or a float array [Q x %d], got %r" % (self.latent_dim, id_rows))
        t = id_rows.detach().cpu() if isinstance(id_rows, torch.Tensor) else torch.from_numpy(np.asarray(id_rows))
        if not t.is_floating_point() or t.dim() != 2 or tuple(t.shape) != (Q, self.latent_dim):
            raise ValueError("id_rows must be a float array [%d x %d], got %s %s" % (Q, self.latent_dim, t.dtype, tuple(t.shape)))
        t = t.float().contiguous()
        if not bool(torch.isfinite(t).all()):
            raise ValueError("id_rows holds an entry that is not finite")
        return ptr, flat, t

    def _check_new_users(self, new):
        if not isinstance(new, NewUsers) or new.num_items != self.num_items or new.num_users != self.num_users:
            raise TypeError("`new` must be the NewUsers handle of this model's fold_in_users()")
        if new.n_users and new.version != getattr(self, "_table_version", 0):
            raise RuntimeError("the cached tables changed since these users were folded in (table version %d, now %d): "
                               "call fold_in_users() again" % (new.version, getattr(self, "_table_version", 0)))

    def mean_user_id_row(self):
        """The mean embedding_user row of the users that have a training interaction (float64 mean, rounded once): float32 [d] on
        the parameters' device -- what fold_in_users(id_rows="mean") gives every new user as its id row."""
        self.plugin.sync_params()
        w = self.embedding_user.weight.detach()
        train = self.dataset.get_user_train_dict()
        active = np.asarray(sorted(int(u) for u, items in train.items() if len(items) and 0 <= int(u) < self.num_users), dtype=np.int64)
        if not active.size:
            return w.new_zeros(w.shape[1])
        return w[torch.from_numpy(active).to(w.device)].double().mean(0).float()

    @torch.no_grad()
    def fold_in_users(self, histories, id_rows=None):
        """Users that arrived after the graph was built, from the items they took -> NewUsers (the rows the cached user table would
        hold for them, on the device). histories: one list of catalogue item ids per user; repeats count as given. The graph stays
        frozen -- no other node's row changes -- and with Out the cached layer-mean table
            OutNew[q] = kappa x0_q + sum_{i in H_q} w_qi Out[U + i]          (ops.segment_row_sum, csrc/foldin.hip: float64 sums)
        with w_qi the off-diagonal entry the adjacency would give the edge (reports.fold_in_weights: the item's TRAINING degree, the
        user's degree = len(H_q)), kappa = reports.isolated_row_scale and x0_q = id_rows[q] in every block. id_rows: None (no id
        term), a float [Q x d], or "mean" = mean_user_id_row(). With id_rows=None this is the mean of the user's layers 1 .. L + 1 in
        the graph extended by that one row -- the neighbourhood aggregate of the history's layer means -- NOT the row training would
        give: layer 0 is unknown for a new user and layer L + 1 takes its place. Y_new = the USER fusion Linear on OutNew plus the
        s_dense heads on its blocks: one ops.linear_fwd_batched call with the weights the cached tables were built with. An empty
        history is allowed: its OutNew row is kappa x0, and with no id_rows its fused block and its heads come from the biases
        alone (every such user gets the same scores, those of the biases' row against each item row: one ranking for all of them,
        not a constant score). A row depends
        on its own history only: one user or a batch of 8192, the same bits. IndexError for an id outside the catalogue,
        ValueError for id_rows of a wrong shape or with a non-finite entry, both before anything touches the device; Q = 0 gives an
        empty handle without a launch."""
        from .reports import fold_in_weights, isolated_row_scale
        ptr, flat, ids = self._new_user_inputs(histories, id_rows)
        U, I, d, Cy = self.num_users, self.num_items, self.latent_dim, self.Cy
        Q = int(ptr.size - 1)
        if Q == 0:
            dev = self._require_gpu()
            self._refuse_partial_tables("fold_in_users()")          # (an empty request is refused like any other; nothing is launched)
            return NewUsers(torch.empty(0, Cy, dtype=torch.float32, device=dev), None, None, getattr(self, "_table_version", 0), U, I,
                            ptr, flat, None, None)
        adj_type = str(self.config["adj_type"])
        weights = fold_in_weights(adj_type, ptr, flat, self._item_degree())
        dev = self._whole_tables("fold_in_users()")
        W = self.__dict__.get("_table_W")
        if W is None:                 # (tables put there by hand, not by a forward of this model)
            raise RuntimeError("fold_in_users() needs the weights the cached tables were built with: call bpr_loss or compute() first")
        f32 = dict(dtype=torch.float32, device=dev)
        hist_ptr = torch.from_numpy(ptr).to(dev)
        hist_items = ops._resident_ids(flat, dev)
        out = torch.empty(Q, self.C, **f32)
        ops.segment_row_sum(self._ws["Out"], ptr, flat.astype(np.int32), weights, out, row_offset=U)
        if ids is not None:
            x0 = self.mean_user_id_row().to(dev).expand(Q, -1) if isinstance(ids, str) else ids.to(dev)
            out += (x0 * isolated_row_scale(adj_type, self.n_layers)).repeat(1, self.C // d)
        table = torch.empty(Q + I, Cy, **f32)
        table[Q:] = self._ws["Y"][U:]
        rows = table[:Q]
        wu = self._fusion_weights(W)[0]
        head = [(out, wu, W["embedding_user_after_GCN.bias"], rows[:, :d])]
        for h, m in enumerate(self._mods):
            blk = slice((h + 1) * d, (h + 2) * d)
            head.append((out[:, blk], W["s_dense_%s.weight" % m], W["s_dense_%s.bias" % m], rows[:, blk]))
        ops.linear_fwd_batched(head)
        sqn = ops.row_sqnorms(table, d, 1 + self.S, torch.empty(Q + I, 1 + self.S, **f32))
        return NewUsers(rows, table, sqn, self._table_version, U, I, ptr, flat, hist_ptr, hist_items, layer_mean=out)

    def _new_user_scores(self, new, scores=None, top_k=0, train_ptr=None, train_items=None, tie_order="id"):
        """The evaluator's scorer (ops.score_topk, what predict_device runs) over the handle's table with U := Q and the users
        0 .. Q - 1 -> (idx, val) [Q x top_k] or (None, None). Under TIE the catalogue mean is the scorer's own pass 1 over the
        trained catalogue, the item rows of the table."""
        self._check_new_users(new)
        dev = self._whole_tables("the readers of fold_in_users()")
        Q, I = new.n_users, self.num_items
        users = torch.arange(Q, dtype=torch.int64, device=dev)
        need = ops.score_workspace(Q, Q, I, self.S, max(top_k, 1), topk_only=scores is None and top_k > 0, d=self.latent_dim)
        if self._ws.get("new_user_score_ws") is None or self._ws["new_user_score_ws"].numel() < need:
            self._ws["new_user_score_ws"] = torch.empty(need, dtype=torch.uint8, device=dev)
        idx = val = None
        if top_k:
            idx = torch.empty(Q, top_k, dtype=torch.int32, device=dev)
            val = torch.empty(Q, top_k, dtype=torch.float32, device=dev)
        ops.score_topk(new.table, Q, I, users, self.latent_dim, self.S, self._head_mask(), self.fusion_mode, self.predict_type,
                       self._ws["new_user_score_ws"], scores=scores, K=top_k, topk_idx=idx, topk_val=val, train_ptr=train_ptr,
                       train_items=train_items, sqnorm=new.sqn, tie_order=tie_order)
        return idx, val

    @torch.no_grad()
    def predict_new_users_device(self, new, out):
        """out [Q x I] (float32, unit column stride, on the device) <- every new user's score of every catalogue item under the
        current predict type and fusion mode: bit for bit what predict() would give a trained user whose cached row is the
        handle's row."""
        self._check_new_users(new)
        if not new.n_users:
            return out
        if tuple(out.shape) != (new.n_users, self.num_items):
            raise ValueError("out must be [%d x %d]" % (new.n_users, self.num_items))
        self._new_user_scores(new, scores=out)
        return out

    def predict_new_users(self, new):
        """Scores of the new users: CPU fp32 [Q x I]."""
        dev = self._require_gpu()
        out = torch.empty(len(new), self.num_items, dtype=torch.float32, device=dev)
        return self.predict_new_users_device(new, out).cpu()

    def _new_user_mask(self, new, exclude_history, exclude, dev):
        """The items left out of each new user's ranking as CSR on the device, (None, None) when there are none: the history (the
        handle's resident lists when nothing else is excluded) and `exclude` = dict q -> item ids."""
        Q = new.n_users
        more = self._excluded(exclude, range(Q), "item") if exclude else None
        if more is None or not more[1].size:
            if not exclude_history or not new.hist_flat.size:
                return None, None
            return new.hist_ptr, new.hist_items
        lists = [np.concatenate((new.hist_flat[new.hist_ptr_host[q]:new.hist_ptr_host[q + 1]] if exclude_history else more[1][:0],
                                 more[1][more[0][q]:more[0][q + 1]])) for q in range(Q)]
        ptr, flat, _ = ops.ragged(lists, dtype=np.int32)
        return torch.from_numpy(ptr).to(dev), torch.from_numpy(flat).to(dev)

    @torch.no_grad()
    def recommend_new_users(self, new, k, exclude_history=True, exclude=None, tie_order="id"):
        """Each new user's top-k catalogue items: CPU (ids int32 [Q x k], scores fp32 [Q x k]) by (score descending, id ascending) --
        tie_order="reference": the evaluator's order among equal scores. exclude_history masks the user's history exactly as the
        evaluator masks train items (the scorer's train_ptr / train_items; an id listed twice is masked once); `exclude` = dict
        q -> further item ids. 1 <= k <= min(256, num_items)."""
        k = int(k)
        if not 1 <= k <= min(self.RECOMMEND_MAX_K, self.num_items):
            raise ValueError("k must lie in [1, %d]" % min(self.RECOMMEND_MAX_K, self.num_items))
        if tie_order not in ops.TIE_ORDERS:
            raise ValueError("tie_order must be id or reference")
        self._check_new_users(new)
        if not new.n_users:
            return torch.empty(0, k, dtype=torch.int32), torch.empty(0, k, dtype=torch.float32)
        dev = self._require_gpu()
        masked = self._new_user_mask(new, exclude_history, exclude, dev)
        idx, val = self._new_user_scores(new, top_k=k, train_ptr=masked[0], train_items=masked[1], tie_order=tie_order)
        return idx.cpu(), val.cpu()

    @torch.no_grad()
    def rank_items_for_new_users(self, new, items, exclude_history=True):
        """The exact catalogue rank of given items for each new user: CPU int32 [Q x longest list], row q = the 0-based positions of
        items[q] in user q's full ranking under the current predict type, padded with -1 -- rank_items over the handle: the scorer's
        block with the history masked (exclude_history), then ops.rank_targets; an item that is itself masked gets -1."""
        self._check_new_users(new)
        Q, I = new.n_users, self.num_items
        if len(items) != Q:
            raise ValueError("one item list per user: %d lists for %d users" % (len(items), Q))
        ptr, flat, lens = self._id_lists(items, "item")
        rank = np.zeros(0, dtype=np.int32)
        if flat.size:
            dev = self._require_gpu()
            index = ops.TargetIndex(ptr, flat.astype(np.int32), Q, I, dev)
            masked = self._new_user_mask(new, exclude_history, None, dev)
            lds = (I + 3) // 4 * 4                # rows 16-byte aligned: the count takes its 16-byte loads
            block = torch.empty(Q, lds, dtype=torch.float32, device=dev)[:, :I]
            self._new_user_scores(new, scores=block, train_ptr=masked[0], train_items=masked[1])
            rank = ops.rank_targets(block, index, None, torch.empty(index.n_targets, dtype=torch.int32, device=dev)).cpu().numpy()
        return torch.from_numpy(ops.ragged_padded(rank, lens))

    def similar_users_to_new(self, new, k, space="fused"):
        """The k TRAINED users closest to each new user by cosine: Neighbours(ids CPU int32 [Q x k], scores CPU fp32 [Q x k]) by
        (score descending, id ascending); space as similar_users. ops.cosine_topk over [the cached user rows' block ; a block of new
        rows] with the new rows as the queries, each leaving out every new row of its block."""
        k = int(k)
        if not 1 <= k <= ops.KNN_MAX_K:
            raise ValueError("k must lie in [1, %d]" % ops.KNN_MAX_K)
        h = self._neighbour_space(space)
        self._check_new_users(new)
        Q, U, d = new.n_users, self.num_users, self.latent_dim
        if not Q:
            return Neighbours(torch.empty(0, k, dtype=torch.int32), torch.empty(0, k, dtype=torch.float32))
        dev = self._whole_tables("similar_users_to_new()")
        sqn = self._block_sqnorms(dev)
        nb = self.NEW_ITEM_QUERY_BLOCK
        table = torch.empty(U + nb, d, dtype=torch.float32, device=dev)
        norms = torch.empty(U + nb, dtype=torch.float32, device=dev)
        table[:U] = self._ws["Y"][:U, h * d:(h + 1) * d]
        norms[:U] = sqn[:U, h]
        idx = torch.empty(Q, k, dtype=torch.int32, device=dev)
        val = torch.empty(Q, k, dtype=torch.float32, device=dev)
        for a in range(0, Q, nb):
            n = min(nb, Q - a)
            table[U:U + n] = new.rows[a:a + n, h * d:(h + 1) * d]
            norms[U:U + n] = new.sqn[a:a + n, h]
            block = np.arange(U, U + n, dtype=np.int64)
            query = ops.NeighbourQuery(block, U + n, dev, np.arange(n + 1, dtype=np.int64) * n, np.tile(block, n))
            ops.cosine_topk(table[:U + n], norms[:U + n], query, k, idx[a:a + n], val[a:a + n], exclude_self=True)
        return Neighbours(idx.cpu(), val.cpu())

    def predict(self, user_ids, candidate_items=None):
        """:96-113. CPU fp32 tensor [len(user_ids) x I]; `candidate_items` is ignored as in the reference."""
        dev = self._require_gpu()
        scores = torch.empty(len(user_ids), self.num_items, dtype=torch.float32, device=dev)
        self.predict_device(user_ids, scores=scores)
        return scores.cpu()
