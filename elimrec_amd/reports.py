"""The reports over the cached tables -- what the lists are made of (EffectReport), where the held-out items stand (RankReport),
whose neighbourhood the fused space copies (NeighbourReport), the lists themselves (ListReport), what diversifying them costs and
buys (DiversifyReport), whether they match each user's own popularity mix (CalibrationReport), which items of a user's history back
them (HistoryReport), how sure the evaluation metrics are
(SignificanceReport), what the learned cosine spaces themselves look like (GeometryReport), whether their neighbourhoods are the
training graph's co-interaction neighbourhoods (CoNeighbourReport) -- and what they share: the user /
item groups, the groups as a checked index on the device, the group means, the table format, the model preflight and the block-wise
top-K lists. The rows come from the model's *_device readers (model.py), the means from ops.group_metric_means."""
import collections

import numpy as np
import torch

from . import ops
from .data_iterator import DataIterator
from .ops import CandidateScoringError

ALL = "all:".ljust(12)


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


def item_train_counts(user_train_dict, num_items):
    """Training interactions per item: int64 [num_items] (an item listed twice by one user counts twice)."""
    counts = np.zeros(num_items, dtype=np.int64)
    for items in user_train_dict.values():
        np.add.at(counts, np.asarray(list(items), dtype=np.int64), 1)
    return counts


def lists_csr(keys, table, device, unique=False, cast=None):
    """table[k] (missing: empty) of every key as CSR on the device: (ptr int64 [n + 1], ids int32, unchecked); unique: each list's
    distinct ids in ascending order; cast: ops.ragged's."""
    lists = [sorted(set(table.get(k, []))) if unique else table.get(k, []) for k in keys]
    ptr, flat, _ = ops.ragged(lists, dtype=np.int32, cast=cast)
    return torch.from_numpy(ptr).to(device), torch.from_numpy(flat).to(device)


def group_index(positions, n_rows, device):
    """Groups given as arrays of row positions into a block of n_rows rows -> the checked ops.GroupIndex resident on `device`."""
    ptr, rows, _ = ops.ragged(positions, dtype=np.int32)
    return ops.GroupIndex(ptr, rows, n_rows, device)


def group_table(rows, index, n_groups):
    """Device rows [n x C] -> host float32 [n_groups x C]: the groups' column means (ops.group_metric_means)."""
    out = torch.empty(n_groups, rows.shape[1], dtype=torch.float32, device=rows.device)
    return ops.group_metric_means(rows, index, None, out).cpu().numpy()


def format_rows(labels, table):
    """One "\\n<label>\\t<%.8f values>" line per row (the reference's grouped_evaluator.py:107-112)."""
    return "".join("\n%s\t%s" % (label, "\t".join(("%.8f" % x).ljust(12) for x in row)) for label, row in zip(labels, table))


def format_table(columns, labels, table):
    """A header of column names and format_rows' lines."""
    return "columns:\t%s" % "\t".join(str(c).ljust(12) for c in columns) + format_rows(labels, table)


def isolated_row_scale(adj_type, L):
    """kappa: the layer mean of a node WITHOUT edges is kappa x0, as the propagation kernels evaluate it in float32 (pure host
    arithmetic). Adjacencies without a diagonal ('plain', 'gcmc', 'pre'): every hop gives the node a zero row, the mean is
    (x0 + 0) * inv with inv = 1.0f / (L + 1). 'norm' and 'mean' (anything else, as create_adj_mat reads it) give an isolated node
    the identity row, so the mean is the sum of L + 1 copies of x0 in hop order times inv. -> a Python float holding the float32."""
    L = int(L)
    if L < 0:
        raise ValueError("L must not be negative, got %d" % L)
    inv = np.float32(1.0) / np.float32(L + 1)
    if adj_type in ("plain", "gcmc", "pre"):
        return float(inv)
    acc = np.float32(1.0)
    for _ in range(L):
        acc = np.float32(acc + np.float32(1.0))
    return float(np.float32(acc * inv))


class _Report(object):
    """What the reports share. A subclass names itself (`name`: its word in the messages and its --<name>_report switch), the model
    method it needs (`needs`), sets num_items / top_k where the model has to match them, and builds what it keeps on a device in
    _make_resident(device)."""
    name = needs = num_items = top_k = None
    block_users, tie_order = 8192, "id"

    def _user_groups(self, users, user_train_dict, group_view):
        """("all:" + the group_view groups' labels, their positions into `users`); sets num_discarded when there is a view."""
        labels, positions = [ALL], [np.arange(len(users), dtype=np.int64)]
        if group_view is not None:
            more, at, self.num_discarded = assign_user_groups(users, user_train_dict, group_view)
            labels, positions = labels + more, positions + at
        return labels, positions

    def _item_groups(self, item_ids, item_counts, item_group_view, prefix=""):
        """The same over item_ids by popularity (assign_item_groups), the groups' labels prefixed."""
        labels, positions = [ALL], [np.arange(len(item_ids), dtype=np.int64)]
        if item_group_view is not None:
            more, at = assign_item_groups(item_ids, item_counts, item_group_view)
            labels, positions = labels + [(prefix + x.strip()).ljust(12) if prefix else x for x in more], positions + at
        return labels, positions

    def _resident(self, device):
        """What the report keeps on `device` (_make_resident), built once per device."""
        hit = self.__dict__.setdefault("_device", {}).get(str(device))
        if hit is None:
            hit = self._device[str(device)] = self._make_resident(device)
        return hit

    def _preflight(self, model):
        """The model can serve this report: it has the reader, its tables are whole on this rank and of the report's catalogue.
        -> the device."""
        if not hasattr(model, self.needs):
            raise TypeError("model must expose %s()" % self.needs)
        if hasattr(model, "_ensure_tables") and getattr(model, "_cache", None) is not None:
            model._ensure_tables()
        if getattr(model, "_eval_shard", None) is not None:
            raise CandidateScoringError("the %s report needs the whole cached item table on this rank; the tables are "
                                        "item-sharded (lean / multi-rank evaluation): run without --%s_report" % (self.name, self.name))
        if self.num_items is not None and model.num_items != self.num_items:
            raise ValueError("the report was built for %d items, the model has %d" % (self.num_items, model.num_items))
        if self.top_k is not None and self.top_k > model.num_items:
            raise CandidateScoringError("%s report of the top-%d lists: the catalogue has %d items" % (self.name, self.top_k, model.num_items))
        return model._require_gpu()

    def top_lists(self, model, users, K, block_users, tie_order, with_values=False):
        """The users' top-K lists under the model's current predict type with their train items masked, in blocks of block_users:
        yields (a, b, users [b - a] int64, lists [b - a x K] int32) per block, on the device; with_values: and the lists' scores
        float32 [b - a x K] as a fifth entry."""
        device = model._require_gpu()
        a = 0
        for batch_users in DataIterator(users, batch_size=block_users, shuffle=False, drop_last=False):
            train_ptr, train_items = lists_csr(batch_users, self.user_pos_train, device)
            users_t = torch.as_tensor(np.asarray(batch_users, dtype=np.int64)).to(device)
            idx, val = model.predict_device(users_t, top_k=K, train_ptr=train_ptr, train_items=train_items, tie_order=tie_order)
            yield (a, a + len(batch_users), users_t, idx) + ((val,) if with_values else ())
            a += len(batch_users)


class EffectReport(_Report):
    """What the test users' top-K lists are made of (--effect_report=K): per (user, rank <= K) pair the effect breakdown of
    EliMRec.effects_device -- ui, its catalogue mean, te, nde, the TE / TIE scores, the heads' cosines -- and its column means
    over all pairs and, with group_view, per user group (assign_user_groups). The lists are the model's top-K under its current
    predict type with train items masked, in user blocks as metric_rows takes them; the means are ops.group_metric_means over
    the [users*K x C] block (float64 sums, the segments = rows of that block): only [1 + groups x C] floats reach the host."""

    name, needs = "effect", "effects_device"

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
        self.group_labels, self._positions = self._user_groups(self.users, user_train_dict, group_view)

    def _make_resident(self, device):
        """The groups over the rows of the [users*K x C] block: user position p holds rows p K .. p K + K - 1."""
        K = self.top_k
        rows = [(p[:, None] * K + np.arange(K, dtype=np.int64)[None, :]).reshape(-1) for p in self._positions]
        return group_index(rows, len(self.users) * K, device)

    def _group_index(self, device):
        return self._resident(device)

    def effect_rows(self, model):
        """The breakdown of every test user's top-K list on the device: ([users*K x C] float32, column names)."""
        device = self._preflight(model)
        columns = ops.effect_columns(model._mods)
        K, C = self.top_k, len(columns)
        rows = torch.empty(len(self.users) * K, C, dtype=torch.float32, device=device)
        for a, b, users_t, idx in self.top_lists(model, self.users, K, self.block_users, self.tie_order):
            cand_ptr = torch.arange(b - a + 1, dtype=torch.int64, device=device) * K
            model.effects_device(users_t, cand_ptr, idx.reshape(-1), rows[a * K:b * K].view(b - a, K, C))
        return rows, columns

    def evaluate(self, model):
        """(final [1 + groups x C] float32: row 0 = all pairs, then one row per user group; buf: a header of column names and
        one line per row in the grouped evaluator's format)."""
        rows, columns = self.effect_rows(model)
        final = group_table(rows, self._group_index(rows.device), len(self.group_labels))
        return final, format_table(columns, self.group_labels, final)


RankTables = collections.namedtuple("RankTables", ("pair_columns", "pair_labels", "pairs", "user_columns", "user_labels", "users"))


class RankReport(_Report):
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

    name, needs = "rank", "rank_items_device"

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
        self.pair_ptr, self.pair_items, _ = ops.ragged(pair_items, dtype=np.int32, check=(I, "test item ids must lie in [0, %d)" % I))
        self.pair_user = np.repeat(np.arange(len(self.users), dtype=np.int64), lens)       # position in self.users
        self.user_n_cand = np.asarray(n_cand, dtype=np.int32)
        self.pair_n_cand = self.user_n_cand[self.pair_user]
        self.num_pairs = int(self.pair_items.size)
        # groups: rows of the user block / of the pair block (a user group's pairs; the pairs by their item's popularity)
        self.user_labels, self._user_pos = self._user_groups(self.users, user_train_dict, group_view)
        by_user = [np.flatnonzero(np.isin(self.pair_user, p)) for p in self._user_pos[1:]]
        counts = item_train_counts(user_train_dict, I) if item_group_view is not None else None
        self.pair_labels, self._pair_pos = self._item_groups(self.pair_items, counts, item_group_view, prefix="item ")
        self.pair_labels[1:1] = self.user_labels[1:]
        self._pair_pos[1:1] = by_user

    @property
    def block_users(self):
        """Users per scoring call: as many as keep the [users x items] float32 block (rows padded to 16 bytes) within block_bytes."""
        return max(1, int(self.block_bytes) // ((self.num_items + 3) // 4 * 16))

    def _make_resident(self, device):
        """The CSRs, candidate counts and group indices resident on the device; blocks: _block's scoring inputs."""
        return dict(pair_ptr=torch.from_numpy(self.pair_ptr).to(device), user_n_cand=torch.from_numpy(self.user_n_cand).to(device),
                    pair_n_cand=torch.from_numpy(np.ascontiguousarray(self.pair_n_cand)).to(device),
                    user_groups=group_index(self._user_pos, len(self.users), device),
                    pair_groups=group_index(self._pair_pos, self.num_pairs, device), blocks={})

    def _block(self, res, a, b, device):
        """Users [a, b) of self.users as one scoring call's inputs, kept on the device: (users, TargetIndex, train_ptr, train_items)."""
        hit = res["blocks"].get((a, b))
        if hit is None:
            ptr = self.pair_ptr[a:b + 1] - self.pair_ptr[a]
            target = ops.TargetIndex(ptr, self.pair_items[self.pair_ptr[a]:self.pair_ptr[b]], b - a, self.num_items, device)
            train = lists_csr(self.users[a:b], self.user_pos_train, device, cast=int)
            hit = (torch.as_tensor(np.asarray(self.users[a:b], dtype=np.int64)).to(device), target) + (train if train[1].numel() else (None, None))
            res["blocks"][(a, b)] = hit
        return hit

    def pair_ranks(self, model):
        """The exact catalogue rank of every pair under the model's current predict type: int32 [num_pairs] on the device."""
        device = self._preflight(model)
        res = self._resident(device)
        ranks = torch.empty(self.num_pairs, dtype=torch.int32, device=device)
        step = self.block_users
        for a in range(0, len(self.users), step):
            b = min(a + step, len(self.users))
            users, target, tptr, titems = self._block(res, a, b, device)
            ranks[self.pair_ptr[a]:self.pair_ptr[b]] = model.rank_items_device(users, target, tptr, titems)[0]
        return ranks

    def _tables(self, pair_rows, pair_columns, user_rows, user_columns, res):
        pairs = group_table(pair_rows, res["pair_groups"], len(self.pair_labels))
        users = group_table(user_rows, res["user_groups"], len(self.user_labels)) if user_rows is not None else None
        final = RankTables(tuple(pair_columns), list(self.pair_labels), pairs, tuple(user_columns),
                           list(self.user_labels) if users is not None else [], users)
        buf = format_table(final.pair_columns, final.pair_labels, final.pairs)
        if users is not None:
            buf += "\n" + format_table(final.user_columns, final.user_labels, final.users)
        return final, buf

    _format = staticmethod(format_table)

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


class NeighbourReport(_Report):
    """Whose neighbourhood the fused space copies (--neighbour_report=K): for EVERY item its top-k neighbour lists by cosine in the
    fused space and in each single-modal head's space (EliMRec.neighbours_device, csrc/knn.hip), items in blocks of block_items,
    and per item the columns of ops.neighbour_columns(mods):
      overlap_<m> = |fused list & head m's list| / k (ops.list_overlap); cos_fused, cos_<m> = the mean score of the list;
      pop_fused, pop_<m> = the mean training-interaction count of the listed neighbours
    (fillers skipped; a column of a row without neighbours is NaN). Their means over all items and -- item_group_view -- per item
    popularity group (assign_item_groups over the items' training interactions) are ops.group_metric_means over the
    [items x C] block: only the [1 + groups x C] table reaches the host. The lists do not depend on the predict type."""

    name, needs = "neighbour", "neighbours_device"

    def __init__(self, dataset, user_train_dict, k, item_group_view=None):
        if not isinstance(user_train_dict, dict):
            raise TypeError("user_train_dict must be a dict")
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1 or k > ops.KNN_MAX_K:
            raise ValueError("k must be an integer in [1, %d], got %r" % (ops.KNN_MAX_K, k))
        self.dataset = dataset
        self.num_items = I = int(dataset.num_items)
        self.k = int(k)
        self.block_items = 8192
        self.item_counts = item_train_counts(user_train_dict, I)
        self.group_labels, self._positions = self._item_groups(np.arange(I, dtype=np.int64), self.item_counts, item_group_view)

    def _make_resident(self, device):
        """The group index, the items' training counts and the blocks' checked queries resident on the device."""
        return dict(groups=group_index(self._positions, self.num_items, device),
                    counts=torch.from_numpy(self.item_counts.astype(np.float64)).to(device), queries={})

    def neighbour_rows(self, model):
        """Every item's row of the report on the device: ([items x C] float32, column names)."""
        device = self._preflight(model)
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
        final = group_table(rows, self._resident(rows.device)["groups"], len(self.group_labels))
        return final, format_table(columns, self.group_labels, final)


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


class ListReport(_Report):
    """The recommendation lists themselves (--list_report=K): every test user's top-K list under the model's current predict
    type with the train items masked (predict_device, users in blocks of block_users as EffectReport takes them), and
      per user the columns of ops.list_columns(mods): ils_fused, ils_<m> = the mean pairwise cosine of the K listed items in the
        fused space and in each head's space (EliMRec.list_similarity_device, csrc/lists.hip: one launch per block for all
        spaces), pop = the mean training-interaction count of the listed items (float64 quotient; NaN for an empty list);
      per item how often it is listed (ops.list_exposure, int32 counters filled block after block).
    The user table is ops.group_metric_means over the rows: all users, then the group_view groups (assign_user_groups). The
    item table is exposure_summary of the counters over all items, then the item_group_view groups (assign_item_groups over the
    items' training interactions); the counters come to the host once per evaluate(): num_items int32 values."""

    name, needs = "list", "list_similarity_device"

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
        self.item_counts = item_train_counts(user_train_dict, I)
        self.group_labels, self._positions = self._user_groups(self.users, user_train_dict, group_view)
        self.item_labels, self._item_positions = self._item_groups(np.arange(I, dtype=np.int64), self.item_counts, item_group_view,
                                                                   prefix="item ")
        self.columns = self.shift_columns = None   # ops.list_columns of the model list_rows() last saw; ("overlap", "d_<column>"...)

    def _make_resident(self, device):
        """The user group index and the items' training counts resident on the device."""
        return dict(groups=group_index(self._positions, len(self.users), device),
                    counts=torch.from_numpy(self.item_counts.astype(np.float64)).to(device))

    def list_rows(self, model):
        """Every test user's row, list and the catalogue's exposure on the device: ([users x C] float32, column names,
        lists int32 [users x K], counts int32 [num_items])."""
        device = self._preflight(model)
        res = self._resident(device)
        columns = self.columns = ops.list_columns(model._mods)
        K, nb, n_users = self.top_k, len(columns) - 1, len(self.users)
        rows = torch.empty(n_users, len(columns), dtype=torch.float32, device=device)
        ils = torch.empty(n_users, nb, dtype=torch.float32, device=device)
        lists = torch.empty(n_users, K, dtype=torch.int32, device=device)
        counts = torch.zeros(self.num_items, dtype=torch.int32, device=device)
        for a, b, _, idx in self.top_lists(model, self.users, K, self.block_users, self.tie_order):
            lists[a:b] = idx
            model.list_similarity_device(lists[a:b], ils[a:b], side="item")
            ops.list_exposure(lists[a:b], counts)
        listed = lists >= 0
        pop = torch.where(listed, res["counts"][lists.clamp(min=0).long()], 0.0).sum(dim=1) / listed.sum(dim=1).double()
        rows[:, :nb] = ils
        rows[:, nb] = pop.float()
        return rows, columns, lists, counts

    def _user_table(self, rows):
        return group_table(rows, self._resident(rows.device)["groups"], len(self.group_labels))

    _format = staticmethod(format_table)

    def evaluate(self, model, rows=None):
        """(final, buf). final = ListTables: users [1 + user groups x C] float32 -- row 0 = all test users -- the means of
        ops.list_columns; items [1 + item groups x 5] float64 -- row 0 = the whole catalogue -- exposure_summary of the counters,
        columns EXPOSURE_COLUMNS. buf: per table a header of column names and one "%.8f" line per row, in the grouped evaluator's
        format. rows: list_rows(model) if the caller already holds it."""
        rows, columns, _, counts = self.list_rows(model) if rows is None else rows
        items = exposure_summary(counts.cpu().numpy(), self._item_positions)
        final = ListTables(tuple(columns), list(self.group_labels), self._user_table(rows), EXPOSURE_COLUMNS, list(self.item_labels), items)
        buf = format_table(final.user_columns, final.user_labels, final.users) + "\n" + format_table(
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
        return final, format_table(self.shift_columns, self.group_labels, final)


AUDIENCE_COLUMNS = ("hit", "first", "act", "score")
AUDIENCE_EXPOSURE_COLUMNS = ("users", "coverage", "gini", "entropy")
AudienceTables = collections.namedtuple("AudienceTables", ("item_columns", "item_labels", "items", "user_columns", "user_labels", "users"))


def audience_item_rows(lists, scores, test_ptr, test_users, user_train_len):
    """The audience report's row of every item, float64 [n x 4] in the columns AUDIENCE_COLUMNS, from its list of user ids (lists
    int [n x k], -1 fillers) and their scores [n x k], its test users (segment i of the CSR test_ptr [n + 1] / test_users) and the
    users' training-history lengths (user_train_len [U]):
      hit = the share of the item's test users found in its list (an item-side recall at k; NaN without test users);
      first = 1 if any test user is listed, else 0; act = the mean training-history length of the listed users;
      score = the mean listed score (both NaN for a list of fillers only). Pure numpy."""
    lists = np.asarray(lists, dtype=np.int64)
    scores = np.asarray(scores, dtype=np.float64)
    ptr = np.asarray(test_ptr, dtype=np.int64).reshape(-1)
    users = np.asarray(test_users, dtype=np.int64).reshape(-1)
    length = np.asarray(user_train_len, dtype=np.float64).reshape(-1)
    n = lists.shape[0]
    out = np.full((n, len(AUDIENCE_COLUMNS)), np.nan, dtype=np.float64)
    for i in range(n):
        listed = lists[i] >= 0
        test = users[ptr[i]:ptr[i + 1]]
        hits = int(np.isin(lists[i][listed], test).sum())
        if test.size:
            out[i, 0] = hits / float(test.size)
        out[i, 1] = 1.0 if hits else 0.0
        if listed.any():
            out[i, 2] = length[lists[i][listed]].sum() / float(listed.sum())
            out[i, 3] = scores[i][listed].sum() / float(listed.sum())
    return out


class AudienceReport(_Report):
    """Whom the model sends an item to (--audience_report=K): for every item with at least one test interaction its top-k audience
    under the model's current predict type with the item's training users left out (EliMRec.audience_device, csrc/audience.hip),
    items in blocks of block_items, and
      per item the columns AUDIENCE_COLUMNS (audience_item_rows; the hit counts are ops.audience_hits on the device), their means
        over all those items and -- item_group_view -- per item popularity group (ops.group_metric_means: only the table reaches the
        host);
      per user how often they are listed (ops.list_exposure over the lists with n_rows = the number of users), summarised by
        exposure_summary over all users in the columns AUDIENCE_EXPOSURE_COLUMNS."""

    name, needs = "audience", "audience_device"

    def __init__(self, dataset, user_train_dict, user_test_dict, k, item_group_view=None):
        if not isinstance(user_train_dict, dict) or not isinstance(user_test_dict, dict):
            raise TypeError("user_train_dict and user_test_dict must be dicts")
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1 or k > ops.AUDIENCE_MAX_K:
            raise ValueError("k must be an integer in [1, %d], got %r" % (ops.AUDIENCE_MAX_K, k))
        self.dataset = dataset
        self.num_items, self.num_users = I, U = int(dataset.num_items), int(dataset.num_users)
        self.k = int(k)
        self.block_items = 8192
        item_test, item_train = {}, {}
        for table, src in ((item_test, user_test_dict), (item_train, user_train_dict)):
            for u, items in src.items():
                for i in items:
                    table.setdefault(int(i), []).append(int(u))
        self.items = sorted(item_test)
        self.item_test = {i: sorted(set(item_test[i])) for i in self.items}
        self.item_train = {i: sorted(set(item_train.get(i, []))) for i in self.items}
        self.user_train_len = np.zeros(U, dtype=np.int64)
        for u, items in user_train_dict.items():
            self.user_train_len[int(u)] = len(items)
        self.item_counts = item_train_counts(user_train_dict, I)
        self.group_labels, self._positions = self._item_groups(np.asarray(self.items, dtype=np.int64), self.item_counts, item_group_view)
        self.shift_columns = ("overlap",) + tuple("d_" + c for c in AUDIENCE_COLUMNS)

    def test_csr(self):
        """The items' test users as CSR on the host: (ptr int64 [n + 1], users int32)."""
        return ops.ragged([self.item_test[i] for i in self.items], dtype=np.int32)[:2]

    def _make_resident(self, device):
        """The group index, the users' history lengths, the items' test users and the blocks' checked queries on the device."""
        ptr, users = self.test_csr()
        ops._checked_csr(ptr, users, len(self.items), self.num_users, "AudienceReport",
                         ("test_ptr", "test_users", "n", "test users span [%d, %d], the model has %d users"))
        return dict(groups=group_index(self._positions, len(self.items), device),
                    length=torch.from_numpy(self.user_train_len.astype(np.float64)).to(device),
                    test_ptr=torch.from_numpy(ptr).to(device), test_users=ops._resident_ids(users, device), queries={})

    def audience_rows(self, model):
        """Every reported item's row, list, scores and the users' exposure on the device: ([n x 4] float32, lists int32 [n x k],
        scores float32 [n x k], counts int32 [num_users])."""
        device = self._preflight(model)
        if model.num_users != self.num_users:
            raise ValueError("the report was built for %d users, the model has %d" % (self.num_users, model.num_users))
        res = self._resident(device)
        n, k, U = len(self.items), self.k, self.num_users
        lists = torch.empty(n, k, dtype=torch.int32, device=device)
        scores = torch.empty(n, k, dtype=torch.float32, device=device)
        counts = torch.zeros(U, dtype=torch.int32, device=device)
        hits = torch.zeros(max(n, 1), dtype=torch.int32, device=device)
        step = max(1, int(self.block_items))
        for a in range(0, n, step):
            b = min(a + step, n)
            query = res["queries"].get((a, b))
            if query is None:
                ptr, flat, _ = ops.ragged([self.item_train[i] for i in self.items[a:b]], dtype=np.int32)
                query = res["queries"][(a, b)] = ops.AudienceQuery(np.asarray(self.items[a:b], dtype=np.int32), self.num_items, U, device,
                                                                   ptr if flat.size else None, flat if flat.size else None)
            model.audience_device(query, k, lists[a:b], scores[a:b])
            ops.list_exposure(lists[a:b], counts)
        rows = torch.empty(n, len(AUDIENCE_COLUMNS), dtype=torch.float32, device=device)
        if n:
            ops.audience_hits(lists, res["test_ptr"], res["test_users"], hits)
            listed = lists >= 0
            m = listed.sum(dim=1).double()
            cnt = hits[:n].double()
            rows[:, 0] = (cnt / (res["test_ptr"][1:] - res["test_ptr"][:-1]).double()).float()
            rows[:, 1] = (cnt > 0).float()
            rows[:, 2] = (torch.where(listed, res["length"][lists.clamp(min=0).long()], 0.0).sum(dim=1) / m).float()
            rows[:, 3] = (torch.where(listed, scores.double(), 0.0).sum(dim=1) / m).float()
        return rows, lists, scores, counts

    def _item_table(self, rows):
        return group_table(rows, self._resident(rows.device)["groups"], len(self.group_labels))

    def evaluate(self, model, rows=None):
        """(final, buf). final = AudienceTables: items [1 + item groups x 4] float32 -- row 0 = every item with a test interaction --
        the means of AUDIENCE_COLUMNS; users [1 x 4] float64: exposure_summary of how often each user is listed, columns
        AUDIENCE_EXPOSURE_COLUMNS. buf: per table a header of column names and one "%.8f" line per row (the shared table format).
        rows: audience_rows(model) if the caller already holds it."""
        rows, _, _, counts = self.audience_rows(model) if rows is None else rows
        users = exposure_summary(counts.cpu().numpy(), [np.arange(self.num_users, dtype=np.int64)])[:, :len(AUDIENCE_EXPOSURE_COLUMNS)]
        final = AudienceTables(AUDIENCE_COLUMNS, list(self.group_labels), self._item_table(rows), AUDIENCE_EXPOSURE_COLUMNS, [ALL], users)
        buf = format_table(final.item_columns, final.item_labels, final.items) + "\n" + format_table(
            final.user_columns, final.user_labels, final.users)
        return final, buf

    def shift(self, lists_te, lists_tie):
        """How the audiences change from TE to TIE (two audience_rows() results of this report): (final [1 + item groups x 5]
        float32, buf) over the columns self.shift_columns: overlap = |list a & list b| / k (ops.list_overlap) and d_<column> = TIE - TE
        for every item column."""
        rows_a, lists_a = lists_te[0], lists_te[1]
        rows_b, lists_b = lists_tie[0], lists_tie[1]
        n, k = len(self.items), self.k
        if (tuple(lists_a.shape) != (n, k) or lists_a.shape != lists_b.shape or tuple(rows_a.shape) != (n, len(AUDIENCE_COLUMNS))
                or rows_a.shape != rows_b.shape or len({t.device for t in (rows_a, rows_b, lists_a, lists_b)}) != 1):
            raise ValueError("shift() takes two audience_rows() results of this report on one device")
        cnt = torch.zeros(max(n, 1), dtype=torch.int32, device=lists_a.device)
        if n:
            ops.list_overlap(lists_a, lists_b, cnt)
        rows = torch.cat(((cnt[:n].double() / k).float()[:, None], rows_b - rows_a), dim=1)
        final = self._item_table(rows)
        return final, format_table(self.shift_columns, self.group_labels, final)


DIVERSIFY_COLUMNS = ("lambda", "recall", "ndcg", "ils_fused", "pop", "overlap", "coverage", "gini", "entropy")
DiversifyTables = collections.namedtuple("DiversifyTables", ("columns", "labels", "table"))


class DiversifyReport(_Report):
    """What diversified re-ranking costs and buys (--diversify_report=K): every test user's top-`pool` list under the model's
    current predict type with the train items masked (ONE top_lists pass with the scores, shared by all lambdas), re-ranked to K
    items per lambda by greedy MMR in the fused space (EliMRec.rerank_device, csrc/rerank.hip: one launch per user block and
    lambda), and per lambda
      per user recall and ndcg at K (ops.rank_metrics), ils_fused = the list's mean pairwise cosine in the fused space
        (list_similarity_device, column 0), pop = the mean training-interaction count of its items (as ListReport), overlap = the
        share of the plain top-K list it keeps (ops.list_overlap);
      coverage, gini, entropy = exposure_summary of how often each item is listed (ops.list_exposure) over the whole catalogue.
    The table has one row per lambda -- DIVERSIFY_COLUMNS: the lambda, the user means (ops.group_metric_means), the three exposure
    columns -- for all test users, then one such block per group_view group (assign_user_groups; the exposure columns from that
    group's lists). lambda = 1 keeps the pool's order: its row holds the plain lists' numbers."""

    name, needs = "diversify", "rerank_device"
    metrics = (2, 4)                     # Recall, NDCG (evaluator.metric_dict)

    def __init__(self, dataset, user_train_dict, user_test_dict, top_k, pool=None, lambdas=(1.0, 0.9, 0.7, 0.5), group_view=None):
        if not isinstance(user_train_dict, dict) or not isinstance(user_test_dict, dict):
            raise TypeError("user_train_dict and user_test_dict must be dicts")
        self.num_items = I = int(dataset.num_items)
        cap = min(ops.LIST_MAX_K, I)
        for what, v in (("top_k", top_k), ("pool", pool)):
            if (v is not None or what == "top_k") and (isinstance(v, bool) or not isinstance(v, (int, np.integer))):
                raise ValueError("%s must be an integer, got %r" % (what, v))
        if pool is None:
            pool = min(4 * int(top_k), cap)
        if not 2 <= top_k <= pool <= cap:
            raise ValueError("need 2 <= top_k <= pool <= min(%d, the catalogue's %d items), got top_k %r, pool %r"
                             % (ops.LIST_MAX_K, I, top_k, pool))
        if isinstance(lambdas, (str, bytes)) or not hasattr(lambdas, "__len__") or not len(lambdas):
            raise ValueError("lambdas must be a non-empty list of numbers in [0, 1], got %r" % (lambdas,))
        for lam in lambdas:
            if isinstance(lam, bool) or not isinstance(lam, (int, float, np.integer, np.floating)) or not 0.0 <= float(lam) <= 1.0:
                raise ValueError("lambdas must be a non-empty list of numbers in [0, 1], got %r" % (lambdas,))
        self.dataset = dataset
        self.user_pos_train = user_train_dict
        self.user_pos_test = user_test_dict
        self.top_k, self.pool = int(top_k), int(pool)
        self.lambdas = tuple(float(lam) for lam in lambdas)
        self.users = list(user_test_dict.keys())
        self.item_counts = item_train_counts(user_train_dict, I)
        self.group_labels, self._positions = self._user_groups(self.users, user_train_dict, group_view)
        self.columns = DIVERSIFY_COLUMNS

    def _make_resident(self, device):
        """The user group index, each group's user positions and the items' training counts resident on the device."""
        return dict(groups=group_index(self._positions, len(self.users), device),
                    positions=[torch.from_numpy(p).to(device) for p in self._positions],
                    counts=torch.from_numpy(self.item_counts.astype(np.float64)).to(device))

    def rerank_rows(self, model):
        """Per lambda every test user's row and list on the device: (rows float32 [lambdas x users x 5] -- recall, ndcg,
        ils_fused, pop, overlap --, lists int32 [lambdas x users x K], counts int32 [lambdas x num_items])."""
        device = self._preflight(model)
        res = self._resident(device)
        K, N, L, n_users, nb = self.top_k, self.pool, len(self.lambdas), len(self.users), 1 + model.S
        rows = torch.empty(L, n_users, 5, dtype=torch.float32, device=device)
        lists = torch.empty(L, n_users, K, dtype=torch.int32, device=device)
        counts = torch.zeros(L, self.num_items, dtype=torch.int32, device=device)
        block = min(self.block_users, max(n_users, 1))
        met = torch.empty(block, len(self.metrics), K, dtype=torch.float32, device=device)
        ils = torch.empty(block, nb, dtype=torch.float32, device=device)
        cnt = torch.empty(block, dtype=torch.int32, device=device)
        for a, b, _, idx, val in self.top_lists(model, self.users, N, self.block_users, self.tie_order, with_values=True):
            truth_ptr, truth_items = lists_csr(self.users[a:b], self.user_pos_test, device, unique=True)
            plain = idx[:, :K].contiguous()
            for li, lam in enumerate(self.lambdas):
                out = lists[li, a:b]
                model.rerank_device(idx, val, K, lam, space="fused", out_idx=out)
                ops.rank_metrics(out, truth_ptr, truth_items, self.metrics, met[:b - a])
                model.list_similarity_device(out, ils[:b - a], side="item")
                ops.list_exposure(out, counts[li])
                ops.list_overlap(plain, out, cnt[:b - a])
                listed = out >= 0
                pop = torch.where(listed, res["counts"][out.clamp(min=0).long()], 0.0).sum(dim=1) / listed.sum(dim=1).double()
                rows[li, a:b, 0:2] = met[:b - a, :, K - 1]
                rows[li, a:b, 2] = ils[:b - a, 0]
                rows[li, a:b, 3] = pop.float()
                rows[li, a:b, 4] = (cnt[:b - a].double() / K).float()
        return rows, lists, counts

    def evaluate(self, model, rows=None):
        """(final, buf). final = DiversifyTables(columns, labels, table float64 [(1 + user groups) * lambdas x 9]): per group (row
        block 0 = all test users) one row per lambda in self.lambdas' order. buf: a header of column names and one "%.8f" line per
        row, in the grouped evaluator's format. rows: rerank_rows(model) if the caller already holds it."""
        rows, lists, counts = self.rerank_rows(model) if rows is None else rows
        res = self._resident(rows.device)
        L, G = len(self.lambdas), len(self.group_labels)
        every = [np.arange(self.num_items, dtype=np.int64)]
        table = np.zeros((G * L, len(DIVERSIFY_COLUMNS)), dtype=np.float64)
        for li, lam in enumerate(self.lambdas):
            means = group_table(rows[li], res["groups"], G)
            for g in range(G):
                c = counts[li]
                if g:                                  # a group's exposure: its own users' lists
                    c = ops.list_exposure(lists[li].index_select(0, res["positions"][g]).contiguous(), torch.zeros_like(c))
                table[g * L + li, 0] = lam
                table[g * L + li, 1:6] = means[g]
                table[g * L + li, 6:9] = exposure_summary(c.cpu().numpy(), every)[0, 1:4]
        labels = [label for label in self.group_labels for _ in self.lambdas]
        final = DiversifyTables(DIVERSIFY_COLUMNS, labels, table)
        return final, format_table(final.columns, final.labels, final.table)


def item_classes(item_ids_or_num_items, train_item_counts, item_group_view):
    """The popularity buckets as item classes: (class_of int32 [I], names) -- class_of[k] = the index of the assign_item_groups
    bucket (cold, (0,b1], ..., (bn,inf); empty buckets omitted, in that order) that entry k of the item ids falls into, names =
    the buckets' labels. An int stands for the whole catalogue 0 .. I - 1. More classes than ops.CALIBRATE_MAX_CLASSES: ValueError."""
    if isinstance(item_ids_or_num_items, (int, np.integer)) and not isinstance(item_ids_or_num_items, bool):
        ids = np.arange(int(item_ids_or_num_items), dtype=np.int64)
    else:
        ids = np.asarray(item_ids_or_num_items, dtype=np.int64).reshape(-1)
    labels, positions = assign_item_groups(ids, train_item_counts, item_group_view)
    if len(labels) > ops.CALIBRATE_MAX_CLASSES:
        raise ValueError("item_group_view gives %d item classes, at most %d are supported" % (len(labels), ops.CALIBRATE_MAX_CLASSES))
    class_of = np.zeros(ids.size, dtype=np.int32)
    for c, at in enumerate(positions):
        class_of[at] = c
    return class_of, labels


def calibration_columns(names):
    """Column names of the calibration report: lambda, recall, ndcg, ckl, pop, overlap, one share_<class> per item class (names:
    the classes' labels, as item_classes gives them), then coverage, gini, entropy."""
    return (("lambda", "recall", "ndcg", "ckl", "pop", "overlap") + tuple("share_" + str(n).strip().rstrip(":") for n in names)
            + ("coverage", "gini", "entropy"))


CalibrationTables = collections.namedtuple("CalibrationTables", ("columns", "labels", "table"))


class CalibrationReport(_Report):
    """Do the lists match each user's own popularity mix, and what does making them match cost (--calibrate_report=K): the items
    are classed by training popularity (item_classes over item_group_view), a user's target is the class shares of their training
    items (ops.class_shares, one launch), and every test user's top-`pool` list under the model's current predict type with the
    train items masked (ONE top_lists pass with the scores, shared by all lambdas) is re-ranked to K items per lambda by greedy
    calibrated re-ranking (EliMRec.calibrate_device, csrc/calibrate.hip: one launch per user block and lambda; Steck, "Calibrated
    recommendations", RecSys 2018). lambda weighs the RELEVANCE, as in DiversifyReport (Steck's lambda weighs the calibration
    term). Per lambda
      per user recall and ndcg at K (ops.rank_metrics), ckl = the list's miscalibration C_KL(target || smoothed list shares) and
        share_<class> = the list's share of every class (ops.list_calibration, one launch per user block and lambda), pop = the mean
        training-interaction count of its items (as ListReport), overlap = the share of the plain top-K list it keeps;
      coverage, gini, entropy = exposure_summary of how often each item is listed (ops.list_exposure) over the whole catalogue.
    The table has one row per lambda -- calibration_columns(names): the lambda, the user means (ops.group_metric_means), the three
    exposure columns -- for all test users, then one such block per group_view group (assign_user_groups; the exposure columns from
    that group's lists). lambda = 1 keeps the pool's order: its row holds the plain lists' numbers -- read under TE and under TIE,
    its ckl says whether TIE alone already moves the lists towards the users' own mix. Below the table one line `target:` holds the
    mean target share of every class over all test users."""

    name, needs = "calibrate", "predict_device"
    metrics = (2, 4)                     # Recall, NDCG (evaluator.metric_dict)

    def __init__(self, dataset, user_train_dict, user_test_dict, top_k, item_group_view, pool=None, lambdas=(1.0, 0.9, 0.7, 0.5),
                 smooth=0.01, group_view=None):
        if not isinstance(user_train_dict, dict) or not isinstance(user_test_dict, dict):
            raise TypeError("user_train_dict and user_test_dict must be dicts")
        self.num_items = I = int(dataset.num_items)
        cap = min(ops.LIST_MAX_K, I)
        for what, v in (("top_k", top_k), ("pool", pool)):
            if (v is not None or what == "top_k") and (isinstance(v, bool) or not isinstance(v, (int, np.integer))):
                raise ValueError("%s must be an integer, got %r" % (what, v))
        if pool is None:
            pool = min(4 * int(top_k), cap)
        if not 2 <= top_k <= pool <= cap:
            raise ValueError("need 2 <= top_k <= pool <= min(%d, the catalogue's %d items), got top_k %r, pool %r"
                             % (ops.LIST_MAX_K, I, top_k, pool))
        if isinstance(lambdas, (str, bytes)) or not hasattr(lambdas, "__len__") or not len(lambdas):
            raise ValueError("lambdas must be a non-empty list of numbers in [0, 1], got %r" % (lambdas,))
        for lam in lambdas:
            if isinstance(lam, bool) or not isinstance(lam, (int, float, np.integer, np.floating)) or not 0.0 <= float(lam) <= 1.0:
                raise ValueError("lambdas must be a non-empty list of numbers in [0, 1], got %r" % (lambdas,))
        if isinstance(smooth, bool) or not isinstance(smooth, (int, float, np.integer, np.floating)) or not 0.0 < float(smooth) < 1.0:
            raise ValueError("smooth must be a number in (0, 1), got %r" % (smooth,))
        self.dataset = dataset
        self.user_pos_train = user_train_dict
        self.user_pos_test = user_test_dict
        self.top_k, self.pool = int(top_k), int(pool)
        self.lambdas = tuple(float(lam) for lam in lambdas)
        self.smooth = float(smooth)
        self.users = list(user_test_dict.keys())
        self.item_counts = item_train_counts(user_train_dict, I)
        self.class_of, self.class_names = item_classes(I, self.item_counts, item_group_view)
        self.num_classes = len(self.class_names)
        self.group_labels, self._positions = self._user_groups(self.users, user_train_dict, group_view)
        self.columns = calibration_columns(self.class_names)

    def _make_resident(self, device):
        """The user group index, each group's user positions, the items' training counts and classes and every test user's target
        (the class shares of their training items: one launch) resident on the device."""
        class_of = torch.from_numpy(self.class_of).to(device)
        ptr, items = lists_csr(self.users, self.user_pos_train, device)
        targets = torch.zeros(len(self.users), self.num_classes, dtype=torch.float32, device=device)
        ops.class_shares(ptr, items, class_of, self.num_classes, targets)
        return dict(groups=group_index(self._positions, len(self.users), device),
                    positions=[torch.from_numpy(p).to(device) for p in self._positions],
                    counts=torch.from_numpy(self.item_counts.astype(np.float64)).to(device), class_of=class_of, targets=targets)

    def targets(self, device):
        """Every test user's target class shares on the device: float32 [users x C]."""
        return self._resident(device)["targets"]

    def calibrate_rows(self, model):
        """Per lambda every test user's row and list on the device: (rows float32 [lambdas x users x (5 + C)] -- recall, ndcg,
        ckl, pop, overlap, then the list's share of every class --, lists int32 [lambdas x users x K], counts int32
        [lambdas x num_items])."""
        device = self._preflight(model)
        if not hasattr(model, "calibrate_device"):
            raise TypeError("model must expose calibrate_device()")
        res = self._resident(device)
        K, N, L, n_users, C = self.top_k, self.pool, len(self.lambdas), len(self.users), self.num_classes
        rows = torch.empty(L, n_users, 5 + C, dtype=torch.float32, device=device)
        lists = torch.empty(L, n_users, K, dtype=torch.int32, device=device)
        counts = torch.zeros(L, self.num_items, dtype=torch.int32, device=device)
        block = min(self.block_users, max(n_users, 1))
        met = torch.empty(block, len(self.metrics), K, dtype=torch.float32, device=device)
        shares = torch.empty(block, C, dtype=torch.float32, device=device)
        kl = torch.empty(block, dtype=torch.float32, device=device)
        cnt = torch.empty(block, dtype=torch.int32, device=device)
        for a, b, _, idx, val in self.top_lists(model, self.users, N, self.block_users, self.tie_order, with_values=True):
            truth_ptr, truth_items = lists_csr(self.users[a:b], self.user_pos_test, device, unique=True)
            plain = idx[:, :K].contiguous()
            target = res["targets"][a:b]
            for li, lam in enumerate(self.lambdas):
                out = lists[li, a:b]
                model.calibrate_device(idx, val, K, lam, res["class_of"], target, smooth=self.smooth, out_idx=out)
                ops.list_calibration(out, res["class_of"], C, shares[:b - a], target=target, smooth=self.smooth, out_kl=kl[:b - a])
                ops.rank_metrics(out, truth_ptr, truth_items, self.metrics, met[:b - a])
                ops.list_exposure(out, counts[li])
                ops.list_overlap(plain, out, cnt[:b - a])
                listed = out >= 0
                pop = torch.where(listed, res["counts"][out.clamp(min=0).long()], 0.0).sum(dim=1) / listed.sum(dim=1).double()
                rows[li, a:b, 0:2] = met[:b - a, :, K - 1]
                rows[li, a:b, 2] = kl[:b - a]
                rows[li, a:b, 3] = pop.float()
                rows[li, a:b, 4] = (cnt[:b - a].double() / K).float()
                rows[li, a:b, 5:] = shares[:b - a]
        return rows, lists, counts

    def evaluate(self, model, rows=None):
        """(final, buf). final = CalibrationTables(columns, labels, table float64 [(1 + user groups) * lambdas x (9 + C)]): per
        group (row block 0 = all test users) one row per lambda in self.lambdas' order. buf: a header of column names, one "%.8f"
        line per row in the grouped evaluator's format, and the line `target:` with the mean target share of every class. rows:
        calibrate_rows(model) if the caller already holds it."""
        rows, lists, counts = self.calibrate_rows(model) if rows is None else rows
        res = self._resident(rows.device)
        L, G, C = len(self.lambdas), len(self.group_labels), self.num_classes
        every = [np.arange(self.num_items, dtype=np.int64)]
        table = np.zeros((G * L, len(self.columns)), dtype=np.float64)
        for li, lam in enumerate(self.lambdas):
            means = group_table(rows[li], res["groups"], G)
            for g in range(G):
                c = counts[li]
                if g:                                  # a group's exposure: its own users' lists
                    c = ops.list_exposure(lists[li].index_select(0, res["positions"][g]).contiguous(), torch.zeros_like(c))
                table[g * L + li, 0] = lam
                table[g * L + li, 1:6 + C] = means[g]
                table[g * L + li, 6 + C:9 + C] = exposure_summary(c.cpu().numpy(), every)[0, 1:4]
        labels = [label for label in self.group_labels for _ in self.lambdas]
        final = CalibrationTables(self.columns, labels, table)
        self.target_mean = res["targets"].double().mean(dim=0).cpu().numpy() if len(self.users) else np.zeros(C)
        buf = format_table(final.columns, final.labels, final.table) + format_rows(["target:".ljust(12)], [self.target_mean])
        return final, buf


CLUSTER_COLUMNS = ("size", "pop", "cohesion", "train_share", "test_share", "slot_share")
CLUSTER_USER_COLUMNS = ("distinct", "ckl")
ClusterTables = collections.namedtuple("ClusterTables", ("cluster_columns", "cluster_labels", "clusters", "user_columns", "user_labels", "users"))
ClusterShift = collections.namedtuple("ClusterShift", ("cluster_columns", "cluster_labels", "clusters", "user_columns", "user_labels", "users"))


def cluster_rows(assign, cos, item_counts, test_counts, exposure, n_clusters):
    """The cluster report's item table in numpy: float64 [n_clusters x 6], columns CLUSTER_COLUMNS. assign [I] (-1 = no cluster) and
    cos [I] as cluster_items gives them; item_counts / test_counts [I] = the items' training / test interactions, exposure [I] = how
    often each is listed. size = the members; pop = their mean training interactions and cohesion = their mean cosine to the
    centroid (NaN for an empty cluster); train_share / test_share / slot_share = the cluster's share of ALL training interactions,
    test interactions and list slots (the items of no cluster hold the rest; 0 where the total is 0)."""
    assign = np.asarray(assign, dtype=np.int64)
    member = assign >= 0
    at = assign[member]
    out = np.zeros((n_clusters, len(CLUSTER_COLUMNS)), dtype=np.float64)
    size = np.bincount(at, minlength=n_clusters).astype(np.float64)
    out[:, 0] = size
    with np.errstate(invalid="ignore", divide="ignore"):
        out[:, 1] = np.bincount(at, weights=np.asarray(item_counts, dtype=np.float64)[member], minlength=n_clusters) / size
        out[:, 2] = np.bincount(at, weights=np.asarray(cos, dtype=np.float64)[member], minlength=n_clusters) / size
    for col, w in ((3, item_counts), (4, test_counts), (5, exposure)):
        w = np.asarray(w, dtype=np.float64)
        total = w.sum()
        if total:
            out[:, col] = np.bincount(at, weights=w[member], minlength=n_clusters) / total
    return out


def cluster_user_rows(lists, classes, n_clusters, targets, smooth=0.01):
    """The cluster report's user rows in numpy: float64 [B x 2], columns CLUSTER_USER_COLUMNS. lists int [B x K] (-1 fillers),
    classes [I] = every item's cluster (-1 = none: such an entry is not listed), targets [B x n_clusters] = the users' own mix.
    distinct = the clusters present in the list; ckl = sum over c with p_c > 0 of p_c log(p_c / ((1 - smooth) q_c + smooth p_c)),
    q = the list's cluster shares (0 when nothing is listed): ops.list_calibration's C_KL in float64."""
    lists, classes = np.asarray(lists, dtype=np.int64), np.asarray(classes, dtype=np.int64)
    out = np.zeros((lists.shape[0], 2), dtype=np.float64)
    for b, row in enumerate(lists):
        ids = row[(row >= 0) & (row < classes.size)]
        cls = classes[ids]
        cls = cls[(cls >= 0) & (cls < n_clusters)]
        cnt = np.bincount(cls, minlength=n_clusters).astype(np.float64)
        out[b, 0] = float((cnt > 0).sum())
        q = cnt / cnt.sum() if cnt.sum() else cnt
        p = np.asarray(targets[b], dtype=np.float64)
        p = np.where(np.isfinite(p) & (p > 0), p, 0.0)
        kl = 0.0
        for c in range(n_clusters):
            if p[c] > 0:
                kl += p[c] * np.log(p[c] / ((1.0 - smooth) * q[c] + smooth * p[c]))
        out[b, 1] = kl
    return out


class ClusterReport(_Report):
    """Which kinds of content the lists concentrate on (--cluster_report=K): the items are grouped into n_clusters content clusters
    by spherical k-means of their rows in one space of the cached tables -- "fused" or a single-modal head (EliMRec.clusters_device,
    csrc/kmeans.hip) --, computed ONCE per table version and shared by the effects; every test user's top-K list under the model's
    current predict type with the train items masked is then read per cluster. One row per cluster, columns CLUSTER_COLUMNS
    (cluster_rows): size, pop, cohesion, train_share, test_share and slot_share = the cluster's share of the K x users list slots
    (ops.list_exposure). Per user, columns CLUSTER_USER_COLUMNS: distinct = the clusters present in the list, ckl = the list's
    miscalibration C_KL against the user's own training mix over the clusters (ops.class_shares + ops.list_calibration; an item of
    no cluster is not listed): the user means (ops.group_metric_means) over all test users, then per group_view group. shift(te,
    tie): d_slot_share per cluster and d_distinct, d_ckl -- does TIE move exposure between kinds of content. 2 <= n_clusters <=
    ops.CALIBRATE_MAX_CLASSES, so that the calibration kernels apply."""

    name, needs = "cluster", "clusters_device"

    def __init__(self, dataset, user_train_dict, user_test_dict, top_k, n_clusters=8, space="fused", iters=25, seed=2022, group_view=None,
                 smooth=0.01):
        if not isinstance(user_train_dict, dict) or not isinstance(user_test_dict, dict):
            raise TypeError("user_train_dict and user_test_dict must be dicts")
        if isinstance(top_k, bool) or not isinstance(top_k, (int, np.integer)) or top_k < 1 or top_k > ops.LIST_MAX_K:
            raise ValueError("top_k must be an integer in [1, %d], got %r" % (ops.LIST_MAX_K, top_k))
        for what, v in (("n_clusters", n_clusters), ("iters", iters), ("seed", seed)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError("%s must be an integer, got %r" % (what, v))
        if not 2 <= n_clusters <= 16:                # ops.CALIBRATE_MAX_CLASSES (csrc/calibrate.hip), known without the library
            raise ValueError("n_clusters must lie in [2, 16] (the calibration kernels' classes), got %d" % n_clusters)
        if iters < 1:
            raise ValueError("iters must be >= 1, got %d" % iters)
        if not isinstance(space, str) or not space:
            raise ValueError("space must be 'fused' or one of the model's heads, got %r" % (space,))
        if isinstance(smooth, bool) or not isinstance(smooth, (int, float, np.integer, np.floating)) or not 0.0 < float(smooth) < 1.0:
            raise ValueError("smooth must be a number in (0, 1), got %r" % (smooth,))
        self.dataset = dataset
        self.num_items = I = int(dataset.num_items)
        self.user_pos_train = user_train_dict
        self.user_pos_test = user_test_dict
        self.top_k, self.num_classes, self.space = int(top_k), int(n_clusters), space
        self.iters, self.seed, self.smooth = int(iters), int(seed), float(smooth)
        self.users = list(user_test_dict.keys())
        self.item_counts = item_train_counts(user_train_dict, I)
        self.test_counts = item_train_counts({u: set(user_test_dict[u]) for u in self.users}, I)
        self.group_labels, self._positions = self._user_groups(self.users, user_train_dict, group_view)
        self.cluster_labels = [("cluster %d:" % c).ljust(12) for c in range(self.num_classes)]
        self._clusters = None                        # (table version, ops.KMeans, targets)

    def _make_resident(self, device):
        return dict(groups=group_index(self._positions, len(self.users), device))

    def clusters(self, model):
        """The item clusters of the model's current tables (ops.KMeans on the device): computed once per table version."""
        device = self._preflight(model)
        version = getattr(model, "_table_version", None)
        if self._clusters is None or version is None or self._clusters[0] != version:
            km = model.clusters_device("item", self.num_classes, self.space, self.iters, self.seed)
            ptr, items = lists_csr(self.users, self.user_pos_train, device)
            targets = torch.zeros(len(self.users), self.num_classes, dtype=torch.float32, device=device)
            ops.class_shares(ptr, items, km.assign, self.num_classes, targets)
            self._clusters = (version, km, targets)
        return self._clusters[1]

    def classes(self, model):
        """Every item's cluster on the device, int32 [I] (-1 = none): the class table the calibration kernels read."""
        return self.clusters(model).assign

    def cluster_lists(self, model):
        """(rows float32 [users x 2] -- distinct, ckl --, lists int32 [users x K], counts int32 [num_items]) on the device."""
        km = self.clusters(model)
        device, targets = km.assign.device, self._clusters[2]
        K, n_users, C = self.top_k, len(self.users), self.num_classes
        rows = torch.empty(n_users, 2, dtype=torch.float32, device=device)
        lists = torch.empty(n_users, K, dtype=torch.int32, device=device)
        counts = torch.zeros(self.num_items, dtype=torch.int32, device=device)
        shares = torch.empty(n_users, C, dtype=torch.float32, device=device)
        for a, b, _, idx in self.top_lists(model, self.users, K, self.block_users, self.tie_order):
            lists[a:b] = idx
            ops.list_exposure(lists[a:b], counts)
        kl = torch.empty(n_users, dtype=torch.float32, device=device)
        ops.list_calibration(lists, km.assign, C, shares, target=targets, smooth=self.smooth, out_kl=kl)     # one launch for all users
        rows[:, 0] = (shares > 0).sum(dim=1).float()
        rows[:, 1] = kl
        return rows, lists, counts

    def evaluate(self, model, rows=None):
        """(final, buf). final = ClusterTables: clusters float64 [n_clusters x 6] (cluster_rows), users float32 [1 + user groups x 2]
        -- row 0 = all test users -- the means of distinct and ckl. buf: per table a header of column names and one "%.8f" line
        per row. rows: cluster_lists(model) if the caller already holds it."""
        rows, _, counts = self.cluster_lists(model) if rows is None else rows
        km = self.clusters(model)
        table = cluster_rows(km.assign.cpu().numpy(), km.cos.cpu().numpy(), self.item_counts, self.test_counts, counts.cpu().numpy(),
                             self.num_classes)
        users = group_table(rows, self._resident(rows.device)["groups"], len(self.group_labels))
        final = ClusterTables(CLUSTER_COLUMNS, list(self.cluster_labels), table, CLUSTER_USER_COLUMNS, list(self.group_labels), users)
        buf = format_table(final.cluster_columns, final.cluster_labels, final.clusters) + "\n" + format_table(
            final.user_columns, final.user_labels, final.users)
        return final, buf

    def shift(self, a, b):
        """How the clusters' exposure and the user means change from a to b (two evaluate() finals, e.g. TE -> TIE): (ClusterShift,
        buf) -- clusters float64 [n_clusters x 1] = d_slot_share, users [1 + user groups x 2] = d_distinct, d_ckl."""
        if not isinstance(a, ClusterTables) or not isinstance(b, ClusterTables) or a.clusters.shape != b.clusters.shape or a.users.shape != b.users.shape:
            raise ValueError("shift() takes two evaluate() results of this report")
        final = ClusterShift(("d_slot_share",), list(self.cluster_labels), b.clusters[:, 5:6] - a.clusters[:, 5:6],
                             tuple("d_" + c for c in CLUSTER_USER_COLUMNS), list(self.group_labels), b.users - a.users)
        buf = format_table(final.cluster_columns, final.cluster_labels, final.clusters) + "\n" + format_table(
            final.user_columns, final.user_labels, final.users)
        return final, buf


class HistoryReport(_Report):
    """Which past items back the lists (--history_report=K): per (test user, rank <= K) pair of the top-K lists under the model's
    current predict type with the train items masked, the support the user's own training history gives the listed item
    (EliMRec.history_support_device, csrc/history.hip): per space -- fused, then every head; one launch per space and user block,
    one-hot weights -- sup_max_<space> = the largest score of a history item against the listed item, sup_mean_<space> = the mean
    over the history, unexpected_<space> = 1 - sup_max_<space> (the usual unexpectedness / serendipity measure), and hist_n = the
    number of history items compared; columns ops.history_columns(mods). The table is ops.group_metric_means over the [users*K x C]
    block: all pairs of the test users with a non-empty training history, then the group_view groups (assign_user_groups) of those
    users. A pair beyond the end of a list that came out short (-1) has no support: its row is -inf / NaN and so is every mean it
    enters. Users go in blocks of block_users; only the tables reach the host."""

    name, needs = "history", "history_support_device"

    def __init__(self, dataset, user_train_dict, user_test_dict, top_k, top=3, group_view=None):
        if not isinstance(user_train_dict, dict) or not isinstance(user_test_dict, dict):
            raise TypeError("user_train_dict and user_test_dict must be dicts")
        self.num_items = I = int(dataset.num_items)
        cap, max_top = min(ops.LIST_MAX_K, I), ops.HISTORY_MAX_TOP
        if isinstance(top_k, bool) or not isinstance(top_k, (int, np.integer)) or not 1 <= top_k <= cap:
            raise ValueError("top_k must be an integer in [1, min(%d, the catalogue's %d items)], got %r" % (ops.LIST_MAX_K, I, top_k))
        if isinstance(top, bool) or not isinstance(top, (int, np.integer)) or not 1 <= top <= max_top:
            raise ValueError("top must be an integer in [1, %d], got %r" % (max_top, top))
        self.dataset = dataset
        self.user_pos_train = user_train_dict
        self.user_pos_test = user_test_dict
        self.top_k, self.top = int(top_k), int(top)
        self.users = list(user_test_dict.keys())
        self.group_labels, self._positions = self._user_groups(self.users, user_train_dict, group_view)
        has = np.fromiter((len(user_train_dict.get(u, [])) > 0 for u in self.users), dtype=bool, count=len(self.users))
        self._positions = [p[has[p]] for p in self._positions]             # the users whose pairs have a history to compare with
        self.columns = self.shift_columns = None    # ops.history_columns of the model history_rows() last saw; "d_<column>"...

    def _make_resident(self, device):
        """The groups over the rows of the [users*K x C] block (user position p holds rows p K .. p K + K - 1) and the test users'
        training histories, segment p = user position p, checked against the catalogue."""
        K = self.top_k
        rows = [(p[:, None] * K + np.arange(K, dtype=np.int64)[None, :]).reshape(-1) for p in self._positions]
        ptr, flat, _ = ops.ragged([self.user_pos_train.get(u, []) for u in self.users], dtype=np.int64, cast=int)
        if not self.users:
            ptr = np.zeros(2, dtype=np.int64)
        return dict(groups=group_index(rows, len(self.users) * K, device), hist=ops.HistoryIndex(ptr, flat, device, n_items=self.num_items))

    def history_rows(self, model):
        """Every (test user, rank <= K) pair's row on the device: [users*K x C] float32, columns self.columns."""
        device = self._preflight(model)
        res = self._resident(device)
        columns = self.columns = ops.history_columns(model._mods)
        spaces = ("fused",) + tuple(model._mods)
        K, nb, n_users = self.top_k, len(spaces), len(self.users)
        rows = torch.empty(n_users * K, len(columns), dtype=torch.float32, device=device)
        block = min(self.block_users, max(n_users, 1))
        idx = torch.empty(block, K, self.top, dtype=torch.int32, device=device)
        val = torch.empty(block, K, self.top, dtype=torch.float32, device=device)
        cnt = torch.empty(block, K, dtype=torch.int32, device=device)
        mean = torch.empty(block, K, dtype=torch.float32, device=device)
        for a, b, _, lists in self.top_lists(model, self.users, K, self.block_users, self.tie_order):
            at = torch.arange(a, b, dtype=torch.int64, device=device)
            out = rows[a * K:b * K]
            for s, space in enumerate(spaces):
                model.history_support_device(at, lists, res["hist"], top=self.top, space=space, out_idx=idx, out_val=val, out_cnt=cnt,
                                             out_mean=mean)
                best = val[:b - a, :, 0].reshape(-1)
                out[:, s] = best
                out[:, nb + s] = mean[:b - a].reshape(-1)
                out[:, 2 * nb + s] = 1.0 - best
            out[:, 3 * nb] = cnt[:b - a].reshape(-1).float()
        return rows

    def _table(self, rows):
        return group_table(rows, self._resident(rows.device)["groups"], len(self.group_labels))

    def evaluate(self, model, rows=None):
        """(final [1 + groups x C] float32: row 0 = all pairs with a history, then one row per user group; buf: a header of column
        names and one "%.8f" line per row, in the grouped evaluator's format). rows: history_rows(model) if the caller holds it."""
        rows = self.history_rows(model) if rows is None else rows
        final = self._table(rows)
        return final, format_table(self.columns, self.group_labels, final)

    def shift(self, rows_a, rows_b):
        """How the support changes from a to b (e.g. TE -> TIE): (final [1 + groups x C] float32, buf) -- the means of b - a per
        column, named d_<column> (self.shift_columns), in evaluate()'s grouping. rows_a / rows_b: two history_rows() results."""
        if self.columns is None or rows_a.shape != rows_b.shape or tuple(rows_a.shape) != (len(self.users) * self.top_k, len(self.columns)) \
                or rows_a.device != rows_b.device:
            raise ValueError("shift() takes the rows of two history_rows() results of this report on one device")
        self.shift_columns = tuple("d_" + c for c in self.columns)
        final = self._table(rows_b - rows_a)
        return final, format_table(self.shift_columns, self.group_labels, final)


BootstrapSummary = collections.namedtuple("BootstrapSummary", ("mean", "se", "lo", "hi", "p"))


def bootstrap_summary(reps, point, level=0.95):
    """Bootstrap replicates float64 [R x G x C] (ops.bootstrap_means) and the point estimates [G x C] -> BootstrapSummary of
    [G x C] arrays: mean = the point estimate as passed in; se = the replicates' standard deviation (ddof = 1; NaN when R = 1);
    lo, hi = the percentile interval, np.quantile at (1 - level) / 2 and 1 - (1 - level) / 2 with linear interpolation;
    p = min(1, 2 min((#{rep <= 0} + 1) / (R + 1), (#{rep >= 0} + 1) / (R + 1))), the two-sided bootstrap p-value of "the mean is 0"
    (it only means something for differences). An entry with a NaN replicate is NaN in all five. Pure numpy, float64."""
    if isinstance(level, bool) or not isinstance(level, (int, float, np.integer, np.floating)) or not 0.0 < float(level) < 1.0:
        raise ValueError("level must be a number in (0, 1), got %r" % (level,))
    reps = np.asarray(reps, dtype=np.float64)
    if reps.ndim != 3 or reps.shape[0] < 1:
        raise ValueError("reps must be [R x G x C] with R >= 1, got shape %r" % (reps.shape,))
    R = reps.shape[0]
    mean = np.array(point, dtype=np.float64)
    if mean.shape != reps.shape[1:]:
        raise ValueError("point must be [G x C] = %r, got shape %r" % (reps.shape[1:], mean.shape))
    bad = np.isnan(reps).any(axis=0)
    clean = np.where(bad[None], 0.0, reps)
    tail = (1.0 - float(level)) / 2.0
    se = np.std(clean, axis=0, ddof=1) if R > 1 else np.full(mean.shape, np.nan)
    lo = np.quantile(clean, tail, axis=0)
    hi = np.quantile(clean, 1.0 - tail, axis=0)
    below, above = (clean <= 0).sum(axis=0), (clean >= 0).sum(axis=0)
    p = np.minimum(1.0, 2.0 * np.minimum(below + 1.0, above + 1.0) / (R + 1.0))
    return BootstrapSummary(*(np.where(bad, np.nan, x) for x in (mean, se, lo, hi, p)))


SignificanceTables = collections.namedtuple("SignificanceTables", ("columns", "labels", "mean", "se", "lo", "hi", "p"), defaults=(None,))


class SignificanceReport(_Report):
    """How sure the evaluation metrics are (--significance_report=R): a non-parametric bootstrap over the test users of the
    evaluator's own per-user metric rows. metric_rows() runs the evaluator's scoring pass under the model's current predict type
    (UniEvaluator.metric_rows over default_users(), so every form of that pass applies) and compacts the rows to the shown columns
    (top_show) on the device; ops.bootstrap_means (csrc/bootstrap.hip) resamples the users of every group -- all users, then the
    group_view groups of assign_user_groups, as GroupedEvaluator splits them -- `replicates` times in ONE launch, one resample per
    (replicate, group) shared by all columns, and only the [replicates x groups x columns] float64 means reach the host, where
    bootstrap_summary turns them into the standard error and the percentile interval at `level`. shift() does the same for the
    paired differences b - a of two passes (e.g. TE -> TIE; one launch, the difference taken in float64 per user) and adds the
    two-sided bootstrap p-value of "no difference". The point estimates: row `all:` is UniEvaluator's own float32 mean of the rows,
    the groups' are ops.group_metric_means -- the numbers the [TEST] lines and the group_view table print.
    The report needs metric rows only, so unlike the other reports it does not ask for whole tables on one rank; it has been run
    on one GPU only."""

    name, needs = "significance", "predict_device"

    def __init__(self, dataset, user_train_dict, user_test_dict, top_k, metric=None, group_view=None, replicates=2000, level=0.95,
                 seed=2022, evaluator=None):
        from .evaluator import UniEvaluator, re_metric_dict
        if not isinstance(user_train_dict, dict) or not isinstance(user_test_dict, dict):
            raise TypeError("user_train_dict and user_test_dict must be dicts")
        if isinstance(replicates, bool) or not isinstance(replicates, (int, np.integer)) or not 1 <= replicates < 2 ** 31:
            raise ValueError("replicates must be an integer in [1, 2^31), got %r" % (replicates,))
        if isinstance(level, bool) or not isinstance(level, (int, float, np.integer, np.floating)) or not 0.0 < float(level) < 1.0:
            raise ValueError("level must be a number in (0, 1), got %r" % (level,))
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 2 ** 64:
            raise ValueError("seed must be an integer in [0, 2^64), got %r" % (seed,))
        if evaluator is None:
            evaluator = UniEvaluator(dataset, user_train_dict, user_test_dict, metric=metric, top_k=top_k)
        elif not isinstance(evaluator, UniEvaluator):
            raise TypeError("evaluator must be a UniEvaluator")
        self.dataset = dataset
        self.evaluator = ev = evaluator
        self.user_pos_train = user_train_dict
        self.user_pos_test = user_test_dict
        self.replicates, self.level, self.seed = int(replicates), float(level), int(seed)
        self.users = ev.default_users()
        self.columns = tuple("%s@%d" % (re_metric_dict[m], k) for m in ev.metrics for k in ev.top_show)
        # the shown columns of the [users x metrics*K] block, in metrics_info()'s order
        self._shown = (np.arange(ev.metrics_num, dtype=np.int64)[:, None] * ev.max_top + (np.asarray(ev.top_show, dtype=np.int64) - 1)[None, :]).reshape(-1)
        self.group_labels, self._positions = self._user_groups(self.users, user_train_dict, group_view)

    def _make_resident(self, device):
        """The user group index and the shown columns' indices resident on the device."""
        return dict(groups=group_index(self._positions, len(self.users), device), shown=torch.from_numpy(self._shown).to(device))

    def metric_rows(self, model):
        """The test users' metric rows under the model's current predict type, compacted to the shown columns on the device:
        ([users x Cs] float32 contiguous, column names like "Recall@10"). One evaluator scoring pass."""
        ev = self.evaluator
        rows = ev._rows_of(model, self.users, None)
        return rows.index_select(1, self._resident(rows.device)["shown"]), self.columns

    def _rows(self, rows, what):
        rows = rows[0] if isinstance(rows, tuple) else rows
        if not isinstance(rows, torch.Tensor) or tuple(rows.shape) != (len(self.users), len(self.columns)):
            raise ValueError("%s takes the rows of this report's metric_rows(): [%d x %d]" % (what, len(self.users), len(self.columns)))
        return rows

    def _tables(self, summary, with_p):
        names = ("mean", "se", "lo", "hi") + (("p",) if with_p else ())
        labels = [("%s %s" % (label.strip(), name)).ljust(20) for label in self.group_labels for name in names]
        table = np.stack([np.asarray(getattr(summary, name), dtype=np.float64) for name in names], axis=1).reshape(len(labels), -1)
        final = SignificanceTables(self.columns, list(self.group_labels), summary.mean, summary.se, summary.lo, summary.hi,
                                   summary.p if with_p else None)
        return final, format_table(self.columns, labels, table)

    def evaluate(self, model, rows=None):
        """(SignificanceTables(columns, labels, mean float32, se, lo, hi float64 [1 + groups x Cs]), buf): per group -- row 0 = all
        test users -- the point estimate, the bootstrap standard error and the percentile interval at `level` of every shown
        metric. buf: a header of column names and one "%.8f" line per (group, statistic): "all: mean", "all: se", "all: lo",
        "all: hi", ... rows: metric_rows(model) if the caller already holds it."""
        rows = self._rows(self.metric_rows(model) if rows is None else rows, "evaluate()")
        res = self._resident(rows.device)
        reps = ops.bootstrap_means(rows, res["groups"], None, self.replicates, self.seed).cpu().numpy()
        point = group_table(rows, res["groups"], len(self.group_labels))
        point[0] = np.mean(rows.cpu().numpy(), axis=0)                     # UniEvaluator._summary's expression: the [TEST] line's bits
        s = bootstrap_summary(reps, point, self.level)
        return self._tables(s._replace(mean=point), False)

    def shift(self, rows_a, rows_b):
        """How the metrics move from pass a to pass b (e.g. TE -> TIE), paired per user: (SignificanceTables(..., p), buf) over the
        differences b - a -- mean = ops.group_metric_means of the float32 difference rows, se / lo / hi from ONE launch over both
        blocks (the difference of a drawn user taken in float64), p = the two-sided bootstrap p-value of "the mean difference is 0".
        rows_a / rows_b: two metric_rows() results of this report on one device."""
        a, b = self._rows(rows_a, "shift()"), self._rows(rows_b, "shift()")
        if a.device != b.device:
            raise ValueError("shift() takes two metric_rows() results of this report on one device")
        res = self._resident(a.device)
        a, b = a.contiguous(), b.contiguous()                              # (one row stride for both blocks)
        reps = ops.bootstrap_means(a, res["groups"], None, self.replicates, self.seed, rows_b=b).cpu().numpy()
        point = group_table(b - a, res["groups"], len(self.group_labels))
        s = bootstrap_summary(reps, point, self.level)
        return self._tables(s._replace(mean=point), True)


GEOMETRY_COLUMNS = ("n", "uniformity", "erank", "top1", "rank99", "centre")
GeometryTables = collections.namedtuple("GeometryTables", ("columns", "labels", "values", "align_columns", "align_labels", "align"))


def spectrum_summary(G, m, n):
    """The spectrum of a space read from its Gram matrix: (erank, top1, rank99, centre) in float64. G [d x d] = the sum of x^ x^T and
    m [d] = the sum of x^ over n unit rows (ops.row_gram). The eigenvalues l are those of the covariance G / n - mu mu^T, mu = m / n,
    clipped at 0 (numpy's eigvalsh of the symmetrised matrix):
      erank  = exp(-sum p log p), p = l / sum l, the terms with p = 0 left out -- the effective rank of Roy & Vetterli, in [1, d];
      top1   = max p, the share of the variance along the first principal direction;
      rank99 = the number of leading directions that hold 99 % of sum l (Jing et al., ICLR'22: dimensional collapse);
      centre = |mu|: 0 for rows spread evenly round the sphere, 1 for fully collapsed rows (NaN when n < 1).
    n < 2 or sum l == 0 (all rows equal) gives NaN for erank, top1 and rank99."""
    G = np.asarray(G, dtype=np.float64)
    m = np.asarray(m, dtype=np.float64).reshape(-1)
    n = int(n)
    nan = float("nan")
    if G.ndim != 2 or G.shape[0] != G.shape[1] or m.size != G.shape[0]:
        raise ValueError("spectrum_summary: G must be [d x d] and m [d], got %s and %s" % (G.shape, m.shape))
    if n < 1:
        return nan, nan, nan, nan
    mu = m / n
    centre = float(np.sqrt(np.dot(mu, mu)))
    if n < 2:
        return nan, nan, nan, centre
    cov = G / n - np.outer(mu, mu)
    lam = np.clip(np.linalg.eigvalsh((cov + cov.T) * 0.5), 0.0, None)[::-1]
    # what rounding leaves of a zero covariance is not a spectrum: eigenvalues below d eps times the unit rows' total power (1)
    lam[lam <= lam.size * np.finfo(np.float64).eps] = 0.0
    total = lam.sum()
    if not total > 0.0:
        return nan, nan, nan, centre
    p = lam / total
    nz = p[p > 0]
    erank = float(np.exp(-(nz * np.log(nz)).sum()))
    rank99 = float(1 + np.searchsorted(np.cumsum(p), 0.99 - 1e-12))
    return erank, float(p[0]), min(rank99, float(p.size)), centre


def geometry_row(S, pairs, n_valid, G, m):
    """One row of GEOMETRY_COLUMNS (float64 [6]) from geometry_device's raw results copied to the host."""
    S, pairs, n = float(np.asarray(S).reshape(-1)[0]), int(np.asarray(pairs).reshape(-1)[0]), int(np.asarray(n_valid).reshape(-1)[0])
    return np.asarray((float(n), ops.uniformity_value(S, pairs)) + spectrum_summary(G, m, n), dtype=np.float64)


def format_geometry(tables):
    """A GeometryTables as text: the geometry rows under their header, then the alignment rows under theirs."""
    return (format_table(tables.columns, tables.labels, tables.values) + "\n"
            + format_table([c.strip() for c in tables.align_columns], tables.align_labels, tables.align))


class GeometryReport(_Report):
    """What the learned spaces look like (--geometry_report=1): per cosine space -- "fused", then every single-modal head -- the
    columns GEOMETRY_COLUMNS (n, uniformity at temperature t, erank, top1, rank99, centre; EliMRec.embedding_geometry explains them)
    of the rows `user` (all user rows) and `item` (all item rows), with group_view one row per user group (assign_user_groups over
    ALL users by their number of training items) and with item_group_view one row per item popularity group (assign_item_groups),
    uniformity and spectrum taken WITHIN the group's rows; a group with a single row has NaN there, an empty group is omitted.
    Then per space the rows align_train / align_test: the mean of 2 - 2 cos(u, i) (EliMRec.alignment_device) over the training
    pairs / the test users' test pairs -- column "all:" -- and over the pairs of each user group and each item group
    (ops.group_metric_means; NaN for a group without a pair). A pair with a row that has no norm has cosine 0 and counts as 2; they
    are not special-cased but counted: num_no_norm[(which, space)] after evaluate(). The all-pairs sums and Gram matrices come
    from EliMRec.geometry_device (csrc/geometry.hip), the d x d spectra are the host's. The spaces do not depend on the predict
    type; the tables are computed once per table version of a model and kept."""

    name, needs = "geometry", "geometry_device"

    def __init__(self, dataset, user_train_dict, user_test_dict, group_view=None, item_group_view=None, t=2.0):
        if not isinstance(user_train_dict, dict) or not isinstance(user_test_dict, dict):
            raise TypeError("user_train_dict and user_test_dict must be dicts")
        self.t = ops._geometry_t("GeometryReport", t)
        self.dataset = dataset
        self.num_users, self.num_items = U, I = int(dataset.num_users), int(dataset.num_items)
        item_counts = item_train_counts(user_train_dict, I) if item_group_view is not None else None
        # the row sets: (label, side, ids within the side; None = every row)
        self.row_sets = [("user", "user", None), ("item", "item", None)]
        user_names, item_names = [], []
        if group_view is not None:
            labels, positions, self.num_discarded = assign_user_groups(list(range(U)), user_train_dict, group_view)
            self.row_sets += [("user " + x.strip(), "user", p.astype(np.int32)) for x, p in zip(labels, positions)]
            user_names = [("(%d,%d]:" % b).ljust(12) for b in zip([0] + list(group_view[:-1]), group_view)]
        if item_group_view is not None:
            labels, positions = assign_item_groups(np.arange(I, dtype=np.int64), item_counts, item_group_view)
            self.row_sets += [("item " + x.strip(), "item", p.astype(np.int32)) for x, p in zip(labels, positions)]
            bounds = [int(b) for b in item_group_view]
            item_names = ["cold:"] + ["(%d,%d]:" % b for b in zip([0] + bounds[:-1], bounds)] + ["(%d,inf):" % bounds[-1]]
            item_names = [x.ljust(12) for x in item_names]
        self.align_columns = [ALL] + user_names + [("item " + x.strip()).ljust(12) for x in item_names]
        # the pairs and their groups as columns of align_columns (a group without a pair keeps NaN)
        self._pairs = {}
        for which, table in (("align_train", user_train_dict), ("align_test", user_test_dict)):
            users = [u for u, items in table.items() if len(items)]
            ptr, items, lens = ops.ragged([table[u] for u in users], dtype=np.int32, check=(I, "item ids must lie in [0, %d)" % I), cast=int)
            pair_user = np.repeat(np.asarray(users, dtype=np.int64), lens)
            if pair_user.size and (pair_user.min() < 0 or pair_user.max() >= U):
                raise IndexError("user ids must lie in [0, %d)" % U)
            cols, positions = [0], [np.arange(items.size, dtype=np.int64)]
            if group_view is not None and items.size:
                try:
                    labels, at, _ = assign_user_groups(users, user_train_dict, group_view)
                except ValueError:                               # no user of this pair list falls into a group
                    labels, at = [], []
                rep = np.repeat(np.arange(len(users), dtype=np.int64), lens)
                for x, p in zip(labels, at):
                    cols.append(self.align_columns.index(x))
                    positions.append(np.flatnonzero(np.isin(rep, p)))
            if item_group_view is not None and items.size:
                labels, at = assign_item_groups(items, item_counts, item_group_view)
                for x, p in zip(labels, at):
                    cols.append(self.align_columns.index(("item " + x.strip()).ljust(12)))
                    positions.append(p)
            self._pairs[which] = (pair_user, items, cols, positions)
        self.num_no_norm = {}
        self._done = {}

    def _make_resident(self, device):
        """The groups' row ids, the pairs and their group indices resident on the device."""
        rows = [None if ids is None else torch.from_numpy(np.ascontiguousarray(ids)).to(device) for _, _, ids in self.row_sets]
        pairs = {}
        for which, (users, items, cols, positions) in self._pairs.items():
            pairs[which] = (torch.from_numpy(users).to(device), torch.from_numpy(np.ascontiguousarray(items)).to(device),
                            group_index(positions, items.size, device) if items.size else None)
        return dict(rows=rows, pairs=pairs)

    def evaluate(self, model):
        """(final, buf). final = GeometryTables: values float64 [spaces x row sets, 6] with labels "<space> <row set>:" under
        `columns` = GEOMETRY_COLUMNS; align float32 [spaces x 2, 1 + groups] with labels "<space> align_train:" / "<space>
        align_test:" under align_columns ("all:", the user groups, the item groups). buf: the two tables in the effect report's
        format. A second call on the same table version of the same model returns the kept result and launches nothing."""
        device = self._preflight(model)
        if model.num_users != self.num_users:
            raise ValueError("the report was built for %d users, the model has %d" % (self.num_users, model.num_users))
        key = (id(model), str(device))
        if hasattr(model, "_cached_tables"):                     # a pending step made real first: it publishes a new table version
            model._cached_tables("the geometry report needs")
        version = getattr(model, "_table_version", None)
        hit = self._done.get(key)
        if hit is not None and version is not None and hit[0] == version:
            return hit[1], hit[2]
        res = self._resident(device)
        spaces = ("fused",) + tuple(model._mods)
        labels, raw = [], []
        for s in spaces:
            for (label, side, _), rows in zip(self.row_sets, res["rows"]):
                labels.append(("%s %s:" % (s, label.rstrip(":"))).ljust(20))
                raw.append(model.geometry_device(side, s, rows, self.t))
        values = np.stack([geometry_row(*[x.cpu().numpy() for x in r]) for r in raw])
        align = np.full((2 * len(spaces), len(self.align_columns)), np.nan, dtype=np.float32)
        sqn = model._block_sqnorms(device)
        for w, which in enumerate(("align_train", "align_test")):
            users, items, index = res["pairs"][which]
            cols = self._pairs[which][2]
            if index is None:
                continue
            rows = model.alignment_device(users, items)
            align[w::2][:, cols] = group_table(rows, index, len(cols)).T
            bare = (sqn[users] == 0) | (sqn[self.num_users + items.long()] == 0)
            for h, n in enumerate(bare.sum(dim=0).cpu().tolist()):
                self.num_no_norm[(which, spaces[h])] = int(n)
        align_labels = [("%s %s:" % (s, which)).ljust(20) for s in spaces for which in ("align_train", "align_test")]
        final = GeometryTables(GEOMETRY_COLUMNS, labels, values, tuple(self.align_columns), align_labels, align)
        buf = format_geometry(final)
        self._done[key] = (version, final, buf)
        return final, buf


def co_neighbour_columns(mods):
    """Column names of the co-neighbour report: n (the items counted), co_n, co_score, co_pop, then co_overlap_<space> per space
    (fused, then the heads' modality letters in head order)."""
    return ("n", "co_n", "co_score", "co_pop") + tuple("co_overlap_" + s for s in ("fused",) + tuple(str(m) for m in mods))


class CoNeighbourReport(_Report):
    """Are the learned neighbourhoods collaborative or content (--co_report=K)? For EVERY item its co-interaction top-k list -- the
    items the same training users took, under `measure` ("count", "cosine", "jaccard"; EliMRec.co_neighbours_device,
    csrc/cooccur.hip) -- beside its cosine top-k list in each space, the fused space and then every single-modal head
    (EliMRec.neighbours_device), items in blocks of block_items. Per item:
      co_n = the listed co-neighbours (fewer than k where fewer items share a user); co_score = their mean score;
      co_pop = their mean training interactions; co_overlap_<space> = the share of the listed co-neighbours that the space's
      cosine list also holds (ops.list_overlap / co_n).
    The table holds their means (ops.group_metric_means: float64 sums, rounded once) over all items that HAVE a co-neighbour and
    -- item_group_view -- per item popularity group (assign_item_groups over the items' training interactions); an item without
    one is in no group, decided on the host from the CSR: an item has a co-neighbour iff one of its users has degree >= 2. Column
    0 of every table row is n, the items counted; a group without such an item has n = 0 and NaN. Only the table reaches the host.
    The lists do not depend on the predict type; the table is computed once per table version of a model and kept."""

    name, needs = "co", "co_neighbours_device"

    def __init__(self, dataset, user_train_dict, k, measure="cosine", item_group_view=None):
        if not isinstance(user_train_dict, dict):
            raise TypeError("user_train_dict must be a dict")
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1 or k > min(ops.COOCCUR_MAX_K, ops.KNN_MAX_K):
            raise ValueError("k must be an integer in [1, %d], got %r" % (min(ops.COOCCUR_MAX_K, ops.KNN_MAX_K), k))
        ops._cooccur_measure("CoNeighbourReport", measure)
        self.dataset = dataset
        self.num_items = I = int(dataset.num_items)
        self.k, self.measure = int(k), measure
        self.block_items = 8192
        self.item_counts = item_train_counts(user_train_dict, I)
        # an item has a co-neighbour iff one of its users has degree >= 2 (the host's reading of the CSR, as CooccurIndex keeps it)
        has = np.zeros(I, dtype=bool)
        for items in user_train_dict.values():
            if len(items) >= 2:
                ids = np.asarray(list(items), dtype=np.int64)
                if ids.size and (ids.min() < 0 or ids.max() >= I):
                    raise IndexError("item ids must lie in [0, %d)" % I)
                if np.unique(ids).size >= 2:
                    has[ids] = True
        self.has_neighbour = has
        labels, positions = self._item_groups(np.arange(I, dtype=np.int64), self.item_counts, item_group_view)
        self.group_labels = labels
        self._positions = [p[has[p]] for p in positions]
        self._done = {}

    def _make_resident(self, device):
        """The group index, the items' training counts and the blocks' checked queries resident on the device."""
        return dict(groups=group_index(self._positions, self.num_items, device),
                    counts=torch.from_numpy(self.item_counts.astype(np.float64)).to(device), queries={})

    def co_rows(self, model):
        """Every item's row of the report on the device: ([items x C] float32, column names without n); a row of an item without
        a co-neighbour is NaN (it is in no group)."""
        device = self._preflight(model)
        res = self._resident(device)
        mods = tuple(model._mods)
        columns = co_neighbour_columns(mods)[1:]
        S, k, I = len(mods), self.k, self.num_items
        rows = torch.empty(I, len(columns), dtype=torch.float32, device=device)
        step = max(1, int(self.block_items))
        B = min(step, I)
        co_idx = torch.empty(B, k, dtype=torch.int32, device=device)
        co_val = torch.empty(B, k, dtype=torch.float32, device=device)
        idx = torch.empty(B, k, dtype=torch.int32, device=device)
        cnt = torch.empty(B, dtype=torch.int32, device=device)
        for a in range(0, I, step):
            b = min(a + step, I)
            ids = np.arange(a, b, dtype=np.int32)
            query = res["queries"].get((a, b))
            if query is None:
                query = res["queries"][(a, b)] = ops.NeighbourQuery(ids, I, device)
            model.co_neighbours_device("item", ids, k, self.measure, co_idx[:b - a], co_val[:b - a])
            listed = co_idx[:b - a] >= 0
            n = listed.sum(dim=1).double()                                         # 0 gives NaN below
            out = rows[a:b]
            out[:, 0] = n.float()
            out[:, 1] = (torch.where(listed, co_val[:b - a].double(), 0.0).sum(dim=1) / n).float()
            pop = res["counts"][co_idx[:b - a].clamp(min=0).long()]
            out[:, 2] = (torch.where(listed, pop, 0.0).sum(dim=1) / n).float()
            for h, space in enumerate(("fused",) + mods):
                model.neighbours_device("item", None, k, space, idx[:b - a], None, query=query)
                ops.list_overlap(co_idx[:b - a], idx[:b - a], cnt)
                out[:, 3 + h] = (cnt[:b - a].double() / n).float()
        return rows, columns

    def evaluate(self, model):
        """(final float64 [1 + item groups x (1 + C)]: row 0 = all items with a co-neighbour, then one row per item popularity
        group; column 0 = n, the items counted, then the float32 means; buf: a header of column names and one "%.8f" line per row,
        in the effect report's format). A second call on the same table version of the same model returns the kept result."""
        device = self._preflight(model)
        key = (id(model), str(device))
        if hasattr(model, "_cached_tables"):                     # a pending step made real first: it publishes a new table version
            model._cached_tables("the co-neighbour report needs")
        version = getattr(model, "_table_version", None)
        hit = self._done.get(key)
        if hit is not None and version is not None and hit[0] == version:
            return hit[1], hit[2]
        rows, columns = self.co_rows(model)
        index = self._resident(device)["groups"]
        means = group_table(rows, index, len(self.group_labels)).astype(np.float64)
        means[index.sizes == 0] = np.nan
        final = np.concatenate([index.sizes.astype(np.float64)[:, None], means], axis=1)
        buf = format_table(("n",) + tuple(columns), self.group_labels, final)
        self._done[key] = (version, final, buf)
        return final, buf


BASELINE_LIST_COLUMNS = ("filled", "pop", "overlap", "coverage", "gini", "entropy")
BaselineTables = collections.namedtuple("BaselineTables", ("columns", "labels", "table"))


class BaselineReport(_Report):
    """Does the model beat a neighbourhood baseline on this split, and do its lists differ from the baseline's at all
    (--baseline_report=K)? Per source a neighbour-vote recommender (EliMRec.knn_recommend_device, csrc/vote.hip) over the test users
    in the evaluator's default order, their train items as the history and left out: "co" = ItemKNN over the training graph under
    `measure`, "fused" / a head letter = content-KNN in that space of the cached tables ("v": recommend what looks like what you
    took -- the single-modal shortcut as a recommender of its own), "rp3" = RP3beta over the training graph under `alpha` and
    `beta` (EliMRec.rp3_items: the graph random walk with a popularity penalty on the target; the defaults are the commonly used
    ones, not tuned here; its list values are scaled by one power of two before they vote, and rp3_info = (scale exponent e,
    zero_votes) says what the vote's fixed point still loses), each item's `neighbours` nearest items voting;
    "ials" = the implicit-feedback ALS factor model of EliMRec.fit_ials under factors / iters / conf / reg / reg_scale (no
    neighbour vote: its lists are the top-K of x_u . y_i, EliMRec.ials_recommend_device; `neighbours` and `measure` do not apply to it;
    the defaults are not tuned here; under the table one line gives the settings and the loss after the first and the last
    half-sweep); "ease" = the closed-form EASE^R item-item model of EliMRec.fit_ease under `l2` (no neighbour vote either: its lists
    are EliMRec.ease_recommend_device's; neighbours, measure, alpha and beta do not apply to it; the default l2 = 500 is the commonly
    quoted value, not tuned here; under the table one line gives l2, the catalogue, the bytes of P and the sweep's smallest pivot).
    metric_rows() is ops.rank_metrics over those lists with the truth CSR, metric ids and shown-column layout of
    SignificanceReport.metric_rows, so the two row blocks pair user by user (SignificanceReport.shift); a -1 filler is a miss (the
    metric kernel compares ids against a truth list of ids >= 0). evaluate() gives one row per source -- with group_view one block of
    group rows per source, through ops.group_metric_means -- over the evaluator's shown metric columns and BASELINE_LIST_COLUMNS:
      filled = the mean share of the list's slots that hold an item; pop = the mean training interactions of a user's listed items
      (0 for an empty list); overlap = the share of the model's own top-K list under the current predict type that the baseline list
      also holds (ops.list_overlap / K); coverage, gini, entropy = exposure_summary of the rows' lists (ops.list_exposure).
    top_k / metric: the evaluator's; list_k: the lists' length (default and at least the largest cutoff, at most 256). The baseline
    lists do not depend on the predict type -- only `overlap` does -- and are kept as EliMRec.neighbour_lists keeps its own."""

    name, needs = "baseline", "knn_recommend_device"

    def __init__(self, dataset, user_train_dict, user_test_dict, top_k, metric=None, sources=("co",), neighbours=50, measure="cosine",
                 group_view=None, list_k=None, alpha=1.0, beta=0.6, factors=64, iters=15, conf=1.0, reg=0.01, reg_scale=0.0,
                 l2=500.0):
        from .evaluator import UniEvaluator, re_metric_dict
        if not isinstance(user_train_dict, dict) or not isinstance(user_test_dict, dict):
            raise TypeError("user_train_dict and user_test_dict must be dicts")
        if isinstance(sources, str) or not len(sources) or any(not isinstance(x, str) or not x for x in sources) or len(set(sources)) != len(sources):
            raise ValueError("sources is a sequence of distinct names: 'co', 'rp3', 'ials', 'ease', 'fused' or a head letter, got %r" % (sources,))
        if isinstance(neighbours, bool) or not isinstance(neighbours, (int, np.integer)) or not 1 <= neighbours <= ops.VOTE_MAX_K:
            raise ValueError("neighbours must be an integer in [1, %d], got %r" % (ops.VOTE_MAX_K, neighbours))
        ops._cooccur_measure("BaselineReport", measure)
        self.alpha, self.beta = ops._rp3_params("BaselineReport", alpha, beta)
        self.rp3_info = None
        self.ials_params, self.ials_objective = ops._ials_params("BaselineReport", factors, iters, conf, reg, reg_scale), None
        self.l2, self.ease_info = ops._ease_params("BaselineReport", l2, dataset.num_items if "ease" in sources else None), None
        self.evaluator = ev = UniEvaluator(dataset, user_train_dict, user_test_dict, metric=metric, top_k=top_k)
        list_k = ev.max_top if list_k is None else list_k
        if isinstance(list_k, bool) or not isinstance(list_k, (int, np.integer)) or not ev.max_top <= list_k <= ops.VOTE_MAX_K:
            raise ValueError("the lists hold the largest cutoff shown (%d) to %d items, got %r" % (ev.max_top, ops.VOTE_MAX_K, list_k))
        self.dataset = dataset
        self.num_items = I = int(dataset.num_items)
        self.user_pos_train = user_train_dict
        self.user_pos_test = user_test_dict
        self.top_k = self.k = int(list_k)
        self.sources, self.neighbours, self.measure = tuple(sources), int(neighbours), measure
        self.users = ev.default_users()
        self.metric_columns = tuple("%s@%d" % (re_metric_dict[m], k) for m in ev.metrics for k in ev.top_show)
        self.columns = self.metric_columns + BASELINE_LIST_COLUMNS
        self._shown = (np.arange(ev.metrics_num, dtype=np.int64)[:, None] * ev.max_top + (np.asarray(ev.top_show, dtype=np.int64) - 1)[None, :]).reshape(-1)
        self.item_counts = item_train_counts(user_train_dict, I)
        self.group_labels, self._positions = self._user_groups(self.users, user_train_dict, group_view)
        self.labels = [("%s %s" % (x, g.strip())).ljust(16) for x in self.sources for g in self.group_labels]
        self._lists = {}

    def _make_resident(self, device):
        """The user group index and positions, the shown columns, the items' training counts, the test users' histories (segment b =
        user b of self.users) and the truth CSR resident on the device."""
        hptr, hflat, _ = ops.ragged([self.user_pos_train.get(u, []) for u in self.users], check=(
            self.num_items, "item ids must lie in [0, %d)" % self.num_items), cast=int)
        return dict(groups=group_index(self._positions, len(self.users), device), shown=torch.from_numpy(self._shown).to(device),
                    positions=[torch.from_numpy(np.asarray(p, dtype=np.int64)).to(device) for p in self._positions],
                    counts=torch.from_numpy(self.item_counts.astype(np.float64)).to(device),
                    hist=ops.HistoryIndex(hptr if len(self.users) else np.zeros(2, dtype=np.int64), hflat, device, n_items=self.num_items),
                    truth=lists_csr(self.users, self.user_pos_test, device, unique=True))

    def knn_lists(self, model, source):
        """The baseline's lists of one source on the device: int32 [test users x K], users in the evaluator's default order, train
        items masked, -1 where fewer than K items are voted for. Kept for as long as the model keeps the source's neighbour lists."""
        if source not in self.sources:
            raise ValueError("source is one of this report's %s, got %r" % ("/".join(self.sources), source))
        device = self._preflight(model)
        res = self._resident(device)
        if source == "ials":
            return self._ials_lists(model, device)
        if source == "ease":
            return self._ease_lists(model, device, res)
        lists = model.neighbour_lists(source, self.neighbours, self.measure, self.alpha, self.beta)
        if source == "rp3":
            self.rp3_info = (lists.scale_exp, lists.zero_votes)
        hit = self._lists.get((source, str(device)))
        if hit is not None and hit[0] is lists:
            return hit[1]
        n, K = len(self.users), self.k
        idx = torch.empty(n, K, dtype=torch.int32, device=device)
        val = torch.empty(min(n, self.block_users), K, dtype=torch.float32, device=device)
        cnt = torch.empty(min(n, self.block_users), K, dtype=torch.int32, device=device)
        for a in range(0, n, self.block_users):
            b = min(n, a + self.block_users)
            model.knn_recommend_device(np.arange(a, b, dtype=np.int64), lists, res["hist"], K, None, idx[a:b], val[:b - a], cnt[:b - a])
        self._lists[(source, str(device))] = (lists, idx)
        return idx

    def _ials_lists(self, model, device):
        """knn_lists of the source "ials": the top-K of x_u . y_i under EliMRec.fit_ials(*self.ials_params) through
        EliMRec.ials_recommend_device, in blocks of block_users with the train items masked. Kept for as long as the model keeps
        the fit; the neighbour-vote settings (neighbours, measure) do not apply."""
        fit = model.fit_ials(*self.ials_params)
        self.ials_objective = (float(fit.objective[0]), float(fit.objective[-1]))
        hit = self._lists.get(("ials", str(device)))
        if hit is not None and hit[0] is fit:
            return hit[1]
        n, K = len(self.users), self.k
        idx = torch.empty(n, K, dtype=torch.int32, device=device)
        val = torch.empty(min(n, self.block_users), K, dtype=torch.float32, device=device)
        for a in range(0, n, self.block_users):
            b = min(n, a + self.block_users)
            ptr, flat, _ = ops.ragged([self.user_pos_train.get(u, []) for u in self.users[a:b]], check=(
                self.num_items, "item ids must lie in [0, %d)" % self.num_items), cast=int)
            model.ials_recommend_device(np.asarray(self.users[a:b], dtype=np.int64), fit, K, (ptr, flat), idx[a:b], val[:b - a])
        self._lists[("ials", str(device))] = (fit, idx)
        return idx

    def _ease_lists(self, model, device, res):
        """knn_lists of the source "ease": the top-K of the EASE scores under EliMRec.fit_ease(self.l2) through
        EliMRec.ease_recommend_device, in blocks of block_users, the train items as the history and left out. Kept for as long as
        the model keeps the fit; the neighbour-vote settings do not apply."""
        fit = model.fit_ease(self.l2)
        self.ease_info = (fit.l2, int(fit.P.shape[0]), fit.bytes, fit.pivot_min)
        hit = self._lists.get(("ease", str(device)))
        if hit is not None and hit[0] is fit:
            return hit[1]
        n, K = len(self.users), self.k
        idx = torch.empty(n, K, dtype=torch.int32, device=device)
        val = torch.empty(min(n, self.block_users), K, dtype=torch.float32, device=device)
        for a in range(0, n, self.block_users):
            b = min(n, a + self.block_users)
            model.ease_recommend_device(np.arange(a, b, dtype=np.int64), fit, K, res["hist"], None, idx[a:b], val[:b - a])
        self._lists[("ease", str(device))] = (fit, idx)
        return idx

    def metric_rows(self, model, source):
        """The test users' metric rows of one source's lists, compacted to the shown columns on the device: ([users x Cs] float32
        contiguous, column names like "Recall@10") -- SignificanceReport.metric_rows' layout and user order."""
        ev = self.evaluator
        lists = self.knn_lists(model, source)
        res = self._resident(lists.device)
        first = lists if self.k == ev.max_top else lists[:, :ev.max_top].contiguous()
        out = torch.empty(len(self.users), ev.metrics_num * ev.max_top, dtype=torch.float32, device=lists.device)
        if len(self.users):
            ops.rank_metrics(first, res["truth"][0], res["truth"][1], ev.metrics, out)
        return out.index_select(1, res["shown"]), self.metric_columns

    def evaluate(self, model):
        """(BaselineTables(columns, labels, table float64 [sources x (1 + groups) x C]), buf): per source row "all:" and then the
        group_view groups, over self.columns. buf: a header of column names and one "%.8f" line per row; with "rp3" among the
        sources one more line: rp3: alpha=... beta=... scale=2^e zero_votes=... (the share of its listed neighbour entries whose
        fixed-point vote is 0)."""
        device = self._preflight(model)
        res = self._resident(device)
        n, K, G, Cs = len(self.users), self.k, len(self.group_labels), len(self.metric_columns)
        own = torch.empty(n, K, dtype=torch.int32, device=device)
        for a, b, _, idx in self.top_lists(model, self.users, K, self.block_users, self.tie_order):
            own[a:b] = idx
        table = np.zeros((len(self.sources) * G, len(self.columns)), dtype=np.float64)
        shared = torch.empty(n, dtype=torch.int32, device=device)
        for s, source in enumerate(self.sources):
            lists = self.knn_lists(model, source)
            rows = torch.empty(n, Cs + 3, dtype=torch.float32, device=device)
            rows[:, :Cs] = self.metric_rows(model, source)[0]
            listed = lists >= 0
            filled = listed.sum(dim=1).double()
            rows[:, Cs] = (filled / K).float()
            pop = torch.where(listed, res["counts"][lists.clamp(min=0).long()], 0.0).sum(dim=1) / filled.clamp(min=1.0)
            rows[:, Cs + 1] = pop.float()
            if n:
                ops.list_overlap(own, lists, shared)
            rows[:, Cs + 2] = (shared.double() / K).float()
            table[s * G:(s + 1) * G, :Cs + 3] = group_table(rows, res["groups"], G)
            for g, at in enumerate(res["positions"]):
                counts = torch.zeros(self.num_items, dtype=torch.int32, device=device)
                if at.numel():
                    ops.list_exposure(lists.index_select(0, at).contiguous(), counts)
                table[s * G + g, Cs + 3:] = exposure_summary(counts.cpu().numpy(), [np.arange(self.num_items)])[0, 1:4]
        final = BaselineTables(self.columns, list(self.labels), table)
        buf = format_table(final.columns, final.labels, final.table)
        if "rp3" in self.sources:
            buf += "\nrp3: alpha=%g beta=%g scale=2^%d zero_votes=%.6f" % ((self.alpha, self.beta) + self.rp3_info)
        if "ials" in self.sources:
            buf += "\nials: factors=%d iters=%d conf=%g reg=%g reg_scale=%g objective=%.8g -> %.8g" % (self.ials_params[:5] + self.ials_objective)
        if "ease" in self.sources:
            buf += "\nease: l2=%g items=%d bytes=%d pivot_min=%.8g" % self.ease_info
        return final, buf


COLDSTART_VARIANTS = ("catalogue", "content", "mean_id")


def cold_test_items(user_train_dict, user_test_dict, num_items):
    """The cold test items of a split: catalogue items without a training interaction and with at least one test interaction ->
    (their ids int64 ascending, the (user, item) test pairs on them in user_test_dict order)."""
    counts = item_train_counts(user_train_dict, num_items)
    pairs = [(u, int(i)) for u, items in user_test_dict.items() for i in items if 0 <= int(i) < num_items and counts[int(i)] == 0]
    return np.unique(np.asarray([i for _, i in pairs], dtype=np.int64)), pairs


def coldstart_columns(ks):
    return ("items", "pairs", "rank", "pct", "rr") + tuple("hit@%d" % int(k) for k in ks)


def coldstart_row(rank, n_cand, ks, n_items):
    """One row of the cold-start table from the pairs' ranks and candidate counts (host, float64): the number of items and pairs,
    then the pair means of rank, pct = rank / (n_cand - 1) (0 when n_cand <= 1), rr = 1 / (rank + 1) and hit@K = (rank < K)."""
    rank, n_cand = np.asarray(rank, dtype=np.float64), np.asarray(n_cand, dtype=np.float64)
    pct = np.where(n_cand > 1, rank / np.maximum(n_cand - 1.0, 1.0), 0.0)
    cols = [rank, pct, 1.0 / (rank + 1.0)] + [(rank < k).astype(np.float64) for k in ks]
    return np.asarray([float(n_items), float(rank.size)] + [float(c.mean()) if c.size else np.nan for c in cols])


def format_coldstart(columns, labels, table):
    """format_table, or the one line of a split without cold test items (columns = None)."""
    if columns is None:
        return "no cold test item in this split (every test item has a training interaction): nothing to report"
    return format_table(columns, labels, table)


class ColdStartReport(_Report):
    """How the model serves items it has no interaction for (--coldstart_report=K): over the cold test items of the split (catalogue
    items without a training interaction and with a test interaction) and the (test user, cold test item) pairs on them, the pair
    means of the rank report's columns for three variants of the item's row:
      catalogue  the item as trained -- its row of the cached table, with its never-updated id row (ops.rank_targets);
      content    its row folded in from its features with a zero id row (EliMRec.fold_in_items, ops.rank_values, its own catalogue
                 column not counted);
      mean_id    the same with the mean embedding row of the items that have training interactions as its id row.
    Ranks are exact, over the whole catalogue with the user's train items masked, under the model's current predict type. Tables:
    [1 + user groups] blocks of one row per variant; the pair rows and their means come from ops.rank_pair_rows /
    ops.group_metric_means. Users go in blocks whose score block stays within block_bytes."""

    name, needs = "coldstart", "predict_new_items_device"

    def __init__(self, dataset, user_train_dict, user_test_dict, top_k, group_view=None):
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
        self.columns = coldstart_columns(self.ks)
        self.block_bytes = 2 << 30
        self.items, pairs = cold_test_items(user_train_dict, user_test_dict, I)
        self.train_items = np.flatnonzero(item_train_counts(user_train_dict, I) > 0)
        self.users, per_user = [], []
        for u, i in pairs:
            if not self.users or self.users[-1] != u:
                self.users.append(u)
                per_user.append([])
            per_user[-1].append(i)
        self.pair_ptr, self.pair_items, lens = ops.ragged(per_user, dtype=np.int32)
        self.pair_user = np.repeat(np.arange(len(self.users), dtype=np.int64), lens)
        self.pair_q = np.searchsorted(self.items, self.pair_items).astype(np.int64)         # position among the cold items
        self.pair_n_cand = np.asarray([I - len(set(int(i) for i in user_train_dict.get(self.users[p], []))) for p in self.pair_user],
                                      dtype=np.int32)
        self.num_pairs = int(self.pair_items.size)
        self.group_labels, self._user_pos = ([ALL], []) if not self.num_pairs else self._user_groups(self.users, user_train_dict, group_view)
        self._pair_pos = [np.flatnonzero(np.isin(self.pair_user, p)) for p in self._user_pos]
        self.group_items = [int(np.unique(self.pair_items[p]).size) for p in self._pair_pos]

    @property
    def block_users(self):
        return max(1, int(self.block_bytes) // ((self.num_items + 3) // 4 * 16))

    def _make_resident(self, device):
        return dict(pair_n_cand=torch.from_numpy(self.pair_n_cand).to(device), groups=group_index(self._pair_pos, self.num_pairs, device))

    def new_items(self, model, variant):
        """The cold test items folded in from the model's own feature rows: variant 'content' (zero id rows) or 'mean_id'."""
        feats = {m: getattr(model, m + "_feat")[torch.from_numpy(self.items).to(getattr(model, m + "_feat").device)] for m in model._mods}
        ids = None
        if variant == "mean_id":
            model.plugin.sync_params()
            w = model.embedding_item.weight.detach()
            mean = w[torch.from_numpy(self.train_items).to(w.device)].double().mean(0).float() if self.train_items.size else w.new_zeros(w.shape[1])
            ids = mean.expand(self.items.size, -1).contiguous()
        return model.fold_in_items(feats, id_rows=ids, normalized=True)

    def pair_ranks(self, model):
        """The exact rank of every pair per variant under the model's current predict type: int32 [3 x num_pairs] on the device.
        Per user block ONE predict_device call into a score block serves all three variants: ops.rank_targets over the pairs' own
        columns, then one ops.rank_values call whose CSR lists, per user, the content values of its pairs and then the mean_id
        values (gathered from predict_new_items_device's [users x cold items] blocks), each with its own column skipped."""
        device = self._preflight(model)
        V = len(COLDSTART_VARIANTS)
        ranks = torch.empty(V, self.num_pairs, dtype=torch.int32, device=device)
        new = [self.new_items(model, v) for v in COLDSTART_VARIANTS[1:]]
        I, step = self.num_items, self.block_users
        lds = (I + 3) // 4 * 4                    # rows 16-byte aligned: the counts take their 16-byte loads
        for a in range(0, len(self.users), step):
            b = min(a + step, len(self.users))
            lo, hi = int(self.pair_ptr[a]), int(self.pair_ptr[b])
            n = hi - lo
            users = torch.as_tensor(np.asarray(self.users[a:b], dtype=np.int64)).to(device)
            train = lists_csr(self.users[a:b], self.user_pos_train, device, cast=int)
            train = train if train[1].numel() else (None, None)
            block = torch.empty(b - a, lds, dtype=torch.float32, device=device)[:, :I]
            model.predict_device(users, scores=block, train_ptr=train[0], train_items=train[1])
            ptr = self.pair_ptr[a:b + 1] - lo
            ops.rank_targets(block, ptr, self.pair_items[lo:hi], ranks[0, lo:hi])
            # per user its pairs once per folded variant: list position = (V - 1) * ptr[u] + v * len(u) + (position among the user's pairs)
            lens = np.diff(ptr)
            first = np.repeat(ptr[:-1], lens)
            within = np.arange(n, dtype=np.int64) - first
            at = [torch.from_numpy((V - 1) * first + v * np.repeat(lens, lens) + within).to(device) for v in range(V - 1)]
            rows = torch.from_numpy(self.pair_user[lo:hi] - a).to(device)
            cols = torch.from_numpy(self.pair_q[lo:hi]).to(device)
            vals = torch.empty((V - 1) * n, dtype=torch.float32, device=device)
            skip = np.empty((V - 1) * n, dtype=np.int32)
            for v, handle in enumerate(new):
                scores = model.predict_new_items_device(users, handle, torch.empty(b - a, handle.n_items, dtype=torch.float32, device=device))
                vals[at[v]] = scores[rows, cols]
                skip[at[v].cpu().numpy()] = self.pair_items[lo:hi]
            out = ops.rank_values(block, (V - 1) * ptr, vals, torch.empty((V - 1) * n, dtype=torch.int32, device=device), skip=skip)
            for v in range(V - 1):
                ranks[1 + v, lo:hi] = out[at[v]]
        return ranks

    def evaluate(self, model, ranks=None):
        """(final, buf). final float32 [1 + user groups x 3 variants x columns] (columns: items, pairs, then the pair means of rank,
        pct, rr, hit@K) -- or None for a split without cold test items, with the one line that says so as buf."""
        if not self.num_pairs:
            self._preflight(model)
            return None, format_coldstart(None, None, None)
        if ranks is None:
            ranks = self.pair_ranks(model)
        res = self._resident(ranks.device)
        G, V, C = len(self.group_labels), len(COLDSTART_VARIANTS), len(self.columns)
        final = np.zeros((G, V, C), dtype=np.float32)
        order = [0, 2, 1] + list(range(3, 3 + len(self.ks)))           # rank_pair_rows gives rank, rr, pct, hit@K
        for v in range(V):
            rows = torch.empty(self.num_pairs, 3 + len(self.ks), dtype=torch.float32, device=ranks.device)
            ops.rank_pair_rows(ranks[v].contiguous(), res["pair_n_cand"], self.ks, rows)
            final[:, v, 2:] = group_table(rows, res["groups"], G)[:, order]
        final[:, :, 0] = np.asarray(self.group_items, dtype=np.float32)[:, None]
        final[:, :, 1] = np.asarray([p.size for p in self._pair_pos], dtype=np.float32)[:, None]
        return final, self._format(self.columns, final)

    def _format(self, columns, final):
        labels = [(v + ":").ljust(12) for v in COLDSTART_VARIANTS]
        return "\n".join(("%s\n" % g.strip() if len(self.group_labels) > 1 else "") + format_coldstart(columns, labels, final[k])
                         for k, g in enumerate(self.group_labels))

    def shift(self, final_a, final_b):
        """TE -> TIE: (final_b - final_a over the mean columns, buf) with columns d_<column>."""
        if final_a is None or final_b is None:
            return None, format_coldstart(None, None, None)
        delta = (final_b - final_a)[:, :, 2:]
        return delta, self._format(tuple("d_" + c for c in self.columns[2:]), delta)


NEWUSER_VARIANTS = ("trained", "history", "history+mean_id")


def fold_in_weights(adj_type, hist_ptr, hist_items, item_degree):
    """The weights of EliMRec.fold_in_users: per history entry the off-diagonal value the frozen adjacency (create_adj_mat) would
    give the edge (new user q, item i), with n = len(H_q) the new user's degree -- repeats count as given -- and deg_i the item's
    TRAINING degree: 'plain' 1; 'gcmc' and 'mean' (anything else, as create_adj_mat reads it) 1 / n; 'norm' 1 / (n + 1) (the row
    is normalised with its diagonal, which itself carries nothing: a new user has no trained row); 'pre' 1 / sqrt(n max(deg_i, 1))
    (a cold item takes degree 1: the new edge is its first). Pure host arithmetic in float64, rounded once -> float32
    [len(hist_items)]. hist_ptr int64 [Q + 1] ascending from 0 to len(hist_items) (ValueError), every id in [0, len(item_degree))
    (IndexError)."""
    ptr = np.ascontiguousarray(np.asarray(hist_ptr), dtype=np.int64).reshape(-1)
    items = np.asarray(hist_items).reshape(-1)
    deg = np.asarray(item_degree).reshape(-1)
    if items.size and not np.issubdtype(items.dtype, np.integer):
        raise TypeError("hist_items must hold integers, got %s" % items.dtype)
    if ptr.size < 1 or ptr[0] != 0 or ptr[-1] != items.size or (np.diff(ptr) < 0).any():
        raise ValueError("hist_ptr must ascend from 0 to len(hist_items) = %d" % items.size)
    items = items.astype(np.int64)
    if items.size and (int(items.min()) < 0 or int(items.max()) >= deg.size):
        raise IndexError("history item ids span [%d, %d], the catalogue has %d items" % (int(items.min()), int(items.max()), deg.size))
    n = np.repeat(np.diff(ptr), np.diff(ptr)).astype(np.float64)
    if adj_type == "plain":
        w = np.ones(items.size, dtype=np.float64)
    elif adj_type == "norm":
        w = 1.0 / (n + 1.0)
    elif adj_type == "pre":
        w = 1.0 / np.sqrt(n * np.maximum(deg[items].astype(np.float64), 1.0))
    else:
        w = 1.0 / n
    return w.astype(np.float32)


def newuser_columns(metric_columns):
    return ("users",) + tuple(metric_columns) + ("overlap", "cos")


def newuser_overall_metrics(metric_rows):
    """The `all:` row's metric columns from per-user metric rows [n x Cs] (host, float32): UniEvaluator._summary's own expression,
    numpy's float32 mean over the users -- a column's mean does not depend on which other columns stand beside it, so the `trained`
    variant repeats the test pass's numbers bit for bit."""
    rows = np.ascontiguousarray(metric_rows, dtype=np.float32)
    return np.mean(rows, axis=0) if rows.shape[0] else np.full(rows.shape[1], np.nan, dtype=np.float32)


def format_newuser(columns, labels, table):
    """format_table, or the one line of a split without a test user that has a training history (columns = None)."""
    if columns is None:
        return "no test user with a training history in this split: nothing to report"
    return format_table(columns, labels, table)


class NewUserReport(_Report):
    """What serving a user WITHOUT retraining costs (--newuser_report=K): over the test users with a non-empty training history, one
    row per variant of the user's row of the cached table:
      trained          the cached row: the evaluator's own lists;
      history          the row folded in from the user's training items with a zero id row (EliMRec.fold_in_users);
      history+mean_id  the same with id_rows="mean".
    Columns: users, the evaluator's shown metrics at top_k (ops.rank_metrics over each variant's top-K lists with the train items
    masked, the evaluator's tie order: the `trained` row of the `all:` block repeats the test pass's numbers bit for bit when every
    test user has a training history and K does not exceed the largest of the topks), overlap = the share of the trained top-k
    list the variant keeps (ops.list_overlap; k = the switch's K) and cos = the mean cosine between the variant's fused row and the
    trained fused row. Overall and, with group_view, per user group (ops.group_metric_means). Users go in blocks of block_users;
    the tables reach the host, and -- for the `all:` block, as in the evaluator's own summary -- the users' shown metric rows."""

    name, needs = "newuser", "fold_in_users"
    tie_order = "reference"               # the evaluator's default; BasicModel hands the test evaluator's over

    def __init__(self, dataset, user_train_dict, user_test_dict, top_k, group_view=None, metric=None, k=None):
        from .evaluator import UniEvaluator, re_metric_dict
        if not isinstance(user_train_dict, dict) or not isinstance(user_test_dict, dict):
            raise TypeError("user_train_dict and user_test_dict must be dicts")
        ks = list(top_k) if isinstance(top_k, (list, tuple, np.ndarray)) else [top_k]
        if not ks or any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) or x < 1 for x in ks):
            raise ValueError("top_k must be a positive integer or a list of them, got %r" % (top_k,))
        ks = sorted(set(int(x) for x in ks))
        k = ks[-1] if k is None else k
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= ks[-1]:
            raise ValueError("k, the overlap's list length, must lie in [1, the largest cutoff %d], got %r" % (ks[-1], k))
        if ks[-1] > 256:
            raise ValueError("the lists hold at most 256 items, got a cutoff of %d" % ks[-1])
        self.evaluator = ev = UniEvaluator(dataset, user_train_dict, user_test_dict, metric=metric, top_k=ks)
        self.dataset = dataset
        self.num_items = int(dataset.num_items)
        self.user_pos_train = user_train_dict
        self.user_pos_test = user_test_dict
        self.top_k, self.k = int(ev.max_top), int(k)
        self.users = [u for u in ev.default_users() if len(user_train_dict.get(u, []))]
        self.metric_columns = tuple("%s@%d" % (re_metric_dict[m], c) for m in ev.metrics for c in ev.top_show)
        self.columns = newuser_columns(self.metric_columns)
        self._shown = (np.arange(ev.metrics_num, dtype=np.int64)[:, None] * ev.max_top + (np.asarray(ev.top_show, dtype=np.int64) - 1)[None, :]).reshape(-1)
        self.group_labels, self._positions = ([ALL], []) if not self.users else self._user_groups(self.users, user_train_dict, group_view)

    def _make_resident(self, device):
        return dict(groups=group_index(self._positions, len(self.users), device), shown=torch.from_numpy(self._shown).to(device))

    def user_rows(self, model):
        """The per-user rows of every variant on the device: float32 [3 x users x (Cs + 2)] -- the shown metrics, overlap, cos --
        and the variants' top-K lists int32 [3 x users x K] (what the tests replay on the host)."""
        device = self._preflight(model)
        res = self._resident(device)
        ev, K, k, d = self.evaluator, self.top_k, self.k, model.latent_dim
        n, Cs, V = len(self.users), len(self.metric_columns), len(NEWUSER_VARIANTS)
        rows = torch.empty(V, n, Cs + 2, dtype=torch.float32, device=device)
        lists = torch.empty(V, n, K, dtype=torch.int32, device=device)
        for a in range(0, n, self.block_users):
            b = min(n, a + self.block_users)
            users = self.users[a:b]
            train_ptr, train_items = lists_csr(users, self.user_pos_train, device, cast=int)
            truth_ptr, truth_items = lists_csr(users, self.user_pos_test, device, unique=True)
            users_t = torch.as_tensor(np.asarray(users, dtype=np.int64)).to(device)
            lists[0, a:b] = model.predict_device(users_t, top_k=K, train_ptr=train_ptr, train_items=train_items, tie_order=self.tie_order)[0]
            own = model._ws["Y"][users_t, :d].double()
            sq_own = (own * own).sum(1)
            metrics = torch.empty(b - a, ev.metrics_num * ev.max_top, dtype=torch.float32, device=device)
            shared = torch.empty(b - a, dtype=torch.int32, device=device)
            first = lists[0, a:b, :k].contiguous()
            for v in range(V):
                fused = own
                if v:
                    new = model.fold_in_users([self.user_pos_train[u] for u in users], id_rows=None if v == 1 else "mean")
                    lists[v, a:b] = model._new_user_scores(new, top_k=K, train_ptr=new.hist_ptr, train_items=new.hist_items,
                                                           tie_order=self.tie_order)[0]
                    fused = new.rows[:, :d].double()
                ops.rank_metrics(lists[v, a:b].contiguous(), truth_ptr, truth_items, ev.metrics, metrics)
                rows[v, a:b, :Cs] = metrics.index_select(1, res["shown"])
                ops.list_overlap(first, lists[v, a:b, :k].contiguous(), shared)
                rows[v, a:b, Cs] = (shared.double() / k).float()
                den = torch.sqrt(sq_own * (fused * fused).sum(1))
                rows[v, a:b, Cs + 1] = torch.where(den > 0, (own * fused).sum(1) / torch.where(den > 0, den, torch.ones_like(den)),
                                                   torch.zeros_like(den)).float()
        return rows, lists

    def evaluate(self, model, rows=None):
        """(final float32 [1 + user groups x 3 variants x columns], buf) -- or (None, the one line that says so) for a split without
        a test user that has a training history. The `all:` block's metric columns are the evaluator's own overall expression over
        the users' metric rows (newuser_overall_metrics: the bits UniEvaluator.evaluate returns when every test user has a
        training history); the group blocks, and overlap / cos everywhere, are ops.group_metric_means' float64 means."""
        if not self.users:
            self._preflight(model)
            return None, format_newuser(None, None, None)
        if rows is None:
            rows = self.user_rows(model)[0]
        res = self._resident(rows.device)
        G, V = len(self.group_labels), len(NEWUSER_VARIANTS)
        final = np.zeros((G, V, len(self.columns)), dtype=np.float32)
        Cs = len(self.metric_columns)
        for v in range(V):
            final[:, v, 1:] = group_table(rows[v], res["groups"], G)
            final[0, v, 1:1 + Cs] = newuser_overall_metrics(rows[v][:, :Cs].contiguous().cpu().numpy())
        final[:, :, 0] = np.asarray([p.size for p in self._positions], dtype=np.float32)[:, None]
        return final, self._format(self.columns, final)

    def _format(self, columns, final):
        labels = [(v + ":").ljust(16) for v in NEWUSER_VARIANTS]
        return "\n".join(("%s\n" % g.strip() if len(self.group_labels) > 1 else "") + format_newuser(columns, labels, final[i])
                         for i, g in enumerate(self.group_labels))

    def shift(self, final_a, final_b):
        """TE -> TIE: (final_b - final_a over the mean columns, buf) with columns d_<column>."""
        if final_a is None or final_b is None:
            return None, format_newuser(None, None, None)
        delta = (final_b - final_a)[:, :, 1:]
        return delta, self._format(tuple("d_" + c for c in self.columns[1:]), delta)
