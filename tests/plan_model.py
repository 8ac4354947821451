"""An exact numpy model of the batch planner in csrc/bpr.hip (elimrec_batch_plan / elimrec_segment_plan), of segment_sum_kernel and of
the two row copies. Integer work and fixed-order float32 sums only, so every comparison with the GPU is bit for bit. No project imports.

The three planner forms (one workgroup, device-wide bitmap, radix sort) promise the same plan, so there is one model. n_lo needs a word:
the bitmap forms compute the rank of split_key in the bitmap (all of n_act when split_key >= key_space, the rank of key 0 -- zero -- when
split_key <= 0); the radix-sort form does not know key_space: finalize_segments_kernel writes 0 when the smallest sorted key is
>= split_key, and otherwise (index of the last segment whose key is < split_key) + 1. For keys in [0, key_space) both are the number of
active keys below split_key, which is what plan() returns."""
import collections

import numpy as np

Plan = collections.namedtuple("Plan", "active seg_info slot_seg members seg_start bitmap active_rows")


def plan(keys, split_key, key_space, pad_key=None):
    """keys: n ids in [0, key_space) (key_space = 0: unknown, any non-negative int32). ->
    active       int32 [n_act]      the unique keys, ascending
    seg_info     int32 [8]          n_act, n_lo, 0, n_lo, n_lo, n_act, 0, n_act
    slot_seg     int32 [n]          index into `active` of every slot's key
    members      int32 [n]          the slots grouped by segment, ascending slot inside a segment (a stable sort of the keys)
    seg_start    int32 [n_act + 1]  members[seg_start[s] : seg_start[s + 1]] is the list of segment s
    bitmap       uint32 [(key_space + 31) // 32] (little-endian bit order: bit k & 31 of word k >> 5), None when key_space = 0
    active_rows  int32 [n]          `active`, then pad_key + r at every r in [n_act, n); None when pad_key is None"""
    keys = np.asarray(keys, dtype=np.int64)
    n = len(keys)
    assert n > 0 and keys.min() >= 0 and (key_space == 0 or keys.max() < key_space)
    active = np.unique(keys)
    n_act = len(active)
    n_lo = int(np.count_nonzero(active < split_key))
    seg_info = np.array([n_act, n_lo, 0, n_lo, n_lo, n_act, 0, n_act], dtype=np.int32)
    slot_seg = np.searchsorted(active, keys).astype(np.int32)
    members = np.argsort(keys, kind="stable").astype(np.int32)
    seg_start = np.concatenate([[0], np.cumsum(np.bincount(slot_seg, minlength=n_act))]).astype(np.int32)
    bitmap = None
    if key_space > 0:
        bitmap = np.zeros((key_space + 31) // 32, dtype=np.uint32)
        np.bitwise_or.at(bitmap, active >> 5, np.uint32(1) << (active & 31).astype(np.uint32))
    active_rows = None
    if pad_key is not None:
        active_rows = (np.int64(pad_key) + np.arange(n, dtype=np.int64)).astype(np.int32)
        active_rows[:n_act] = active
    return Plan(active.astype(np.int32), seg_info, slot_seg, members, seg_start, bitmap, active_rows)


def batch_keys(users, pos, neg, U, I):
    """-> (keys int32 [3B], err_bits). Slot 3b + j reads users[b] / pos[b] / neg[b] for j = 0 / 1 / 2; an id outside [0, U) (users) or
    [0, I) (items), compared as int64, sets bit j and counts as id 0; the key is the id for a user and U + id for an item."""
    cols = [np.asarray(a, dtype=np.int64) for a in (users, pos, neg)]
    B = len(cols[0])
    keys = np.empty(3 * B, dtype=np.int64)
    err = 0
    for j, (ids, lim, base) in enumerate(zip(cols, (U, I, I), (0, U, U))):
        bad = (ids < 0) | (ids >= lim)
        if bad.any():
            err |= 1 << j
        keys[j::3] = base + np.where(bad, 0, ids)
    return keys.astype(np.int32), err


def segment_sums_f32(rows, members, seg_start, scale=None):
    """segment_sum_kernel exactly: per segment and column a float32 accumulator starts at +0, adds the member rows one by one in list
    order (float32 additions, nothing fused), then one float32 multiply by scale (1 when None). -> float32 [n_seg, cols]."""
    rows = np.asarray(rows, dtype=np.float32)
    members = np.asarray(members, dtype=np.int64)
    seg_start = np.asarray(seg_start, dtype=np.int64)
    lens = np.diff(seg_start)
    acc = np.zeros((len(lens), rows.shape[1]), dtype=np.float32)
    order = np.argsort(-lens, kind="stable")                       # segments by falling length: step k touches a prefix of them
    sorted_lens = lens[order]
    for k in range(int(lens.max()) if len(lens) else 0):
        live = order[:np.searchsorted(-sorted_lens, -k, side="left")]          # the segments with more than k members
        acc[live] = acc[live] + rows[members[seg_start[live] + k]]
    sc = np.float32(1.0 if scale is None else scale)
    return (acc * sc).astype(np.float32)


def triplet_rows(users, pos, neg, U, src=None, cols=None):
    """elimrec_triplet_rows (unchecked): -> (rows int32 [3B], the leading `cols` columns of src at those rows, or None)."""
    users, pos, neg = (np.asarray(a, dtype=np.int64) for a in (users, pos, neg))
    rows = np.empty(3 * len(users), dtype=np.int64)
    rows[0::3], rows[1::3], rows[2::3] = users, U + pos, U + neg
    out = None if src is None else np.ascontiguousarray(np.asarray(src)[rows, :cols])
    return rows.astype(np.int32), out


def gather_rows(src, rows, dst, count=None):
    """elimrec_gather_rows: dst[r] = src[rows[r]] for r < min(count, len(rows)); the other rows of dst stay. -> a copy of dst."""
    out = np.array(dst, copy=True)
    lim = len(rows) if count is None else min(int(count), len(rows))
    out[:lim] = np.asarray(src)[np.asarray(rows[:lim], dtype=np.int64)]
    return out
