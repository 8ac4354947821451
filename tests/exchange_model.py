"""Exact host models of the kernels that move rows between ranks in the multi-rank step (csrc/lookup.hip: counts, pack, unpack,
peer_cols_to_rows; csrc/merge_rows.h + csrc/slab.hip: merge_rows and rows_bitmap), and the case builders of
tests/test_exchange_gpu.py. numpy only: nothing here calls a project kernel.

All of these operations are exact -- copies, 16-bit -> fp32 widening, integer range searches and fp32 additions in a fixed order
(rank order, then block order; sums only, so no fma) -- and the models produce the very bits the kernels must produce. The
models work from the definitions (who owns a node, which list names it), not from the kernels' binary searches.

Conventions: an id list is int32, ascending without repeats in its valid prefix, negative padding (PAD) behind it. Node n < U is
user n, node U + i is item i. Rank o owns the users [ub[o], ub[o+1]) and the items [ib[o], ib[o+1]); its local table holds its
users, then its items.
"""
import types

import numpy as np

PAD = -(1 << 30)
MAX_RANKS = 16               # lookup.MAX_RANKS / ELIMREC_MAX_RANKS
SLAB_MAX_RANKS = 64          # kSlabMaxRanks
GRID_ROWS = 2048 * 4         # rows one trip of the pack / unpack grid covers: at most 2048 workgroups of 4 rows
LANES = 64                   # column loop of pack (16-byte pieces) and unpack (float4 pieces): one wave per row


def merge_rows_chunk(N):
    """Rows per workgroup of merge_rows / rows_bitmap: about 1024 workgroups, whole bitmap words, 32 at least."""
    chunk = (int(N) + 1023) // 1024
    chunk = (chunk + 31) // 32 * 32
    return max(chunk, 32)


def roundup(n, m):
    return (int(n) + m - 1) // m * m


def valid(lst):
    lst = np.asarray(lst)
    return lst[lst >= 0].astype(np.int64)


def owner_of(node, U, ub, ib):
    """(owner, row in the owner's local table) of one node, by scanning the blocks."""
    W = len(ub) - 1
    for o in range(W):
        if node < U and ub[o] <= node < ub[o + 1]:
            return o, int(node - ub[o])
        if node >= U and ib[o] <= node - U < ib[o + 1]:
            return o, int((ub[o + 1] - ub[o]) + (node - U - ib[o]))
    raise ValueError("node %d has no owner" % node)


def owners(nodes, U, ub, ib):
    """Vector form of owner_of: (owner, local row) arrays."""
    nodes = np.asarray(nodes, dtype=np.int64)
    ub, ib = np.asarray(ub, dtype=np.int64), np.asarray(ib, dtype=np.int64)
    user = nodes < U
    ou = np.searchsorted(ub, nodes, side="right") - 1             # the last o with ub[o] <= node: its block is not empty
    oi = np.searchsorted(ib, nodes - U, side="right") - 1
    o = np.where(user, ou, oi)
    W = len(ub) - 1
    oc = np.clip(o, 0, W - 1)
    loc = np.where(user, nodes - ub[oc], (ub[oc + 1] - ub[oc]) + (nodes - U - ib[oc]))
    return o, loc


def owner_counts(lists, U, ub, ib):
    """counts[r][o] = how many of list r's valid ids rank o owns."""
    W = len(ub) - 1
    lists = np.asarray(lists)
    out = np.zeros((lists.shape[0], W), np.int32)
    for r in range(lists.shape[0]):
        o, _ = owners(valid(lists[r]), U, ub, ib)
        out[r] = np.bincount(o, minlength=W)
    return out


def pack_model(lists, U, ub, ib, me, table_bytes, row_bytes):
    """Owner `me`: (send bytes [total x row_bytes] uint8, send_off int32 [W + 1]). Requester by requester, within a requester in
    list order -- ascending ids, so users before items. table_bytes: the owner's local table as uint8 [rows x row_bytes]."""
    lists = np.asarray(lists)
    table_bytes = np.asarray(table_bytes).reshape(-1, row_bytes)
    chunks, off = [], [0]
    for r in range(lists.shape[0]):
        v = valid(lists[r])
        o, loc = owners(v, U, ub, ib)
        mine = loc[o == me]
        chunks.append(table_bytes[mine])
        off.append(off[-1] + len(mine))
    return np.concatenate(chunks, axis=0) if chunks else table_bytes[:0], np.asarray(off, np.int32)


def widen(raw, dtype):
    """Stored elements -> fp32, exactly. raw: uint8 [..., n * element size]; dtype 'f32' | 'f16' | 'bf16'."""
    raw = np.ascontiguousarray(raw)
    if dtype == "f32":
        return raw.view(np.float32)
    if dtype == "f16":
        return raw.view(np.float16).astype(np.float32)
    if dtype == "bf16":
        return (raw.view(np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)
    raise ValueError(dtype)


def unpack_model(act, U, ub, ib, me, rows_bytes, row_bytes, dtype, sum_d, direct):
    """Requester `me`: (S fp32 [n x sum_d], c fp32 [n]) for the n valid ids of `act`, in list order, from the STORED bytes.
    direct = False: rows_bytes is the receive buffer, owner by owner, each owner's chunk in list order (what pack_model of that
    owner wrote for this list). direct = True: rows_bytes is one local table and every id must be a row of it."""
    v = valid(act)
    o, loc = owners(v, U, ub, ib)
    rows_bytes = np.asarray(rows_bytes).reshape(-1, row_bytes)
    if direct:
        assert len(set(o.tolist())) <= 1, "direct: the rows of one local table only"
        pos = loc
    else:
        order = np.argsort(o, kind="stable")                     # receive order: owner by owner, list order within
        pos = np.empty(len(v), np.int64)
        pos[order] = np.arange(len(v))
    raw = rows_bytes[pos]
    es = 4 if dtype == "f32" else 2
    S = widen(raw[:, :sum_d * es], dtype).reshape(len(v), sum_d)
    if dtype == "f32":
        c = widen(raw[:, sum_d * 4:sum_d * 4 + 4], dtype).reshape(-1)
    else:
        hl = widen(raw[:, sum_d * 2:sum_d * 2 + 4], dtype).reshape(-1, 2)
        c = (hl[:, 0].astype(np.float32) + hl[:, 1].astype(np.float32)).astype(np.float32)      # one fp32 add
    return S.copy(), c.copy()


def peer_cols_model(recv):
    """recv [W x R x 2 dl] -> (out0, out1) [R x W dl]: out_h[r, q dl + c] = recv[q, r, h dl + c]."""
    recv = np.asarray(recv)
    W, R, two = recv.shape
    dl = two // 2
    r4 = recv.reshape(W, R, 2, dl)
    return (np.ascontiguousarray(r4[:, :, 0].transpose(1, 0, 2)).reshape(R, W * dl),
            np.ascontiguousarray(r4[:, :, 1].transpose(1, 0, 2)).reshape(R, W * dl))


def bitmap_model(lists, N):
    """uint32 [(N + 31) / 32]: bit n <=> some list names node n."""
    flags = np.zeros(roundup(N, 32), np.uint32)
    flags[valid(np.asarray(lists).reshape(-1))] = 1
    return (flags.reshape(-1, 32) << np.arange(32, dtype=np.uint32)).sum(axis=1, dtype=np.uint64).astype(np.uint32)


def merge_model(rows, keys, W, R, U, N, d, M, srcA=None, srcB=None):
    """Dense (SrcA, SrcB) fp32 [N x d] and the bitmap after merge_rows. rows fp32 [W R x (M d if M > 0 else 2 d)], keys [W R].
    M = 0: a row is [H | G]. M >= 1: a row is M blocks, G = block 0, H = the blocks added in block order. M = -1: [H | G] and
    H always goes to SrcA. Otherwise H goes to SrcA on user rows and to SrcB on item rows, G to the other table. Across ranks:
    the first rank that names a node writes it, every later one adds to what is there, in rank order; all adds fp32.
    srcA / srcB: what the tables held before (zeros if None); rows no list names keep it."""
    rows = np.asarray(rows, dtype=np.float32)
    keys = np.asarray(keys).reshape(W, R)
    A = np.zeros((N, d), np.float32) if srcA is None else np.array(srcA, dtype=np.float32)
    B = np.zeros((N, d), np.float32) if srcB is None else np.array(srcB, dtype=np.float32)
    seen = np.zeros(N, bool)
    for r in range(W):
        for s in range(R):
            node = int(keys[r, s])
            if node < 0:
                continue
            row = rows[r * R + s]
            if M > 0:
                g = row[:d].copy()
                h = row[:d].copy()
                for mb in range(1, M):
                    h = (h + row[mb * d:(mb + 1) * d]).astype(np.float32)
            else:
                h, g = row[:d], row[d:2 * d]
            hT, gT = (A, B) if (M == -1 or node < U) else (B, A)
            if seen[node]:
                hT[node] = (hT[node] + h).astype(np.float32)
                gT[node] = (gT[node] + g).astype(np.float32)
            else:
                hT[node] = h
                gT[node] = g
                seen[node] = True
    return A, B, bitmap_model(keys, N)


# ------------------------------------------------------------------------------------------------------------ case builders
def pad_list(ids, R):
    ids = np.unique(np.asarray(ids, dtype=np.int64))
    assert len(ids) <= R, (len(ids), R)
    return np.concatenate([ids, np.full(R - len(ids), PAD, np.int64)]).astype(np.int32)


def uneven_bounds(n, W, empty):
    """W blocks over [0, n): uneven sizes, block `empty` (None: none) of size 0, every other block non-empty."""
    if W == 1:
        return np.array([0, n], np.int64)
    wt = np.array([1 + (o * 7) % 5 for o in range(W)], np.float64)
    if empty is not None:
        wt[empty] = 0
    size = np.floor(n * wt / wt.sum()).astype(np.int64)
    size[(wt > 0) & (size == 0)] = 1
    last = max(o for o in range(W) if wt[o] > 0)
    size[last] += n - size.sum()
    assert size.min() >= 0 and size[last] > 0 and size.sum() == n
    return np.concatenate([[0], np.cumsum(size)]).astype(np.int64)


def boundary_ids(U, I, ub, ib):
    """Every id an owner search can be off by one at: first and last user / item of every non-empty block, U - 1, U, N - 1."""
    users, items = set(), set()
    for o in range(len(ub) - 1):
        if ub[o + 1] > ub[o]:
            users.update([int(ub[o]), int(ub[o + 1] - 1)])
        if ib[o + 1] > ib[o]:
            items.update([int(U + ib[o]), int(U + ib[o + 1] - 1)])
    users.add(U - 1)
    items.update([U, U + I - 1])
    return sorted(users), sorted(items)


PATTERNS = ("full", "allpad", "users", "items", "ragged", "one")


def lookup_case(W, k=0, U=300, I=420, R=64, seed=0):
    """W requesters' lists over uneven owner blocks with an empty user block (W / 2) and an empty item block (the next one).
    List r has pattern PATTERNS[(r + k) % 6]: full (R ids: every boundary if they fit, else every second, + random), allpad, users only (every user boundary),
    items only (every item boundary), ragged (U - 1, U and a few random), one (a single id: the first item, node U)."""
    rng = np.random.RandomState(1000 * W + 10 * k + seed)
    eu, ei = (W // 2, (W // 2 + 1) % W) if W > 1 else (None, None)
    ub, ib = uneven_bounds(U, W, eu), uneven_bounds(I, W, ei)
    bu, bi = boundary_ids(U, I, ub, ib)
    N = U + I
    lists, pats = [], []
    for r in range(W):
        p = PATTERNS[(r + k) % len(PATTERNS)]
        if p == "full":
            keep = bu + bi if len(bu) + len(bi) <= R else (bu + bi)[::2][:R - 2] + [U - 1, U]
            ids = set(keep)
            while len(ids) < R:
                ids.add(int(rng.randint(0, N)))
        elif p == "allpad":
            ids = set()
        elif p == "users":
            ids = set(bu) | set(rng.randint(0, U, 6).tolist())
        elif p == "items":
            ids = set(bi) | set((U + rng.randint(0, I, 6)).tolist())
        elif p == "ragged":
            ids = {U - 1, U} | set(rng.randint(0, N, R // 3).tolist())
        else:
            ids = {U}
        lists.append(pad_list(sorted(ids), R))
        pats.append(p)
    return types.SimpleNamespace(W=W, U=U, I=I, N=N, R=R, ub=ub, ib=ib, lists=np.stack(lists), patterns=pats, bu=bu, bi=bi,
                                 empty_user_block=eu, empty_item_block=ei, what="lookup W %d k %d" % (W, k))


def lookup_case_r1(W, U=300, I=420):
    """R = 1: requester r asks for the r-th boundary id; requester 1 (of three or more) for nothing."""
    c = lookup_case(W, 0, U, I)
    b = c.bu + c.bi
    ids = [[b[(5 * r) % len(b)]] for r in range(W)]
    if W >= 3:
        ids[1] = []
    c.lists = np.stack([pad_list(x, 1) for x in ids])
    c.R, c.patterns, c.what = 1, ["one"] * W, "lookup W %d R 1" % W
    return c


def own_rows_list(c, me, R=None):
    """A list made of rank `me`'s own rows only (first / last user and item it owns, and every third row between)."""
    R = c.R if R is None else R
    u = np.arange(c.ub[me], c.ub[me + 1])
    i = c.U + np.arange(c.ib[me], c.ib[me + 1])
    edges = np.unique(np.concatenate([u[:1], u[-1:], i[:1], i[-1:]]))
    inner = np.setdiff1d(np.concatenate([u[1:-1:3], i[1:-1:3]]), edges)
    step = max(1, -(-len(inner) // max(R - len(edges), 1)))
    return pad_list(np.concatenate([edges, inner[::step]])[:R], R)


def grid_case():
    """W = 2, R = 9000 over U + I = 20000: owner 0 holds 95 % of the rows, so it packs more than GRID_ROWS rows (a second trip of
    the pack loop) and every requester unpacks R > GRID_ROWS rows (a second trip of the unpack loop)."""
    U = I = 10000
    W, R = 2, 9000
    ub = np.array([0, 9500, U], np.int64)
    ib = np.array([0, 9500, I], np.int64)
    rng = np.random.RandomState(77)
    lists = []
    for r in range(W):
        ids = set([0, 9499, 9500, U - 1, U, U + 9499, U + 9500, U + I - 1])
        ids.update(rng.choice(U + I, R - len(ids) - (0 if r == 0 else 300), replace=False).tolist())
        lists.append(pad_list(sorted(ids)[:R], R))
    return types.SimpleNamespace(W=W, U=U, I=I, N=U + I, R=R, ub=ub, ib=ib, lists=np.stack(lists), what="lookup grid-stride")


CHUNK_NS = (20, 2592, 32800, 65540)


def chunk_case(N, W=3, R=96):
    """Key lists on the workgroup and word edges of merge_rows / rows_bitmap at N rows: lo, lo + 31, lo + 32 and hi - 1 of the
    first, a middle and the last workgroup, the first and last id of the last bitmap word. Rank 0 names every edge, rank 1 every
    second edge and some others (shared and private nodes), rank 2 is all padding."""
    chunk = merge_rows_chunk(N)
    groups = (N + chunk - 1) // chunk
    edges = set()
    for b in sorted({0, groups // 2, groups - 1}):
        lo, hi = b * chunk, min((b + 1) * chunk, N)
        edges.update([lo, lo + 31, lo + 32, hi - 1, lo + chunk - 32, lo + chunk - 1])
    last_word = (N - 1) // 32 * 32
    edges.update([last_word, N - 1, 0])
    U = N // 2 + 1
    edges.update([U - 1, U])
    edges = sorted(e for e in edges if 0 <= e < N)
    rng = np.random.RandomState(N % 9973)
    r0 = set(edges) | set(rng.randint(0, N, 20).tolist())
    r1 = set(edges[::2]) | set(rng.randint(0, N, 20).tolist())
    lists = [pad_list(sorted(r0)[:R], R), pad_list(sorted(r1)[:R], R), pad_list([], R)][:W]
    return types.SimpleNamespace(N=N, U=U, I=N - U, W=len(lists), R=R, chunk=chunk, groups=groups, edges=edges,
                                 keys=np.stack(lists), what="chunk N %d" % N)


MERGE_GEOMS = {1: (1, 4), 2: (1, 8), 6: (3, 8), 16: (2, 32), 80: (10, 32)}          # nc4 -> (ns, w); lanes per row 1, 2, 8, 16, 64
MERGE_MS = (0, 1, 3, -1)
MERGE_WS = (1, 2, 5, 64)


def merge_forms():
    """(M, W, nc4): every M with every W (the geometry rotating), and every M with every geometry at W = 5."""
    geoms = sorted(MERGE_GEOMS)
    out = []
    for im, M in enumerate(MERGE_MS):
        for iw, W in enumerate(MERGE_WS):
            out.append((M, W, geoms[(im + iw) % len(geoms)]))
        for nc4 in geoms:
            if (M, 5, nc4) not in out:
                out.append((M, 5, nc4))
    return out


def merge_case(W, R=None, U=None, I=None):
    """Key lists of W ranks over N = U + I (five workgroups; twelve at 64 ranks, which need more private nodes): nodes U - 1 and U named by every rank that names anything, a node on
    either side named by ranks 0 and W - 1 only, private nodes for every rank, rank 1 of three or more all padding."""
    if R is None:
        R = 8 if W == SLAB_MAX_RANKS else 16
    if U is None:
        U, I = (150, 203) if W > 16 else (70, 91)
    N = U + I
    rng = np.random.RandomState(31 * W + R)
    lists = []
    two_u, two_i = 5, U + 40
    taken = {U - 1, U, two_u, two_i}
    for r in range(W):
        if W >= 3 and r == 1:
            lists.append(pad_list([], R))
            continue
        ids = {U - 1, U}
        if r in (0, W - 1):
            ids.update([two_u, two_i])
        if R == 1:
            ids = {U - 1} if r % 2 == 0 else {U}
        else:
            want = min(R, len(ids) + 1 + (r % 3))
            while len(ids) < want:
                n = int(rng.randint(0, N))
                if n not in taken:                                   # private: no other rank names it
                    taken.add(n)
                    ids.add(n)
        lists.append(pad_list(sorted(ids), R))
    return types.SimpleNamespace(W=W, R=R, U=U, I=I, N=N, keys=np.stack(lists), two=(two_u, two_i), what="merge W %d R %d" % (W, R))


def naming_ranks(keys, node):
    return [r for r in range(keys.shape[0]) if node in set(valid(keys[r]).tolist())]


def merge_rows_input(W, R, cols, seed):
    """fp32 rows whose sums round: normal draws scaled over several binades, so a wrong order or a dropped addend shows in the bits."""
    rng = np.random.RandomState(seed)
    return (rng.standard_normal((W * R, cols)) * np.exp2(rng.randint(-6, 7, (W * R, 1)))).astype(np.float32)
