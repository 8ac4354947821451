"""tests/exchange_model.py checked on the host: the models against brute-force dictionaries and loops at tiny sizes, the case
builders against what they claim to contain (every boundary id, every chunk count, every second loop trip the GPU tests rely on),
and the c = hi + lo split of lookup.FeatureShard's 16-bit storage against c. No GPU, no project kernel."""
import numpy as np
import pytest
import torch

import exchange_model as em


def _blocks(rng, n, W):
    cuts = np.sort(rng.randint(0, n + 1, W - 1))
    return np.concatenate([[0], cuts, [n]]).astype(np.int64)


def _random_lists(rng, W, R, N):
    return np.stack([em.pad_list(rng.choice(N, rng.randint(0, min(R, N) + 1), replace=False), R) for _ in range(W)])


# ------------------------------------------------------------------------------------------------------------------ the models
@pytest.mark.parametrize("W", [1, 2, 3, 7])
def test_owner_counts_pack_and_unpack_against_dictionaries(W):
    """Every node's (owner, local row) from a scan of the blocks; a send buffer built one dictionary look-up at a time; the
    receive buffer cut out of the owners' send buffers by the counts; unpack must hand every requester its own nodes' rows."""
    rng = np.random.RandomState(W)
    U, I, R, rb = 11, 13, 9, 16
    for trial in range(20):
        ub, ib = _blocks(rng, U, W), _blocks(rng, I, W)
        lists = _random_lists(rng, W, R, U + I)
        where = {n: em.owner_of(n, U, ub, ib) for n in range(U + I)}
        o, loc = em.owners(np.arange(U + I), U, ub, ib)
        assert [(int(a), int(b)) for a, b in zip(o, loc)] == [where[n] for n in range(U + I)]
        counts = em.owner_counts(lists, U, ub, ib)
        want = np.zeros((W, W), np.int32)
        for r in range(W):
            for n in lists[r]:
                if n >= 0:
                    want[r, where[int(n)][0]] += 1
        assert np.array_equal(counts, want)
        # local tables whose rows spell (owner, local row, node): fp32 [3 values | c] in 16 bytes
        tables = []
        for q in range(W):
            nodes = [n for n in range(U + I) if where[n][0] == q]
            nodes.sort(key=lambda n: where[n][1])
            assert [where[n][1] for n in nodes] == list(range(len(nodes)))              # users first, then items, no gaps
            tables.append(np.array([[q, where[n][1], n, 1000 + n] for n in nodes], np.float32).reshape(len(nodes), 4).view(np.uint8))
        sends = []
        for q in range(W):
            send, off = em.pack_model(lists, U, ub, ib, q, tables[q], rb)
            assert np.array_equal(off, np.concatenate([[0], np.cumsum(counts[:, q])]))
            rows = send.view(np.float32).reshape(-1, 4)
            k = 0
            for r in range(W):
                for n in lists[r]:                                                       # ascending: users before items
                    if n >= 0 and where[int(n)][0] == q:
                        assert rows[k].tolist() == [q, where[int(n)][1], n, 1000 + n]
                        k += 1
            assert k == len(rows)
            sends.append(send)
        for r in range(W):
            recv = np.concatenate([sends[q][int(counts[:r, q].sum()):int(counts[:r + 1, q].sum())] for q in range(W)])
            S, c = em.unpack_model(lists[r], U, ub, ib, r, recv, rb, "f32", 3, False)
            v = em.valid(lists[r])
            assert np.array_equal(S[:, 2], v.astype(np.float32)) and np.array_equal(c, (1000 + v).astype(np.float32))
            assert all(S[j, 0] == where[int(n)][0] and S[j, 1] == where[int(n)][1] for j, n in enumerate(v))
        # direct: the rows of one local table
        for q in range(W):
            own = np.array([n for n in range(U + I) if where[n][0] == q], np.int64)
            S, c = em.unpack_model(em.pad_list(own, U + I), U, ub, ib, q, tables[q], rb, "f32", 3, True)
            assert np.array_equal(S[:, 2], np.sort(own).astype(np.float32))


def test_widening_and_c_of_16_bit_rows():
    """f16 / bf16 elements widen to the fp32 of the same value (subnormals, the largest value, signed zero), and c is ONE fp32 add."""
    h = np.array([1.0, -0.0, 6.1e-5, 5.96e-8, 65504.0, -1.5], np.float16)
    assert np.array_equal(em.widen(h.view(np.uint8), "f16").view(np.uint32), h.astype(np.float32).view(np.uint32))
    f = np.array([1.0, -0.0, 3.0e38, 1.0e-38, -1.5, 0.33], np.float32)
    top = (f.view(np.uint32) >> 16).astype(np.uint16)
    assert np.array_equal(em.widen(top.view(np.uint8), "bf16").view(np.uint32), (f.view(np.uint32) & 0xffff0000))
    row = np.array([0.5, 0.25, 0.75, 1.0, 0.7001953125, 2.0 ** -14, 0, 0], np.float16)     # sum_d = 4, then hi, lo
    S, c = em.unpack_model(np.array([0], np.int32), 1, [0, 1], [0, 0], 0, row.view(np.uint8), 16, "f16", 4, True)
    assert S.tolist() == [[0.5, 0.25, 0.75, 1.0]] and c[0] == np.float32(0.7001953125) + np.float32(2.0 ** -14)


def test_peer_cols_and_bitmap_against_loops():
    rng = np.random.RandomState(3)
    W, R, dl = 3, 5, 4
    recv = rng.standard_normal((W, R, 2 * dl)).astype(np.float32)
    o0, o1 = em.peer_cols_model(recv)
    for q in range(W):
        for r in range(R):
            for c in range(dl):
                assert o0[r, q * dl + c] == recv[q, r, c] and o1[r, q * dl + c] == recv[q, r, dl + c]
    for N in (1, 31, 32, 33, 70):
        lists = _random_lists(rng, 3, 8, N)
        words = em.bitmap_model(lists, N)
        assert len(words) == (N + 31) // 32 and words.dtype == np.uint32
        named = set(int(n) for n in lists.reshape(-1) if n >= 0)
        for n in range(em.roundup(N, 32)):
            assert ((int(words[n // 32]) >> (n % 32)) & 1) == (n in named)


@pytest.mark.parametrize("M", [0, 1, 3, -1])
def test_merge_model_against_a_dictionary_of_addends(M):
    """Per node: the list of (rank, row) that name it, in rank order; H and G by the form's definition; one fp32 add per later rank;
    the side swap at U; rows nobody names keep what the tables held."""
    rng = np.random.RandomState(5 + M)
    W, R, U, N, d = 4, 6, 7, 16, 4
    keys = _random_lists(rng, W, R, N)
    keys[2] = em.PAD
    cols = M * d if M > 0 else 2 * d
    rows = em.merge_rows_input(W, R, cols, 9)
    pre = np.full((N, d), np.float32(-7.5))
    A, B, bits = em.merge_model(rows, keys, W, R, U, N, d, M, srcA=pre, srcB=pre)
    assert np.array_equal(bits, em.bitmap_model(keys, N))
    addends = {}
    for r in range(W):
        for s in range(R):
            if keys[r, s] >= 0:
                addends.setdefault(int(keys[r, s]), []).append(rows[r * R + s])
    assert any(len(v) > 1 for v in addends.values()) and len(addends) < N
    for n in range(N):
        if n not in addends:
            assert (A[n] == -7.5).all() and (B[n] == -7.5).all()
            continue
        H = G = None
        for row in addends[n]:
            if M > 0:
                g, h = row[:d], row[:d]
                for mb in range(1, M):
                    h = np.float32(h) + row[mb * d:(mb + 1) * d]
            else:
                h, g = row[:d], row[d:]
            H = h if H is None else (H + h).astype(np.float32)
            G = g if G is None else (G + g).astype(np.float32)
        hT, gT = (A, B) if (M == -1 or n < U) else (B, A)
        assert np.array_equal(hT[n], H) and np.array_equal(gT[n], G), n
    if M == 1:
        named = sorted(addends)
        assert np.array_equal(A[named], B[named])                                      # one block: H = G


# ------------------------------------------------------------------------------------------------------- the case builders
def test_merge_rows_chunk_steps():
    assert [em.merge_rows_chunk(n) for n in (1, 20, 32768, 32769, 32800, 65536, 65537, 65540)] == [32, 32, 32, 64, 64, 64, 96, 96]


@pytest.mark.parametrize("W", [1, 2, 5, 16])
def test_lookup_cases_hold_every_boundary_and_pattern(W):
    ks = range(6) if W < 3 else (0, 3)
    seen_patterns = set()
    for k in ks:
        c = em.lookup_case(W, k)
        assert c.lists.shape == (W, 64) and c.lists.dtype == np.int32
        assert c.ub[0] == 0 and c.ub[-1] == c.U and c.ib[0] == 0 and c.ib[-1] == c.I and (np.diff(c.ub) >= 0).all() and (np.diff(c.ib) >= 0).all()
        if W > 1:
            assert c.ub[c.empty_user_block] == c.ub[c.empty_user_block + 1] and c.ib[c.empty_item_block] == c.ib[c.empty_item_block + 1]
            assert (np.diff(c.ub) == 0).sum() == 1 and (np.diff(c.ib) == 0).sum() == 1 and (W == 2 or len(set(np.diff(c.ub).tolist())) > 2)
        for l in c.lists:
            v = em.valid(l)
            assert (np.diff(v) > 0).all() and (l[len(v):] < 0).all() and (v < c.N).all()
        for r, p in enumerate(c.patterns):
            v = em.valid(c.lists[r])
            seen_patterns.add(p)
            if p == "full":
                assert len(v) == c.R and c.U - 1 in v and c.U in v
            elif p == "allpad":
                assert len(v) == 0
            elif p == "users":
                assert len(v) and (v < c.U).all() and set(c.bu) <= set(v.tolist())
            elif p == "items":
                assert len(v) and (v >= c.U).all() and set(c.bi) <= set(v.tolist())
            elif p == "ragged":
                assert 2 < len(v) < c.R and c.U - 1 in v and c.U in v
            else:
                assert v.tolist() == [c.U]
        if W >= 3:                # (k = 0) an all-padding requester between two that ask for something
            assert k or any(c.patterns[r] == "allpad" and len(em.valid(c.lists[r - 1])) and len(em.valid(c.lists[r + 1])) for r in range(1, W - 1))
            named = set(em.valid(c.lists.reshape(-1)).tolist())
            for o in range(W):    # ub[o], ub[o+1] - 1, U + ib[o], U + ib[o+1] - 1 of every block that has rows; U - 1, U, N - 1
                if c.ub[o + 1] > c.ub[o]:
                    assert {int(c.ub[o]), int(c.ub[o + 1] - 1)} <= named
                if c.ib[o + 1] > c.ib[o]:
                    assert {int(c.U + c.ib[o]), int(c.U + c.ib[o + 1] - 1)} <= named
            assert {c.U - 1, c.U, c.N - 1, 0} <= named
    assert seen_patterns == set(em.PATTERNS)
    c1 = em.lookup_case_r1(W)
    assert c1.lists.shape == (W, 1) and (W < 3 or c1.lists[1, 0] < 0) and len(em.valid(c1.lists.reshape(-1))) == W - (W >= 3)
    for me in range(W):
        own = em.valid(em.own_rows_list(c, me))
        o, _ = em.owners(own, c.U, c.ub, c.ib)
        assert (o == me).all()
        nu, ni = c.ub[me + 1] - c.ub[me], c.ib[me + 1] - c.ib[me]
        if nu:
            assert c.ub[me] in own and c.ub[me + 1] - 1 in own
        if ni:
            assert c.U + c.ib[me] in own and c.U + c.ib[me + 1] - 1 in own


def test_width_and_grid_cases_take_the_second_trips():
    # widths (tests/test_exchange_gpu.py WIDTHS): 16-byte pieces per row in pack, float4 pieces per row in unpack
    for dtype, sum_d, row16, d4 in (("f32", 4, 2, 1), ("f32", 260, 66, 65), ("f16", 12, 2, 3), ("bf16", 520, 66, 130)):
        es, nc = (4, 1) if dtype == "f32" else (2, 2)
        rb = em.roundup((sum_d + nc) * es, 16)
        assert rb // 16 == row16 and sum_d // 4 == d4
    assert 66 > em.LANES and 65 > em.LANES and 130 > 2 * em.LANES
    g = em.grid_case()
    counts = em.owner_counts(g.lists, g.U, g.ub, g.ib)
    assert counts[:, 0].sum() > em.GRID_ROWS                       # owner 0 packs more rows than one trip of the grid covers
    assert (g.W * g.R + 3) // 4 > 2048                             # ... and the launch is at the grid cap
    assert all(len(em.valid(l)) > em.GRID_ROWS for l in g.lists) and g.R > em.GRID_ROWS and len(em.valid(g.lists[1])) < g.R
    assert 19000 <= g.N <= 21000


@pytest.mark.parametrize("N", em.CHUNK_NS)
def test_chunk_cases_reach_the_words_they_claim(N):
    c = em.chunk_case(N)
    want = {20: (32, 1), 2592: (32, 81), 32800: (64, 513), 65540: (96, 683)}[N]
    assert (c.chunk, c.groups) == want and c.chunk == em.merge_rows_chunk(N)
    named = set(em.valid(c.keys.reshape(-1)).tolist())
    assert set(c.edges) <= set(em.valid(c.keys[0]).tolist()) and max(named) == N - 1 and 0 in named
    lo_last = (c.groups - 1) * c.chunk
    guarded = [w for w in range(c.chunk // 32) if not lo_last + 32 * w < em.roundup(N, 32)]
    if N == 32800:                # the last workgroup's second word lies behind roundup(N, 32): the guard must hold it back
        assert guarded == [1] and lo_last // 32 + 1 == (N + 31) // 32
    elif N == 65540:
        assert guarded == [] and lo_last // 32 + 2 == (N + 31) // 32 - 1
    if c.chunk > 32:              # bit >= 32: keys in a workgroup's second word, in the first and the last workgroup
        assert {31, 32, c.chunk - 32, c.chunk - 1} <= named and any(lo_last <= n < lo_last + 32 for n in named)
        assert (N == 65540) == any(n >= lo_last + 32 for n in named)
        mid = (c.groups // 2) * c.chunk
        assert {mid, mid + 31, mid + 32, mid + c.chunk - 1} <= named
    assert (N % 32 == 0) == (N in (2592, 32800)) and (N < 32) == (N == 20)
    assert {c.U - 1, c.U} <= named
    shared = set(em.valid(c.keys[0]).tolist()) & set(em.valid(c.keys[1]).tolist())
    assert shared and set(em.valid(c.keys[1]).tolist()) - shared and len(em.valid(c.keys[2])) == 0


def test_merge_cases_share_nodes_on_both_sides_of_U():
    forms = em.merge_forms()
    assert {(M, W) for M, W, _ in forms} == {(M, W) for M in em.MERGE_MS for W in em.MERGE_WS}
    assert {(M, g) for M, W, g in forms if W == 5} == {(M, g) for M in em.MERGE_MS for g in em.MERGE_GEOMS}
    assert {ns * (w // 4) for ns, w in em.MERGE_GEOMS.values()} == {1, 2, 6, 16, 80} == set(em.MERGE_GEOMS)
    for W in em.MERGE_WS:
        c = em.merge_case(W)
        assert c.keys.shape == (W, 8 if W == 64 else 16) and em.merge_rows_chunk(c.N) == 32
        active = [r for r in range(W) if len(em.valid(c.keys[r]))]
        assert em.naming_ranks(c.keys, c.U - 1) == active and em.naming_ranks(c.keys, c.U) == active         # shared by all, both sides
        if W >= 3:
            assert 1 not in active and len(active) == W - 1
            for n in c.two:
                assert em.naming_ranks(c.keys, n) == [0, W - 1]
            assert c.two[0] < c.U <= c.two[1]
        private = [n for n in set(em.valid(c.keys.reshape(-1)).tolist()) if len(em.naming_ranks(c.keys, n)) == 1]
        assert any(n < c.U for n in private) and any(n >= c.U for n in private)
        for l in c.keys:
            assert (np.diff(em.valid(l)) > 0).all()
    c = em.merge_case(5, R=1)
    assert c.keys.reshape(-1).tolist() == [c.U - 1, em.PAD, c.U - 1, c.U, c.U - 1]
    rows = em.merge_rows_input(5, 16, 24, 1)
    s32 = (rows[0, :8] + rows[0, 8:16]).astype(np.float32)
    assert (s32.astype(np.float64) != rows[0, :8].astype(np.float64) + rows[0, 8:16].astype(np.float64)).any()   # the adds round


# ------------------------------------------------------------------------------------------------- c = hi + lo (FeatureShard)
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_feature_shard_c_split_against_c(dtype):
    """lookup.FeatureShard stores c as two 16-bit values, hi = rn(c) and lo = rn(c - float(hi)); unpack returns fl32(hi + lo).
    With p significant bits (f16: 11, bf16: 8), round-to-nearest has |x - rn(x)| <= 2^-p |x| / (1 + 2^-p) in the normal range;
    f16 values below 2^-14 are multiples of 2^-24, so there the error is <= 2^-25 instead.
      * r = c - float(hi) is exact in fp32: c has 24 bits, hi is c rounded to p of them, so r is a multiple of ulp(c) below 2^-p |c|.
      * |r - lo| <= 2^-p |r| <= 2^-2p |c| / (1 + 2^-p)^2, or (f16, |r| < 2^-14) <= 2^-25. Hence e = |c - (hi + lo)|, taken exactly,
        is <= 2^-22 |c| (1 - 2^-11) + 2^-25 for f16 and <= 2^-16 |c| (1 - 2^-8) for bf16 (bf16 has fp32's exponent range: no
        subnormal term for c >= 1e-6).
      * the fp32 add rounds once more: <= 2^-24 (|c| + e). Its second-order part 2^-24 e is <= 2^-46 |c| + 2^-49, which the slack
        2^-33 |c| (f16; it needs |c| >= 2^-16, and below that e <= 2^-24 altogether) and 2^-24 |c| (bf16) of the first term covers.
    So |c - fl32(hi + lo)| <= (2^-22 + 2^-24) |c| + 2^-25 for f16 and <= (2^-16 + 2^-24) |c| for bf16, asserted in float64 with
    nothing added. c is drawn from [0, 1] and log-uniformly from [1e-6, 1e-3]: the f16 draws below 6e-5 have a subnormal hi, and
    every draw below 0.03 a subnormal lo. FeatureShard builds on CPU tensors without the library, so this is the class itself --
    the constructor and from_local -- not a copy of its formula."""
    from elimrec_amd.lookup import FeatureShard, RowOwnerMap
    U, I = 3000, 5000
    N = U + I
    g = torch.Generator().manual_seed(5)
    c = torch.rand(N, generator=g)
    small = torch.exp(torch.empty(N // 2).uniform_(float(np.log(1e-6)), float(np.log(1e-3)), generator=g))
    c[::2] = small
    c[1], c[3] = 1.0, 1e-6
    tabs = [torch.randn(N, 4, generator=g)]
    owners = RowOwnerMap(U, I, 2)
    for o in range(2):
        nodes = torch.from_numpy(owners.nodes(o))
        a = FeatureShard(owners, o, tabs, c, dtype=dtype)
        b = FeatureShard.from_local(owners, o, [tabs[0][nodes]], c[nodes], dtype=dtype)
        assert torch.equal(a.table.view(torch.int16), b.table.view(torch.int16)) and a.row_bytes == 16 and a.table.shape == (len(nodes), 8)
        raw = a.table.contiguous().view(torch.uint8).numpy().reshape(len(nodes), 16)
        S, got = em.unpack_model(em.pad_list(owners.nodes(o), len(nodes)), U, owners.ub, owners.ib, o, raw, 16, dtype, 4, True)
        assert np.array_equal(S, tabs[0][nodes].to(a.table.dtype).float().numpy())
        want = c[nodes].numpy().astype(np.float64)
        err = np.abs(want - got.astype(np.float64))
        bound = (2.0 ** -22 + 2.0 ** -24) * want + 2.0 ** -25 if dtype == "f16" else (2.0 ** -16 + 2.0 ** -24) * want
        assert (err <= bound).all(), (dtype, float((err / bound).max()))
        assert err.max() > 0                                                           # and it is a split, not c itself
        if dtype == "f16":
            hi = raw[:, 8:10].copy().view(np.float16).reshape(-1)
            assert (np.abs(hi[want < 5e-5]) < 2.0 ** -14).all() and (want < 5e-5).sum() > 100     # subnormal hi reached
