"""The kernels that move rows between ranks in the multi-rank step, bit for bit against the exact host models of
tests/exchange_model.py: csrc/lookup.hip (counts, pack, unpack, peer_cols_to_rows), csrc/merge_rows.h under csrc/slab.hip
(merge_rows at M = 0, M >= 1 and M = -1; rows_bitmap) and under csrc/gemm.hip (the merge fused into the weight-gradient launch).
Calls go through elimrec_amd.lookup, slab and ops only.

Every operation here is exact (copies, 16-bit -> fp32 widening, integer range searches, fp32 adds in rank order then block
order), so there is no tolerance anywhere in this file: floats are compared with fp64_tools.same_bits, integers and bytes with
torch.equal. Every output and every pad region starts as NaN (a sentinel word or byte for integer buffers) and whatever the contract
leaves unwritten must still hold it: rows behind a list's valid prefix, columns outside the S_out window, mask words in front of
and behind the (N + 31) / 32 the kernels own, send bytes behind send_off[W]. Every launch is repeated into fresh buffers and must
give the same bits. The case builders put ids on every boundary by construction, and tests/test_exchange_model_cpu.py proves that
they reach what they claim: merge chunks of 64 and 96 rows, a guarded tail word, more than 8192 packed and unpacked rows, more
than 64 16-byte / float4 pieces per row, nodes shared on both sides of U.

The fused launch has no plain form: elimrec_linear_bwd_w_batched_merge requires M >= 0 (the multi-rank M = -1 call of shard.py goes
to slab.merge_rows, which the forms test covers at every world size). test_fused_merge_at_three_ranks therefore runs M = 0 and
M = 3 at world = 3 and asserts that M = -1 is refused before anything is launched.

No test here exposed a bug in the kernels.

Mutants (each built into a library of its own, this file run once against it, none committed); all eight are caught. The tests
that fail:
  * merge: `was` forced false -- test_chunk_edges (all four N), test_merge_forms (all 31 cases with W >= 2, every M, R = 1 too),
    test_fused_merge_at_three_ranks. The W = 1 cases pass, as they must.
  * merge: `node < U` -> `node <= U` -- test_chunk_edges (all four N), test_merge_forms (every M = 0 and M = 3 case),
    test_fused_merge_at_three_ranks. The M = -1 cases (no side swap) and the M = 1 cases (one block: H = G) pass, as they must.
  * merge: the M-block sum starts at mb = 2 -- test_merge_forms (all nine M = 3 cases), test_fused_merge_at_three_ranks.
  * merge and bitmap: tail guard `<` -> `<=` -- test_chunk_edges[32800] and test_fused_merge_at_three_ranks: the sentinel word
    behind the (N + 31) / 32 the kernels own is overwritten. In bounds: that word is one of the two trailing sentinels of the
    test's own buffer; at the other N no workgroup has a word behind the guard.
  * unpack: `s_rg[o].ucnt +` dropped on the item branch -- test_lookup_boundaries (W = 1, 5, 16, every dtype), test_lookup_widths,
    test_lookup_grid_stride. (W = 2 passes: with an empty user block and an empty item block each of two ranks owns one side only.)
  * unpack: cval returns h[0] alone -- test_lookup_boundaries and test_lookup_widths, all f16 and bf16 cases.
  * unpack bf16: load4 swaps the halves of v.x -- test_lookup_boundaries and test_lookup_widths, all bf16 cases.
  * pack: n_users_loc taken from rank 0 -- test_lookup_boundaries (W = 5, 16, every dtype). Run as min(rank 0's count, the rank's own):
    where rank 0 owns more users than the packing rank the mutant would read past that rank's local table, so that direction
    was not tried; W = 2 and the grid case have no rank with more users than rank 0 and items of its own.

Time of the whole file on an MI355X: about 3.5 s for 64 tests (slowest case 0.8 s, the first to touch the device; every other case under
0.1 s). For comparison, the three earlier exchange tests of tests/test_shard_gpu.py (14 cases) take about 3.2 s at the parent commit.
"""
import ctypes

import numpy as np
import pytest
import torch

import exchange_model as em
from fp64_tools import NAN, all_nan, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -0x5a5a5a5b             # sentinel word of integer outputs (0xa5a5a5a5)
SENT_BYTE = 0xa5
DIMS = (8, 4, 12)              # three tables side by side: sum_d = 24


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def _bits_equal(got, want_np, what):
    want = _dev(np.asarray(want_np, dtype=np.float32))
    assert same_bits(got.contiguous(), want.view(got.shape)), what


def _dense(t):
    """Row-major view of a slab-major table, by torch indexing alone."""
    return t.data.view(t.ns, t.n, t.w).permute(1, 0, 2).reshape(t.n, t.ns * t.w)


# ---------------------------------------------------------------------------------------------------------------------- lookup
def _shards(c, dtype, dims, seed):
    """W FeatureShards over random tables with a few values at the formats' edges, and each local table's stored bytes."""
    from elimrec_amd.lookup import FeatureShard, RowOwnerMap
    g = torch.Generator().manual_seed(seed)
    tabs = [torch.randn(c.N, D, generator=g) for D in dims]
    tabs[0][0, 0], tabs[0][1, 0], tabs[0][2, 0], tabs[0][c.U, 1], tabs[0][c.N - 1, 3] = -0.0, 6e-8, 65504.0, 1e-30, -3.0e-5
    cv = torch.rand(c.N, generator=g)
    cv[::3] *= 1e-4
    owners = RowOwnerMap(c.U, c.I, c.W, ub=c.ub, ib=c.ib)
    shards = [FeatureShard(owners, o, tabs, cv, dtype=dtype, device=DEV) for o in range(c.W)]
    raw = [s.table.contiguous().view(torch.uint8).cpu().numpy().reshape(-1, s.row_bytes) if s.table.numel() else
           np.zeros((0, s.row_bytes), np.uint8) for s in shards]
    for o, s in enumerate(shards):
        assert s.table.shape[0] == sum(owners.rows(o)) and s.sum_d == sum(dims)
    return shards, raw


def _unpack_and_check(shard, act_np, rows_dev, rows_np, c, dtype, direct, window, what):
    """One unpack into NaN buffers (S_out a column window of a wider tensor where `window`), twice, against the model."""
    R, sd, rb = len(act_np), shard.sum_d, shard.row_bytes
    want_S, want_c = em.unpack_model(act_np, c.U, c.ub, c.ib, shard.rank, rows_np, rb, dtype, sd, direct)
    n = len(want_c)
    act = _dev(act_np)
    got = []
    for _ in range(2):
        wide = _nan(R + 1, sd + 8) if window else _nan(R + 1, sd)
        S = wide[:, 4:4 + sd] if window else wide
        cr = _nan(R + 1)
        shard.unpack(act, rows_dev, S[:R], cr[:R], direct=direct)
        _bits_equal(S[:n], want_S, what + ": S")
        _bits_equal(cr[:n], want_c, what + ": c")
        assert all_nan(S[n:]) and all_nan(cr[n:]), what + ": rows behind the valid prefix"
        if window:
            assert all_nan(wide[:, :4]) and all_nan(wide[:, 4 + sd:]), what + ": columns outside the window"
        got.append((wide.clone(), cr.clone()))
    assert same_bits(got[0][0], got[1][0]) and same_bits(got[0][1], got[1][1]), what + ": second launch"


def _check_lookup(c, dtype, dims, seed, window=False):
    shards, raw = _shards(c, dtype, dims, seed)
    W, R, rb = c.W, c.R, shards[0].row_bytes
    acts = _dev(c.lists)
    want_counts = em.owner_counts(c.lists, c.U, c.ub, c.ib)
    for o in (0, W - 1):
        counts = torch.full((W + 1, W), SENT, dtype=torch.int32, device=DEV)
        shards[o].counts(acts, out=counts[:W])
        assert torch.equal(counts[:W], _dev(want_counts)) and bool((counts[W] == SENT).all()), c.what + ": counts"
    packed, models = [], []
    for o in range(W):
        want_send, want_off = em.pack_model(c.lists, c.U, c.ub, c.ib, o, raw[o], rb)
        assert np.array_equal(want_off, np.concatenate([[0], np.cumsum(want_counts[:, o])]))
        total = int(want_off[-1])
        bufs = []
        for _ in range(2):
            send = torch.full(((W * R + 2) * rb,), SENT_BYTE, dtype=torch.uint8, device=DEV)
            off = torch.full((W + 3,), SENT, dtype=torch.int32, device=DEV)
            shards[o].pack(acts, send, off)
            assert torch.equal(off[:W + 1], _dev(want_off)) and bool((off[W + 1:] == SENT).all()), "%s: send_off of owner %d" % (c.what, o)
            assert torch.equal(send[:total * rb], _dev(want_send.reshape(-1))), "%s: send bytes of owner %d" % (c.what, o)
            assert bool((send[total * rb:] == SENT_BYTE).all()), "%s: bytes behind send_off[W], owner %d" % (c.what, o)
            bufs.append(send)
        assert torch.equal(bufs[0], bufs[1])
        packed.append(bufs[0])
        models.append((want_send, want_off))
    for q in range(W):                     # the exchange by hand: owner o's chunk for requester q, owner by owner
        chunks = [packed[o][int(models[o][1][q]) * rb:int(models[o][1][q + 1]) * rb] for o in range(W)]
        recv = torch.cat(chunks + [torch.full((rb,), SENT_BYTE, dtype=torch.uint8, device=DEV)])
        recv_np = np.concatenate([models[o][0][int(models[o][1][q]):int(models[o][1][q + 1])] for o in range(W)])
        _unpack_and_check(shards[q], c.lists[q], recv, recv_np, c, dtype, False, window, "%s %s requester %d" % (c.what, dtype, q))
    return shards, raw


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("W", [1, 2, 5, 16])
def test_lookup_boundaries(W, dtype):
    """counts, pack, the exchange by hand and unpack on uneven owner blocks (an empty user block and an empty item block), lists of
    every pattern (full, ragged, users only, items only, one id, all padding -- between two others at W >= 3), ids on every
    owner boundary and on U - 1 / U, R = 64 and R = 1; S_out as a column window of a wider NaN tensor on every second case; direct
    unpack from the local table at W = 1 and, at W > 1, on lists of a rank's own rows."""
    cases = [em.lookup_case(W, k) for k in (range(6) if W < 3 else (0, 3))] + [em.lookup_case_r1(W)]
    for i, c in enumerate(cases):
        shards, raw = _check_lookup(c, dtype, DIMS, 100 * W + i, window=bool(i % 2))
        if W == 1:
            _unpack_and_check(shards[0], c.lists[0], None, raw[0], c, dtype, True, not i % 2, c.what + " direct")
    c = cases[0]
    shards, raw = _shards(c, dtype, DIMS, 7)
    for me in sorted({0, W // 2, (W // 2 + 1) % W, W - 1}):
        own = em.own_rows_list(c, me)
        assert len(em.valid(own)) >= 2
        _unpack_and_check(shards[me], own, None, raw[me], c, dtype, True, me % 2 == 0, "%s direct on rank %d's own rows" % (c.what, me))


@pytest.mark.parametrize("dtype,sum_d", [("f32", 4), ("f32", 260), ("f16", 12), ("f16", 520), ("bf16", 12), ("bf16", 520)])
def test_lookup_widths(dtype, sum_d):
    """Rows of one 16-byte piece and of 66 (pack) / of one float4 and of 65 or 130 (unpack): the column loops' second and third trip.
    Three ranks: one owns users and items, one items only, one users only."""
    for k in (0, 2):
        _check_lookup(em.lookup_case(3, k), dtype, (sum_d,), sum_d + k, window=bool(k))


def test_lookup_grid_stride():
    """W = 2, R = 9000: owner 0 packs 16771 rows and each requester unpacks more than 8192, so both grid-stride loops take a second
    (pack: and a third) trip."""
    _check_lookup(em.grid_case(), "f32", (4,), 3)


@pytest.mark.parametrize("W,R,dl", [(1, 1, 4), (16, 3, 4), (3, 257, 12), (5, 33, 8)])
def test_peer_cols_to_rows(W, R, dl):
    from elimrec_amd import ops
    rng = np.random.RandomState(W * R)
    recv = rng.standard_normal((W, R, 2 * dl)).astype(np.float32)
    w0, w1 = em.peer_cols_model(recv)
    got = []
    for _ in range(2):
        big0, big1 = _nan(R + 1, W * dl + 8), _nan(R + 1, W * dl + 4)               # ld0 != ld1, both wider than W dl
        ops.peer_cols_to_rows(_dev(recv), big0[:R, :W * dl], big1[:R, 4:])
        _bits_equal(big0[:R, :W * dl], w0, "out0")
        _bits_equal(big1[:R, 4:], w1, "out1")
        assert all_nan(big0[:R, W * dl:]) and all_nan(big1[:R, :4]) and all_nan(big0[R]) and all_nan(big1[R])
        got.append((big0, big1))
    assert same_bits(got[0][0], got[1][0]) and same_bits(got[0][1], got[1][1])


# ------------------------------------------------------------------------------------------------------- merge_rows, rows_bitmap
def _mask_buffer(N):
    """Two sentinel words, the (N + 31) / 32 words the kernels own, two sentinel words; the kernels get the middle."""
    words = (N + 31) // 32
    buf = torch.full((words + 4,), SENT, dtype=torch.int32, device=DEV)
    return buf, buf[2:2 + words]


def _mask_ok(buf, want_words, what):
    assert torch.equal(buf[2:-2], _dev(want_words.view(np.int32))), what + ": bitmap words"
    assert bool((buf[:2] == SENT).all()) and bool((buf[-2:] == SENT).all()), what + ": words outside (N + 31) / 32"


def _tables(N, ns, w, fill):
    from elimrec_amd import slab
    a, b = slab.SlabTable(N, ns, w, DEV), slab.SlabTable(N, ns, w, DEV)
    a.data.fill_(fill)
    b.data.fill_(fill)
    return a, b


def _merge_and_check(keys_np, W, R, U, I, ns, w, M, seed, what, named_only=True):
    """slab.merge_rows into zeroed tables (as shard.py does), twice; then into NaN tables, where the rows no list names must stay
    NaN and the named ones come out the same. Returns the launch's inputs and the zero-prefilled outputs."""
    from elimrec_amd import slab
    N, d = U + I, ns * w
    rows_np = em.merge_rows_input(W, R, (M if M > 0 else 2) * d, seed)
    rows, keys = _dev(rows_np), _dev(keys_np.reshape(-1))
    wA, wB, wbits = em.merge_model(rows_np, keys_np, W, R, U, N, d, M)
    outs = []
    for _ in range(2):
        sa, sb = _tables(N, ns, w, 0.0)
        buf, mask = _mask_buffer(N)
        slab.merge_rows(rows, keys, W, U, I, sa, sb, mask, M=M)
        _bits_equal(_dense(sa), wA, what + ": SrcA")
        _bits_equal(_dense(sb), wB, what + ": SrcB")
        _mask_ok(buf, wbits, what)
        outs.append((sa, sb, buf))
    assert same_bits(outs[0][0].data, outs[1][0].data) and same_bits(outs[0][1].data, outs[1][1].data), what + ": second launch"
    if named_only:
        sa, sb = _tables(N, ns, w, NAN)
        pre = np.full((N, d), np.nan, np.float32)
        nA, nB, _ = em.merge_model(rows_np, keys_np, W, R, U, N, d, M, srcA=pre, srcB=pre)
        buf, mask = _mask_buffer(N)
        slab.merge_rows(rows, keys, W, U, I, sa, sb, mask, M=M)
        named = np.zeros(N, bool)
        named[em.valid(keys_np.reshape(-1))] = True
        assert not np.isnan(nA[named]).any() and np.isnan(nA[~named]).all()
        _bits_equal(_dense(sa), nA, what + ": SrcA over NaN (named rows only)")
        _bits_equal(_dense(sb), nB, what + ": SrcB over NaN (named rows only)")
        _mask_ok(buf, wbits, what)
    return rows, keys, outs[0]


@pytest.mark.parametrize("N", em.CHUNK_NS)
def test_chunk_edges(N):
    """N = 20 (one partial word), 2592 (a multiple of 32, chunk 32), 32800 (chunk 64: two seen[] words per workgroup, bit >= 32, and
    the last workgroup's second word held back by the tail guard), 65540 (chunk 96): keys on lo, lo + 31, lo + 32 and hi - 1 of the
    first, a middle and the last workgroup. rows_bitmap's words == merge_rows' words == the model's, in a buffer of exactly
    (N + 31) / 32 words between sentinels."""
    from elimrec_amd import slab
    c = em.chunk_case(N)
    want = em.bitmap_model(c.keys, N)
    for _ in range(2):
        buf, mask = _mask_buffer(N)
        slab.rows_bitmap(_dev(c.keys), N, mask)
        _mask_ok(buf, want, c.what + " rows_bitmap")
    for M in (0, -1):
        _merge_and_check(c.keys, c.W, c.R, c.U, c.I, 1, 8, M, N + M, "%s merge M %d" % (c.what, M), named_only=(M == 0))


@pytest.mark.parametrize("M,W,nc4,R", [f + (None,) for f in em.merge_forms()] + [(0, 5, 2, 1), (3, 5, 6, 1), (-1, 2, 1, 1)])
def test_merge_forms(M, W, nc4, R):
    """Every form (M = 0: [H | G]; M = 1, 3: dOut blocks, G = block 0, H = their sum in block order; M = -1: no side swap) at
    1, 2, 5 and 64 ranks and at 1, 2, 6, 16 and 80 float4 per row (1, 2, 8 with two idle lanes, 16 and 64 lanes per row with a second
    trip): nodes U - 1 and U named by every rank, one node per side by two ranks, private nodes, an all-padding rank, R = 1."""
    ns, w = em.MERGE_GEOMS[nc4]
    c = em.merge_case(W, R)
    _merge_and_check(c.keys, c.W, c.R, c.U, c.I, ns, w, M, 1000 * W + 10 * nc4 + M, "%s M %d nc4 %d" % (c.what, M, nc4))


def test_fused_merge_at_three_ranks():
    """ops.linear_bwd_w_batched(..., merge=) at world = 3 and N = 32800 (chunk 64, a guarded tail word): srcA, srcB and the mask
    have the bits of slab.merge_rows on the same input (itself compared with the model), and the weight gradients those of the
    call without merge=. M = 0 and M = 3; M = -1 is refused on the host."""
    from elimrec_amd import ops
    c = em.chunk_case(32800)
    N, ns, w = c.N, 1, 8
    g = torch.Generator().manual_seed(2)
    Rw = 150
    A, B = torch.randn(Rw, 64, generator=g).to(DEV), torch.randn(Rw, 128, generator=g).to(DEV)
    wsp = torch.empty(ops.linear_bwd_w_batched_workspace([(Rw, 64, 128)]), dtype=torch.uint8, device=DEV)

    def problem():
        o = dict(w=_nan(64, 128), b=_nan(64))
        return o, [dict(A=A, B=B, out=o["w"], colsum=o["b"])]

    ref, pr = problem()
    ops.linear_bwd_w_batched(pr, wsp)
    assert not bool(torch.isnan(ref["w"]).any()) and not bool(torch.isnan(ref["b"]).any())
    for M in (0, 3):
        rows, keys, (sa, sb, buf1) = _merge_and_check(c.keys, c.W, c.R, c.U, c.I, ns, w, M, 50 + M, "fused M %d: merge_rows" % M, named_only=False)
        for _ in range(2):
            ta, tb = _tables(N, ns, w, 0.0)
            buf2, mask2 = _mask_buffer(N)
            got, pr = problem()
            ops.linear_bwd_w_batched(pr, torch.empty_like(wsp), merge=dict(rows=rows, keys=keys, world=c.W, U=c.U, I=c.I, srcA=ta, srcB=tb,
                                                                           mask=mask2, M=M))
            assert same_bits(ta.data, sa.data) and same_bits(tb.data, sb.data) and torch.equal(buf1, buf2), "fused M %d" % M
            assert same_bits(got["w"], ref["w"]) and same_bits(got["b"], ref["b"]), "fused M %d: weight gradients" % M
    ta, tb = _tables(N, ns, w, NAN)
    buf2, mask2 = _mask_buffer(N)
    got, pr = problem()
    rows = _dev(em.merge_rows_input(c.W, c.R, 2 * ns * w, 1))
    with pytest.raises((AssertionError, RuntimeError)):
        ops.linear_bwd_w_batched(pr, wsp, merge=dict(rows=rows, keys=_dev(c.keys.reshape(-1)), world=c.W, U=c.U, I=c.I, srcA=ta, srcB=tb,
                                                     mask=mask2, M=-1))
    torch.cuda.synchronize()
    assert all_nan(ta.data) and all_nan(tb.data) and all_nan(got["w"]) and bool((buf2 == SENT).all())


# -------------------------------------------------------------------------------------------------------------- argument checks
def test_bad_arguments_are_refused_on_the_host():
    """Bounds that do not cover [0, U), descending bounds, row_bytes not a multiple of 16 or too small for sum_d + c, dtype 3,
    65 ranks for merge_rows / rows_bitmap: the library's error, and nothing is launched -- every output still holds its sentinel."""
    from elimrec_amd import slab
    c = em.lookup_case(2, 0)
    shards, _ = _shards(c, "f32", DIMS, 1)
    sh = shards[0]
    W, R, rb = c.W, c.R, sh.row_bytes
    acts = _dev(c.lists)
    counts = torch.full((W, W), SENT, dtype=torch.int32, device=DEV)
    send = torch.full((W * R * rb,), SENT_BYTE, dtype=torch.uint8, device=DEV)
    off = torch.full((W + 1,), SENT, dtype=torch.int32, device=DEV)
    S, cr = _nan(R, sh.sum_d), _nan(R)
    good = sh.owners._ub

    def calls():
        return (lambda: sh.counts(acts, out=counts), lambda: sh.pack(acts, send, off), lambda: sh.unpack(acts[0], send, S, cr))

    for bad, msg in (([0, 100, c.U - 1], "bounds must cover"), ([1, 100, c.U], "bounds must cover"), ([0, c.U + 5, c.U], "ascending")):
        sh.owners._ub = (ctypes.c_int64 * (W + 1))(*bad)
        for call in calls():
            with pytest.raises(RuntimeError, match=msg):
                call()
    sh.owners._ub = good
    for bad_rb, msg, which in ((rb + 4, "multiple of 16", (1,)), (rb + 4, "row_bytes too small", (2,)), (16, "row_bytes too small", (2,))):
        sh.row_bytes = bad_rb
        for i in which:
            with pytest.raises(RuntimeError, match=msg):
                calls()[i]()
    sh.row_bytes = rb
    sh.code = 3
    with pytest.raises(RuntimeError, match="dtype 0"):
        calls()[2]()
    sh.code = 0
    Wm, Rm, N = em.SLAB_MAX_RANKS + 1, 4, 64
    keys = _dev(np.tile(em.pad_list([1, 40], Rm), Wm))
    sa, sb = _tables(N, 1, 8, NAN)
    buf, mask = _mask_buffer(N)
    with pytest.raises(RuntimeError, match="ranks"):
        slab.merge_rows(_nan(Wm * Rm, 16), keys, Wm, 32, 32, sa, sb, mask)
    with pytest.raises(RuntimeError, match="rows_bitmap"):
        slab.rows_bitmap(keys.view(Wm, Rm), N, mask)
    torch.cuda.synchronize()
    assert bool((counts == SENT).all()) and bool((send == SENT_BYTE).all()) and bool((off == SENT).all()) and all_nan(S) and all_nan(cr)
    assert all_nan(sa.data) and all_nan(sb.data) and bool((buf == SENT).all())
    calls()[0]()                                                                # and the restored shard still works
    assert torch.equal(counts, _dev(em.owner_counts(c.lists, c.U, c.ub, c.ib)))
