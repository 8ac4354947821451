"""The batch planner of csrc/bpr.hip -- elimrec_segment_plan / elimrec_batch_plan in their three forms, segment_sum_kernel, and the row
copies triplet_rows / triplet_rows_checked / gather_rows -- against tests/plan_model.py, bit for bit.

Forms are chosen by shape alone (no environment variable here) and every case asserts the form through ops.segment_plan_form. Outputs
start as sentinels or NaN and lie between guard words; the guards behind the bitmap's (key_space + 31) / 32 words and around the
workspace included. The workspace layout stays private: the order of a member list is observed through segment_apply's float32 sums,
which test_plan_cpu.py shows to change bits under a reversed or rotated list for every list of three or more slots of every case here.
The radix-sort cases sort_* hold the key lists of their dev_* twins with key_space = 0: both are compared with the same model output."""
import numpy as np
import pytest
import torch

import plan_cases as pc
import plan_model as pm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                      # guard elements (rows, for 2-D buffers) on either side of every output
SENT = -7                       # integer outputs start as this
E_BADARG, E_WORKSPACE = "rc=10001", "rc=10003"


def _t(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)


class Guarded(object):
    """A buffer of `fill` with GUARD elements (rows) before and after the view handed to the library."""

    def __init__(self, shape, dtype, fill):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        self.n = shape[0]
        self.buf = torch.full((self.n + 2 * GUARD,) + shape[1:], fill, dtype=dtype, device=DEV)
        self.before = self.buf.cpu().numpy().tobytes()
        self.view = self.buf[GUARD:GUARD + self.n]

    def result(self, what):
        host = self.buf.cpu().numpy()
        raw, row = host.tobytes(), host[0].nbytes if host.ndim > 1 else host.itemsize
        lo, hi = GUARD * row, (GUARD + self.n) * row
        assert raw[:lo] == self.before[:lo] and raw[hi:] == self.before[hi:], "a write outside " + what
        return host[GUARD:GUARD + self.n]

    def untouched(self):
        return self.buf.cpu().numpy().tobytes() == self.before


def _same(got, want):
    want = np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.ascontiguousarray(got).tobytes() == want.tobytes()


def _where(got, want):
    bad = np.nonzero(np.asarray(got).reshape(len(got), -1) != np.asarray(want).reshape(len(want), -1))[0]
    return len(bad), bad[:5].tolist()


class PlanRun(object):
    """One call of segment_plan (keys given) or batch_plan (batch given) into guarded outputs."""

    def __init__(self, n, key_space, bitmap):
        from elimrec_amd import ops
        self.n, self.key_space = n, key_space
        self.need = ops.segment_plan_workspace(n)
        # the workspace between 256 guard bytes of its own (GUARD = 64 bytes would misalign it)
        self.ws_buf = torch.full((self.need + 512,), 0xA5, dtype=torch.uint8, device=DEV)
        self.ws_view = self.ws_buf[256:256 + self.need]
        self.act = Guarded(n, torch.int32, SENT)
        self.seg = Guarded(8, torch.int32, SENT)
        self.slot_seg = Guarded(n, torch.int32, SENT)
        self.bitmap = Guarded((key_space + 31) // 32, torch.int32, 0x5A5A5A5A) if bitmap else None

    def segment_plan(self, keys, split):
        from elimrec_amd import ops
        ops.segment_plan(keys if isinstance(keys, torch.Tensor) else _t(keys), split, self.key_space, self.act.view, self.seg.view, self.slot_seg.view, self.ws_view,
                         key_bitmap=self.bitmap.view if self.bitmap else None)
        return self

    def batch_plan(self, batch, err, pad_key=pc.PAD_KEY):
        from elimrec_amd import ops
        self.keys = Guarded(self.n, torch.int32, SENT)
        ops.batch_plan(_t(batch.users), _t(batch.pos), _t(batch.neg), batch.U, batch.I, self.keys.view, self.act.view, self.seg.view,
                       self.slot_seg.view, self.ws_view, err, pad_key, key_bitmap=self.bitmap.view if self.bitmap else None)
        return self

    def check(self, want, padded):
        """active rows (and their tail), the 8 seg_info values, the slot map and the bitmap against the model's plan."""
        torch.cuda.synchronize()
        ws = self.ws_buf.cpu().numpy()
        assert (ws[:256] == 0xA5).all() and (ws[256 + self.need:] == 0xA5).all(), "a write outside the workspace"
        seg = self.seg.result("seg_info")
        assert seg.tolist() == want.seg_info.tolist()
        n_act = int(want.seg_info[0])
        act = self.act.result("active_rows")
        assert _same(act[:n_act], want.active), _where(act[:n_act], want.active)
        tail = want.active_rows[n_act:] if padded else np.full(self.n - n_act, SENT, dtype=np.int32)
        assert _same(act[n_act:], tail), ("tail of active_rows", _where(act[n_act:], tail))
        slot_seg = self.slot_seg.result("slot_seg")
        assert _same(slot_seg, want.slot_seg), _where(slot_seg, want.slot_seg)
        if self.bitmap:
            words = self.bitmap.result("the key bitmap").view(np.uint32)
            assert _same(words, want.bitmap), _where(words, want.bitmap)

    def check_sums(self, want, ld=pc.LD):
        """segment_apply over the plan left in the workspace, unscaled and scaled: rows [0, n_act) carry the model's bits, the rest stay."""
        from elimrec_amd import ops
        n_act = int(want.seg_info[0])
        rows = pc.rows(self.n, ld)
        rows_d = _t(rows)
        for scale in (None, pc.SCALE):
            red = Guarded((self.n, ld), torch.float32, float("nan"))
            ops.segment_apply(rows_d, self.seg.view, red.view, self.ws_view,
                              scale=None if scale is None else torch.full((1,), scale, dtype=torch.float32, device=DEV))
            torch.cuda.synchronize()
            got = red.result("the segment sums")
            exp = pm.segment_sums_f32(rows, want.members, want.seg_start, scale)
            assert _same(got[:n_act], exp), ("segment sums", scale, _where(got[:n_act].view(np.uint32), exp.view(np.uint32)))
            assert np.isnan(got[n_act:]).all(), "a sum written beyond the active segments"


def _assert_form(n, key_space, form):
    from elimrec_amd import ops
    assert ops.segment_plan_form(n, key_space) == form, (n, key_space, ops.segment_plan_form(n, key_space), form)


# ---------------------------------------------------------------------------------------------------- segment_plan
@pytest.mark.parametrize("name", list(pc.segment_cases()))
def test_segment_plan_bitwise(name):
    """Every decision edge of the form choice and every sort tier (plan_cases.segment_cases), without and with a key bitmap.

    dev_8193_one_key is the smallest list that reaches the top tier (a rank sort through global scratch in one workgroup, 67 M
    comparisons, then plan_copy_long_kernel). Measured on the MI355X, events around the planner call: 12.2 ms for dev_8193_one_key
    (its radix-sort twin sort_8193_one_key: 0.07 ms), 12.3 ms for dev_tiers, 14.7 ms for dev_two_beyond_lds (lists of 9000 and 8193
    slots, a workgroup each); each of these tests takes under 0.2 s in all. Milliseconds, as expected, and no more."""
    case = pc.segment_cases()[name]
    n = len(case.keys)
    _assert_form(n, case.key_space, case.form)
    want = pm.plan(case.keys, case.split, case.key_space)
    keys_d = _t(case.keys)
    for bitmap in ((False, True) if case.key_space else (False,)):
        run = PlanRun(n, case.key_space, bitmap)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        run.segment_plan(keys_d, case.split)
        t1.record()
        torch.cuda.synchronize()
        print("%s: form %d, n %d, planner call %.3f ms" % (name, case.form, n, t0.elapsed_time(t1)))
        run.check(want, padded=False)
        run.check_sums(want)


@pytest.mark.parametrize("name", pc.WIDE_CASES)
def test_segment_sums_beyond_one_pass_of_the_lanes(name):
    """260 columns = 65 float4: segment_sum_kernel's 64 lanes come round a second time for the last one."""
    case = pc.segment_cases()[name]
    _assert_form(len(case.keys), case.key_space, case.form)
    run = PlanRun(len(case.keys), case.key_space, False).segment_plan(case.keys, case.split)
    run.check_sums(pm.plan(case.keys, case.split, case.key_space), ld=pc.WIDE_LD)


@pytest.mark.parametrize("name", ["wg_tiers", "wg_ks32", "wg_max_key_space", "dev_ks33", "dev_7680_big_key_space", "sort_300_big_key_space",
                                  "sort_two_beyond_lds"])
def test_split_keys(name):
    """split_key below 0, at 0, at a word boundary, mid-word, at an absent key, at the largest key, at key_space and above it."""
    case = pc.segment_cases()[name]
    _assert_form(len(case.keys), case.key_space, case.form)
    seen = set()
    for split in pc.split_keys(case):
        want = pm.plan(case.keys, split, case.key_space)
        PlanRun(len(case.keys), case.key_space, True if case.key_space else False).segment_plan(case.keys, split).check(want, padded=False)
        seen.add(int(want.seg_info[1]))
    assert 0 in seen and int(want.seg_info[0]) in seen and (len(seen) > 2 or want.seg_info[0] < 2)


# ---------------------------------------------------------------------------------------------------- batch_plan
@pytest.mark.parametrize("bitmap", [False, True], ids=["nobitmap", "bitmap"])
@pytest.mark.parametrize("name", list(pc.batches()))
def test_batch_plan_valid(name, bitmap):
    """keys out, err left exactly as it was (0 and an unrelated bit), the plan, its padded tail, the sums."""
    b = pc.batches()[name]
    n = 3 * len(b.users)
    _assert_form(n, b.U + b.I, b.form)
    keys, bits = pm.batch_keys(b.users, b.pos, b.neg, b.U, b.I)
    assert bits == 0
    want = pm.plan(keys, b.U, b.U + b.I, pad_key=pc.PAD_KEY)
    for err0 in (0, 8):
        err = Guarded(1, torch.int32, err0)
        run = PlanRun(n, b.U + b.I, bitmap).batch_plan(b, err.view)
        torch.cuda.synchronize()
        assert err.untouched()
        assert _same(run.keys.result("keys"), keys)
        run.check(want, padded=True)
    run.check_sums(want)


@pytest.mark.parametrize("name", list(pc.batches()))
def test_batch_plan_bad_ids(name):
    """One bad user / positive / negative, alone and together, at -1, the limit and 2^40 + 5: the bit ORed into err (preloaded with an
    unrelated bit), id 0 in its place, and the plan of the clamped keys."""
    good = pc.batches()[name]
    n = 3 * len(good.users)
    _assert_form(n, good.U + good.I, good.form)
    for label, b, bits in pc.bad_batches(name):
        keys, model_bits = pm.batch_keys(b.users, b.pos, b.neg, b.U, b.I)
        assert model_bits == bits
        want = pm.plan(keys, b.U, b.U + b.I, pad_key=pc.PAD_KEY)
        err = Guarded(1, torch.int32, 8)
        run = PlanRun(n, b.U + b.I, True).batch_plan(b, err.view)
        torch.cuda.synchronize()
        assert err.result("err").tolist() == [8 | bits], label
        assert _same(run.keys.result("keys"), keys), label
        run.check(want, padded=True)


# ---------------------------------------------------------------------------------------------------- the row copies
U_ROWS, I_ROWS = 23, 40
WINDOW = 4                      # the copied columns start here in tables 8 columns wider


def _ids(B, seed):
    rng = np.random.default_rng(seed)
    u, p, q = rng.integers(0, U_ROWS, B), rng.integers(0, I_ROWS, B), rng.integers(0, I_ROWS, B)
    u[0], p[0], q[-1] = U_ROWS - 1, 0, I_ROWS - 1
    return u.astype(np.int64), p.astype(np.int64), q.astype(np.int64)


def _table(rows, cols, seed):
    """A float32 table 8 columns wider than the window [WINDOW, WINDOW + cols), NaN outside the window."""
    t = np.full((rows, cols + 8), np.nan, dtype=np.float32)
    t[:, WINDOW:WINDOW + cols] = np.random.default_rng(seed).standard_normal((rows, cols)).astype(np.float32)
    return t


def _window_result(dst, n, cols, what):
    """The window of a guarded NaN table after a copy; everything outside it must still be NaN."""
    full = dst.result(what)
    outside = np.delete(full, np.s_[WINDOW:WINDOW + cols], axis=1)
    assert np.isnan(outside).all(), "columns outside the window of " + what
    return full[:, WINDOW:WINDOW + cols]


@pytest.mark.parametrize("B", [1, 5, 6, 341])            # 3B = 3, 15, 18, 1023: below, just below, above and far above 16 slots a block
def test_triplet_rows_bitwise(B):
    from elimrec_amd import ops
    u, p, q = _ids(B, B)
    du, dp, dq = _t(u), _t(p), _t(q)
    want_rows, _ = pm.triplet_rows(u, p, q, U_ROWS)
    rows = Guarded(3 * B, torch.int32, SENT)
    ops.triplet_rows(du, dp, dq, U_ROWS, rows.view)
    torch.cuda.synchronize()
    assert _same(rows.result("rows"), want_rows)
    for cols in (4, 64, 68, 260):                        # 1, 16, 17 and 65 float4: under, at and over one pass of the 16 lanes
        src = _table(U_ROWS + I_ROWS, cols, cols)
        _, want = pm.triplet_rows(u, p, q, U_ROWS, src[:, WINDOW:], cols)
        rows = Guarded(3 * B, torch.int32, SENT)
        dst = Guarded((3 * B, cols + 8), torch.float32, float("nan"))
        ops.triplet_rows(du, dp, dq, U_ROWS, rows.view, src=_t(src)[:, WINDOW:WINDOW + cols], dst=dst.view[:, WINDOW:WINDOW + cols])
        torch.cuda.synchronize()
        assert _same(rows.result("rows"), want_rows), cols
        assert _same(_window_result(dst, 3 * B, cols, "dst"), want), cols
    # range-checked: valid ids leave err alone; a bad id sets its bit beside the one already there and reads as id 0
    for err0 in (0, 8):
        rows, err = Guarded(3 * B, torch.int32, SENT), Guarded(1, torch.int32, err0)
        ops.triplet_rows(du, dp, dq, U_ROWS, rows.view, I=I_ROWS, err=err.view)
        torch.cuda.synchronize()
        assert err.untouched() and _same(rows.result("rows"), want_rows)
    for j, bad in ((0, -1), (0, U_ROWS), (1, I_ROWS), (1, (1 << 40) + 5), (2, -1), (2, I_ROWS)):
        cols3 = [u.copy(), p.copy(), q.copy()]
        cols3[j][B // 2] = bad
        keys, bits = pm.batch_keys(*cols3, U_ROWS, I_ROWS)
        assert bits == 1 << j
        rows, err = Guarded(3 * B, torch.int32, SENT), Guarded(1, torch.int32, 8)
        ops.triplet_rows(*(_t(c) for c in cols3), U_ROWS, rows.view, I=I_ROWS, err=err.view)
        torch.cuda.synchronize()
        assert err.result("err").tolist() == [8 | bits] and _same(rows.result("rows"), keys), (j, bad)


@pytest.mark.parametrize("cols", [4, 64, 68, 260])
def test_gather_rows_bitwise(cols):
    from elimrec_amd import ops
    n_src = 50
    src = _table(n_src, cols, 900 + cols)
    src_d = _t(src)[:, WINDOW:WINDOW + cols]
    rng = np.random.default_rng(cols)
    lists = {"random": rng.integers(0, n_src, 37), "duplicates": np.array([7, 7, 0, 49, 7, 49, 0, 0] * 4 + [49]),
             "descending": np.arange(n_src - 1, -1, -1)[:35], "one": np.array([49])}
    for label, ids in lists.items():
        ids = ids.astype(np.int32)
        n = len(ids)
        for count in (None, 0, n // 2, n - 1, n, n + 1, n + 1000):
            dst = Guarded((n, cols + 8), torch.float32, float("nan"))
            ops.gather_rows(src_d, _t(ids), dst.view[:, WINDOW:WINDOW + cols],
                            count=None if count is None else torch.full((1,), count, dtype=torch.int32, device=DEV))
            torch.cuda.synchronize()
            got = _window_result(dst, n, cols, "dst")
            want = pm.gather_rows(src[:, WINDOW:WINDOW + cols], ids, np.full((n, cols), np.nan, dtype=np.float32), count)
            lim = n if count is None else min(count, n)
            assert _same(got[:lim], want[:lim]) and np.isnan(got[lim:]).all() and np.isnan(want[lim:]).all(), (label, count)


# ---------------------------------------------------------------------------------------------------- argument checks
def _plan_outputs_untouched(run):
    torch.cuda.synchronize()
    return all(g.untouched() for g in (run.act, run.seg, run.slot_seg) + ((run.bitmap,) if run.bitmap else ())) and \
        bool((run.ws_buf == 0xA5).all())


@pytest.mark.parametrize("name", ["wg_tiers", "dev_ks33", "sort_300_big_key_space"])
def test_workspace_one_byte_short(name):
    from elimrec_amd import ops
    case = pc.segment_cases()[name]
    run = PlanRun(len(case.keys), case.key_space, True)
    run.ws_view = run.ws_buf[256:256 + run.need - 1]
    with pytest.raises(RuntimeError, match=E_WORKSPACE):
        run.segment_plan(case.keys, case.split)
    assert _plan_outputs_untouched(run)
    red = Guarded((len(case.keys), pc.LD), torch.float32, float("nan"))
    with pytest.raises(RuntimeError, match=E_WORKSPACE):
        ops.segment_apply(_t(pc.rows(len(case.keys))), run.seg.view, red.view, run.ws_view)
    torch.cuda.synchronize()
    assert red.untouched()
    b = pc.batches()["wg_B100"]
    run = PlanRun(300, b.U + b.I, False)
    run.ws_view = run.ws_buf[256:256 + run.need - 1]
    err = Guarded(1, torch.int32, 8)
    with pytest.raises(RuntimeError, match=E_WORKSPACE):
        run.batch_plan(b, err.view)
    assert _plan_outputs_untouched(run) and run.keys.untouched() and err.untouched()


def test_bad_arguments_are_errors():
    from elimrec_amd import ops
    case = pc.segment_cases()["wg_ks33"]
    run = PlanRun(len(case.keys), 0, False)
    run.bitmap = Guarded(2, torch.int32, 0x5A5A5A5A)                       # a bitmap without a key space
    with pytest.raises(RuntimeError, match=E_BADARG):
        run.segment_plan(case.keys, case.split)
    assert _plan_outputs_untouched(run)
    run = PlanRun(len(case.keys), case.key_space, True)                    # n = 0
    with pytest.raises(RuntimeError, match=E_BADARG):
        ops.segment_plan(run.act.view[:0], 0, case.key_space, run.act.view, run.seg.view, run.slot_seg.view, run.ws_view,
                         key_bitmap=run.bitmap.view)
    assert _plan_outputs_untouched(run)
    u, p, q = (_t(a) for a in _ids(5, 5))                                  # cols = 6 (the leading dimensions are multiples of 4)
    src = _t(_table(U_ROWS + I_ROWS, 8, 1))
    rows, dst = Guarded(15, torch.int32, SENT), Guarded((15, 16), torch.float32, float("nan"))
    with pytest.raises(RuntimeError, match=E_BADARG):
        ops.triplet_rows(u, p, q, U_ROWS, rows.view, src=src[:, 4:10], dst=dst.view[:, 4:10])
    with pytest.raises(RuntimeError, match=E_BADARG):
        ops.gather_rows(src[:, 4:10], _t(np.arange(15, dtype=np.int32)), dst.view[:, 4:10])
    torch.cuda.synchronize()
    assert rows.untouched() and dst.untouched()
    red = Guarded((len(case.keys), 6), torch.float32, float("nan"))        # segment_apply: ld = 6
    with pytest.raises(RuntimeError, match=E_BADARG):
        ops.segment_apply(torch.zeros(len(case.keys), 6, device=DEV), run.seg.view, red.view, run.ws_view)
    torch.cuda.synchronize()
    assert red.untouched()
