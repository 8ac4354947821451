"""The evaluation scorers of csrc/eval.hip against a float64 model of predict() (tests/score_model.py, itself pinned to the
reference's recorded predict() by test_score_model_cpu.py) -- not against the scorer's own EXACT mode.

Every case: outputs pre-filled with NaN, the reference computed with float64 torch on the device from the same table, every
unmasked element within the rule of score_model.tolerance (EXACT: max(4 E32, 2.4e-7), E32 = what plain float32 torch loses on the
same inputs; FAST, fp32 or bf16 pieces: + 4e-7), masked positions exactly -inf and no others, the sentinel columns behind the [B, I]
window of a padded matrix untouched, a second launch bit-identical, no range violation counted. Every table but the shard tables
of test_item_shards (contiguous copies: ldy = (1 + S) d) is a column window of a wider NaN-filled tensor (ldy > (1 + S) d); every
user list of four or more is a permutation's head with one id repeated and users 0 and U - 1 present (B = 1: user U - 1 alone).
The saturated family departs from "40 item rows x 6" on purpose: x 6 alone gives logits of standard deviation 8 at recdim 64,
nowhere near +-88, so 30 rows are scaled x 6 and 10 more x 40 -- those are the ones whose sigmoids saturate.

Case -> kernel form (the dispatch conditions of score_topk_impl):
  test_generic_scorer_*           score_mfma_kernel<1|2>: recdim 4 / 48 / 200 / 256 (below, across, beyond the 64-column staging), S 0..4
  test_t16_scorer_*               score_t16_kernel<1|2, NB 2..4, 7 (type, fusion), FAST 0|1, D 32|64|128>
  test_user_counts                both, B 1 / 15 / 16 / 17 / 128 / 129 / 200 (lane group and workgroup short, exact, over), sqnorm= given
  test_catalogue_sizes            both, I 5 / 16 / 17 / 8192 / 8207 / 16384 (tail tile; one / two tiles per workgroup; the largest chunk)
  test_matrix_in_chunks           I 16385 / 18433 / 40000, S = 3: score_t16b_kernel<1|2, NB 4, 7 (type, fusion), D 32|64> +
                                  split3_items_kernel (FAST, bf16x3 on), score_t16_kernel chunk by chunk (bf16x3 off, EXACT,
                                  recdim 128, and a workspace without room for the planes)
  test_chunked_forms_over_heads   the same at S = 1 / 2: score_t16b_kernel<1|2, NB 2|3, 7 (type, fusion), D 32|64> (its own LDS
                                  window and norm stride per NB), the chunk-by-chunk score_t16_kernel at NB 2|3, D 32|64|128,
                                  matrix and top-K only
  test_head_masks                 every mask of the issue x every fusion, t16 / generic / t16b
  test_input_families             saturated, zero / tiny head blocks, I = 37 / 300 (the row mean's divisor), t16 / generic / t16b
  test_topk_only                  chunked lists (pilot chunk, store threshold, running list: topk_tiles_kernel), K = 300 (private
                                  matrix), unchunked t16 (tile-guided), generic (topk_select / topk_kernel) -- without the project's
                                  own score matrix
  test_item_shards                elimrec_score_topk_shard phases 1 / 2: mean_from_sum_kernel, id_offset, I_total
  test_candidate_lists            score_cand_kernel<NB 1..4, DT 1|2|0, FAST 0|1>, TIE fed by phase 1
  test_workspace_for_is_exact     elimrec_score_workspace_for against what the call accepts (one plan for both), generic / t16 / t16b
  test_row_sqnorms_*              row_sqnorm_kernel against float64 sums of squares, (d + 4) 2^-24 relative

Worst err / tol measured on an MI355X (run with -s: every case prints err, tol and E32, the module its worst ratios at the end):
  generic (score_mfma_kernel)        EXACT 0.39   FAST 0.27      saturated rows, recdim 48: TE sum / normal
  t16 (score_t16_kernel)             EXACT 0.49   FAST 0.21      saturated rows, recdim 64: TE sum / normal
  t16b (score_t16b_kernel, bf16x3)                FAST 0.31      saturated rows, 18 433 items, recdim 64: normal
  item shards (t16, phases 1 / 2)    EXACT 0.25   FAST 0.16
  candidates (score_cand_kernel)     EXACT 0.32   FAST 0.16
The kernels' own error is that of plain float32 torch (err ~ E32 ~ 1e-7 on every case); no ratio came near 1, no kernel changed.
The whole file takes 6.8 s (pytest's total; the slowest call 0.8 s) on the GPU box (cap: 40 s).

Value-only mutants of eval.hip this file was run against once each (all in bounds, none committed); every one is caught:
  tail tile of score_t16_kernel loads item row i - 1         57 of 102 fail: every t16 case whose I is not a multiple of 16
                                                             (test_t16_scorer_*, test_catalogue_sizes, test_matrix_in_chunks
                                                             16385 / 18433, test_chunked_forms_over_heads, ...); 40 000 passes
  item inverse norm of head h ^ 1 in score_t16_kernel        54 fail: every t16 case with S >= 2 and TE / TIE
  mean_div = I - 1 in score_topk_impl                        87 fail: every test with a TIE case that owns its pass 1, first of
                                                             all test_small_catalogue_row_mean (candidates and shards, whose
                                                             mean comes from phase 1 sums and I_total, rightly pass)
  hi x mid piece product dropped in score_t16b_kernel        13 of the 96 tests the file had before test_chunked_forms_over_heads was added:
                                                             exactly the FAST cases on the bf16 planes (test_matrix_in_chunks
                                                             recdim 32 / 64, test_head_masks[fast-32-18433],
                                                             test_input_families[fast-*-18433], test_topk_only[fast-64-18433 / 32-40000])
"""
import numpy as np
import pytest
import torch

import score_model as sm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
PAD = 5                      # sentinel columns behind the [B, I] window
WORST = {}                   # (kernel form, math mode) -> (err / tol, case)


@pytest.fixture(params=["exact", "fast"])
def eval_math(request):
    """The math mode a test runs its cases in. Only the name: _Switches sets and restores the library's switches around every call."""
    return request.param


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for key in sorted(WORST):
        print("worst err/tol  %-10s %-5s  %.3f  at %s" % (key + WORST[key]))


@pytest.fixture(autouse=True)
def _no_range_violations():
    from elimrec_amd import ops
    ops.score_range_violations()               # (clears what earlier tests left)
    yield
    assert ops.score_range_violations() == 0


class _Switches(object):
    """The math / bf16x3 switches for one block, restored on the way out."""

    def __init__(self, fast, b3=1):
        self.fast, self.b3 = fast, b3

    def __enter__(self):
        from elimrec_amd import _lib
        self.lib = _lib.load()
        self.before = (int(self.lib.elimrec_score_get_math()), int(self.lib.elimrec_score_get_bf16x3()))
        self.lib.elimrec_score_set_math(1 if self.fast else 0)
        self.lib.elimrec_score_set_bf16x3(1 if self.b3 else 0)

    def __exit__(self, *exc):
        self.lib.elimrec_score_set_math(self.before[0])
        self.lib.elimrec_score_set_bf16x3(self.before[1])


def _form(d, S, I, fast, b3, roomy=True):
    """The scorer form score_topk_impl picks for a call shape."""
    if d in (32, 64, 128) and 1 <= S <= 3:
        if I > 16384 and fast and b3 and d in (32, 64) and roomy:
            return "t16b"
        return "t16"
    return "generic"


def _note(form, fast, err, tol, what):
    key = (form, "FAST" if fast else "EXACT")
    r = err / tol
    if key not in WORST or r > WORST[key][0]:
        WORST[key] = (r, what)


def _users(U, B, seed):
    """A permutation's first B ids with users 0 and U - 1 among them and one id twice (B >= 4)."""
    g = torch.Generator().manual_seed(seed)
    if B == 1:
        return torch.tensor([U - 1])
    if B < 4:
        return torch.tensor([0, U - 1, 1][:B])
    rest = (torch.randperm(U - 2, generator=g) + 1)[:B - 3]
    ids = torch.cat([torch.tensor([0, U - 1]), rest, rest[:1]])
    return ids[torch.randperm(B, generator=g)]


class Case(object):
    """One table, user list and train mask on the device, with the model's logits and cosines in float64 and float32."""

    def __init__(self, family, U, I, d, S, B, seed=0, train=True):
        from elimrec_amd import ops
        assert U >= B
        self.family, self.U, self.I, self.d, self.S, self.B = family, U, I, d, S, B
        W = (1 + S) * d
        wide = torch.full((U + I, W + 8), NAN, device=DEV)
        wide[:, 4:4 + W] = sm.make_table(family, U, I, d, S, seed).to(DEV)
        self.Y = wide[:, 4:4 + W]                         # ldy = W + 8, 16 bytes into the row
        self.users = _users(U, B, seed + 1).to(DEV)
        ub, ib = sm.blocks(self.Y.double(), U, self.users, d, S)
        self.a64, self.z64 = sm.logits(ub, ib), sm.cosines(ub, ib)
        ub, ib = sm.blocks(self.Y, U, self.users, d, S)
        self.a32, self.z32 = sm.logits(ub, ib), sm.cosines(ub, ib)
        self.sqn = torch.full((U + I, 1 + S), NAN, device=DEV)
        ops.row_sqnorms(self.Y, d, 1 + S, self.sqn)
        rng = np.random.default_rng(seed + 2)
        lists = []
        for b in range(B):
            n = int(rng.integers(0, max(1, min(30, I // 3)))) if train and b != 0 else 0
            lists.append(sorted(rng.choice(I, size=n, replace=False).tolist()))
        if train and B > 1 and I >= 5:
            lists[1] = sorted(set(lists[1]) | {0, I - 1})
        self.lists = lists
        ptr = np.zeros(B + 1, np.int64)
        ptr[1:] = np.cumsum([len(x) for x in lists])
        self.ptr = torch.from_numpy(ptr).to(DEV)
        self.items = torch.tensor([i for x in lists for i in x] + [0], dtype=torch.int32, device=DEV)
        self.tmask = torch.zeros(B, I, dtype=torch.bool, device=DEV)
        for b, x in enumerate(lists):
            if x:
                self.tmask[b, torch.tensor(x, device=DEV)] = True

    def refs(self, mask, fusion, ptype, mean64=None, mean32=None):
        return (sm.predict(self.a64, self.z64, mask, fusion, ptype, mean64), sm.predict(self.a32, self.z32, mask, fusion, ptype, mean32))

    def what(self, *more):
        return "%s U=%d I=%d d=%d S=%d B=%d %s" % (self.family, self.U, self.I, self.d, self.S, self.B, " ".join(str(m) for m in more))


def _pairs(S):
    return [(p, f) for p, f in sm.PAIRS if S > 0 or f == "rubi"]


def _bits_equal(x, y):
    return torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def _check_matrix(c, mask, fusion, ptype, fast, b3=1, sqn=False, roomy=True):
    """scores= given: the whole contract of the module docstring for one call shape."""
    from elimrec_amd import ops
    U, I, d, S, B = c.U, c.I, c.d, c.S, c.B
    ref64, ref32 = c.refs(mask, fusion, ptype)
    keep = ~c.tmask
    tol, e32 = sm.tolerance(ref64, ref32, fast, keep)
    nbytes = ops.score_workspace(B, U, I, S, 0, d=d) if roomy else ops.score_workspace(B, U, I, S, 0)
    outs = []
    with _Switches(fast, b3):
        for rep in range(2):
            ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
            buf = torch.full((B, I + PAD), NAN, device=DEV)
            ops.score_topk(c.Y, U, I, c.users, d, S, mask, fusion, ptype, ws, scores=buf[:, :I], train_ptr=c.ptr, train_items=c.items,
                           sqnorm=c.sqn if sqn else None)
            outs.append(buf)
    what = c.what(ptype, fusion, "mask=%d" % mask, "b3=%d" % b3, "" if roomy else "no room for planes")
    got = outs[0][:, :I]
    assert bool(torch.isnan(outs[0][:, I:]).all()), ("wrote behind the [B, I] window", what)
    assert _bits_equal(outs[0], outs[1]), ("second launch differs", what)
    assert torch.equal(got == -np.inf, c.tmask), ("-inf is not exactly the masked positions", what)
    err = sm.worst_error(got, ref64, keep)
    print("%-8s %-5s err %.3e tol %.3e E32 %.3e  %s" % (_form(d, S, I, fast, b3, roomy), "FAST" if fast else "EXACT", err, tol, e32, what))
    _note(_form(d, S, I, fast, b3, roomy), fast, err, tol, what)
    assert err <= tol, (what, "err", err, "tol", tol, "E32", e32)


def _check_topk(c, mask, fusion, ptype, fast, K, b3=1):
    """Top-K only, against float64 alone: (a) values within tolerance of ref64 at the returned ids, (b) no id masked, repeated or
    out of range, (c) values non-increasing, (d) no unmasked item outside the list beats the list's worst by more than 2 tol."""
    from elimrec_amd import ops
    U, I, d, S, B = c.U, c.I, c.d, c.S, c.B
    ref64, ref32 = c.refs(mask, fusion, ptype)
    keep = ~c.tmask
    tol, e32 = sm.tolerance(ref64, ref32, fast, keep)
    nbytes = ops.score_workspace(B, U, I, S, K, topk_only=True, d=d)
    outs = []
    with _Switches(fast, b3):
        for rep in range(2):
            ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
            idx = torch.full((B, K), -1, dtype=torch.int32, device=DEV)
            val = torch.full((B, K), NAN, device=DEV)
            ops.score_topk(c.Y, U, I, c.users, d, S, mask, fusion, ptype, ws, K=K, topk_idx=idx, topk_val=val, train_ptr=c.ptr,
                           train_items=c.items)
            outs.append((idx, val))
    what = c.what(ptype, fusion, "K=%d" % K, "b3=%d" % b3)
    idx, val = outs[0]
    assert torch.equal(idx, outs[1][0]) and _bits_equal(val, outs[1][1]), ("second launch differs", what)
    li = idx.long()
    assert bool(((li >= 0) & (li < I)).all()), ("id out of range", what)
    assert not bool(c.tmask.gather(1, li).any()), ("masked item returned", what)
    srt = li.sort(1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all()), ("repeated id", what)
    at = ref64.gather(1, li)
    err = sm.worst_error(val, at)
    form = _form(d, S, I, fast, b3)
    print("%-8s %-5s err %.3e tol %.3e E32 %.3e  top-K %s" % (form, "FAST" if fast else "EXACT", err, tol, e32, what))
    _note(form, fast, err, tol, "top-K " + what)
    assert err <= tol, (what, "err", err, "tol", tol, "E32", e32)
    assert bool((val[:, 1:] <= val[:, :-1]).all()), ("values increase", what)
    outside = keep.clone()
    outside.scatter_(1, li, False)
    best_out = ref64.masked_fill(~outside, -np.inf).max(1).values
    assert bool((best_out <= at.min(1).values + 2 * tol).all()), ("a better item was left out", what, float((best_out - at.min(1).values).max()), tol)


# --------------------------------------------------------------------------- the squared-norm table
@pytest.mark.parametrize("d,S", [(4, 0), (36, 3), (64, 3), (200, 1), (256, 4)])
def test_row_sqnorms_against_float64(d, S):
    """row_sqnorm_kernel on a column window: every block's sum of squares within (d + 4) 2^-24 relative of the float64 sum (the
    bound of a d-term fp32 sum), exact zeros for zero blocks, the 1e-10 block not flushed."""
    c = Case("zero" if S else "benign", 70, 333, d, S, 8, seed=d)
    want = (c.Y.double().reshape(-1, 1 + S, d) ** 2).sum(-1)
    err = (c.sqn.double() - want).abs()
    assert bool((err <= (d + 4) * 2.0 ** -24 * want).all()), float((err / want.clamp_min(1e-300)).max())
    if S:
        assert float(c.sqn[1, 1]) == 0.0 and 0.5e-20 < float(c.sqn[c.U + 3, S]) < 2e-20


# --------------------------------------------------------------------------- score matrix, every form
@pytest.mark.parametrize("d", [4, 48, 200, 256])
def test_generic_scorer_over_recdims_and_heads(d, eval_math):
    fast = eval_math == "fast"
    for S in (0, 1, 3, 4):
        c = Case("benign", 50, 210, d, S, 33, seed=d + S)
        for ptype, fusion in _pairs(S):
            _check_matrix(c, (1 << S) - 1, fusion, ptype, fast)


@pytest.mark.parametrize("d", [32, 64, 128])
def test_t16_scorer_over_recdims_and_heads(d, eval_math):
    fast = eval_math == "fast"
    for S in (1, 2, 3):
        c = Case("benign", 50, 210, d, S, 33, seed=d + S)
        for ptype, fusion in _pairs(S):
            _check_matrix(c, (1 << S) - 1, fusion, ptype, fast)


@pytest.mark.parametrize("d", [64, 48])
def test_user_counts(d, eval_math):
    """One lane group (16 users) short / exact / over, one workgroup (128) exact / over, two workgroups; sqnorm= supplied."""
    fast = eval_math == "fast"
    for B in (1, 15, 16, 17, 128, 129, 200):
        c = Case("benign", 210, 150, d, 3, B, seed=B)
        for ptype, fusion in _pairs(3):
            _check_matrix(c, 0b111, fusion, ptype, fast, sqn=True)


@pytest.mark.parametrize("d", [64, 48])
def test_catalogue_sizes(d, eval_math):
    """Below one tile, one tile, a tail tile, the last shape with one tile per workgroup (512 x 16 items) and the first with two,
    the largest catalogue that is a single chunk."""
    fast = eval_math == "fast"
    for I in (5, 16, 17, 8192, 8207, 16384):
        c = Case("benign", 40, I, d, 3, 33, seed=I)
        for ptype, fusion in _pairs(3):
            _check_matrix(c, 0b111, fusion, ptype, fast)


@pytest.mark.parametrize("I", [16385, 18433, 40000])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_matrix_in_chunks(d, I):
    """A catalogue beyond one chunk (16 384 items): FAST on the bf16 piece planes (recdim 32 / 64) and with the switch off, recdim
    128 (chunks without planes); at 18 433 also EXACT and a workspace WITHOUT room for the planes, where score_topk_impl silently
    takes the fp32 form -- held to the same FAST tolerance either way. 40 000 items at recdim 64 runs 200 users (two user groups)."""
    B = 200 if (d, I) == (64, 40000) else 40
    c = Case("benign", 210, I, d, 3, B, seed=d + I)
    for ptype, fusion in _pairs(3):
        _check_matrix(c, 0b111, fusion, ptype, True, b3=1)
        if d != 128:
            _check_matrix(c, 0b111, fusion, ptype, True, b3=0)
        if I == 18433:
            _check_matrix(c, 0b111, fusion, ptype, False)
            if d != 128:
                _check_matrix(c, 0b111, fusion, ptype, True, b3=1, roomy=False, sqn=True)


@pytest.mark.parametrize("d,I", [(64, 210), (48, 210), (32, 18433)])
def test_head_masks(d, I, eval_math):
    """rubi honours the mask, hm and sum do not: every mask of S = 3 and of S = 1, every fusion, TE and TIE."""
    fast = eval_math == "fast"
    for S, masks in ((3, (0b000, 0b001, 0b010, 0b101, 0b111)), (1, (0b0, 0b1))):
        c = Case("benign", 50, I, d, S, 33, seed=d + S)
        for mask in masks:
            for ptype, fusion in _pairs(S):
                if ptype != "normal":
                    _check_matrix(c, mask, fusion, ptype, fast, sqn=True)


@pytest.mark.parametrize("d,I", [(64, 3000), (48, 3000), (64, 18433), (32, 18433)])
@pytest.mark.parametrize("family", ["saturated", "zero"])
def test_input_families(family, d, I, eval_math):
    """Saturated sigmoids (logits beyond +-88), all-zero head blocks (cosine 0, never NaN) and a head block of norm 1e-10."""
    fast = eval_math == "fast"
    c = Case(family, 50, I, d, 3, 33, seed=d)
    for ptype, fusion in _pairs(3):
        _check_matrix(c, 0b111, fusion, ptype, fast, sqn=(family == "zero"))


@pytest.mark.parametrize("d,S", [(64, 3), (48, 3), (128, 2), (32, 1)])
@pytest.mark.parametrize("I", [37, 300])
def test_small_catalogue_row_mean(I, d, S, eval_math):
    """TIE at a catalogue small enough that a mean over the wrong count (I - 1, a padded tile) moves the scores by hundreds of
    tolerances."""
    fast = eval_math == "fast"
    c = Case("benign", 50, I, d, S, 33, seed=I + d)
    for fusion in ("rubi", "hm", "sum"):
        _check_matrix(c, (1 << S) - 1, fusion, "TIE", fast)


@pytest.mark.parametrize("d", [32, 64, 128])
def test_chunked_forms_over_heads(d, eval_math):
    """The chunked launches at one and two heads (test_matrix_in_chunks holds three): 18 433 items, the score matrix for all 7
    pairs and a top-20 list without a matrix. FAST at recdim 32 / 64: the bf16 piece planes, whose NB = 2 / 3 instances have their
    own LDS window (4 tiles against 3 at NB = 4, recdim 64) and their own norm stride -- and the same calls with the switch off;
    EXACT and recdim 128: score_t16_kernel chunk by chunk."""
    fast = eval_math == "fast"
    for S in (1, 2):
        c = Case("benign", 60, 18433, d, S, 40, seed=d + S)
        for b3 in ((1, 0) if fast and d != 128 else (1,)):
            for ptype, fusion in _pairs(S):
                _check_matrix(c, (1 << S) - 1, fusion, ptype, fast, b3=b3)
            for ptype, fusion in TOPK_PAIRS:
                _check_topk(c, (1 << S) - 1, fusion, ptype, fast, 20, b3=b3)


# --------------------------------------------------------------------------- top-K only
TOPK_PAIRS = [("TIE", "rubi"), ("TIE", "hm"), ("TE", "sum"), ("normal", "rubi")]


@pytest.mark.parametrize("d,I", [(64, 18433), (32, 40000), (128, 18433), (64, 3000), (48, 3000), (48, 18433)])
def test_topk_only(d, I, eval_math):
    """Lists without a score matrix. Recdim 32 / 64 / 128 beyond one chunk: the chunked form (pilot chunk of 2 048, store threshold,
    running list) for K <= 256 -- on the bf16 planes and off -- and the private matrix for K = 300; 3 000 items: the tile-guided
    selection over one launch; recdim 48: the generic scorer with topk_select / topk_kernel."""
    fast = eval_math == "fast"
    c = Case("benign", 60, I, d, 3, 40, seed=d + I)
    for K in (1, 20, 256, 300):
        for ptype, fusion in TOPK_PAIRS:
            _check_topk(c, 0b111, fusion, ptype, fast, K)
            if fast and d in (32, 64) and I > 16384 and K == 20:
                _check_topk(c, 0b111, fusion, ptype, fast, K, b3=0)


# --------------------------------------------------------------------------- item shards
def test_item_shards(eval_math):
    """W = 3 uneven shards, TIE and TE: phase-1 sums against the float64 sum of sigmoid(u.i) over the shard's items (relative
    (I_shard + 4) 2^-24), phase-2 scores against the float64 model of the WHOLE catalogue, list ids offset by id_offset."""
    from elimrec_amd import ops
    fast = eval_math == "fast"
    U, I, d, S, B, K = 90, 7000, 64, 3, 70, 20
    c = Case("benign", U, I, d, S, B, seed=11)
    bounds = [0, 1503, 1503 + 3217, I]
    ui64 = torch.sigmoid(c.a64)
    with _Switches(fast):
        for ptype, fusion in (("TIE", "rubi"), ("TIE", "hm"), ("TE", "rubi")):
            ref64, ref32 = c.refs(0b111, fusion, ptype)
            keep = ~c.tmask
            tol, e32 = sm.tolerance(ref64, ref32, fast, keep)
            shards = []
            total = torch.zeros(B, device=DEV)
            for i0, i1 in zip(bounds[:-1], bounds[1:]):
                n = i1 - i0
                Ysh = torch.cat([c.Y[:U], c.Y[U + i0:U + i1]]).contiguous()
                loc = [[i - i0 for i in x if i0 <= i < i1] for x in c.lists]
                lp = np.zeros(B + 1, np.int64)
                lp[1:] = np.cumsum([len(x) for x in loc])
                li = torch.tensor([i for x in loc for i in x] + [0], dtype=torch.int32, device=DEV)
                ws = torch.empty(ops.score_workspace(B, U, n, S, K), dtype=torch.uint8, device=DEV)
                part = torch.full((B,), NAN, device=DEV)
                ops.score_topk_shard(Ysh, U, n, c.users, d, S, 0b111, fusion, ptype, ws, 1, part, I, i0)
                if ptype == "TIE":
                    want = ui64[:, i0:i1].sum(1)
                    assert bool(((part.double() - want).abs() <= (n + 4) * 2.0 ** -24 * want).all()), ("phase-1 sum", fusion, i0)
                    total += part
                else:
                    assert bool(torch.isnan(part).all())           # a no-op outside TIE
                shards.append((i0, i1, Ysh, torch.from_numpy(lp).to(DEV), li, ws))
            for i0, i1, Ysh, lp, li, ws in shards:
                n = i1 - i0
                outs = []
                for rep in range(2):
                    buf = torch.full((B, n + PAD), NAN, device=DEV)
                    idx = torch.full((B, K), -1, dtype=torch.int32, device=DEV)
                    val = torch.full((B, K), NAN, device=DEV)
                    ops.score_topk_shard(Ysh, U, n, c.users, d, S, 0b111, fusion, ptype, ws, 2, total, I, i0, scores=buf[:, :n], K=K,
                                         topk_idx=idx, topk_val=val, train_ptr=lp, train_items=li)
                    outs.append((buf, idx, val))
                buf, idx, val = outs[0]
                what = c.what(ptype, fusion, "shard", i0, i1)
                assert _bits_equal(buf, outs[1][0]) and torch.equal(idx, outs[1][1]) and _bits_equal(val, outs[1][2]), what
                assert bool(torch.isnan(buf[:, n:]).all()), what
                assert torch.equal(buf[:, :n] == -np.inf, c.tmask[:, i0:i1]), what
                err = sm.worst_error(buf[:, :n], ref64[:, i0:i1], keep[:, i0:i1])
                _note("shard/" + _form(d, S, n, fast, 1), fast, err, tol, what)
                assert err <= tol, (what, err, tol, e32)
                gi = idx.long()
                assert bool(((gi >= i0) & (gi < i1)).all()), ("ids not offset into the shard's range", what)
                assert not bool(c.tmask.gather(1, gi).any()), what
                assert sm.worst_error(val, ref64.gather(1, gi)) <= tol, what
                outside = keep.clone()
                outside.scatter_(1, gi, False)
                outside[:, :i0] = False
                outside[:, i1:] = False
                best_out = ref64.masked_fill(~outside, -np.inf).max(1).values
                assert bool((best_out <= ref64.gather(1, gi).min(1).values + 2 * tol).all()), what


# --------------------------------------------------------------------------- workspace sizing
PLANES_IN_SIZING = (32, 64)      # recdims whose elimrec_score_workspace_for figure holds room for the bf16 piece planes


def test_workspace_for_is_exact():
    """The sizing function and the call share one plan: a workspace of exactly ops.score_workspace(..., d=d) bytes is accepted and
    gives the bits of a workspace 1 MiB larger (lists, and the matrix where one is passed); 256 bytes fewer is refused as too small.
    FAST math only (the bf16x3 gate depends on the size). 18 433 items: the 2 048-item pilot chunk, one full chunk and a 1-item
    tail; K = 300 is beyond the tile-guided selection: the private [B x I] block, scored in chunks.
    The refusal is NOT asserted at recdim 64: there the figure includes the piece planes, which the call treats as optional (without
    them it takes the fp32 form), so a workspace 256 bytes short of it is accepted -- the rule the call has always had."""
    from elimrec_amd import ops
    B, U, S = 5, 7, 3
    g = torch.Generator().manual_seed(7)
    users = torch.tensor([0, 6, 3, 1, 3], device=DEV)
    with _Switches(True):
        for d in (48, 64, 128):
            for I in (300, 18433):
                Y = torch.randn((U + I, (1 + S) * d), generator=g).to(DEV)
                for K in (10, 300):
                    for want_scores in (False, True):
                        def call(nbytes):
                            ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
                            idx = torch.full((B, K), -1, dtype=torch.int32, device=DEV)
                            val = torch.full((B, K), NAN, device=DEV)
                            sc = torch.full((B, I), NAN, device=DEV) if want_scores else None
                            ops.score_topk(Y, U, I, users, d, S, 0b111, "hm", "TIE", ws, scores=sc, K=K, topk_idx=idx, topk_val=val)
                            return idx, val, sc
                        what = "d=%d I=%d K=%d scores=%s" % (d, I, K, want_scores)
                        need = ops.score_workspace(B, U, I, S, K, topk_only=not want_scores, d=d)
                        idx, val, sc = call(need)
                        idx2, val2, sc2 = call(need + (1 << 20))
                        assert torch.equal(idx, idx2) and _bits_equal(val, val2), ("lists differ with a roomier workspace", what)
                        assert bool((idx >= 0).all()) and not bool(torch.isnan(val).any()), what
                        if want_scores:
                            assert _bits_equal(sc, sc2) and not bool(torch.isnan(sc).any()), ("matrix differs with a roomier workspace", what)
                        if d not in PLANES_IN_SIZING:
                            with pytest.raises(RuntimeError, match="workspace too small"):
                                call(need - 256)


# --------------------------------------------------------------------------- candidate lists
@pytest.mark.parametrize("d", [36, 64, 128, 200])
def test_candidate_lists(d, eval_math):
    """score_cand_kernel (register forms of recdim <= 64, <= 128, the generic one), S = 0 .. 3: ragged lists with an empty row, a
    repeated id, ids 0 and I - 1 and a row wider than 64, against the float64 model gathered at the listed ids; -inf behind each
    row's end, the padded out untouched behind `width`; TIE's mean from phase 1 of the shard entry."""
    from elimrec_amd import ops
    fast = eval_math == "fast"
    U, I, B = 40, 300, 24
    for S in (0, 1, 2, 3):
        c = Case("benign", U, I, d, S, B, seed=d + S, train=False)
        rng = np.random.default_rng(d + S)
        lists = [rng.integers(0, I, size=int(n)).tolist() for n in rng.integers(1, 70, size=B)]
        lists[5] = []
        lists[6] = [0, I - 1, 7, 7, 0]
        lists[7] = rng.integers(0, I, size=97).tolist()
        width = max(len(x) for x in lists)
        ptr = torch.from_numpy(np.cumsum([0] + [len(x) for x in lists]).astype(np.int64)).to(DEV)
        flat = torch.tensor([i for x in lists for i in x], dtype=torch.int32, device=DEV)
        col = torch.zeros(B, width, dtype=torch.int64, device=DEV)
        live = torch.zeros(B, width, dtype=torch.bool, device=DEV)
        for b, x in enumerate(lists):
            if x:
                col[b, :len(x)] = torch.tensor(x, device=DEV)
                live[b, :len(x)] = True
        with _Switches(fast):
            for ptype, fusion in _pairs(S):
                mask = (1 << S) - 1
                ref64, ref32 = c.refs(mask, fusion, ptype)
                tol, e32 = sm.tolerance(ref64.gather(1, col), ref32.gather(1, col), fast, live)
                row_sum = None
                if ptype == "TIE":
                    ws = torch.empty(ops.score_workspace(B, U, I, S, 1, d=d), dtype=torch.uint8, device=DEV)
                    row_sum = torch.full((B,), NAN, device=DEV)
                    ops.score_topk_shard(c.Y, U, I, c.users, d, S, mask, fusion, ptype, ws, 1, row_sum, I, 0, sqnorm=c.sqn)
                outs = []
                for rep in range(2):
                    buf = torch.full((B, width + 3), NAN, device=DEV)
                    ops.score_candidates(c.Y, U, I, c.users, d, S, mask, fusion, ptype, ptr, flat, buf[:, :width], sqnorm=c.sqn,
                                         row_sum=row_sum, I_total=I)
                    outs.append(buf)
                what = c.what("candidates", ptype, fusion)
                got = outs[0][:, :width]
                assert _bits_equal(outs[0], outs[1]), what
                assert bool(torch.isnan(outs[0][:, width:]).all()), what
                assert torch.equal(got == -np.inf, ~live), what
                err = sm.worst_error(got, ref64.gather(1, col), live)
                _note("cand", fast, err, tol, what)
                assert err <= tol, (what, err, tol, e32)
