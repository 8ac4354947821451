"""The dense forward projection (linear_fwd_kernel of csrc/gemm.hip: elimrec_linear_fwd, elimrec_linear_fwd_batched) against the
float64 model of tests/linear_model.py, element by element, at its tile edges: 64 x 64 tiles, wave w on rows 32 (w & 1) and columns
32 (w >> 1), K staged 16 at a time. The contract, the criterion (fp64_tools.assert_close, K_eff = K + 2, scale = |A||W|^T +
|rowscale||bias| + |add|; under relu the same bound and +0.0 bit for bit wherever ref < -bound), the poison and the shapes are
described there; tests/test_linear_model_cpu.py shows without a GPU that the criterion rejects the defects these cases look for and
that the shapes reach the branches they are meant for.

Conventions (those of tests/test_step_tail_gpu.py): every output buffer starts as NaN and everything the contract does not name
must still hold the same NaN bits afterwards; whatever a call must not read holds NaN; no case holds an out-of-bounds index or
pointer; inputs are unchanged bit for bit; a second launch gives the same bits; comparisons are element-wise.

A. plain form through ops.linear_fwd; B. the descriptor's optional fields through ops.linear_fwd_batched with one problem; C. several
problems per launch, both pipeline depths; D. refusals; E. one layer of elimrec_amd.MLP, both directions. ops.linear_fwd_batched
cannot pass `act`, and torch gives an empty tensor no address, so the relu forms of B and C and every M == 0 problem go through the
same entry point with descriptors filled in here (`_raw`).

Two bit pins go beyond the header's wording, because the project relies on them (test_batch_row_head_equals_full_tables,
materialize_tables of shard.py: the tables of a batch-row step and the tables built over all rows must be the same numbers): row m of
the gathered form (row_index, compact C) equals row row_index[m] of the full form over all rows, and the rows of a row_range call
equal the same rows of the unrestricted call -- a row's chain of additions may not depend on which tile row it lands in. Likewise
each problem of a batch equals that problem called alone, and the rows two launches on either side of the depth threshold share
are the same bits (the register pipeline's depth moves loads, not additions).

Unreachable through the current host code and not tested: the persistent multi-tile walk (wg_budget = 1 << 30) and the <128, 1> and
<64, 4> instantiations.
"""
import pytest
import torch

import linear_model as lm
from fp64_tools import NAN, same_bits, tau, TINY, within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORST = {}          # family -> worst err / tol seen in this session (printed by the last test)
BADARG = r"rc=10001"


def _ops():
    from elimrec_amd import ops
    return ops


def _up(t):
    return None if t is None else t.to(DEV)


def _dev(c):
    """The inputs of a case on the device (the whole poisoned buffers)."""
    d = {k: _up(c[k]) for k in ("A", "W", "bias", "rowscale", "add", "idx")}
    d["rng"] = None if c["rng"] is None else torch.tensor(list(c["rng"]), dtype=torch.int32, device=DEV)
    return d


def _views(c, d, out):
    """(A, W, bias, out, rowscale, add, row_index, row_range) as ops.linear_fwd_batched takes them: the windows of the buffers."""
    N, K, o = c["N"], c["K"], c["add_off"]
    return (d["A"][:, :K], d["W"][:N, :K], d["bias"], out[:c["M"], c["c_off"]:c["c_off"] + N], d["rowscale"],
            None if d["add"] is None else d["add"][:, o:o + N], d["idx"], d["rng"])


def _ptr(t, col=0):
    return None if t is None else t.data_ptr() + 4 * col


def _desc(c, d, out, act=None):
    from elimrec_amd import _lib
    return _lib.LinearDesc(_ptr(d["A"]), d["A"].stride(0), _ptr(d["W"]), d["W"].stride(0), _ptr(d["bias"]), _ptr(out, c["c_off"]),
                           out.stride(0), c["M"], c["N"], c["K"], _ptr(d["rowscale"]), _ptr(d["add"], c["add_off"]),
                           0 if d["add"] is None else d["add"].stride(0), _ptr(d["idx"]), _ptr(d["rng"]),
                           c["act"] if act is None else act)


def _raw(descs):
    """elimrec_linear_fwd_batched on descriptors filled in here."""
    from elimrec_amd import _lib
    arr = (_lib.LinearDesc * max(len(descs), 1))(*descs)
    _lib.check(_lib.load().elimrec_linear_fwd_batched(arr, len(descs), _ops()._stream()), "linear_fwd_batched")


def _launch(cases, devs, outs, how):
    ops = _ops()
    if how == "plain":
        (c,), (d,), (out,) = cases, devs, outs
        a, w, b, o = _views(c, d, out)[:4]
        ops.linear_fwd(a, w, b, o, act="relu" if c["act"] else None)
    elif how == "batched":
        ops.linear_fwd_batched([_views(c, d, o) for c, d, o in zip(cases, devs, outs)])
    else:
        _raw([_desc(c, d, o) for c, d, o in zip(cases, devs, outs)])
    torch.cuda.synchronize()


def _how(cases):
    return "batched" if all(c["act"] == 0 and c["M"] > 0 for c in cases) else "raw"


def _fresh(cases, share):
    outs = []
    for i, c in enumerate(cases):
        outs.append(outs[share[i]] if i in share else c["C0"].to(DEV))
    return outs


def _once(cases, how=None, share=None):
    """One launch on NaN outputs: the output buffers, on the host."""
    devs = [_dev(c) for c in cases]
    outs = _fresh(cases, share or {})
    _launch(cases, devs, outs, how or _how(cases))
    return [o.cpu() for o in outs]


def _go(cases, what, family, how=None, share=None):
    """Launch, check every problem against float64 and its padding and inputs against what they were; twice, same bits. share:
    {problem: the earlier problem whose output buffer it writes into}. Returns the host output buffers."""
    share = share or {}
    how = how or _how(cases)
    devs = [_dev(c) for c in cases]
    keep = [{k: (None if v is None else v.clone()) for k, v in d.items()} for d in devs]
    runs = []
    for rep in range(2):
        outs = _fresh(cases, share)
        _launch(cases, devs, outs, how)
        runs.append([o.cpu() for o in outs])
    for i, c in enumerate(cases):
        mates = [j for j in range(len(cases)) if j != i and (share.get(j, j) == share.get(i, i))]
        elsewhere = None
        for j in mates:
            elsewhere = lm.written(cases[j]) if elsewhere is None else (elsewhere | lm.written(cases[j]))
        r = lm.check(c, runs[0][i], "%s[%d]" % (what, i), elsewhere=elsewhere)
        WORST[family] = max(WORST.get(family, 0.0), r)
        assert same_bits(runs[0][i], runs[1][i]), "%s[%d]: second launch differs" % (what, i)
        for k, v in devs[i].items():
            assert v is None or same_bits(v, keep[i][k]), "%s[%d]: input %s changed" % (what, i, k)
    return runs[0]


def _rows_equal(c, buf, rows, other, other_rows, what):
    """The window of `buf` at `rows` is bit for bit the window of `other` at `other_rows`."""
    w = slice(c["c_off"], c["c_off"] + c["N"])
    a, b = buf[rows, w], other[other_rows, w]
    assert bool(torch.isfinite(a).all()), what
    assert same_bits(a, b), "%s: %d elements differ in their bits" % (what, int((a.view(torch.int32) != b.view(torch.int32)).sum()))


# ============================================================================= A. plain form, one problem
@pytest.mark.parametrize("j", range(len(lm.plain_triples())))
def test_plain_form_is_inside_the_bound_at_every_tile_edge(j):
    """M, N on and beside the wave and tile edges, K with G = 1 .. 128 stages and partial last chunks, padded lda / ldw, the output
    a column window at an odd offset of a buffer with an odd ldc; with and without bias, with and without relu."""
    for bias in (True, False):
        for act in (0, 1):
            c = lm.plain_case(j, bias, act)
            assert lm.form_of([c])["depth"] == 8
            _go([c], "plain %s bias=%d act=%d" % (lm.plain_triples()[j], bias, act), "plain", how="plain")


def test_plain_form_with_no_rows_writes_nothing():
    from elimrec_amd import _lib
    c = lm.case(0, 33, 20, seed=1)
    d, out = _dev(c), c["C0"].to(DEV)
    lib = _lib.load()
    _lib.check(lib.elimrec_linear_fwd(_ptr(d["A"]), d["A"].stride(0), _ptr(d["W"]), d["W"].stride(0), _ptr(d["bias"]), _ptr(out),
                                      out.stride(0), 0, c["N"], c["K"], _ops()._stream()), "linear_fwd")
    torch.cuda.synchronize()
    assert lm.check(c, out.cpu(), "M == 0") == 0.0


# ============================================================================= B. the descriptor's fields
@pytest.mark.parametrize("name", list(lm.FIELD_CASES))
def test_descriptor_fields_are_inside_the_bound(name):
    """rowscale (mixed signs, an exact zero; without a bias it has no effect), add as a window of a wider table, row_index as a
    permutation / a hot list / longer than A, every row_range of the list (clamped at either end, empty twice), all four together
    as _fold_problems of model.py builds them, and its compact form."""
    c = lm.field_case(name)
    assert lm.form_of([c])["depth"] == 8
    out = _go([c], name, "descriptor fields")[0]
    if len(c["rows"]) == 0:
        assert same_bits(out, c["C0"])


def test_rowscale_without_a_bias_has_no_effect():
    c = lm.field_case("rowscale, no bias")
    with_rs = _once([c])[0]
    without = _once([dict(c, rowscale=None)])[0]
    assert same_bits(with_rs, without)


@pytest.mark.parametrize("name", ["index perm", "index hot", "index tall", "all four", "all four, relu",
                                  "all four, inner range, relu", "all four, hot"])
def test_gathered_rows_are_the_bits_of_the_full_form(name):
    """Row m of the gathered form equals bit for bit row row_index[m] of the same problem over all rows of A (beyond the header's
    wording; see the module docstring). The rows of A nothing names are NaN in both and are not compared."""
    c = lm.field_case(name)
    ra = c["A"].shape[0]
    full = dict(c, M=ra, idx=None, rng=None, rows=torch.arange(ra), C0=torch.full((ra, c["C0"].shape[1]), NAN))
    got, ref = _once([c])[0], _once([full])[0]
    _rows_equal(c, got, c["rows"], ref, lm.source_rows(c), name)


@pytest.mark.parametrize("name", ["range %d %d" % r for r in lm.RANGES[1:6]] + ["compact", "compact, relu"])
def test_ranged_rows_are_the_bits_of_the_unrestricted_call(name):
    """The rows a row_range call produces equal bit for bit the same rows of the call without a range: the tiles start at the
    range's begin, so a row sits in another tile row, and that may not change its sum."""
    c = lm.field_case(name)
    got, ref = _once([c])[0], _once([dict(c, rng=None)])[0]
    _rows_equal(c, got, c["rows"], ref, c["rows"], name)


# ============================================================================= C. several problems per launch
@pytest.mark.parametrize("n", [2, 3, 5, 8])
def test_batch_of_different_shapes(n):
    """A different (M, N, K) each, so the workgroups of the smaller problems leave early; from five on an M == 0 problem, an empty
    range and N = 130 beside N = 5; the fields and relu mixed. And each problem's output is the bits of that problem alone."""
    cases = lm.batch_cases(n)
    outs = _go(cases, "batch of %d" % n, "batched")
    for i, c in enumerate(cases):
        alone = _once([c])[0]
        assert same_bits(outs[i], alone), "batch of %d: problem %d differs from the same problem called alone" % (n, i)


def test_batch_of_empty_problems_writes_nothing():
    cases = [lm.case(0, N, K, seed=6000 + i) for i, (N, K) in enumerate([(5, 4), (64, 16), (130, 132)])]
    assert lm.form_of(cases)["depth"] is None
    outs = _go(cases, "all M == 0", "batched")
    assert all(same_bits(o, c["C0"]) for o, c in zip(outs, cases))


@pytest.mark.parametrize("n_lo", [0, 1, 63, 64, 65, 150])
def test_two_problems_write_disjoint_row_ranges_of_one_window(n_lo):
    """The fused head of _fwd_head (model.py): rows (0, n_lo) from one side's weights and bias, rows (n_lo, n) from the other's,
    into the same output window."""
    a, b = lm.split_cases(n_lo)
    assert len(a["rows"]) == n_lo and len(b["rows"]) == 150 - n_lo
    out = _go([a, b], "split at %d" % n_lo, "batched", share={1: 0})[0]
    assert bool(torch.isfinite(out[:, a["c_off"]:a["c_off"] + a["N"]]).all())


@pytest.mark.parametrize("which", ["one problem", "eight problems"])
def test_both_pipeline_depths_at_the_threshold(which):
    """768 workgroups run the 8-deep register pipeline, one tile row more the 1-deep one: each against float64, the rows they share
    bit for bit."""
    lo, hi = lm.threshold_single() if which == "one problem" else lm.threshold_batch()
    assert (lm.form_of(lo)["wgs"], lm.form_of(lo)["depth"]) == (768, 8) and lm.form_of(hi)["depth"] == 1
    assert lm.form_of(hi)["wgs"] == (769 if which == "one problem" else 792)
    out_lo = _go(lo, which + ", depth 8", "batched")
    out_hi = _go(hi, which + ", depth 1", "batched")
    shared = torch.arange(lo[0]["M"])
    _rows_equal(lo[0], out_lo[0], shared, out_hi[0], shared, which)
    for i in range(1, len(lo)):
        assert same_bits(out_lo[i], out_hi[i]), "%s: problem %d differs between the depths" % (which, i)


@pytest.mark.parametrize("K", lm.WIDE_KS)
def test_depth_one_at_short_and_long_pipelines(K):
    """780 workgroups by way of a wide N: the 1-deep form at G = 1, 9 and 128 stages."""
    c = lm.case(lm.WIDE_M, lm.WIDE_N, K, seed=5000)
    f = lm.form_of([c])
    assert f["depth"] == 1 and f["G"] == [-(-K // 16)]
    _go([c], "wide K=%d" % K, "batched")


# ============================================================================= D. refusals
def _refused(call, outs):
    keep = [o.clone() for o in outs]
    with pytest.raises(RuntimeError, match=BADARG):
        call()
    torch.cuda.synchronize()
    assert all(same_bits(o, k) and bool(torch.isnan(o).all()) for o, k in zip(outs, keep))


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def _plain_buffers(M=33, N=5, K=20, a_cols=None, w_cols=None):
    """Buffers allocated for the documented contract: a launch would stay inside them."""
    return torch.randn(M, a_cols or K, device=DEV), torch.randn(N, w_cols or K, device=DEV), torch.randn(N, device=DEV), _nan(M, N)


@pytest.mark.parametrize("what", ["K", "lda", "ldw", "A alignment", "W alignment"])
def test_refuses_what_the_float4_loads_cannot_take(what):
    ops = _ops()
    K = 18 if what == "K" else 20
    cols = {"K": 20, "lda": 21, "ldw": 21, "A alignment": 24, "W alignment": 24}[what]
    A, W, b, out = _plain_buffers(a_cols=cols if what in ("K", "lda", "A alignment") else None,
                                  w_cols=cols if what in ("K", "ldw", "W alignment") else None)
    a = A[:, 1:1 + K] if what == "A alignment" else A[:, :K]
    w = W[:, 1:1 + K] if what == "W alignment" else W[:, :K]
    if what.endswith("alignment"):
        assert a.stride(0) % 4 == 0 and w.stride(0) % 4 == 0 and (a.data_ptr() % 16 != 0 or w.data_ptr() % 16 != 0)
    _refused(lambda: ops.linear_fwd(a, w, b, out), [out])
    _refused(lambda: ops.linear_fwd_batched([(a, w, b, out)]), [out])
    # as the second problem of a batch it refuses the whole launch
    A2, W2, b2, out2 = _plain_buffers()
    _refused(lambda: ops.linear_fwd_batched([(A2, W2, b2, out2), (a, w, b, out)]), [out, out2])


def test_refuses_no_problem_and_nine_problems():
    ops = _ops()
    sets = [_plain_buffers() for _ in range(9)]
    outs = [s[3] for s in sets]
    _refused(lambda: ops.linear_fwd_batched([]), outs)
    _refused(lambda: ops.linear_fwd_batched(sets), outs)
    ops.linear_fwd_batched(sets[:8])                                   # eight are taken
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(o).all()) for o in outs[:8]) and bool(torch.isnan(outs[8]).all())


@pytest.mark.parametrize("what", ["N == 0", "act == 2"])
def test_refuses_an_empty_width_and_an_unknown_activation(what):
    """Through descriptors filled in here: the wrapper never passes act = 2, and an N == 0 tensor has no address."""
    c = lm.case(33, 5, 20, seed=2)
    d, out = _dev(c), c["C0"].to(DEV)
    desc = _desc(c, d, out, act=2 if what == "act == 2" else 0)
    if what == "N == 0":
        desc.N = 0
    _refused(lambda: _raw([desc]), [out])
    good_c = lm.case(33, 5, 20, seed=3)
    good_d, good_out = _dev(good_c), good_c["C0"].to(DEV)
    _refused(lambda: _raw([_desc(good_c, good_d, good_out), desc]), [out, good_out])


# ============================================================================= E. one MLP layer
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", lm.MLP_SHAPES)
def test_one_mlp_layer_forward_and_backward(shape, relu):
    """elimrec_amd.mlp's Linear (zero-padded to multiples of 4 where needed) against float64 autograd: y with the forward bound,
    dX with tau(n_out + 2) |g||W|, dW and db with the contraction bound tau(rows) |g|^T |x|. The inputs leave the relu mask
    unambiguous (tests/test_linear_model_cpu.py), so nothing is masked out of the comparison."""
    from elimrec_amd.mlp import MLP, _LinearFn
    m = lm.mlp_case(*shape)
    ref = lm.mlp_reference(m, relu)
    x, w, b = [m[k].to(DEV).requires_grad_(True) for k in ("x", "w", "b")]
    y = _LinearFn.apply(x, w, b, relu)
    y.backward(m["gy"].to(DEV))
    torch.cuda.synchronize()
    for name, got in (("y", y), ("dx", x.grad), ("dw", w.grad), ("db", b.grad)):
        want, scale, K = ref[name]
        assert got.shape == want.shape, name
        ok = within(got, want, scale, K)
        err, tol = (got.detach().double().cpu() - want).abs(), tau(K) * scale + TINY
        WORST["MLP"] = max(WORST.get("MLP", 0.0), float((err / tol).max()))
        assert bool(ok.all()), "MLP %s relu=%d %s: %d of %d outside the bound, worst err / tol %.3f" % (
            shape, relu, name, int((~ok).sum()), ok.numel(), float((err / tol).max()))
    if relu:
        _, scale, K = ref["y"]
        dead = ref["pre"] < -(tau(K) * scale + TINY)
        assert bool((y.detach().cpu().view(torch.int32)[dead] == 0).all())
    else:                                                             # the public class with one layer is the same launch
        net = MLP(shape[0], [shape[1]]).to(DEV)
        with torch.no_grad():
            net.linears[0].weight.copy_(w)
            net.linears[0].bias.copy_(b)
        assert same_bits(net(x.detach()).detach(), y.detach())
    for k, t in (("x", x), ("w", w), ("b", b)):
        assert same_bits(t.detach().cpu(), m[k]), "input %s changed" % k


def test_zz_report_the_worst_ratios():
    """Prints the worst err / tol per family of this session (pytest -s shows it; the figures of the commit message)."""
    print("\nworst err / tol: " + ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))
    assert all(v <= 1.0 for v in WORST.values())
