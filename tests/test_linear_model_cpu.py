"""The float64 model, the criterion and the branch helper of tests/linear_model.py, checked without a GPU and without a project
kernel, on the very inputs tests/test_linear_fwd_gpu.py uses:

1. the criterion accepts fp32 arithmetic of the formula: torch's float32 CPU product, and a second summation order (16-wide K
   chunks added one after the other, as the kernel stages them); the worst error / bound is printed;
2. the criterion rejects mutants, each on at least one element: a float4 group of k dropped (K = 64 and K = 2048), two output
   rows swapped, bias not multiplied by rowscale, add / rowscale taken from row m instead of row row_index[m], the range end off by
   one in both directions, relu omitted, operands rounded to bf16;
3. the shapes reach the branches they are meant for (fwd_form), the threshold at exactly 768 and 769 workgroups included;
4. the MLP inputs leave the relu mask unambiguous: no float64 pre-activation lies within 4 bounds of zero.
"""
import pytest
import torch

import linear_model as lm
from fp64_tools import TINY, tau, within


# ============================================================================= the cases of the GPU file
def _gpu_cases():
    for j in range(len(lm.plain_triples())):
        for bias in (True, False):
            for act in (0, 1):
                yield "plain %d bias=%d act=%d" % (j, bias, act), lm.plain_case(j, bias, act)
    for name in lm.FIELD_CASES:
        yield "fields: " + name, lm.field_case(name)
    for n in (2, 3, 5, 8):
        for i, c in enumerate(lm.batch_cases(n)):
            yield "batch of %d [%d]" % (n, i), c
    for n_lo in (0, 1, 63, 64, 65, 150):
        for i, c in enumerate(lm.split_cases(n_lo)):
            yield "split at %d [%d]" % (n_lo, i), c
    for pair in (lm.threshold_single(), lm.threshold_batch()):
        for k, cases in enumerate(pair):
            for i, c in enumerate(cases):
                yield "threshold side %d [%d]" % (k, i), c
    for K in lm.WIDE_KS:
        yield "wide K=%d" % K, lm.case(lm.WIDE_M, lm.WIDE_N, K, seed=5000)


def _f32(c, chunked=False):
    """The formula in float32 torch on the CPU, in the kernel's epilogue order: product + rowscale * bias + add, then relu."""
    a, w, b, rs, ad = lm.operands(c)
    if chunked:
        acc = torch.zeros(a.shape[0], w.shape[0])
        for k0 in range(0, c["K"], lm.KCHUNK):
            acc = acc + a[:, k0:k0 + lm.KCHUNK] @ w[:, k0:k0 + lm.KCHUNK].T
    else:
        acc = a @ w.T
    if b is not None:
        acc = acc + (b[None, :] if rs is None else rs[:, None] * b[None, :])
    if ad is not None:
        acc = acc + ad
    assert acc.dtype == torch.float32
    return acc.clamp_min(0.0) if c["act"] == 1 else acc


def test_criterion_accepts_fp32_arithmetic_in_two_summation_orders():
    worst = {"torch": 0.0, "chunks of 16": 0.0}
    count = 0
    for what, c in _gpu_cases():
        ref = lm.reference(c)
        for order, chunked in (("torch", False), ("chunks of 16", True)):
            worst[order] = max(worst[order], lm.check(c, lm.place(c, _f32(c, chunked)), what + ", " + order, ref=ref))
        count += 1
    print("\nfp32 emulation over %d cases: worst error / bound " % count + ", ".join("%s %.3f" % kv for kv in sorted(worst.items())))
    assert max(worst.values()) < 1.0


def test_the_poison_is_where_the_conventions_put_it():
    for what, c in _gpu_cases():
        N, K, named = c["N"], c["K"], c["named"]
        other = torch.ones(c["A"].shape[0], dtype=torch.bool)
        other[named] = False
        assert bool(torch.isnan(c["C0"]).all()), what
        assert bool(torch.isnan(c["A"][:, K:]).all()) and bool(torch.isnan(c["W"][:, K:]).all()), what
        assert bool(torch.isnan(c["A"][other]).all()) and bool(torch.isfinite(c["A"][named, :K]).all()), what
        if c["idx"] is not None:
            inside = torch.zeros(c["M"], dtype=torch.bool)
            inside[c["rows"]] = True
            assert bool((c["idx"][~inside] == c["A"].shape[0] - 1).all()) and bool(torch.isnan(c["A"][-1]).all()), what
            assert int(c["idx"].min()) >= 0 and int(c["idx"].max()) < c["A"].shape[0], what
        if c["rowscale"] is not None:
            assert bool(torch.isnan(c["rowscale"][other]).all()), what
            if len(named):
                z = c["rowscale"][named]
                assert bool((z == 0).any()) and (len(named) < 12 or (bool((z < 0).any()) and bool((z > 0).any()))), what
        if c["add"] is not None:
            o = c["add_off"]
            assert c["add"].shape[1] > N and bool(torch.isnan(c["add"][other]).all()), what
            assert bool(torch.isnan(c["add"][:, :o]).all()) and bool(torch.isnan(c["add"][:, o + N:]).all()), what
        for t in lm.operands(c):
            assert t is None or bool(torch.isfinite(t).all()), what
    hot = lm.field_case("index hot")
    assert float((hot["idx"] == 3).float().mean()) > 0.6
    tall = lm.field_case("index tall")
    assert tall["M"] > tall["A"].shape[0]
    perm = lm.field_case("index perm")
    assert perm["A"].shape[0] > perm["M"] and len(perm["idx"].unique()) == perm["M"]


# ============================================================================= mutants
def _mutant(c, relu=None, **over):
    """The formula in float64 with some operands replaced (keys a, w, b, rs, ad; poison read as zero)."""
    a, w, b, rs, ad = [over.get(k, t) for k, t in zip(("a", "w", "b", "rs", "ad"), lm.operands(c))]
    a, w, b, rs, ad = [None if t is None else torch.nan_to_num(t.double(), nan=0.0) for t in (a, w, b, rs, ad)]
    v = a @ w.T
    if b is not None:
        v = v + (b[None, :] if rs is None else rs[:, None] * b[None, :])
    if ad is not None:
        v = v + ad
    return v.clamp_min(0.0) if (c["act"] == 1 if relu is None else relu) else v


def _rejected(c, values=None, buf=None):
    """check() raises on the mutant; a mutant given as values lies outside the bound on at least one element."""
    if buf is None:
        buf = lm.place(c, values)
        _, want, scale = lm.reference(c)
        assert not bool(within(values.float(), want, scale, c["K"] + 2.0).all()), "no element of the mutant is outside the bound"
    with pytest.raises(AssertionError):
        lm.check(c, buf, "mutant")
    return True


def test_the_unmutated_float64_formula_passes():
    for name in ("all four, relu", "compact", "range 64 128", "index tall"):
        c = lm.field_case(name)
        assert lm.check(c, lm.place(c, _mutant(c)), name) < 0.05


@pytest.mark.parametrize("M,N,K", [(65, 65, 64), (33, 33, 2048)])
def test_mutant_one_float4_group_of_k_dropped(M, N, K):
    c = lm.case(M, N, K, seed=77)
    for k0 in (0, K // 2, K - 4):
        a = lm.operands(c)[0].clone()
        a[:, k0:k0 + 4] = 0.0
        assert _rejected(c, _mutant(c, a=a))
        a = lm.operands(c)[0].clone()
        a[M // 2, k0:k0 + 4] = 0.0                                  # in one row only
        assert _rejected(c, _mutant(c, a=a))


def test_mutant_two_output_rows_swapped():
    c = lm.field_case("all four")
    v = _mutant(c)
    v[[63, 64]] = v[[64, 63]]
    assert _rejected(c, v)


def test_mutant_bias_not_multiplied_by_rowscale():
    for name in ("rowscale", "all four, relu", "compact"):
        c = lm.field_case(name)
        assert _rejected(c, _mutant(c, rs=torch.ones(len(c["rows"]))))
    c = lm.field_case("rowscale, no bias")                             # and without a bias the rowscale has no effect
    assert lm.check(c, lm.place(c, _mutant(c, rs=torch.ones(len(c["rows"])))), "no bias") < 0.05


def test_mutant_add_or_rowscale_taken_from_row_m():
    for name in ("all four", "all four, relu", "all four, inner range, relu"):
        c = lm.field_case(name)
        rows, o = c["rows"], c["add_off"]
        assert _rejected(c, _mutant(c, ad=c["add"][rows, o:o + c["N"]]))
        assert _rejected(c, _mutant(c, rs=c["rowscale"][rows]))


def test_mutant_range_end_off_by_one():
    c = lm.field_case("range 64 128")
    good = lm.place(c, _mutant(c))
    short = good.clone()
    short[127] = c["C0"][127]                                          # the last row left as it was
    assert _rejected(c, buf=short)
    wide = good.clone()
    wide[128, c["c_off"]:c["c_off"] + c["N"]] = 0.5                    # one row written beyond the end
    assert _rejected(c, buf=wide)
    early = good.clone()
    early[63, c["c_off"]:c["c_off"] + c["N"]] = 0.5                    # and one before the begin
    assert _rejected(c, buf=early)
    beside = good.clone()
    beside[100, c["c_off"] + c["N"]] = 0.0                             # a column behind N inside ldc
    assert _rejected(c, buf=beside)
    for name in ("range 40 40", "range 50 20"):
        e = lm.field_case(name)
        assert len(e["rows"]) == 0 and lm.check(e, e["C0"].clone(), name) == 0.0
        touched = e["C0"].clone()
        touched[40, e["c_off"]] = 0.0
        assert _rejected(e, buf=touched)


def test_mutant_relu_omitted_and_negative_zero():
    c = lm.field_case("all four, relu")
    assert _rejected(c, _mutant(c, relu=False))
    v = _mutant(c)
    pre, _, scale = lm.reference(c)
    dead = (pre < -lm.bound(c, scale)).nonzero()[0]
    v = v.float()
    v[dead[0], dead[1]] = -0.0                                         # inside the bound, but not +0.0 bit for bit
    with pytest.raises(AssertionError):
        lm.check(c, lm.place(c, v), "negative zero")


def test_mutant_operands_rounded_to_bf16():
    c = lm.case(65, 65, 64, seed=78)
    a, w = lm.operands(c)[:2]
    assert _rejected(c, _mutant(c, a=a.bfloat16().float(), w=w.bfloat16().float()))


# ============================================================================= branches
def test_fwd_form_reaches_the_intended_branches():
    assert [lm.fwd_form([(1, 1, K)])["G"][0] for K in lm.KS] == lm.KS_G
    tr = lm.plain_triples()
    assert 30 <= len(tr) <= 34 and all(t in tr for t in lm.EXTREMES)
    for vals, col in ((lm.MS, 0), (lm.NS, 1), (lm.KS, 2)):
        assert all(sum(1 for t in tr if t[col] == v) >= 2 for v in vals), col
    layouts = [lm.plain_layout(j) for j in range(len(tr))]
    for key, vals in (("lda_pad", (0, 4, 24)), ("ldw_pad", (0, 8)), ("c_off", (0, 3, 8)), ("c_pad", (0, 5))):
        assert {l[key] for l in layouts} == set(vals)
    # everything small runs the 8-deep pipeline
    for j in range(len(tr)):
        assert lm.form_of([lm.plain_case(j, True, 0)])["depth"] == 8
    assert lm.form_of([lm.field_case("all four")]) == dict(tiles_m=4, tiles_n=2, wgs=8, depth=8, G=[3])
    for n in (2, 3, 5, 8):
        cs = lm.batch_cases(n)
        f = lm.form_of(cs)
        assert f["depth"] == 8 and len({(c["M"], c["N"], c["K"]) for c in cs}) == n
        if n >= 5:
            assert any(c["M"] == 0 for c in cs) and any(c["M"] > 0 and len(c["rows"]) == 0 for c in cs)
            assert {5, 130} <= {c["N"] for c in cs} and f["tiles_n"] == 3
    assert lm.fwd_form([(0, 5, 4), (0, 64, 16)])["depth"] is None
    # the threshold, from both sides
    lo, hi = lm.threshold_single()
    assert (lm.form_of(lo)["wgs"], lm.form_of(lo)["depth"]) == (768, 8) and (lm.form_of(hi)["wgs"], lm.form_of(hi)["depth"]) == (769, 1)
    lo, hi = lm.threshold_batch()
    assert len(lo) == len(hi) == 8
    assert (lm.form_of(lo)["wgs"], lm.form_of(lo)["depth"]) == (768, 8) and (lm.form_of(hi)["wgs"], lm.form_of(hi)["depth"]) == (792, 1)
    # depth 1 at G = 1, 9, 128
    forms = [lm.fwd_form([(lm.WIDE_M, lm.WIDE_N, K)]) for K in lm.WIDE_KS]
    assert [f["depth"] for f in forms] == [1, 1, 1] and [f["G"][0] for f in forms] == [1, 9, 128] and forms[0]["wgs"] == 780
    # the ranges cut M = 200 where the issue says: clamped at both ends, and empty twice
    assert [lm.clamp_range(r, lm.FM) for r in lm.RANGES] == [(0, 200), (17, 200), (64, 128), (70, 71), (150, 200), (0, 10), (0, 0), (0, 0)]


# ============================================================================= the MLP inputs
def test_mlp_inputs_leave_the_relu_mask_unambiguous():
    """A condition on the inputs: on the float64 reference no pre-activation lies within 4 bounds of zero, so `out > 0` of a
    kernel inside the bound is the reference's mask on every element and nothing needs masking out of the comparison."""
    assert {s[0] for s in lm.MLP_SHAPES} == {10, 24, 100} and {s[1] for s in lm.MLP_SHAPES} == {6, 16, 64}
    assert {s[2] for s in lm.MLP_SHAPES} == {37, 130}
    for shape in lm.MLP_SHAPES:
        m = lm.mlp_case(*shape)
        r = lm.mlp_reference(m, True)
        _, scale, K = r["y"]
        assert bool((r["pre"].abs() > 4.0 * (tau(K) * scale + TINY)).all()), shape
