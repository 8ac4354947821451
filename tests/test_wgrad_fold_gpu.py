"""The weight gradients' slab reduce folded into the projection weights' optimizer spans (elimrec_slab_hop_adam_wgrad; csrc/bwd_w.h
reduce_adam_body, csrc/slab.hip sell_tier_adam_fold_kernel).

1. The folded call against the two-step path it replaces -- elimrec_linear_bwd_w_reduce as a call of its own, then
   elimrec_slab_hop_adam with the same tail jobs --, bit for bit on every buffer a job or a problem names (updated weights, both
   moments, the stored gradient, the snapshot copy; the NaN guards around and between the spans included) and on the hop's own
   p / m / v and loss sum. Chunk counts 1, 3, 4, 5, 9: the q / q+4 / q+8 dealing of chunks to an element's four lanes has empty
   lanes, one full round, a ragged second round and a third. Output sizes: 12 x 20 (+ 12: not a multiple of the 64 elements a
   workgroup takes), 4 x 4 (the smallest the contraction accepts; its column sum would be one group of four). A problem with and one
   without a column sum, and a batch of 8 of unequal sizes (an empty range, an accumulating problem, an output no job covers).
   The spans hold more than the problems write -- four elements with a gradient of their own in front of, between and behind the
   outputs --, so the fold has to split them, and a copy-only job rides along.
2. The same cases against float64, in the independent steps and with the tolerances of tests/test_step_tail_gpu.py: the stored
   gradient against the float64 contraction (bw_check: tau(K) |A|^T |B|), the updated p / m / v against float64 Adam fed that stored
   gradient (adam_assert: the bound of that module's docstring, section B).
3. The same folded call twice on the same inputs: identical bytes.
4. The engine on a 200 x 300 synthetic graph at B = 64 with the fold on and off (ELIMREC_FUSE_WGRAD_FOLD): losses, parameters and
   moments bit for bit, issued from Python (5 steps) and through the native one-call program (14 steps, which it must accept).
"""
import numpy as np
import pytest
import torch

from fp64_tools import NAN, same_bits
from test_step_tail_gpu import (B1, B2, EPS, LR, WD, _hop_setup, _nan, adam_assert, adam_inputs, bw_case, bw_check, bw_dims,
                                bw_workspace)

DEV = "cuda:0"
gpu = pytest.mark.gpu

# name -> [(R, n1, n2, colsum, kwargs of bw_case)]
_CHUNKS = {1: 50, 3: 150, 4: 256, 5: 300, 9: 560}
CASES = {"chunks-%d" % c: [(R, 64, 64, "plain", {})] for c, R in _CHUNKS.items()}
CASES["odd-size"] = [(300, 12, 20, "weighted", dict(index="hot"))]
CASES["one-group-no-colsum"] = [(150, 4, 4, None, {})]
CASES["batch-8"] = [(300, 64, 64, "plain", {}), (1000, 4, 36, None, dict(index="perm")), (560, 68, 32, "weighted", dict(index="hot")),
                    (40, 128, 64, "plain", dict(rng=(3, 37))), (700, 64, 68, None, dict(accumulate=True)), (0, 60, 4, "plain", {}),
                    (150, 12, 20, "weighted", dict(index="perm")), (900, 64, 128, "plain", {})]
STEP_A, STEP_B = 3, 1000


def _layout(specs):
    """Element offsets in the flat buffers. Job A: gap, then the first half of the problems each followed by a gap (a gap = 4 elements
    with a gradient of their own); job B: the other problems back to back -- but the LAST problem of a batch lies outside every job;
    job C: 300 copy-only elements. 4 NaN floats between the jobs."""
    n = len(specs)
    in_a = max(1, n // 2)
    off, prob, jobs = 4, [], []
    a0 = off
    off += 4
    for k in range(in_a):
        R, n1, n2, cs, _ = specs[k]
        prob.append((off, off + n1 * n2 if cs else None))
        off += n1 * n2 + (n1 if cs else 0) + 4
    jobs.append(("A", a0, off))
    off += 4
    if n > 1:
        b0 = off
        for k in range(in_a, n):
            R, n1, n2, cs, _ = specs[k]
            if k == n - 1 and n > 2:
                jobs.append(("B", b0, off))
                off += 4
            prob.append((off, off + n1 * n2 if cs else None))
            off += n1 * n2 + (n1 if cs else 0)
        if n == 2:
            jobs.append(("B", b0, off))
        off += 4
    jobs.append(("C", off, off + 300))
    return prob, jobs, off + 300 + 4


class _State(object):
    """The flat buffers, the problems writing into `g`, the tail jobs; fresh for every run, the same bits every time."""

    def __init__(self, name, wd):
        from elimrec_amd import _lib
        specs = CASES[name]
        self.specs, self.wd = specs, wd
        prob, jobs, total = _layout(specs)
        seed = 500 + sorted(CASES).index(name)
        x = adam_inputs(total, seed, "long")
        self.buf = {k: _nan(total) for k in ("p", "g", "m", "v", "out", "copy")}
        for _, lo, hi in jobs:
            for key, t in zip("pgmv", x):
                self.buf[key][lo:hi] = t[lo:hi].to(DEV)
        self.cases, self.problems = [], []
        for k, ((R, n1, n2, cs, kw), (o, co)) in enumerate(zip(specs, prob)):
            c = bw_case(R, n1, n2, colsum=cs, seed=20 + k, **kw)
            c["out"] = self.buf["g"][o:o + n1 * n2].view(n1, n2)
            if not c["accumulate"]:
                c["out"].fill_(NAN)                          # the reduce must write it, not add to it
            c["out0"] = c["out"].clone()
            p = dict(A=c["A"][:, :n1], B=c["B"][:, :n2], out=c["out"], rows=R, accumulate=c["accumulate"])
            if cs:
                c["cs"] = self.buf["g"][co:co + n1]
                if not c["accumulate"]:
                    c["cs"].fill_(NAN)
                c["cs0"] = c["cs"].clone()
                p["colsum"] = c["cs"]
            if cs == "weighted":
                p["colsum_weight"] = c["w"]
            if c["idx"] is not None:
                p["row_index"] = c["idx"]
            if c["rng"] is not None:
                p["rng"] = c["rng"]
            self.cases.append(c)
            self.problems.append(p)
        ptr = lambda key, lo: self.buf[key].data_ptr() + 4 * lo
        self.jobs, self.spans = [], []
        for tag, lo, hi in jobs:
            if tag == "A":          # in place, with the snapshot of the pre-update weights
                self.jobs.append(_lib.AdamJob(ptr("p", lo), ptr("p", lo), ptr("g", lo), ptr("m", lo), ptr("v", lo), ptr("copy", lo), hi - lo, STEP_A))
                self.spans.append((lo, hi, "p", STEP_A))
            elif tag == "B":        # into a second buffer
                self.jobs.append(_lib.AdamJob(ptr("p", lo), ptr("out", lo), ptr("g", lo), ptr("m", lo), ptr("v", lo), None, hi - lo, STEP_B))
                self.spans.append((lo, hi, "out", STEP_B))
            else:
                self.jobs.append(_lib.AdamJob(ptr("p", lo), None, None, None, None, ptr("copy", lo), hi - lo, 0))
        self.before = {k: v.clone() for k, v in self.buf.items()}


def _run(name, wd, fold, hop):
    """One optimizer launch of the case, folded or as the two calls. Returns (state, the hop's p_out / m / v, the loss word)."""
    from elimrec_amd import ops, slab
    plan, x, gs, xin, loss_rows = hop
    st = _State(name, wd)
    h = ops.linear_bwd_w_batched(st.problems, bw_workspace(st.cases), defer_reduce=True)
    p_in, mm, vv = (t.to(DEV).clone() for t in (xin[0], xin[2], xin[3]))
    p_out, loss_out = _nan(p_in.numel()), _nan(3)
    args = (plan, x, None, gs, None, None, 0.5, p_in, p_out, mm, vv, LR, B1, B2, EPS, wd, 7)
    if fold:
        assert 0 <= slab.wgrad_fold_jobs(st.jobs, h) <= 8
        slab.hop_adam(*args, tail_jobs=st.jobs, loss_sum=(loss_rows, loss_out[1:2]), wgrad=h)
    else:
        ops.linear_bwd_w_reduce(h)
        slab.hop_adam(*args, tail_jobs=st.jobs, loss_sum=(loss_rows, loss_out[1:2]))
    torch.cuda.synchronize()
    return st, (p_out, mm, vv), loss_out


@pytest.fixture(scope="module")
def hop():
    plan, x, gs = _hop_setup(300, 23)
    xin = adam_inputs(300 * 64, 77, "step1")
    loss_rows = torch.randn(1500, generator=torch.Generator().manual_seed(3)).to(DEV)
    return plan, x, gs, xin, loss_rows


def test_chunk_counts_of_the_cases():
    """The rows chosen for the lane dealing give the chunk counts the issue names (bw_dims restates the host's decomposition)."""
    assert [bw_dims(R, 64, 64)[:2] for R in _CHUNKS.values()] == [(64, c) for c in _CHUNKS]
    for name, specs in CASES.items():
        prob, jobs, total = _layout(specs)
        spans = sorted([(lo, hi) for _, lo, hi in jobs])
        assert all(a[1] + 4 <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] + 4 == total, name


@gpu
@pytest.mark.parametrize("wd", [0.0, WD])
@pytest.mark.parametrize("name", sorted(CASES))
def test_folded_call_equals_reduce_then_adam_and_float64(name, wd, hop):
    ref, ref_hop, ref_loss = _run(name, wd, False, hop)
    got, got_hop, got_loss = _run(name, wd, True, hop)
    again, again_hop, again_loss = _run(name, wd, True, hop)
    for k in ref.buf:
        assert same_bits(got.buf[k], ref.buf[k]), "%s: buffer '%s' differs from reduce-then-Adam" % (name, k)
        assert same_bits(again.buf[k], got.buf[k]), "%s: buffer '%s' differs between two launches" % (name, k)
    for a, b, c in zip(got_hop, ref_hop, again_hop):
        assert same_bits(a, b) and same_bits(c, a), name + ": the hop's own p / m / v"
    assert same_bits(got_loss, ref_loss) and same_bits(again_loss, got_loss) and not bool(torch.isnan(got_loss[1]))
    # float64: the stored gradient, then Adam on that gradient
    for k, c in enumerate(got.cases):
        bw_check(c, "%s[%d]" % (name, k))
    for lo, hi, dst, step in got.spans:
        inputs = (got.before["p"][lo:hi], got.buf["g"][lo:hi], got.before["m"][lo:hi], got.before["v"][lo:hi])
        assert not bool(torch.isnan(inputs[1]).any()), name + ": a gradient element of a span was not written"
        adam_assert((got.buf[dst][lo:hi], got.buf["m"][lo:hi], got.buf["v"][lo:hi]), inputs, step, wd,
                    "%s span at %d" % (name, lo), "wgrad fold")
        if dst == "p":
            assert same_bits(got.buf["copy"][lo:hi], got.before["p"][lo:hi]), name + ": snapshot"
    # an output outside every job is reduced and stored, nothing else of it is touched
    assert all(same_bits(got.buf[k][:4], got.before[k][:4]) for k in got.buf)


@gpu
def test_fold_is_refused_where_it_does_not_apply(hop):
    """A strided output and an output that straddles the end of a job's gradient range: wgrad_fold_jobs says -1, the launch fails and
    writes nothing."""
    from elimrec_amd import _lib, ops, slab
    plan, x, gs, xin, loss_rows = hop
    for kind in ("strided", "straddle"):
        c = bw_case(150, 64, 64, colsum=None)
        g = _nan(64 * 68 + 8)
        out = g[4:4 + 64 * 68].view(64, 68)[:, :64] if kind == "strided" else g[4:4 + 64 * 64].view(64, 64)
        n_job = 64 * 68 if kind == "strided" else 64 * 64 - 4
        bufs = {k: torch.randn(64 * 68 + 8, device=DEV) for k in "pmv"}
        bufs["v"].abs_()
        keep = {k: v.clone() for k, v in bufs.items()}
        job = _lib.AdamJob(bufs["p"].data_ptr() + 16, bufs["p"].data_ptr() + 16, g.data_ptr() + 16, bufs["m"].data_ptr() + 16,
                           bufs["v"].data_ptr() + 16, None, n_job, 2)
        h = ops.linear_bwd_w_batched([dict(A=c["A"], B=c["B"], out=out, rows=150)], bw_workspace([c]), defer_reduce=True)
        assert slab.wgrad_fold_jobs([job], h) == -1
        p_in, mm, vv = (t.to(DEV).clone() for t in (xin[0], xin[2], xin[3]))
        with pytest.raises(RuntimeError):
            slab.hop_adam(plan, x, None, gs, None, None, 1.0, p_in, p_in, mm, vv, LR, B1, B2, EPS, 0.0, 1, tail_jobs=[job], wgrad=h)
        torch.cuda.synchronize()
        assert all(same_bits(bufs[k], keep[k]) for k in bufs) and same_bits(p_in, xin[0].to(DEV))


@gpu
@pytest.mark.parametrize("native,steps", [("0", 5), ("1", 14)])
def test_engine_steps_with_the_fold_on_and_off(native, steps, monkeypatch):
    """200 users x 300 items, recdim 64, three layers, B = 64: the step with the reduce folded into the Adam hop's launch (the
    adjoint's second hop then a plain one) and with it behind the second hop's tiles -- losses, every parameter and both moments
    bit for bit; issued launch by launch from Python, and as the native one-call program."""
    import os
    from helpers import ROOT
    from elimrec_amd import (ColumnShardEngine, ColumnShardTrainer, Configurator, EliMRec, FusedAdam, PairwiseSamplerV2, SyntheticDataset,
                             set_seed)
    monkeypatch.setenv("ELIMREC_NATIVE_STEP", native)
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        cfg = Configurator(os.path.join(ROOT, "NeuRec.properties"), default_section="hyperparameters",
                           argv=["x", "--data.input.dataset=synthetic", "--alpha=0.5", "--loss=bpr_loss", "--recdim=64", "--layer_num=3",
                                 "--verbose=0"])
    finally:
        os.chdir(cwd)
    ds = SyntheticDataset(200, 300, 3000, feat_dims=(128, 128, 128), seed=0)
    B = 64
    u, p, n = PairwiseSamplerV2(ds, batch_size=B, device=DEV).sample_epoch()
    nb = int(u.numel()) // B
    assert nb >= 2
    batches = [(u[j * B:(j + 1) * B], p[j * B:(j + 1) * B], n[j * B:(j + 1) * B]) for j in range(nb)]
    out = {}
    for fold in ("1", "0"):
        monkeypatch.setenv("ELIMREC_FUSE_WGRAD_FOLD", fold)
        set_seed(1)
        model = EliMRec(cfg, ds).to(DEV)
        opt = FusedAdam(model.parameters(), lr=cfg["lr"], weight_decay=cfg["weight_decay"])
        eng = ColumnShardEngine(model)
        tr = ColumnShardTrainer(eng, opt)
        losses = torch.stack([tr.step(*batches[s % nb]) for s in range(steps)]).cpu().numpy()
        assert eng._fuse_wgrad_fold() == (fold == "1") and eng._fuse_adam() and eng._fuse_bwd_w()
        assert getattr(eng, "_fold_ok", (None, False))[1] == (fold == "1"), "the fold was not taken"
        st = tr._native_state()
        if native == "1":
            assert st["failed"] is None and st["native_steps"] > 0, st
        else:
            assert st["native_steps"] == 0
        eng.sync_to_model()
        os_ = eng.optimizer_state()
        out[fold] = (losses, {k: v.detach().clone() for k, v in model.state_dict().items()}, os_["exp_avg"].clone(), os_["exp_avg_sq"].clone(),
                     opt.export_state(model.named_parameters()))
    assert np.array_equal(out["1"][0], out["0"][0]) and np.isfinite(out["1"][0]).all()
    for k, v in out["0"][1].items():
        assert torch.equal(out["1"][1][k], v), k
    assert torch.equal(out["1"][2], out["0"][2]) and torch.equal(out["1"][3], out["0"][3])
    for k, s0 in out["0"][4].items():
        s1 = out["1"][4][k]
        assert s1["step"] == s0["step"] and torch.equal(s1["exp_avg"], s0["exp_avg"]) and torch.equal(s1["exp_avg_sq"], s0["exp_avg_sq"]), k
