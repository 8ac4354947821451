"""Grouped evaluation on the device: the segmented float64 column means (csrc/eval.hip group_partial_kernel /
group_finish_kernel) against float64 numpy at their edge shapes, their fixed bits and argument checks, and GroupedEvaluator end
to end on the fixtures -- full catalogue, sampled negatives, user slices -- against the inner evaluator's own rows.

Tolerance of every comparison with a float64 mean: 1 float32 ulp of the expected value. A float64 sum of n <= 2^17 non-negative
terms is relatively accurate to n 2^-53 < 2^-36, far inside half a float32 ulp, so the rounded result is the nearest float32 of
the exact mean or its neighbour; no measured number is involved."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import build_model_from_fixture, csr_dict, load_golden, sub

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VIEW = [1, 3, 5]
SIZES = {"ml3": [25, 30], "kwai": [16, 19]}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _assert_1ulp(got, want, what=""):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    assert (err <= ulp).all(), (what, float((err / ulp).max()))


def _lengths():
    from elimrec_amd import ops
    chunk = ops.GROUP_MEAN_CHUNK
    return [1, 63, 64, 65, chunk - 1, chunk, chunk + 1, 2 * chunk + 3]


def _segments(lens, n_rows, rng):
    """Row lists of the given lengths over rows [0, n_rows - 10) -- the last ten rows are in no segment -- with the first row of
    segment 0 listed again by the next non-empty segment."""
    segs = [rng.integers(0, n_rows - 10, size=n).astype(np.int32) for n in lens]
    full = [s for s in segs if s.size]
    if len(full) > 1:
        full[1][-1] = full[0][0]
    return segs


def _csr(segs):
    ptr = np.zeros(len(segs) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in segs], out=ptr[1:])
    return ptr, np.concatenate(segs).astype(np.int32) if ptr[-1] else np.zeros(0, np.int32)


def _want(block, segs):
    b64 = block.astype(np.float64)
    return np.stack([b64[s].mean(0).astype(np.float32) if s.size else np.zeros(block.shape[1], np.float32) for s in segs])


def _means(block_dev, segs, workspace=None):
    from elimrec_amd import ops
    ptr, rows = _csr(segs)
    out = torch.full((len(segs), block_dev.shape[1]), 7.0, device=DEV)
    ops.group_metric_means(block_dev, ptr, rows, out, workspace=workspace)
    return out.cpu().numpy()


@pytest.mark.parametrize("C", [1, 3, 30, 63, 64, 65, 2048])
def test_group_means_against_float64(C):
    """Random rows in [0, 1], the block a column slice (ld = C + 5) of a wider one. G = 1: every segment length on its own;
    G = 2: the lengths in pairs, and an empty segment beside a full one; G = 64: every length eight times, one segment empty."""
    rng = np.random.default_rng(C)
    n_rows = 1500
    wide = rng.random((n_rows, C + 5), dtype=np.float32)
    block = wide[:, 2:2 + C]
    block_dev = _t(wide)[:, 2:2 + C]
    assert block_dev.stride(0) == C + 5
    lens = _lengths()
    cases = [[n] for n in lens] + [lens[i:i + 2] for i in range(0, len(lens), 2)] + [[0, lens[6]], [lens[3], 0]]
    many = (lens * 8)[:64]
    many[5] = 0
    cases.append(many)
    assert sorted(set(len(c) for c in cases)) == [1, 2, 64]
    for case in cases:
        segs = _segments(case, n_rows, rng)
        got = _means(block_dev, segs)
        _assert_1ulp(got, _want(block, segs), (C, case[:4]))
        for g, s in enumerate(segs):
            if not s.size:
                assert not got[g].any()


def test_group_means_accumulate_in_float64():
    """One segment of 65 537 rows: column 0 = 1.0 followed by 2^16 values of 2^-25, column 1 = 0.5 throughout. The exact mean of
    column 0 is (1 + 2^-9) / 65 537; a float32 running sum stays at 1.0 and misses it by 2e-3 relative."""
    n = 65537
    block = np.empty((n, 2), dtype=np.float32)
    block[:, 0] = 2.0 ** -25
    block[0, 0] = 1.0
    block[:, 1] = 0.5
    segs = [np.arange(n, dtype=np.int32)]
    got = _means(_t(block), segs)
    want = np.asarray([[(1.0 + 2.0 ** -9) / n, 0.5]], dtype=np.float64).astype(np.float32)
    assert np.array_equal(_want(block, segs), want)                  # (numpy's float64 mean is exact here too)
    assert abs(np.float32(1.0 / n) - want[0, 0]) > 1e-3 * want[0, 0]    # what a float32 accumulator would give
    _assert_1ulp(got, want)


def test_group_means_have_fixed_bits():
    """The same call twice; a group alone (G = 1) against its row of the 64-group call; a workspace full of NaN bytes."""
    from elimrec_amd import _lib
    rng = np.random.default_rng(3)
    n_rows, C = 1500, 65
    block_dev = _t(rng.random((n_rows, C), dtype=np.float32))
    lens = (_lengths() * 8)[:64]
    segs = _segments(lens, n_rows, rng)
    first = _means(block_dev, segs)
    assert np.array_equal(first, _means(block_dev, segs))
    for g in (7, 62):                                                 # 2 chunk + 3 rows (three chunks); chunk + 1 rows
        assert len(segs[g]) in (lens[7], lens[6])
        assert np.array_equal(_means(block_dev, [segs[g]])[0], first[g])
    need = int(_lib.load().elimrec_group_metric_means_workspace(sum(lens), C, 64))
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    assert np.array_equal(_means(block_dev, segs, workspace=ws), first)


def test_group_means_argument_checks():
    """C = 0, C = 2049, a too-small workspace and a null output are the library's errors; an index outside the block is
    refused on the host, before any launch."""
    from elimrec_amd import _lib, ops
    lib = _lib.load()
    n_rows, C = 40, 8
    block = torch.rand(n_rows, 2049, device=DEV)
    ptr, rows = _t(np.asarray([0, 3], np.int64)), _t(np.asarray([0, 1, 2], np.int32))
    out = torch.zeros(1, 2049, device=DEV)
    ws = torch.empty(int(lib.elimrec_group_metric_means_workspace(3, 2049, 1)), dtype=torch.uint8, device=DEV)
    assert ws.numel() == 2049 * 8

    def call(C, out_ptr=out.data_ptr(), ws_bytes=ws.numel()):
        rc = lib.elimrec_group_metric_means(block.data_ptr(), n_rows, C, block.stride(0), ptr.data_ptr(), rows.data_ptr(), 3, 1,
                                            out_ptr, ws.data_ptr(), ws_bytes, None)
        _lib.check(rc, "group_metric_means")

    call(C)
    torch.cuda.synchronize()
    _assert_1ulp(out[0, :C].cpu().numpy(), block[:3, :C].double().mean(0).float().cpu().numpy())
    for bad_c in (0, 2049):
        with pytest.raises(RuntimeError, match="1 <= C <= 2048"):
            call(bad_c)
    with pytest.raises(RuntimeError, match="workspace too small"):
        call(C, ws_bytes=C * 8 - 1)
    with pytest.raises(RuntimeError, match="null pointer"):
        call(C, out_ptr=None)
    with pytest.raises(RuntimeError, match="ld < C"):
        lib_rc = lib.elimrec_group_metric_means(block.data_ptr(), n_rows, C, C - 1, ptr.data_ptr(), rows.data_ptr(), 3, 1,
                                                out.data_ptr(), ws.data_ptr(), ws.numel(), None)
        _lib.check(lib_rc, "group_metric_means")
    small = block[:, :C]
    res = torch.zeros(1, C, device=DEV)
    for bad_rows in ([0, 1, n_rows], [0, -1, 2]):
        with pytest.raises(IndexError):
            ops.group_metric_means(small, [0, 3], bad_rows, res)
        with pytest.raises(IndexError):                               # device tensors are copied back and checked as well
            ops.group_metric_means(small, ptr, _t(np.asarray(bad_rows, np.int32)), res)
    with pytest.raises(IndexError):                                   # an index checked for a taller block
        ops.group_metric_means(small[:10], ops.GroupIndex([0, 1], [39], n_rows, DEV), None, res)
    assert not res.any()
    # the torch.ops registration: the same numbers, the same host-side check
    from elimrec_amd import torch_ops
    t = torch_ops.load()
    assert torch.equal(t.group_metric_means(small, ptr, rows), ops.group_metric_means(small, ptr, rows, res))
    with pytest.raises(RuntimeError, match="the block has 40 rows"):
        t.group_metric_means(small, ptr, _t(np.asarray([0, 1, n_rows], np.int32)))


# --------------------------------------------------------------------------- GroupedEvaluator on the fixtures
def _load_cache(model, g):
    """The reference's cached tables after the fixture's parameters, as the evaluator's scoring table."""
    ws = model._workspace(8)
    c = sub(g, "cache")
    U, d = model.num_users, model.latent_dim
    Y = ws["Y"]
    Y[:U, :d] = _t(c["all_users"])
    Y[U:, :d] = _t(c["all_items"])
    for h, m in enumerate(model._mods):
        Y[:U, (h + 1) * d:(h + 2) * d] = _t(c["pre_fusion_user_" + m])
        Y[U:, (h + 1) * d:(h + 2) * d] = _t(c["pre_fusion_item_" + m])
    model._publish_cache(Y)


def _check_grouped(model, grouped, plain, name):
    """grouped: a GroupedEvaluator; plain: a UniEvaluator built from the same arguments without group_view."""
    inner = grouped.evaluator
    assert grouped.group_sizes == SIZES[name] and grouped.num_discarded == 15
    assert grouped.group_labels == ["(1,3]:".ljust(12), "(3,5]:".ljust(12)]
    users = inner.default_users()
    final, buf = grouped.evaluate(model)
    assert final.dtype == np.float32 and final.shape == (2, inner.metrics_num * len(inner.top_show))
    assert buf == grouped.format_groups(final) and buf.count("\n") == 2
    rows = inner.metric_rows(model, users).cpu().numpy().astype(np.float64)
    for g, label in enumerate(grouped.group_labels):
        members = grouped.grouped_user[label]
        at = [users.index(u) for u in members]
        assert len(at) == grouped.group_sizes[g]
        want = rows[at].mean(0).reshape(inner.metrics_num, inner.max_top)[:, inner.top_show - 1].reshape(-1)
        _assert_1ulp(final[g], want.astype(np.float32), (name, label))
        # the reference's way -- one evaluator pass over the group's users, a float32 row-by-row mean: n - 1 additions, each
        # within 2^-24 relative of a partial sum that never exceeds the total, and the division
        per_group, _ = inner.evaluate(model, members)
        bound = (len(members) - 1) * 2.0 ** -24 * want + 2.0 ** -24
        assert (np.abs(final[g].astype(np.float64) - per_group.astype(np.float64)) <= bound).all(), (name, label)
    overall, overall_buf, group_final, group_buf = grouped.evaluate_with_overall(model)
    want_final, want_buf = plain.evaluate(model)
    assert np.array_equal(overall, want_final) and overall.dtype == want_final.dtype and overall_buf == want_buf
    assert np.array_equal(group_final, final) and group_buf == buf
    return final, buf


@pytest.mark.parametrize("tie_order", ["reference", "id"])
@pytest.mark.parametrize("name", ["ml3", "kwai"])
def test_grouped_evaluation_end_to_end(name, tie_order):
    from elimrec_amd.evaluator import GroupedEvaluator
    g = load_golden(name)
    model, _ = build_model_from_fixture(g, DEV, extra_argv=["--group_view=[1,3,5]", "--tie_order=" + tie_order])
    plain, _ = build_model_from_fixture(g, DEV, extra_argv=["--tie_order=" + tie_order])
    for m in (model, plain):
        _load_cache(m, g)
    grouped = model.test_evaluator.evaluator
    assert isinstance(grouped, GroupedEvaluator) and grouped.evaluator.tie_order == tie_order
    final, buf = _check_grouped(model, grouped, plain.test_evaluator.evaluator, name)
    facade_final, facade_buf = model.test_evaluator.evaluate(model)
    assert np.array_equal(facade_final, final) and facade_buf == buf
    got = model.test_with_overall()
    want = plain.test()
    assert np.array_equal(got[0], want[0]) and got[1] == want[1] and np.array_equal(got[2], final)
    assert plain.test_with_overall()[2:] == (None, None)


def _sampled_evaluators(name, n_neg, top_k, tie_order):
    """GroupedEvaluator and UniEvaluator over the fixture's test users with n_neg sampled negatives each (outside the user's
    train, valid and test items)."""
    from elimrec_amd.evaluator import GroupedEvaluator, UniEvaluator
    g = load_golden(name)
    model, _ = build_model_from_fixture(g, DEV)
    _load_cache(model, g)
    train, test, valid = csr_dict(g, "train"), csr_dict(g, "test"), csr_dict(g, "valid")
    rng = np.random.default_rng(7)
    neg = {}
    for u in range(model.num_users):
        seen = set(train.get(u, [])) | set(test.get(u, [])) | set(valid.get(u, []))
        neg[u] = sorted(rng.choice(sorted(set(range(model.num_items)) - seen), size=n_neg, replace=False).tolist())
    metric = ["Precision", "Recall", "MAP", "NDCG", "MRR"]
    grouped = GroupedEvaluator(None, train, test, neg, metric=metric, group_view=list(VIEW), top_k=top_k)
    plain = UniEvaluator(None, train, test, neg, metric=metric, top_k=top_k)
    grouped.tie_order = plain.tie_order = tie_order
    return model, grouped, plain


@pytest.mark.parametrize("tie_order", ["reference", "id"])
def test_grouped_evaluation_of_sampled_candidates(tie_order):
    """user_neg_test given: 12 negatives per user, K up to 12 <= neg + 1."""
    model, grouped, plain = _sampled_evaluators("ml3", 12, [1, 5, 12], tie_order)
    assert grouped.evaluator.user_neg_test is not None and grouped.evaluator.tie_order == tie_order
    _check_grouped(model, grouped, plain, "ml3")


def test_grouped_evaluation_of_sliced_users():
    """The inner rows computed as the slices shard = (0, 2) and (1, 2) and summed by hand (what the all-reduce of a two-rank
    job does) give the unsliced result bit for bit -- full catalogue and sampled candidates."""
    from elimrec_amd.evaluator import GroupedEvaluator
    g = load_golden("kwai")
    model, _ = build_model_from_fixture(g, DEV)
    _load_cache(model, g)
    full = GroupedEvaluator(None, csr_dict(g, "train"), csr_dict(g, "test"), group_view=list(VIEW), top_k=[5, 10])
    sampled_model, sampled, _ = _sampled_evaluators("kwai", 12, [5, 10], "reference")
    for m, grouped in ((model, full), (sampled_model, sampled)):
        inner = grouped.evaluator
        users = inner.default_users()
        final, buf = grouped.evaluate(m)
        halves = [inner.metric_rows(m, users, shard=(r, 2), reduce=False) for r in range(2)]
        n = len(users)
        assert not halves[0][n // 2:].any() and not halves[1][:n // 2].any()
        got_final, got_buf = grouped.evaluate_rows(halves[0] + halves[1])
        assert np.array_equal(got_final, final) and got_buf == buf
