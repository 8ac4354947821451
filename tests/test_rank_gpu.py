"""Exact catalogue ranks on the device (csrc/rank.hip) against the numpy model of tests/rank_model.py.

The count is an integer: ops.rank_targets is compared with int32 EQUALITY against the definition evaluated on the block copied back,
at the segment and targets-per-pass edges (placed from ops.RANK_SEGMENT / ops.RANK_TARGETS_PER_PASS), on padded rows whose
padding holds +inf (reading a padding column shows up as a wrong count). The row kernels compute in double and round once, as the
model does: rank and hit@K are exact, rr / pct / auc / mrr_full are allowed one float32 ulp (the two double values can only straddle
a rounding boundary). Group means: the bound of tests/test_group_eval_gpu.py, one float32 ulp of the float64 mean."""
import os

import numpy as np
import pytest
import torch

import rank_model as rm
from helpers import ROOT, build_model_from_fixture, csr_dict, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 5
FAMILIES = ("normal", "equal", "few", "masked", "zeros")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _edges():
    from elimrec_amd import ops
    return ops.RANK_SEGMENT, ops.RANK_TARGETS_PER_PASS


def _scores(family, I, rng):
    if family == "normal":
        x = rng.standard_normal((B, I))
    elif family == "equal":
        x = np.full((B, I), 0.25)
    elif family == "few":
        x = rng.integers(0, 3, size=(B, I)) * 0.5 - 0.5
    elif family == "masked":
        x = rng.standard_normal((B, I))
        x[:, rng.permutation(I)[:(I + 2) // 3]] = -np.inf           # a third of the items (at least one), every row
    else:
        x = np.where(rng.integers(0, 2, size=(B, I)) == 1, -0.0, 0.0)
    return x.astype(np.float32)


def _lists(I, P, rng, shift):
    """B = 5 lists with lengths out of {0, 1, P - 1, P, P + 1, 3 P + 2} (capped at what I allows, ids repeat), rotated by `shift`
    so that every length is met; row 1 is always the empty list between two non-empty ones."""
    lens = [1, P - 1, P, P + 1, 3 * P + 2]
    lens = lens[shift % 5:] + lens[:shift % 5]
    lens = [lens[0], 0, lens[1], lens[2], lens[3 + shift % 2]]
    out = []
    for n in lens:
        n = min(n, 3 * I + 2)
        ids = rng.integers(0, I, size=n)
        if n >= 2:
            ids[-1] = ids[0]                                          # a repeated target
        out.append(ids.tolist())
    assert len(out[0]) and not out[1] and len(out[2])
    return out


def _i_values():
    SEG, _ = _edges()
    return [1, 3, 4, 5, SEG - 1, SEG, SEG + 1, 2 * SEG + 7]


@pytest.mark.parametrize("family", FAMILIES)
def test_count_is_exact(family):
    from elimrec_amd import ops
    SEG, P = _edges()
    rng = np.random.default_rng(FAMILIES.index(family))
    case = 0
    for I in _i_values():
        for pad in (0, 12):
            lds = (I + 3) // 4 * 4 + pad
            host = np.full((B, lds), np.inf, dtype=np.float32)        # +inf in every padding column
            host[:, :I] = _scores(family, I, rng)
            lists = _lists(I, P, rng, case)
            case += 1
            if family == "masked":
                lists[0][0] = int(np.flatnonzero(host[0, :I] == -np.inf)[0])      # a masked item among the targets
            ptr, items = rm.csr(lists)
            want = rm.ranks(host[:, :I], ptr, items)
            assert (family == "masked") == bool((want == -1).any())
            block = _t(host)[:, :I]
            n = len(items)
            out = torch.full((n + 9,), 7, dtype=torch.int32, device=DEV)
            ops.rank_targets(block, ptr, items, out)
            first = out.cpu().numpy()
            assert (first[n:] == 7).all(), (family, I, lds)           # nothing behind the last pair is touched
            assert np.array_equal(first[:n], want), (family, I, lds, np.flatnonzero(first[:n] != want)[:8])
            index = ops.TargetIndex(ptr, items, B, I, DEV)
            again = torch.full((n + 9,), 7, dtype=torch.int32, device=DEV)
            ops.rank_targets(block, index, None, again)
            assert torch.equal(again, out), (family, I, lds)          # the same counts whatever order the adds arrive in
            assert torch.equal(block.cpu(), torch.from_numpy(host[:, :I]))
    assert case >= 10                                                 # every rotation of the list lengths was met twice


def test_count_on_rows_that_take_the_unaligned_form():
    """A row stride that is no multiple of 4 floats (and a base off the 16-byte grid) cannot take the 16-byte loads."""
    from elimrec_amd import ops
    SEG, P = _edges()
    rng = np.random.default_rng(11)
    I, lds = SEG + 6, SEG + 9
    flat = torch.full((B * lds + 1,), float("inf"), dtype=torch.float32, device=DEV)
    block = flat[1:].view(B, lds)[:, :I]
    host = rng.integers(0, 4, size=(B, I)).astype(np.float32)
    block.copy_(_t(host))
    ptr, items = rm.csr(_lists(I, P, rng, 3))
    out = torch.empty(len(items), dtype=torch.int32, device=DEV)
    ops.rank_targets(block, ptr, items, out)
    assert np.array_equal(out.cpu().numpy(), rm.ranks(host, ptr, items))


def test_rank_targets_argument_checks():
    from elimrec_amd import ops
    block = torch.zeros(2, 8, device=DEV)
    out = torch.empty(4, dtype=torch.int32, device=DEV)
    with pytest.raises(IndexError):
        ops.rank_targets(block, [0, 1, 2], [0, 8], out)
    with pytest.raises(ValueError):
        ops.rank_targets(block, [0, 2, 1], [0, 1], out)
    with pytest.raises(ValueError):
        ops.rank_targets(block, [0, 3, 5], [0, 1, 2, 3, 4], out)     # out too short
    with pytest.raises(IndexError):
        ops.rank_targets(block, ops.TargetIndex([0, 1], [0], 1, 8, DEV), None, out)      # built for another block
    with pytest.raises(TypeError):
        ops.rank_targets(block, [0, 1, 2], [0, 1], out.float())
    assert ops.rank_targets(block, [0, 0, 0], [], out) is out        # nothing listed: nothing launched


def test_torch_op_equals_the_ctypes_binding():
    from elimrec_amd import ops, torch_ops
    SEG, P = _edges()
    rng = np.random.default_rng(5)
    I = SEG + 5
    host = _scores("masked", I, rng)
    ptr, items = rm.csr(_lists(I, P, rng, 4))
    block = _t(host)
    out = torch.empty(len(items), dtype=torch.int32, device=DEV)
    ops.rank_targets(block, ptr, items, out)
    got = torch_ops.load().rank_targets(block, _t(ptr), _t(items))
    assert got.dtype == torch.int32 and torch.equal(got, out)
    assert np.array_equal(got.cpu().numpy(), rm.ranks(host, ptr, items))
    with pytest.raises(RuntimeError):
        torch_ops.load().rank_targets(block, _t(ptr), _t(np.full_like(items, I)))


# --------------------------------------------------------------------------- the row kernels
def _assert_1ulp(got, want64, what):
    """got float32 against the model's float64: NaN exactly where the model has it, elsewhere within one float32 ulp."""
    got = np.asarray(got)
    assert got.dtype == np.float32
    nan = np.isnan(want64)
    assert np.array_equal(np.isnan(got), nan), what
    want32 = want64.astype(np.float32)
    err = np.abs(got[~nan].astype(np.float64) - want32[~nan].astype(np.float64))
    assert (err <= np.spacing(np.abs(want32[~nan])).astype(np.float64)).all(), what


def test_pair_rows_against_float64():
    from elimrec_amd import ops
    rng = np.random.default_rng(3)
    n = 1000                                                          # four workgroups of 256, the last one partial
    rank = rng.integers(0, 100000, size=n).astype(np.int32)
    rank[:40] = np.arange(40)
    rank[rng.permutation(n)[:50]] = -1
    n_cand = (rank.astype(np.int64) + rng.integers(1, 5000, size=n)).clip(1, None).astype(np.int32)
    n_cand[5], rank[5] = 1, 0                                         # a single candidate: pct = 0
    for ks in ([10], [1, 5, 20, 50], []):
        out = torch.full((n, 3 + len(ks)), -3.0, device=DEV)
        ops.rank_pair_rows(_t(rank), _t(n_cand), ks, out)
        got, want = out.cpu().numpy(), rm.pair_rows(rank, n_cand, ks)
        _assert_1ulp(got, want, ks)
        ok = rank >= 0
        assert np.array_equal(got[ok][:, 0], want[ok][:, 0]) and np.array_equal(got[ok][:, 3:], want[ok][:, 3:])      # exact columns
        assert np.isnan(got[~ok]).all() and got[5, 2] == 0.0
    with pytest.raises(ValueError):
        ops.rank_pair_rows(_t(rank), _t(n_cand), [10], torch.empty(n, 3, device=DEV))


def test_user_rows_against_float64():
    from elimrec_amd import ops
    rng = np.random.default_rng(4)
    lens = [0, 1, 2, 63, 64, 65, 200, 1, 3, 5]                        # around the wave's 64 targets per step; 10 users = 3 workgroups
    lists = []
    for n in lens:
        r = rng.integers(0, 5000, size=n)
        if n >= 3:
            r[1] = r[0]                                               # equal ranks (a repeated target)
            r[2] = -1                                                 # a masked target among valid ones
        lists.append(r.tolist())
    lists[7] = [-1]                                                   # no valid target
    ptr, rank = rm.csr(lists)
    n_cand = np.asarray([6000] * 10, dtype=np.int32)
    n_cand[8] = 2                                                     # user 8 has 2 valid targets: no negative is left
    out = torch.full((10, 3), -3.0, device=DEV)
    ops.rank_user_rows(_t(rank), _t(ptr), _t(n_cand), out)
    got, want = out.cpu().numpy(), rm.user_rows(rank, ptr, n_cand)
    assert np.isnan(want[[0, 7, 8]]).all() and not np.isnan(want[[1, 2, 3, 4, 5, 6, 9]]).any()
    _assert_1ulp(got, want, "user rows")
    ok = ~np.isnan(want[:, 2])
    assert np.array_equal(got[ok, 2], want[ok, 2])                    # first_rank is exact


# --------------------------------------------------------------------------- the model on the fixtures
def _masked_predict(model, users, train):
    block = model.predict(users).numpy().copy()
    for b, u in enumerate(users):
        block[b, train.get(u, [])] = -np.inf
    return block


@pytest.mark.parametrize("name", ["ml3", "kwai"])
def test_rank_items_on_a_fixture(name):
    from elimrec_amd import ops
    g = load_golden(name)
    model, _ = build_model_from_fixture(g, DEV)
    model.bpr_loss(_t(g["step1/users"]), _t(g["step1/pos"]), _t(g["step1/neg"]))
    train, test = csr_dict(g, "train"), csr_dict(g, "test")
    users = [u for u in test if test[u]][:40]
    lists = [test[u] for u in users]
    ptr, items = rm.csr(lists)
    width = max(len(x) for x in lists)
    for ptype in ("TE", "TIE"):
        model.predict_type = ptype
        block = _masked_predict(model, users, train)
        want = rm.ranks(block, ptr, items)
        got = model.rank_items(users, lists, exclude=train)
        assert got.dtype == torch.int32 and got.device.type == "cpu" and got.shape == (len(users), width)
        for b, x in enumerate(lists):
            assert got[b, :len(x)].tolist() == want[ptr[b]:ptr[b + 1]].tolist(), (name, ptype, b)
            assert bool((got[b, len(x):] == -1).all())
        # the lists of the same call: rank < K exactly for the listed targets, at the listed position
        tptr, titems = rm.csr([train.get(u, []) for u in users])
        index = ops.TargetIndex(ptr, items, len(users), model.num_items, DEV)
        rank, idx, val = model.rank_items_device(users, index, _t(tptr), _t(titems), top_k=10)
        rank, idx = rank.cpu().numpy(), idx.cpu().numpy()
        assert np.array_equal(rank, want) and val.shape == idx.shape == (len(users), 10)
        for b in range(len(users)):
            top = idx[b].tolist()
            for p in range(int(ptr[b]), int(ptr[b + 1])):
                t = int(items[p])
                assert (rank[p] < 10 and rank[p] >= 0) == (t in top), (name, ptype, b, t)
                if t in top:
                    assert top.index(t) == rank[p], (name, ptype, b, t)
        r0, i0, v0 = model.rank_items_device(users, index, _t(tptr), _t(titems))
        assert i0 is None and v0 is None and np.array_equal(r0.cpu().numpy(), want)
    assert model.rank_items([], []).shape == (0, 0)


# --------------------------------------------------------------------------- the report and the driver's switch
def _net(tmp_path, extra, shape="[60,200,1200]"):
    import importlib
    import sys
    sys.path.insert(0, ROOT)
    main = importlib.import_module("main")
    from elimrec_amd import Configurator, set_seed
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        args = Configurator(os.path.join(ROOT, "NeuRec.properties"), default_section="hyperparameters",
                            argv=["main.py", "--data.input.dataset=synthetic", "--alpha=0.5", "--synthetic_shape=" + shape,
                                  "--synthetic_dims=[16,8,12]", "--recdim=32", "--loss=bpr_loss", "--batch_size=512", "--num_epoch=2",
                                  "--test_step=1", "--verbose=0", "--save_flag=0", "--path=%s" % str(tmp_path / "ck")] + list(extra))
        set_seed(args["seed"])
        return main.Net(args)
    finally:
        os.chdir(cwd)


def _run(net):
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        net.run()
    finally:
        os.chdir(cwd)


def _mean_1ulp(got, rows64, what):
    want = rows64.astype(np.float32).astype(np.float64).mean(0)
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)).all(), (what, got, want)


def test_rank_report_on_a_synthetic_data_set(tmp_path):
    from elimrec_amd.evaluator import CandidateScoringError, RankReport
    net = _net(tmp_path, [], shape="[200,120,900]")                  # users with 1 .. 6 training items: every group of the view is met
    rec = net.recommender
    _run(net)
    train, test = net.dataset.get_user_train_dict(), net.dataset.get_user_test_dict()
    ks = [5, 20]
    report = RankReport(net.dataset, train, test, ks, group_view=[1, 3, 5], item_group_view=[1, 4])
    lds = (rec.num_items + 3) // 4 * 4
    report.block_bytes = (len(report.users) + 1) // 2 * lds * 4      # two user blocks
    assert -(-len(report.users) // report.block_users) == 2
    rec.predict_type = "TIE"
    ranks = report.pair_ranks(rec)
    assert ranks.dtype == torch.int32 and ranks.shape == (report.num_pairs,) and ranks.device.type == "cuda"
    block = _masked_predict(rec, report.users, train)
    want = rm.ranks(block, report.pair_ptr, report.pair_items)
    assert np.array_equal(ranks.cpu().numpy(), want) and (want >= 0).all()
    final, buf = report.evaluate(rec)
    pair64 = rm.pair_rows(want, report.pair_n_cand, ks)
    user64 = rm.user_rows(want, report.pair_ptr, report.user_n_cand)
    assert not np.isnan(pair64).any() and not np.isnan(user64).any()
    assert final.pair_columns == ("rank", "rr", "pct", "hit@5", "hit@20") and final.user_columns == ("auc", "mrr_full", "first_rank")
    assert final.pairs.dtype == np.float32 and final.pairs.shape == (len(report.pair_labels), 5)
    assert final.users.dtype == np.float32 and final.users.shape == (len(report.user_labels), 3)
    assert len(report.user_labels) == 4 and sum(x.startswith("item ") for x in report.pair_labels) >= 2
    for g, at in enumerate(report._pair_pos):
        _mean_1ulp(final.pairs[g], pair64[at], report.pair_labels[g])
    for g, at in enumerate(report._user_pos):
        _mean_1ulp(final.users[g], user64[at], report.user_labels[g])
    lines = buf.split("\n")
    assert len(lines) == 2 + len(report.pair_labels) + len(report.user_labels)
    assert lines[0].startswith("columns:") and "hit@20" in lines[0] and lines[1].startswith("all:")
    assert [ln[:12] for ln in lines[1:1 + len(report.pair_labels)]] == [x[:12] for x in report.pair_labels]
    assert lines[1 + len(report.pair_labels)].startswith("columns:") and "auc" in lines[1 + len(report.pair_labels)]
    # a shift against itself is nothing; against TE it is the model's difference, row 0 by hand
    same, _ = report.shift(ranks, ranks)
    assert same.pair_columns == ("delta", "improved", "worsened") and same.users is None and not same.pairs.any()
    rec.predict_type = "TE"
    te = report.pair_ranks(rec)
    moved, sbuf = report.shift(te, ranks)
    a, b = te.cpu().numpy().astype(np.int64), want.astype(np.int64)
    rows = np.stack([a - b, b < a, b > a], axis=1).astype(np.float64)
    for g, at in enumerate(report._pair_pos):
        w = rows[at].mean(0)
        assert (np.abs(moved.pairs[g] - w) <= np.spacing(np.abs(w).astype(np.float32))).all(), report.pair_labels[g]
    assert sbuf.split("\n")[0].startswith("columns:") and len(sbuf.split("\n")) == 1 + len(report.pair_labels)
    rec._eval_shard = object()
    try:
        with pytest.raises(CandidateScoringError):
            report.pair_ranks(rec)
    finally:
        rec._eval_shard = None


class _Capture(object):
    def __init__(self):
        self.lines = []

    def log(self, *msg):
        self.lines.append("\t".join(str(m) for m in msg))


def _test_lines(tmp_path, extra):
    """The lines Net.test_all_effects() logs after a two-epoch synthetic run."""
    from elimrec_amd import Logger
    net = _net(tmp_path, extra)
    before = Logger.logger
    try:
        _run(net)
        cap = Logger.logger = _Capture()
        cwd = os.getcwd()
        os.chdir(ROOT)
        try:
            net.test_all_effects()
        finally:
            os.chdir(cwd)
    finally:
        Logger.logger = before
    return cap.lines


def test_driver_switch(tmp_path):
    """--rank_report=1 logs the rank tables under both effects and the TE->TIE shift table; the [TEST] metric lines are those of a
    run that never had the switch, and --rank_report=0 logs nothing else."""
    absent = _test_lines(tmp_path / "a", [])
    assert len(absent) == 2 and absent[0].startswith("  [TE]\t") and absent[1].startswith("  [TIE]\t")
    assert _test_lines(tmp_path / "b", ["--rank_report=0"]) == absent
    on = _test_lines(tmp_path / "c", ["--rank_report=1", "--group_view=[10,30]", "--item_group_view=[1,4]"])
    assert [ln for ln in on if ln.startswith("  [TE]\t") or ln.startswith("  [TIE]\t")] == absent
    tables = [ln for ln in on if "catalogue rank of the test items" in ln]
    assert len(tables) == 2 and tables[0].startswith("  [TE] ") and tables[1].startswith("  [TIE] ")
    assert all(t.count("columns:") == 2 and "\nall:" in t and "\n(0,10]:" in t and "\nitem " in t and "auc" in t for t in tables)
    shift = [ln for ln in on if ln.startswith("  [TE->TIE] rank shift")]
    assert len(shift) == 1 and "delta" in shift[0] and "\nall:" in shift[0] and on.index(shift[0]) > on.index(tables[1])
