"""Audience lists on the device (csrc/audience.hip) against the float64 model of tests/audience_model.py.

Every (item, slot) of every case goes through audience_model.check_lists: rules 1-4 with the tolerance of score_model.tolerance
(from the float64 / float32 models, never from the code under test). Tables come from score_model.make_table; the shapes sit at
the kernel's edges (ops.AUDIENCE_TILE / ops.AUDIENCE_CHUNK, K = 64 / 65, d = 32 / 64 / 20). For TIE the row_sum handed to the kernel
is the scorer's pass 1 (ops.score_topk_shard phase 1), and the model's mean is that row_sum / I: the test isolates the new kernel."""
import os

import numpy as np
import pytest
import torch

import audience_model as am
import score_model as sm
from helpers import ROOT, build_model_from_fixture, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I_CAT = 40


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _edges():
    from elimrec_amd import ops
    return ops.AUDIENCE_TILE, ops.AUDIENCE_CHUNK


class _math(object):
    def __init__(self, fast):
        from elimrec_amd import _lib
        self.lib, self.fast = _lib.load(), fast

    def __enter__(self):
        self.before = int(self.lib.elimrec_score_get_math())
        self.lib.elimrec_score_set_math(1 if self.fast else 0)

    def __exit__(self, *exc):
        self.lib.elimrec_score_set_math(self.before)


def _csr(excl):
    ptr = np.zeros(len(excl) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(list(x)) for x in excl])
    flat = np.asarray([u for x in excl for u in x], dtype=np.int32)
    return ptr, flat


def _row_sum(Yd, U, I, d, S, mask, fusion, sqn):
    """sum_i sigmoid(u . i) of every user from the scorer's pass 1, in user blocks of at most 8192."""
    from elimrec_amd import ops
    out = torch.empty(U, dtype=torch.float32, device=DEV)
    for lo in range(0, U, 8192):
        users = torch.arange(lo, min(U, lo + 8192), dtype=torch.int64, device=DEV)
        ws = torch.empty(ops.score_workspace(users.numel(), U, I, S, 1, topk_only=True, d=d), dtype=torch.uint8, device=DEV)
        part = torch.empty(users.numel(), dtype=torch.float32, device=DEV)
        ops.score_topk_shard(Yd, U, I, users, d, S, mask, fusion, "TIE", ws, 1, part, I, 0, sqnorm=sqn)
        out[lo:lo + users.numel()] = part
    return out


class _Table(object):
    """A table on the device with its norms, and per (fusion) the pass-1 row sums."""

    def __init__(self, family, U, d, S, seed, Y=None):
        from elimrec_amd import ops
        self.U, self.d, self.S = U, d, S
        self.Y = sm.make_table(family, U, I_CAT, d, S, seed) if Y is None else Y
        self.Yd = self.Y.to(DEV)
        self.sqn = ops.row_sqnorms(self.Yd, d, 1 + S, torch.empty(U + I_CAT, 1 + S, dtype=torch.float32, device=DEV))
        self._rs = {}

    def row_sum(self, mask, fusion):
        if (mask, fusion) not in self._rs:
            self._rs[(mask, fusion)] = _row_sum(self.Yd, self.U, I_CAT, self.d, self.S, mask, fusion, self.sqn)
        return self._rs[(mask, fusion)]

    def run(self, items, mask, fusion, ptype, K, excl=None, rows_out=None, via_torch=False):
        from elimrec_amd import ops, torch_ops
        Q = len(items)
        rs = self.row_sum(mask, fusion) if ptype == "TIE" else None
        ptr, flat = _csr(excl) if excl is not None else (None, None)
        if via_torch:
            idx, val = torch_ops.load().audience_topk(
                self.Yd, self.U, I_CAT, _t(np.asarray(items, dtype=np.int32)), None if ptr is None else _t(ptr), None if ptr is None else _t(flat),
                self.d, self.S, mask, ops.FUSION_MODES[fusion], ops.PREDICT_TYPES.get(ptype, 0), K, self.sqn, rs, I_CAT)
        else:
            idx = torch.full((rows_out or Q, K), -7, dtype=torch.int32, device=DEV)
            val = torch.full((rows_out or Q, K), 7.0, dtype=torch.float32, device=DEV)
            query = ops.AudienceQuery(np.asarray(items, dtype=np.int32), I_CAT, self.U, DEV, ptr, flat)
            ops.audience_topk(self.Yd, self.U, I_CAT, query, self.d, self.S, mask, fusion, ptype, K, idx, val, sqnorm=self.sqn, row_sum=rs)
        torch.cuda.synchronize()
        return idx.cpu().numpy(), val.cpu().numpy()

    def models(self, items, mask, fusion, ptype):
        rs = self.row_sum(mask, fusion).cpu() if ptype == "TIE" else None
        kw = dict(row_sum=rs, I_total=I_CAT) if rs is not None else {}
        s64 = am.columns(self.Y.double(), self.U, items, self.d, self.S, mask, fusion, ptype, **kw).numpy()
        s32 = am.columns(self.Y, self.U, items, self.d, self.S, mask, fusion, ptype, **kw).numpy()
        return s64, s32


def _excl_for(U, Q, rng):
    """Query 0 excludes nobody, query 1 everybody, the others a few users (one id repeated)."""
    excl = []
    for q in range(Q):
        if q == 0:
            excl.append([])
        elif q == 1:
            excl.append(list(range(U)))
        else:
            ids = rng.integers(0, U, size=4).tolist()
            excl.append(ids + ids[:1])
    return excl


def _items(Q):
    return [(7 * q + 3) % I_CAT for q in range(Q)]          # every catalogue item at Q >= 40, repeats beyond


def _check_case(tab, Q, K, mask, pairs, fast, seed, what):
    rng = np.random.default_rng(seed)
    items, excl = _items(Q), _excl_for(tab.U, Q, rng)
    ok = am.eligible_mask(tab.U, Q, excl)
    for ptype, fusion in pairs:
        with _math(fast):
            idx, val = tab.run(items, mask, fusion, ptype, K, excl)
        s64, s32 = tab.models(items, mask, fusion, ptype)
        worst, tol = am.check_lists(idx, val, s64, s32, ok, K, fast, what + (ptype, fusion, fast))
        print("audience %s %s/%s fast=%d: worst |val - fp64| %.3g, tol %.3g" % (what, ptype, fusion, fast, worst, tol))
        if Q > 1:
            assert (idx[1] == -1).all() and np.isneginf(val[1]).all()


TIE_HM = [("TIE", "hm")]


def _shapes():
    T, C = _edges()
    # (name, family, U, Q, K, d, S, mask, pairs, math modes)
    return [
        ("mid", "benign", C + 1, 17, 10, 64, 3, 7, sm.PAIRS, (True, False)),
        ("few-users", "benign", 5, 1, 10, 32, 1, 1, TIE_HM + [("TE", "rubi")], (True,)),
        ("chunk-1", "saturated", C - 1, 16, 64, 32, 3, 5, TIE_HM + [("TE", "rubi")], (True, False)),
        ("three-chunks", "zero", 2 * C + 37, T + 1, 65, 64, 3, 5, TIE_HM + [("TIE", "rubi")], (True,)),
        ("general-d", "benign", C + 1, 17, 256, 20, 3, 7, TIE_HM + [("TIE", "rubi")], (True,)),
        ("no-heads", "benign", C - 1, T + 1, 1, 20, 0, 0, TIE_HM + [("normal", "rubi")], (False,)),
        ("one-head", "saturated", 2 * C + 37, 16, 10, 20, 1, 1, TIE_HM + [("TE", "sum")], (False,)),
        ("k256", "zero", C + 1, 1, 256, 64, 3, 5, TIE_HM + [("TE", "rubi")], (True,)),
        ("d32-k65", "saturated", C + 1, 17, 65, 32, 3, 7, TIE_HM, (True,)),
    ]


@pytest.mark.parametrize("case", range(9))
def test_lists_at_the_kernel_edges(case):
    name, family, U, Q, K, d, S, mask, pairs, modes = _shapes()[case]
    tab = _Table(family, U, d, S, 11 + case)
    for fast in modes:
        _check_case(tab, Q, K, mask, pairs, fast, 5 + case, (name, family, U, Q, K, d, S, mask))


RISING_U, RISING_Q, RISING_D = 4096 + 17, 17, 32
RISING_SCORINGS = [("normal", "rubi", 0, 0), ("TIE", "hm", 3, 7)]       # predict type, fusion, S, head mask


@pytest.mark.parametrize("K", [1, 64, 65, 256])
def test_rising_scores(K):
    """Every user beats the running threshold (audience_model.rising_table): every 16-row tile appends to every live list, the lists
    are cut in mid-chunk, a second chunk of 17 users and the merge take part. The scores' gaps are beyond the near-tie allowance
    (test_audience_cpu.py asserts it on the float64 model), so the ids are the model's exactly."""
    T, C = _edges()
    U, Q, d = RISING_U, RISING_Q, RISING_D
    assert U == C + 17 and Q == 17
    items, excl = list(range(Q)), am.rising_excl(U, Q)
    ok = am.eligible_mask(U, Q, excl)
    for ptype, fusion, S, mask in RISING_SCORINGS:
        tab = _Table("benign", U, d, S, 0, Y=am.rising_table(U, I_CAT, d, S))
        s64, s32 = tab.models(items, mask, fusion, ptype)
        for fast in (True, False):
            with _math(fast):
                idx, val = tab.run(items, mask, fusion, ptype, K, excl)
            worst, tol = am.check_lists(idx, val, s64, s32, ok, K, fast, ("rising", ptype, fusion, K, fast))
            print("audience rising %s/%s K=%d fast=%d: worst |val - fp64| %.3g, tol %.3g" % (ptype, fusion, K, fast, worst, tol))
            assert am.min_gap(s64, ok) > 2 * tol
            want = np.stack([np.flatnonzero(ok[:, q])[np.argsort(-s64[ok[:, q], q], kind="stable")][:K] for q in range(Q)])
            assert np.array_equal(idx, want), ("rising", ptype, fusion, K, fast)
        assert not set(idx[1].tolist()) & set(excl[1]) and idx[0, 0] == U - 1


def test_exclusions():
    T, C = _edges()
    U, d, S, mask, K = C + 1, 64, 3, 7, 10
    tab = _Table("benign", U, d, S, 21)
    items = [4, 9, 17, 30]
    s64, s32 = tab.models(items, mask, "hm", "TIE")
    top3 = np.argsort(-s64[:, 2], kind="stable")[:3].tolist()
    excl = [[], list(range(U)), top3 + top3[:1], [2, 2, 2]]
    ok = am.eligible_mask(U, 4, excl)
    idx, val = tab.run(items, mask, "hm", "TIE", K, excl)
    am.check_lists(idx, val, s64, s32, ok, K, True, "exclusions")
    assert (idx[1] == -1).all() and np.isneginf(val[1]).all()
    assert not set(idx[2].tolist()) & set(top3) and 2 not in idx[3].tolist()
    plain, _ = tab.run(items, mask, "hm", "TIE", K + 3)
    assert set(plain[2, :3].tolist()) == set(top3) and idx[2].tolist() == plain[2, 3:].tolist()        # the next ones move up
    assert idx[0].tolist() == plain[0, :K].tolist()
    # no exclusion CSR at all gives query 0's list for everyone; the torch op gives the same bits
    none_idx, none_val = tab.run(items, mask, "hm", "TIE", K)
    assert np.array_equal(none_idx[0], idx[0]) and np.array_equal(none_val[0], val[0])
    t_idx, t_val = tab.run(items, mask, "hm", "TIE", K, excl, via_torch=True)
    assert np.array_equal(t_idx, idx) and t_val.tobytes() == val.tobytes()


@pytest.mark.parametrize("d,K", [(64, 10), (32, 65), (20, 10)])
def test_a_row_does_not_depend_on_its_company(d, K):
    T, C = _edges()
    U, S, mask = C + 1, 3, 5
    tab = _Table("saturated", U, d, S, 31)
    for ptype, fusion in (("TIE", "hm"), ("TE", "rubi")):
        alone = tab.run([6], mask, fusion, ptype, K, [[3, 8]])
        again = tab.run([6], mask, fusion, ptype, K, [[3, 8]])
        assert alone[0].tobytes() == again[0].tobytes() and alone[1].tobytes() == again[1].tobytes()
        others = _items(T)
        first = tab.run([6] + others, mask, fusion, ptype, K, [[3, 8]] + [[1]] * T)
        last = tab.run(others[::-1] + [6], mask, fusion, ptype, K, [[]] * T + [[8, 3, 3]])
        twice = tab.run([6, 11, 6], mask, fusion, ptype, K, [[3, 8], [], [3, 8]])
        for got, row in ((first, 0), (last, T), (twice, 0), (twice, 2)):
            assert got[0][row].tobytes() == alone[0][0].tobytes() and got[1][row].tobytes() == alone[1][0].tobytes()
    idx, val = tab.run([6, 7], mask, "hm", "TIE", K, rows_out=3)
    assert (idx[2] == -7).all() and (val[2] == 7.0).all()                    # beyond [Q x K]: left alone


def test_argument_checks_on_the_device():
    from elimrec_amd import ops
    tab = _Table("benign", 50, 32, 1, 3)
    idx = torch.empty(2, 4, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="row_sum"):
        ops.audience_topk(tab.Yd, 50, I_CAT, [0, 1], 32, 1, 1, "hm", "TIE", 4, idx)
    with pytest.raises(ValueError):
        ops.audience_topk(tab.Yd, 50, I_CAT, [0, 1], 32, 1, 1, "hm", "TE", 4, idx.cpu().to(DEV).t().contiguous().t())
    with pytest.raises(ValueError):
        ops.audience_topk(tab.Yd, 50, I_CAT, [0, 1], 32, 1, 1, "hm", "TE", 257, idx)
    with pytest.raises(IndexError):
        ops.audience_topk(tab.Yd, 50, I_CAT, [I_CAT], 32, 1, 1, "hm", "TE", 4, idx)
    assert ops.audience_topk(tab.Yd, 50, I_CAT, [], 32, 1, 1, "hm", "TE", 4, idx) is idx


# --------------------------------------------------------------------------- the model on the fixtures
def _forward(name, extra=()):
    g = load_golden(name)
    model, _ = build_model_from_fixture(g, DEV, extra_argv=extra)
    model.bpr_loss(_t(g["step1/users"]), _t(g["step1/pos"]), _t(g["step1/neg"]))
    return model, g


def _ranked(scores, ok, K):
    return am.topk32(scores, ok, K)


@pytest.mark.parametrize("name", ["ml3", "kwai"])
def test_model_audience_on_a_fixture(name):
    from elimrec_amd import Audience
    from elimrec_amd.evaluator import CandidateScoringError
    g = load_golden(name)
    fresh, _ = build_model_from_fixture(g, DEV)
    with pytest.raises(RuntimeError):
        fresh.audience([0], 3)
    model, g = _forward(name)
    U, I, d, S = model.num_users, model.num_items, model.latent_dim, model.S
    rng = np.random.default_rng(5)
    items = rng.permutation(I)[:min(I, 20)].tolist()
    k = 7
    train = model.dataset.get_user_train_dict()
    item_train = {}
    for u, its in train.items():
        for i in its:
            item_train.setdefault(int(i), []).append(int(u))
    exclude = {i: item_train.get(i, []) for i in items}
    fast = bool(model_math())
    for ptype in ("normal", "TE", "TIE"):
        model.predict_type = ptype
        got = model.audience(items, k)
        assert isinstance(got, Audience) and got.users.dtype == torch.int32 and got.scores.dtype == torch.float32
        assert got.users.device.type == "cpu" and tuple(got.users.shape) == tuple(got.scores.shape) == (len(items), k)
        Y = model._ws["Y"].cpu()
        mask = model._head_mask()
        s64 = am.columns(Y.double(), U, items, d, S, mask, model.fusion_mode, ptype).numpy()
        s32 = am.columns(Y, U, items, d, S, mask, model.fusion_mode, ptype).numpy()
        ok = np.ones((U, len(items)), dtype=bool)
        am.check_lists(got.users.numpy(), got.scores.numpy(), s64, s32, ok, k, fast, (name, ptype))
        # the composition the kernel replaces: every user scores the same items, ranked per column
        comp = model.predict_candidates(list(range(U)), [items] * U).numpy()
        c_idx, c_val = _ranked(comp, ok, k)
        am.check_lists(c_idx, c_val, s64, s32, ok, k, fast, (name, ptype, "composition"))
        got_x = model.audience(items, k, exclude=exclude)
        ok_x = am.eligible_mask(U, len(items), [exclude[i] for i in items])
        am.check_lists(got_x.users.numpy(), got_x.scores.numpy(), s64, s32, ok_x, k, fast, (name, ptype, "exclude"))
        for b, i in enumerate(items):
            assert not set(got_x.users[b].tolist()) & set(exclude[i])
    # the cached row sums: no second pass 1 on unchanged tables, refreshed by the next forward
    model.predict_type = "TIE"
    model.audience(items, k)
    cached, calls = model._ws["aud_row_sum"], []
    inner = model._catalogue_row_sum
    model._catalogue_row_sum = lambda *a, **kw: calls.append(1) or inner(*a, **kw)
    model.audience(items[:3], k)
    assert not calls and model._ws["aud_row_sum"] is cached
    model.bpr_loss(_t(g["step1/users"]), _t(g["step1/pos"]), _t(g["step1/neg"]))
    model.audience(items[:3], k)
    assert calls and model._ws["aud_row_sum"] is not cached
    model._catalogue_row_sum = inner
    with pytest.raises(IndexError):
        model.audience([I], 3)
    with pytest.raises(ValueError):
        model.audience([0], 0)
    model._eval_shard = object()
    try:
        with pytest.raises(CandidateScoringError):
            model.audience([0], 3)
    finally:
        model._eval_shard = None
    assert tuple(model.audience([], 3).users.shape) == (0, 3)


def model_math():
    from elimrec_amd import _lib
    return int(_lib.load().elimrec_score_get_math())


def _mean_1ulp(got, want, what):
    err = np.abs(got.astype(np.float64) - want)
    ok = (err <= np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)) | (np.isnan(want) & np.isnan(got))
    assert ok.all(), (what, got, want)


@pytest.mark.parametrize("view", [None, [1, 4]])
def test_audience_report(view):
    from elimrec_amd import reports
    from elimrec_amd.evaluator import AudienceReport, AudienceTables
    model, _ = _forward("ml3")
    train, test = model.dataset.get_user_train_dict(), model.dataset.get_user_test_dict()
    k = 5
    report = AudienceReport(model.dataset, train, test, k, item_group_view=view)
    report.block_items = (len(report.items) + 1) // 2                         # two item blocks
    shown = {}
    for ptype in ("TE", "TIE"):
        model.predict_type = ptype
        shown[ptype] = report.audience_rows(model)
        final, buf = report.evaluate(model, shown[ptype])
        rows, lists, scores, counts = [x.cpu().numpy() for x in shown[ptype]]
        # the lists are the model's own, the items' training users left out
        want_lists = model.audience(report.items, k, exclude=report.item_train)
        assert np.array_equal(lists, want_lists.users.numpy()) and scores.tobytes() == want_lists.scores.numpy().tobytes()
        ptr, users = report.test_csr()
        want_rows = am.item_rows(lists, scores, ptr, users, report.user_train_len)
        for c in range(4):
            _mean_1ulp(rows[:, c], want_rows[:, c], ("row column", c))
        assert np.array_equal(counts, np.bincount(lists[lists >= 0], minlength=model.num_users))
        assert isinstance(final, AudienceTables) and final.items.shape == (len(report.group_labels), 4) and final.users.shape == (1, 4)
        assert (len(report.group_labels) > 1) == (view is not None)
        for gi, at in enumerate(report._positions):
            _mean_1ulp(final.items[gi], want_rows[at].mean(axis=0), report.group_labels[gi])
        assert np.array_equal(final.users, reports.exposure_summary(counts, [np.arange(model.num_users)])[:, :4])
        lines = buf.split("\n")
        assert len(lines) == 1 + len(report.group_labels) + 2 and lines[0].startswith("columns:") and lines[1].startswith("all:")
    final, buf = report.shift(shown["TE"], shown["TIE"])
    a, b = shown["TE"][1].cpu().numpy(), shown["TIE"][1].cpu().numpy()
    overlap = np.array([len(set(x[x >= 0]) & set(y[y >= 0])) / k for x, y in zip(a, b)])
    _mean_1ulp(final[0, :1], np.array([overlap.mean()]), "overlap")
    assert final.shape == (len(report.group_labels), 5) and "d_hit" in buf and report.shift_columns[0] == "overlap"


# --------------------------------------------------------------------------- the driver's switch
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


class _Capture(object):
    def __init__(self):
        self.lines = []

    def log(self, *msg):
        self.lines.append("\t".join(str(m) for m in msg))


def _driver(tmp_path, extra):
    """(lines Net.test_all_effects() logs after a two-epoch synthetic run, evaluate()[0], test()[0])."""
    from elimrec_amd import Logger
    net = _net(tmp_path, extra)
    before = Logger.logger
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        net.run()
        cap = Logger.logger = _Capture()
        net.test_all_effects()
        rec = net.recommender
        rec.predict_type = "TIE"
        return cap.lines, np.asarray(rec.evaluate()[0]), np.asarray(rec.test()[0])
    finally:
        os.chdir(cwd)
        Logger.logger = before


def test_driver_switch(tmp_path):
    off, ev0, te0 = _driver(tmp_path / "a", [])
    assert len(off) == 2 and not any("audience" in ln for ln in off)
    on, ev1, te1 = _driver(tmp_path / "b", ["--audience_report=5", "--item_group_view=[1,4]"])
    assert [on[0], on[2]] == off and len(on) == 5
    for effect, table in (("TE", on[1]), ("TIE", on[3])):
        assert table.startswith("  [%s] top-5 audiences" % effect) and "columns:" in table and "\nall:" in table
        assert all(c in table for c in ("hit", "first", "act", "score", "users", "coverage", "gini", "entropy"))
    assert on[4].startswith("  [TE->TIE] audience shift:") and "overlap" in on[4] and "d_score" in on[4]
    assert ev0.tobytes() == ev1.tobytes() and te0.tobytes() == te1.tobytes()
