"""Validation-pass time of the device evaluator at the Tiktok shape: best of n passes per setting (tie order id / reference). Dev tool.
    python tools/eval_time.py [n] [--group_view=[10,30,50,100] [--out=FILE.json]]
--group_view: also one grouped pass (GroupedEvaluator.evaluate_with_overall) against one ungrouped pass and against the reference's way
(one UniEvaluator.evaluate(model, users_of_group) pass per group), alternated, and the reduction's own time (device events around
ops.group_metric_means) at 3 x 10 and 5 x 256 columns; --out writes the numbers as JSON."""
import json, os, sys, time, torch
sys.path.insert(0, os.environ.get("GRAFT_REPO_ROOT", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import bench
cfg, ds, model = bench.build(None, "cuda:0")
model = model.to("cuda:0")
from elimrec_amd import ColumnShardEngine, ColumnShardTrainer, FusedAdam, PairwiseSamplerV2
opt = FusedAdam(model.parameters(), lr=cfg["lr"], weight_decay=cfg["weight_decay"])
tr = ColumnShardTrainer(ColumnShardEngine(model), opt)
u, p, n = PairwiseSamplerV2(ds, batch_size=2048, device="cuda:0").sample_epoch()
for i in range(3): tr.step(u[i * 2048:(i + 1) * 2048], p[i * 2048:(i + 1) * 2048], n[i * 2048:(i + 1) * 2048])
model.predict_type = "TIE"
ev = model.valid_evaluator.evaluator
N_PASSES = next((int(a) for a in sys.argv[1:] if not a.startswith("--")), 8)
OPTS = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
for order in ("id", "reference"):
    ev.tie_order = order
    ts = []
    for k in range(N_PASSES):
        torch.cuda.synchronize(); t0 = time.perf_counter(); res, buf = model.evaluate(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    print("tie_order=%s: best %.5f s, median %.5f s  (%s)" % (order, min(ts), sorted(ts)[len(ts) // 2], buf.replace("\t", " ")[:60]))
from elimrec_amd import _lib
print("scorer cross-check: rows checked %d, mismatch rows %d, bf16x3 scorer on: %d" % (ev.scorer_checked_rows, ev.scorer_mismatch_rows, int(_lib.load().elimrec_score_get_bf16x3())))


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); out = fn(); torch.cuda.synchronize()
    return time.perf_counter() - t0, out


if "group_view" in OPTS:
    import numpy as np
    from elimrec_amd import ops
    from elimrec_amd.evaluator import GroupedEvaluator
    view = json.loads(OPTS["group_view"])
    ge = GroupedEvaluator(None, ev.user_pos_train, ev.user_pos_test, metric=cfg["metric"], group_view=view, top_k=cfg["topks"],
                          batch_size=cfg["test_batch_size"])
    ge.tie_order = ev.tie_order = "reference"
    members = [ge.grouped_user[label] for label in ge.group_labels]
    forms = {"grouped_pass": lambda: ge.evaluate_with_overall(model),
             "ungrouped_pass": lambda: ev.evaluate(model),
             "pass_per_group": lambda: [ev.evaluate(model, users) for users in members]}
    for fn in forms.values():            # every shape once before the timed window (the per-group user blocks are not cached)
        fn()
    ts = {k: [] for k in forms}
    for k in range(N_PASSES):            # alternated: the three forms see the same machine
        for name, fn in forms.items():
            ts[name].append(timed(fn)[0])
    overall, _, group_final, group_buf = ge.evaluate_with_overall(model)
    assert np.array_equal(overall, ev.evaluate(model)[0])
    res = {"shape": "Tiktok (bench.py WORKLOAD)", "predict_type": "TIE", "tie_order": "reference", "top_k": list(map(int, cfg["topks"])),
           "metric": list(cfg["metric"]), "group_view": view, "group_sizes": ge.group_sizes, "discarded_users": ge.num_discarded,
           "test_users": len(ev.default_users()), "passes": N_PASSES}
    for name in forms:
        res[name + "_s"] = {"best": min(ts[name]), "median": sorted(ts[name])[len(ts[name]) // 2]}
        print("%s: best %.5f s, median %.5f s" % (name, min(ts[name]), sorted(ts[name])[len(ts[name]) // 2]))
    print("groups:%s" % group_buf.replace("\t", " "))
    index = ge._group_index(torch.device("cuda:0"))
    n_users = len(ev.default_users())
    res["reduction_kernel_us"] = {}
    for n_metrics, K in ((3, 10), (5, 256)):
        rows = torch.rand(n_users, n_metrics * K, device="cuda:0")
        out = torch.empty(index.n_groups, n_metrics * K, device="cuda:0")
        ws = torch.empty(int(_lib.load().elimrec_group_metric_means_workspace(index.n_listed, n_metrics * K, index.n_groups)),
                         dtype=torch.uint8, device="cuda:0")
        for _ in range(5):
            ops.group_metric_means(rows, index, None, out, workspace=ws)
        reps = 200
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            ops.group_metric_means(rows, index, None, out, workspace=ws)
        b.record(); torch.cuda.synchronize()
        us = a.elapsed_time(b) * 1e3 / reps
        res["reduction_kernel_us"]["%dx%d" % (n_metrics, K)] = {"per_call_us": us, "rows": n_users, "listed_rows": index.n_listed,
                                                                "bytes_read": index.n_listed * n_metrics * K * 4, "back_to_back_calls": reps}
        print("group_metric_means %d x %d columns, %d listed rows: %.2f us per call (two launches, %d calls back to back)"
              % (n_metrics, K, index.n_listed, us, reps))
    if "out" in OPTS:
        os.makedirs(os.path.dirname(os.path.abspath(OPTS["out"])), exist_ok=True)
        with open(OPTS["out"], "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
