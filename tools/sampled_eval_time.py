"""Sampled-negative validation pass at the Tiktok shape (rec.evaluate.neg = 100 and 1000, TE and TIE) beside the full-catalogue
pass in the same process, after three training steps. Dev tool.

    python tools/sampled_eval_time.py [--passes N] [--out summary.json]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/sampled_eval_time.py --passes 3 --profile
    python tools/sampled_eval_time.py --merge summary.json --trace-dir DIR      # candidate-kernel times + gathered bytes / time

--profile runs the sampled passes only, in a fixed order (neg 100 TE, TIE, neg 1000 TE, TIE; --passes each), so the trace's
score_cand_kernel dispatches split into those four groups in launch order."""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NEGS = (100, 1000)
TYPES = ("TE", "TIE")


def _setup():
    import torch
    import bench
    from elimrec_amd import ColumnShardEngine, ColumnShardTrainer, FusedAdam, PairwiseSamplerV2
    cfg, ds, model = bench.build(None, "cuda:0")
    model = model.to("cuda:0")
    opt = FusedAdam(model.parameters(), lr=cfg["lr"], weight_decay=cfg["weight_decay"])
    tr = ColumnShardTrainer(ColumnShardEngine(model), opt)
    u, p, n = PairwiseSamplerV2(ds, batch_size=2048, device="cuda:0").sample_epoch()
    for i in range(3):
        tr.step(u[i * 2048:(i + 1) * 2048], p[i * 2048:(i + 1) * 2048], n[i * 2048:(i + 1) * 2048])
    torch.cuda.synchronize()
    return cfg, ds, model


def _evaluator(cfg, ds, neg):
    from elimrec_amd import ProxyEvaluator
    return ProxyEvaluator(ds, ds.get_user_train_dict(), ds.get_user_valid_dict(), ds.get_user_valid_neg_dict(neg),
                          metric=cfg["metric"], top_k=cfg["topks"], batch_size=cfg["test_batch_size"])


def _time(fn, passes):
    import torch
    ts = []
    for _ in range(passes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts), sorted(ts)[len(ts) // 2]


def run(args):
    cfg, ds, model = _setup()
    valid = ds.get_user_valid_dict()
    row_bytes = (1 + model.S) * model.latent_dim * 4
    out = {"shape": {"users": ds.num_users, "items": ds.num_items, "recdim": model.latent_dim, "heads": model.S,
                     "valid_users": len(valid), "item_row_bytes": row_bytes}, "passes": args.passes, "sampled": []}
    evs = {neg: _evaluator(cfg, ds, neg) for neg in NEGS}          # (negatives drawn before any timing)
    if not args.profile:
        for pt in TYPES:
            model.predict_type = pt
            model.evaluate()
            best, med = _time(model.evaluate, args.passes)
            out["full_%s" % pt] = {"best_s": best, "median_s": med}
    for neg in NEGS:
        ev = evs[neg]
        pairs = sum(len(valid[u]) + len(ev.evaluator.user_neg_test[u]) for u in valid)
        for pt in TYPES:
            model.predict_type = pt
            if args.profile:
                for _ in range(args.passes):
                    ev.evaluate(model)
                continue
            res, buf = ev.evaluate(model)
            best, med = _time(lambda: ev.evaluate(model), args.passes)
            out["sampled"].append({"neg": neg, "predict_type": pt, "pairs": pairs, "gathered_bytes": pairs * row_bytes,
                                   "best_s": best, "median_s": med, "metrics": buf.split()})
            print("neg=%d %s: best %.5f s, median %.5f s, %d pairs (%s)" % (neg, pt, best, med, pairs, " ".join(buf.split())))
    if not args.profile:
        for pt in TYPES:
            print("full %s: best %.5f s, median %.5f s" % (pt, out["full_" + pt]["best_s"], out["full_" + pt]["median_s"]))
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


def merge(args):
    """Adds the candidate kernel's dispatch times (rocprofv3 kernel trace) to the summary: per (neg, predict type) group the
    mean of its passes' summed dispatch durations, and gathered bytes / that time."""
    with open(args.merge) as f:
        out = json.load(f)
    import sqlite3
    rows = []
    for fn in glob.glob(os.path.join(args.trace_dir, "**", "*.db"), recursive=True):          # rocprofv3's default (rocpd) output
        with sqlite3.connect(fn) as db:
            rows += db.execute("SELECT start, end - start FROM kernels WHERE name LIKE '%score_cand_kernel%'").fetchall()
    for fn in glob.glob(os.path.join(args.trace_dir, "**", "*kernel_trace.csv"), recursive=True):   # --output-format csv
        with open(fn) as f:
            for r in csv.DictReader(f):
                if "score_cand_kernel" in r.get("Kernel_Name", ""):
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    groups = len(NEGS) * len(TYPES)
    per = len(rows) // groups
    if per == 0 or per * groups != len(rows):
        raise SystemExit("expected a multiple of %d score_cand_kernel dispatches, found %d" % (groups, len(rows)))
    passes = int(args.profile_passes)
    for k, s in enumerate(out["sampled"]):
        g = rows[k * per:(k + 1) * per]
        t = sum(d for _, d in g) / passes * 1e-9
        s["candidate_kernel_s"] = t
        s["candidate_kernel_dispatches_per_pass"] = per // passes
        s["gathered_TB_per_s"] = s["gathered_bytes"] / t / 1e12
    with open(args.merge, "w") as f:
        json.dump(out, f, indent=1)
    for s in out["sampled"]:
        print("neg=%d %s: kernel %.1f us per pass, %.2f TB/s" % (s["neg"], s["predict_type"], s["candidate_kernel_s"] * 1e6,
                                                               s["gathered_TB_per_s"]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampled_eval_tiktok.json"))
    ap.add_argument("--merge")
    ap.add_argument("--trace-dir")
    ap.add_argument("--profile-passes", default=3)
    a = ap.parse_args()
    merge(a) if a.merge else run(a)
