"""The rank report's pass at the Tiktok shape beside what it sits next to: after three training steps, on the test users,
one RankReport.pair_ranks pass (scoring into a block + the count, every user block), one top-K test pass of the evaluator
(model.test_evaluator.evaluate), and on the first user block the count launch alone (ops.rank_targets: time and GB/s over the
block bytes it reads) with a clone() of the same block as the memory-rate yardstick. Passes are wall-clock around a device
synchronisation (best and median of `--reps`), launches device times from events around `--calls` back-to-back calls. Dev tool.

    python tools/rank_time.py [--out profiles/rank_report_tiktok.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from _timing import _events, _setup, _wall  # noqa: E402


def run(args):
    import numpy as np
    import torch
    from elimrec_amd import ops
    from elimrec_amd.evaluator import RankReport
    cfg, ds, model = _setup()
    dev = "cuda:0"
    train, test = ds.get_user_train_dict(), ds.get_user_test_dict()
    report = RankReport(ds, train, test, cfg["topks"])
    model.predict_type = "TIE"
    out = {"shape": {"users": model.num_users, "items": model.num_items, "recdim": model.latent_dim, "heads": model.S,
                     "test_users": len(report.users), "pairs": report.num_pairs, "dropped_pairs": report.num_dropped,
                     "block_users": report.block_users, "block_bytes": report.block_bytes},
           "predict_type": "TIE", "reps": args.reps, "calls": args.calls}
    best, med = _wall(lambda: report.pair_ranks(model), args.reps)
    out["rank_pass"] = {"best_s": best, "median_s": med}
    print("rank pass (score + count, %d users, %d pairs): best %.2f ms, median %.2f ms" % (len(report.users), report.num_pairs, best * 1e3, med * 1e3))
    best, med = _wall(lambda: model.test_evaluator.evaluate(model), args.reps)
    out["topk_test_pass"] = {"best_s": best, "median_s": med}
    print("top-K test pass of the evaluator: best %.2f ms, median %.2f ms" % (best * 1e3, med * 1e3))
    out["rank_pass_over_topk_pass"] = out["rank_pass"]["median_s"] / med

    # the first user block: the count alone, and a clone() of the block it reads
    b = min(report.block_users, len(report.users))
    users, target, tptr, titems = report._block(report._resident(dev), 0, b, dev)
    I = model.num_items
    block = torch.empty(b, (I + 3) // 4 * 4, dtype=torch.float32, device=dev)[:, :I]
    model.predict_device(users, scores=block, train_ptr=tptr, train_items=titems)
    rank = torch.empty(target.n_targets, dtype=torch.int32, device=dev)
    read = int(np.count_nonzero(target.sizes)) * I * 4                # rows without a target are not read
    best, med = _events(lambda: ops.rank_targets(block, target, None, rank), args.calls, args.reps)
    out["count_kernel"] = {"rows": b, "rows_read": int(np.count_nonzero(target.sizes)), "targets": target.n_targets, "bytes_read": read,
                           "best_s": best, "median_s": med, "GB_per_s": read / med / 1e9}
    print("count launch (%d rows, %d targets): best %.1f us, median %.1f us, %.0f GB/s read" % (b, target.n_targets, best * 1e6, med * 1e6,
                                                                                               read / med / 1e9))
    full = block.numel() * 4
    best, med = _events(lambda: block.clone(), args.calls, args.reps)
    out["clone"] = {"bytes_read": full, "bytes_written": full, "best_s": best, "median_s": med, "GB_per_s_read": full / med / 1e9}
    print("clone() of the block: best %.1f us, median %.1f us, %.0f GB/s read (+ as much written)" % (best * 1e6, med * 1e6, full / med / 1e9))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_report_tiktok.json"))
    run(ap.parse_args())
