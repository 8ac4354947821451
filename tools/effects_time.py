"""The effect breakdown launch at the Tiktok shape beside what it replaces: 8192 users' top-50 lists after three training steps;
the breakdown (ops.score_effects), ops.score_candidates on the same lists under TE and under TIE, and the pass-1 launch that gives
the catalogue row sums. Device times from events around `--calls` back-to-back launches, best and median of `--reps`. Dev tool.

    python tools/effects_time.py [--users 8192] [--k 50] [--out profiles/effects_tiktok.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from _timing import _events, _setup  # noqa: E402


def run(args):
    import torch
    from elimrec_amd import _lib, ops
    _, ds, model = _setup()
    dev = "cuda:0"
    B, K = min(args.users, ds.num_users), args.k
    U, I, d, S = model.num_users, model.num_items, model.latent_dim, model.S
    users = torch.arange(B, device=dev, dtype=torch.int64)
    model.predict_type = "TIE"
    idx, _ = model.predict_device(users, top_k=K)
    ptr = torch.arange(B + 1, device=dev, dtype=torch.int64) * K
    items = idx.reshape(-1).contiguous()
    Y, sqn, mask, fusion = model._ws["Y"], model._block_sqnorms(dev), model._head_mask(), model.fusion_mode
    ws = torch.empty(ops.score_workspace(B, U, I, S, 1, topk_only=True, d=d), dtype=torch.uint8, device=dev)
    row_sum = torch.empty(B, device=dev)
    C = 6 + S
    fx = torch.empty(B, K, C, device=dev)
    sc = torch.empty(B, K, device=dev)
    launches = {
        "effects": lambda: ops.score_effects(Y, U, I, users, d, S, mask, fusion, ptr, items, fx, sqn, row_sum, I),
        "candidates_TE": lambda: ops.score_candidates(Y, U, I, users, d, S, mask, fusion, "TE", ptr, items, sc, sqnorm=sqn),
        "candidates_TIE": lambda: ops.score_candidates(Y, U, I, users, d, S, mask, fusion, "TIE", ptr, items, sc, sqnorm=sqn,
                                                       row_sum=row_sum, I_total=I),
        "pass1_row_sums": lambda: ops.score_topk_shard(Y, U, I, users, d, S, mask, fusion, "TIE", ws, 1, row_sum, I, 0, sqnorm=sqn),
    }
    launches["pass1_row_sums"]()
    row_bytes = (1 + S) * d * 4
    gathered = B * K * row_bytes
    out = {"shape": {"users": U, "items": I, "recdim": d, "heads": S, "listed_users": B, "k": K, "item_row_bytes": row_bytes,
                     "columns": C}, "fusion": fusion, "math": "fast" if int(_lib.load().elimrec_score_get_math()) else "exact",
           "calls": args.calls, "reps": args.reps, "gathered_bytes": gathered, "launches": {}}
    for name, fn in launches.items():
        best, med = _events(fn, args.calls, args.reps)
        rec = {"best_s": best, "median_s": med}
        if name != "pass1_row_sums":
            rec["stored_bytes"] = B * K * 4 * (C if name == "effects" else 1)
            rec["gathered_TB_per_s"] = gathered / med / 1e12
        out["launches"][name] = rec
        print("%-16s best %.2f us, median %.2f us%s" % (name, best * 1e6, med * 1e6,
                                                        "" if "gathered_TB_per_s" not in rec else ", %.2f TB/s gathered" % rec["gathered_TB_per_s"]))
    two = out["launches"]["candidates_TE"]["median_s"] + out["launches"]["candidates_TIE"]["median_s"]
    out["effects_over_two_candidate_calls"] = out["launches"]["effects"]["median_s"] / two
    print("one breakdown / two candidate calls: %.2f" % out["effects_over_two_candidate_calls"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=8192)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "effects_tiktok.json"))
    run(ap.parse_args())
