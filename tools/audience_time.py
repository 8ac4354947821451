"""Audience lists at the Tiktok shape beside the torch-visible composition of the same lists: after three training steps, for
Q = 8192 query items, K = 10 and 50, under TE and TIE,
  * the launch pair alone (ops.audience_topk: the chunk kernel + topk_merge; TIE's row sums are cached, as EliMRec.audience_device
    keeps them; events around `--calls` calls);
  * the composition: EliMRec.predict_candidates_device with EVERY user listing the same items, in item blocks of `--block` (the
    [U x block] score block stays within 2 GiB), then torch.topk(dim=0) per block -- its TIE pass 1 runs per call, as that API does;
  * the share of items whose K ids are identical in both, the algorithmic TFLOP/s of the kernel (2 U Q (1 + S) d), and the bytes of
    the score block the composition writes and the kernel does not;
  * the whole report pass (AudienceReport.audience_rows + evaluate) against ONE evaluator test pass (model.test()).
Best and median of `--reps`. Dev tool.

    python tools/audience_time.py [--out profiles/audience_tiktok.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from _timing import _events, _setup, _wall  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audience_tiktok.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--block", type=int, default=2048)
    args = ap.parse_args()
    import numpy as np
    import torch
    from elimrec_amd import ops
    from elimrec_amd.evaluator import AudienceReport
    cfg, ds, model = _setup()
    dev = "cuda:0"
    U, I, d, S = model.num_users, model.num_items, model.latent_dim, model.S
    Q = min(args.queries, I)
    block = min(args.block, Q, (2 << 30) // (4 * U))
    items = np.random.default_rng(0).permutation(I)[:Q].astype(np.int32)
    train, test = ds.get_user_train_dict(), ds.get_user_test_dict()
    model.predict_type = "TIE"
    test_pass = _wall(lambda: model.test(), args.reps)
    result = {"shape": {"users": U, "items": I, "recdim": d, "heads": S, "queries": Q, "composition_item_block": block},
              "device": torch.cuda.get_device_name(0), "reps": args.reps, "calls": args.calls,
              "evaluator_test_pass_s": {"best": test_pass[0], "median": test_pass[1]}, "runs": []}
    users = torch.arange(U, dtype=torch.int64, device=dev)
    ptr = torch.arange(U + 1, dtype=torch.int64, device=dev) * block
    scores = torch.empty(U, block, dtype=torch.float32, device=dev)
    items_d = torch.from_numpy(items).to(dev)
    for K in (10, 50):
        query = ops.AudienceQuery(items, I, U, dev)
        idx = torch.empty(Q, K, dtype=torch.int32, device=dev)
        val = torch.empty(Q, K, dtype=torch.float32, device=dev)
        comp_idx = torch.empty(Q, K, dtype=torch.int64, device=dev)
        for ptype in ("TE", "TIE"):
            model.predict_type = ptype
            hip = _events(lambda: model.audience_device(query, K, idx, val), args.calls, args.reps)

            def composition():
                for a in range(0, Q, block):
                    blk = items_d[a:a + block]
                    if blk.numel() < block:                  # the last, shorter block: padded with its first item
                        blk = torch.cat((blk, blk[:1].expand(block - blk.numel())))
                    model.predict_candidates_device(users, ptr, blk.repeat(U), scores)
                    top = torch.topk(scores, K, dim=0).indices.t()
                    comp_idx[a:a + block] = top[:min(block, Q - a)]
            ref = _events(composition, 1, args.reps)
            same = float((comp_idx == idx.long()).all(dim=1).double().mean().item())
            report = AudienceReport(ds, train, test, K, item_group_view=[1, 10, 100])
            whole = _wall(lambda: report.evaluate(model), args.reps)
            result["runs"].append({
                "K": K, "predict_type": ptype,
                "audience_topk_s": {"best": hip[0], "median": hip[1]},
                "audience_topk_tflops": 2.0 * U * Q * (1 + S) * d / hip[1] * 1e-12,
                "composition_s": {"best": ref[0], "median": ref[1]},
                "hip_over_composition": hip[1] / ref[1],
                "identical_lists_share": same,
                "score_block_bytes_not_written": 4 * U * Q,
                "report_items": len(report.items),
                "report_pass_s": {"best": whole[0], "median": whole[1]},
                "report_over_test_pass": whole[1] / test_pass[1],
            })
            print(json.dumps(result["runs"][-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
