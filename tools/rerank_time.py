"""Diversified re-ranking at the Tiktok shape beside a torch composition of the same greedy rule: after three training steps, over
ALL test users' top-N pools (predict_device, TIE, train items masked), for (N, K) = (40, 10), (200, 50), (256, 256) at lambda 0.7,
  * the re-rank launch alone (EliMRec.rerank_device, csrc/rerank.hip; events around `--calls` calls) and which form (N, d) selects;
  * the yardstick: K rounds of torch.bmm + max over gathered, normalised rows on the same GPU, in blocks of 8192 users -- R =
    normalize(T[pool]) [B x N x d] once, then per round cos = bmm(R, R[picked]), pen = max(pen, cos), argmax of
    lam rel - (1 - lam) pen over the positions not picked yet -- and the share of users whose lists agree entirely (the two
    differ where objectives tie within fp32 rounding);
  * the launch whose candidates' rows stay in global memory at its largest shape, N = K = d = 256, over a random table of the
    catalogue's size (the model's recdim is 64);
  * the whole report pass (DiversifyReport.evaluate: K = 10 of the top-40 pools at four lambdas; wall-clock around a device
    synchronisation) against ONE evaluator test pass (model.test()).
Best and median of `--reps`. Dev tool.

    python tools/rerank_time.py [--out profiles/rerank_tiktok.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from _timing import _events, _setup, _wall  # noqa: E402

LAM = 0.7


def torch_mmr(T, idx, val, K, lam, block=8192):
    """The greedy rule as torch ops: int64 [B x K] pool positions (pools without unlisted entries)."""
    import torch
    import torch.nn.functional as F
    out = []
    for a in range(0, idx.shape[0], block):
        ids, s = idx[a:a + block].long(), val[a:a + block]
        B, N = ids.shape
        ar = torch.arange(B, device=ids.device)
        R = F.normalize(T, dim=1)[ids]
        lo, hi = s.min(dim=1, keepdim=True)[0], s.max(dim=1, keepdim=True)[0]
        rel = torch.where(hi > lo, (s - lo) / (hi - lo), torch.zeros_like(s))
        pen = torch.zeros_like(s)
        taken = torch.zeros(B, N, dtype=torch.bool, device=ids.device)
        picks = torch.empty(B, K, dtype=torch.int64, device=ids.device)
        for t in range(K):
            obj = (lam * rel - (1.0 - lam) * pen).masked_fill(taken, float("-inf"))
            p = obj.argmax(dim=1)
            picks[:, t] = p
            taken[ar, p] = True
            cos = torch.bmm(R, R[ar, p][:, :, None])[:, :, 0]
            pen = cos if t == 0 else torch.maximum(pen, cos)
        out.append(picks)
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rerank_tiktok.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    from elimrec_amd import ops
    from elimrec_amd.evaluator import DiversifyReport
    from elimrec_amd.reports import lists_csr
    cfg, ds, model = _setup()
    dev = "cuda:0"
    U, I, d = model.num_users, model.num_items, model.latent_dim
    model.predict_type = "TIE"
    train, test = ds.get_user_train_dict(), ds.get_user_test_dict()
    users = list(test.keys())
    test_pass = _wall(lambda: model.test(), args.reps)
    result = {"shape": {"users": U, "items": I, "recdim": d, "test_users": len(users)}, "lambda": LAM,
              "device": torch.cuda.get_device_name(0), "reps": args.reps, "calls": args.calls,
              "evaluator_test_pass_s": {"best": test_pass[0], "median": test_pass[1]}, "runs": []}
    train_ptr, train_items = lists_csr(users, train, dev)
    users_t = torch.as_tensor(np.asarray(users, dtype=np.int64)).to(dev)
    T = model._ws["Y"][U:U + I, :d]
    for N, K in ((40, 10), (200, 50), (256, 256)):
        idx, val = model.predict_device(users_t, top_k=N, train_ptr=train_ptr, train_items=train_items)
        B = idx.shape[0]
        out = [torch.empty(B, K, dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.float32)]
        hip = _events(lambda: model.rerank_device(idx, val, K, LAM, out_idx=out[0], out_pos=out[1], out_val=out[2]), args.calls, args.reps)
        ref = _wall(lambda: torch_mmr(T, idx, val, K, LAM), max(1, args.reps // 2))
        full = bool((idx >= 0).all())
        same = float((torch_mmr(T, idx, val, K, LAM) == out[1].long()).all(dim=1).float().mean().item()) if full else None
        result["runs"].append({
            "N": N, "K": K, "d": d, "lists": B, "rows_in_lds": ops.mmr_rows_in_lds(N, d),
            "mmr_rerank_s": {"best": hip[0], "median": hip[1]},
            "mmr_rerank_gflops": 2.0 * B * N * (K - 1) * d / hip[0] * 1e-9,        # every step scores all N positions at most
            "torch_rounds_s": {"best": ref[0], "median": ref[1]},
            "hip_over_torch": hip[0] / ref[0],
            "share_of_identical_lists": same,
        })
        print(json.dumps(result["runs"][-1]), flush=True)
    # the largest shape of the form that keeps the candidates' rows in global memory
    N = K = D = 256
    g = torch.Generator(device=dev).manual_seed(1)
    wide = torch.randn(I, D, device=dev, generator=g)
    sq = (wide.double() ** 2).sum(dim=1).float()
    B = len(users)
    idx = torch.stack([torch.randperm(I, device=dev, generator=g)[:N] for _ in range(64)]).int().repeat((B + 63) // 64, 1)[:B].contiguous()
    val = torch.rand(B, N, device=dev, generator=g).sort(dim=1, descending=True)[0].contiguous()
    out = torch.empty(B, K, dtype=torch.int32, device=dev)
    hip = _events(lambda: ops.mmr_rerank(wide, sq, idx, val, K, LAM, out), 1, args.reps)
    result["global_rows_largest"] = {"N": N, "K": K, "d": D, "lists": B, "rows_in_lds": ops.mmr_rows_in_lds(N, D),
                                     "mmr_rerank_s": {"best": hip[0], "median": hip[1]},
                                     "mmr_rerank_gflops": 2.0 * B * N * (K - 1) * D / hip[0] * 1e-9,
                                     "rows_read_gbs": B * (K - 1) * N * D * 4.0 / hip[0] * 1e-9}
    print(json.dumps(result["global_rows_largest"]), flush=True)
    report = DiversifyReport(ds, train, test, 10, pool=40, group_view=[10, 30, 50, 100])
    whole = _wall(lambda: report.evaluate(model), args.reps)
    result["report"] = {"K": report.top_k, "pool": report.pool, "lambdas": list(report.lambdas),
                        "report_pass_s": {"best": whole[0], "median": whole[1]}, "report_over_test_pass": whole[0] / test_pass[0],
                        "table": report.evaluate(model)[1]}
    print(json.dumps(result["report"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
