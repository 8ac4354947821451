"""Calibrated re-ranking at the Tiktok shape beside a torch composition of the same greedy rule: after three training steps, over
ALL test users' top-N pools (predict_device, TIE, train items masked), the items classed into C = 5 popularity buckets
(reports.item_classes, item_group_view [1, 10, 100]: cold, (0,1], (1,10], (10,100], (100,inf)) and every user's target the class
shares of their training items, for (N, K) = (40, 10) and (200, 50) at lambda 0.5,
  * the re-rank launch alone (EliMRec.calibrate_device, csrc/calibrate.hip; events around `--calls` calls);
  * the yardstick: K rounds on the same GPU, in blocks of 8192 users, all in float64 -- one-hot counts of the picks so far, per
    class the KL of the target against the smoothed shares with one more item of that class, a gather of the value of every
    position's class, argmax of lam rel - (1 - lam) KL over the positions not picked yet -- and the share of users whose lists agree
    entirely;
  * the whole report pass (CalibrationReport.evaluate: K = 10 of the top-40 pools at four lambdas, four user groups; wall-clock
    around a device synchronisation) against ONE evaluator test pass (model.test());
  * with --bench PARENT.json THIS.json: the result lines of `bench.py --gpus 1 --steps 300 --warmup 50` at the parent commit and at
    this one, run beside each other, copied into the record (the step's code is untouched: the two agree within their spread).
Best and median of `--reps`. Dev tool.

    python tools/calibrate_time.py [--out profiles/calibrate_tiktok.json] [--bench PARENT.json THIS.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from _timing import _events, _setup, _wall  # noqa: E402

LAM, SMOOTH, VIEW = 0.5, 0.01, [1, 10, 100]


def torch_calibrate(idx, val, class_of, target, K, lam, smooth, block=8192):
    """The greedy rule as torch ops in float64: int64 [B x K] pool positions (pools without unlisted entries)."""
    import torch
    out = []
    for a in range(0, idx.shape[0], block):
        cls = class_of[idx[a:a + block].long()].long()
        s, p = val[a:a + block].double(), target[a:a + block].double()
        B, N = cls.shape
        C = p.shape[1]
        ar = torch.arange(B, device=cls.device)
        lo, hi = s.min(dim=1, keepdim=True)[0], s.max(dim=1, keepdim=True)[0]
        rel = torch.where(hi > lo, (s - lo) / (hi - lo), torch.zeros_like(s))
        on = p > 0
        safe = torch.where(on, p, torch.ones_like(p))
        counts = torch.zeros(B, C, dtype=torch.float64, device=cls.device)
        eye = torch.eye(C, dtype=torch.float64, device=cls.device)
        taken = torch.zeros(B, N, dtype=torch.bool, device=cls.device)
        picks = torch.empty(B, K, dtype=torch.int64, device=cls.device)
        for t in range(K):
            q = (counts[:, None, :] + eye[None, :, :]) / float(t + 1)                     # [B x C' x C]
            term = safe[:, None, :] * torch.log(safe[:, None, :] / ((1.0 - smooth) * q + smooth * safe[:, None, :]))
            kl = torch.where(on[:, None, :], term, torch.zeros_like(term)).sum(dim=2)     # [B x C']
            obj = (lam * rel - (1.0 - lam) * kl.gather(1, cls)).masked_fill(taken, float("-inf"))
            pick = obj.argmax(dim=1)
            picks[:, t] = pick
            taken[ar, pick] = True
            counts[ar, cls[ar, pick]] += 1.0
        out.append(picks)
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calibrate_tiktok.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--bench", nargs=2, metavar=("PARENT.json", "THIS.json"), default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from elimrec_amd import ops
    from elimrec_amd.evaluator import CalibrationReport
    from elimrec_amd.reports import lists_csr
    cfg, ds, model = _setup()
    dev = "cuda:0"
    U, I, d = model.num_users, model.num_items, model.latent_dim
    model.predict_type = "TIE"
    train, test = ds.get_user_train_dict(), ds.get_user_test_dict()
    users = list(test.keys())
    test_pass = _wall(lambda: model.test(), args.reps)
    report = CalibrationReport(ds, train, test, 10, VIEW, pool=40, smooth=SMOOTH, group_view=[10, 30, 50, 100])
    C = report.num_classes
    result = {"shape": {"users": U, "items": I, "recdim": d, "test_users": len(users), "classes": C}, "lambda": LAM, "smooth": SMOOTH,
              "item_group_view": VIEW, "device": torch.cuda.get_device_name(0), "reps": args.reps, "calls": args.calls,
              "evaluator_test_pass_s": {"best": test_pass[0], "median": test_pass[1]}, "runs": []}
    train_ptr, train_items = lists_csr(users, train, dev)
    users_t = torch.as_tensor(np.asarray(users, dtype=np.int64)).to(dev)
    class_of = torch.from_numpy(report.class_of).to(dev)
    target = report.targets(dev)
    shares = _events(lambda: ops.class_shares(train_ptr, train_items, class_of, C, target), args.calls, args.reps)
    result["class_shares_s"] = {"best": shares[0], "median": shares[1], "entries": int(train_items.numel())}
    for N, K in ((40, 10), (200, 50)):
        idx, val = model.predict_device(users_t, top_k=N, train_ptr=train_ptr, train_items=train_items)
        B = idx.shape[0]
        out = [torch.empty(B, K, dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.float32)]
        hip = _events(lambda: model.calibrate_device(idx, val, K, LAM, class_of, target, smooth=SMOOTH, out_idx=out[0], out_pos=out[1],
                                                     out_val=out[2]), args.calls, args.reps)
        ref = _wall(lambda: torch_calibrate(idx, val, class_of, target, K, LAM, SMOOTH), max(1, args.reps // 2))
        full = bool((idx >= 0).all())
        same = float((torch_calibrate(idx, val, class_of, target, K, LAM, SMOOTH) == out[1].long()).all(dim=1).float().mean().item()) if full else None
        result["runs"].append({
            "N": N, "K": K, "C": C, "lists": B,
            "calibrate_rerank_s": {"best": hip[0], "median": hip[1]},
            "torch_rounds_s": {"best": ref[0], "median": ref[1]},
            "hip_over_torch": hip[0] / ref[0],
            "share_of_identical_lists": same,
        })
        print(json.dumps(result["runs"][-1]), flush=True)
    whole = _wall(lambda: report.evaluate(model), args.reps)
    result["report"] = {"K": report.top_k, "pool": report.pool, "lambdas": list(report.lambdas),
                        "report_pass_s": {"best": whole[0], "median": whole[1]}, "report_over_test_pass": whole[0] / test_pass[0],
                        "table": report.evaluate(model)[1]}
    print(json.dumps(result["report"]), flush=True)
    if args.bench:
        lines = []
        for path in args.bench:
            with open(path) as f:
                lines.append(json.loads([ln for ln in f.read().splitlines() if ln.strip().startswith("{")][-1]))
        result["bench_gpus1_steps300_warmup50"] = {"parent": lines[0], "this": lines[1]}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
