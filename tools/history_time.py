"""History support at the Tiktok shape: after three training steps, the test users' TIE top-K lists (K = 10, then 50) against
their training histories, top = 3, fused space,
  * the launch alone (EliMRec.history_support_device, csrc/history.hip; events around `--calls` calls) and the rate of the rows it
    gathers -- per user ceil(K / 16) walks of the history plus the K target rows, d floats each (TB/s; the table fits the caches,
    this is not an HBM rate);
  * the yardstick: the same four outputs as torch ops on the same GPU, in blocks of `--block` users -- the histories gathered
    padded to the block's longest, F.normalize, bmm against the normalized targets, a -inf mask over the padding and the target
    itself, topk, a masked mean -- and the share of (pair, slot) entries on which the two name the same item (they differ where
    scores tie within fp32 rounding);
  * the whole report pass (reports.HistoryReport.evaluate: the lists, one launch per space and user block, the group means)
    against one evaluator test pass.
Best and median of `--reps`. Dev tool.

    python tools/history_time.py [--out profiles/history_tiktok.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from _timing import _events, _setup, _wall  # noqa: E402


def torch_support(T, lists, hptr, hitems, top, block):
    """(idx int64 [B x K x top], val, cnt, mean) of the fused block T [I x d] as torch ops; segment b of the CSR is row b's."""
    import torch
    import torch.nn.functional as F
    B, K = lists.shape
    lens = hptr[1:] - hptr[:-1]
    out = [[], [], [], []]
    for a in range(0, B, block):
        b = min(B, a + block)
        ln = lens[a:b]
        H = max(int(ln.max().item()), 1)
        col = torch.arange(H, device=T.device)[None, :]
        valid = col < ln[:, None]
        ids = hitems[(hptr[a:b, None] + col).clamp(max=hitems.numel() - 1)].long().masked_fill(~valid, 0)
        rows = F.normalize(T[ids], dim=2)
        tg = lists[a:b].long()
        s = torch.bmm(F.normalize(T[tg.clamp(min=0)], dim=2), rows.transpose(1, 2))
        listed = valid[:, None, :] & (ids[:, None, :] != tg[:, :, None]) & (tg >= 0)[:, :, None]
        s = s.masked_fill(~listed, float("-inf"))
        k = min(top, H)
        v, p = s.topk(k, dim=2)
        i = torch.gather(ids[:, None, :].expand(-1, K, -1), 2, p).masked_fill(torch.isneginf(v), -1)
        if k < top:
            v = F.pad(v, (0, top - k), value=float("-inf"))
            i = F.pad(i, (0, top - k), value=-1)
        c = listed.sum(dim=2)
        m = s.masked_fill(~listed, 0.0).double().sum(dim=2) / c.double()
        for o, x in zip(out, (i, v, c.int(), m.float())):
            o.append(x)
    return [torch.cat(o) for o in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "history_tiktok.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--block", type=int, default=512)
    args = ap.parse_args()
    import numpy as np
    import torch
    from elimrec_amd.evaluator import HistoryReport
    cfg, ds, model = _setup()
    dev = "cuda:0"
    U, I, d = model.num_users, model.num_items, model.latent_dim
    model.predict_type = "TIE"
    train, test = ds.get_user_train_dict(), ds.get_user_test_dict()
    test_pass = _wall(lambda: model.test(), args.reps)
    top = 3
    result = {"shape": {"users": U, "items": I, "recdim": d, "test_users": len(test)}, "space": "fused", "top": top,
              "predict_type": "TIE", "device": torch.cuda.get_device_name(0), "reps": args.reps, "calls": args.calls,
              "torch_block_users": args.block, "evaluator_test_pass_s": {"best": test_pass[0], "median": test_pass[1]}, "runs": []}
    for K in (10, 50):
        report = HistoryReport(ds, train, test, K, top=top, group_view=[10, 30, 50, 100])
        res = report._resident(torch.device(dev))
        hist = res["hist"]
        n = len(report.users)
        lists = torch.cat([idx for _, _, _, idx in report.top_lists(model, report.users, K, report.block_users, report.tie_order)])
        at = torch.arange(n, dtype=torch.int64, device=dev)
        out = model.history_support_device(at, lists, hist, top=top)
        launch = _events(lambda: model.history_support_device(at, lists, hist, top, "fused", True, *out), args.calls, args.reps)
        lens = np.asarray(hist.sizes, dtype=np.int64)
        walks = -(-K // 16)
        gathered = (float(lens.sum()) * walks + n * K) * d * 4.0
        T = model._ws["Y"][U:U + I, :d]
        ref = _wall(lambda: torch_support(T, lists, hist.ptr, hist.items, top, args.block), max(1, args.reps // 2))
        want = torch_support(T, lists, hist.ptr, hist.items, top, args.block)
        same = float((want[0] == out[0].long()).float().mean().item())
        same_cnt = bool(torch.equal(want[2], out[2]))
        diff = float((want[1] - out[1]).abs().nan_to_num(posinf=0.0)[out[0] >= 0].max().item())
        whole = _wall(lambda: report.evaluate(model), args.reps)
        result["runs"].append({
            "K": K, "pairs": n * K, "history_entries": int(lens.sum()), "longest_history": int(lens.max()),
            "history_support_s": {"best": launch[0], "median": launch[1]},
            "gathered_rows_tbs": gathered / launch[0] * 1e-12,
            "scored_pairs_gflops": 2.0 * float(lens.sum()) * K * d / launch[0] * 1e-9,
            "torch_composition_s": {"best": ref[0], "median": ref[1]}, "hip_over_torch": launch[0] / ref[0],
            "share_of_identical_slots": same, "counts_identical": same_cnt, "max_abs_value_diff_to_torch": diff,
            "report_pass_s": {"best": whole[0], "median": whole[1]}, "report_over_test_pass": whole[0] / test_pass[0],
        })
        print(json.dumps(result["runs"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
