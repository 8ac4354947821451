"""Cold-start items at the synthetic Tiktok shape:
  * the fold-in of Q = 4096 items (EliMRec.fold_in_items: host checks, upload, two linear_fwd_batched launches, the overlay table);
  * ops.rank_values for 8192 users x Q = 16 / 1024 / 4096 values (no read back, events around `--calls` calls) against two torch
    compositions on the same block: the sliced comparison `(block[:, None, :] >= v[:, :, None]).sum(-1)` in slices that fit
    1 GiB, and `torch.sort` of the rows plus `searchsorted`; the share of identical counts;
  * the whole report pass (ColdStartReport.evaluate; a fresh report each time) against ONE evaluator test pass;
  * with --bench PARENT.json THIS.json: the result lines of `bench.py --gpus 1 --steps 300 --warmup 50` at the parent commit and at
    this one, copied into the record.
Best and median of `--reps`. Dev tool. On a shared machine run every GPU step under its own time limit, chained:

    timeout -k 10 600 python tools/coldstart_time.py [--out profiles/coldstart_tiktok.json] [--bench PARENT.json THIS.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from _timing import _events, _setup, _wall  # noqa: E402


def torch_sliced(block, vals, budget=1 << 30):
    """#{j: block[b, j] >= vals[b, q]} by one broadcast comparison per slice of users (the bool block of a slice stays within budget)."""
    import torch
    B, I = block.shape
    Q = vals.shape[1]
    step = max(1, budget // (I * Q))
    out = torch.empty(B, Q, dtype=torch.int32, device=block.device)
    for a in range(0, B, step):
        out[a:a + step] = (block[a:a + step, None, :] >= vals[a:a + step, :, None]).sum(-1)
    return out


def torch_sorted(block, vals):
    """The same counts from sorted rows: I - searchsorted(sorted row, v, left)."""
    import torch
    srt = torch.sort(block, dim=1)[0]
    return (block.shape[1] - torch.searchsorted(srt, vals.contiguous(), right=False)).int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coldstart_tiktok.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--users", type=int, default=8192)
    ap.add_argument("--bench", nargs=2, metavar=("PARENT.json", "THIS.json"), default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from elimrec_amd import ops
    from elimrec_amd.evaluator import ColdStartReport
    cfg, ds, model = _setup()
    dev = torch.device("cuda:0")
    U, I = model.num_users, model.num_items
    model.predict_type = "TIE"
    train, test = ds.get_user_train_dict(), ds.get_user_test_dict()
    test_pass = _wall(lambda: model.test(), args.reps)
    result = {"shape": {"users": U, "items": I}, "device": torch.cuda.get_device_name(0), "reps": args.reps, "calls": args.calls,
              "segment": ops.RANK_VALUES_SEGMENT, "values_per_pass": ops.RANK_VALUES_PER_PASS,
              "evaluator_test_pass_s": {"best": test_pass[0], "median": test_pass[1]}, "runs": []}

    rng = np.random.default_rng(0)
    Q = 4096
    feats = {m: rng.standard_normal((Q, getattr(model, m + "_feat").shape[1])).astype(np.float32) for m in model._mods}
    fold = _wall(lambda: model.fold_in_items(feats), args.reps)
    result["fold_in"] = {"Q": Q, "s": {"best": fold[0], "median": fold[1]}}
    print(json.dumps(result["fold_in"]), flush=True)
    new = model.fold_in_items(feats)

    B = min(args.users, U)
    users = torch.arange(B, dtype=torch.int64, device=dev)
    lds = (I + 3) // 4 * 4
    block = torch.empty(B, lds, dtype=torch.float32, device=dev)[:, :I]
    model.predict_device(users, scores=block)
    all_vals = model.predict_new_items_device(users, new, torch.empty(B, Q, dtype=torch.float32, device=dev))
    for q in (16, 1024, 4096):
        vals = all_vals[:, :q].contiguous()
        ptr = torch.arange(B + 1, dtype=torch.int64, device=dev) * q
        out = torch.empty(B * q, dtype=torch.int32, device=dev)
        t = _events(lambda: ops.rank_values(block, ptr, vals.view(-1), out), args.calls, args.reps)
        t_sl = _events(lambda: torch_sliced(block, vals), 1, max(1, args.reps // 2))
        t_so = _events(lambda: torch_sorted(block, vals), 1, max(1, args.reps // 2))
        got = out.view(B, q)
        run = {"users": B, "Q": q, "s": {"best": t[0], "median": t[1]},
               "torch_sliced_s": {"best": t_sl[0], "median": t_sl[1]}, "torch_sort_searchsorted_s": {"best": t_so[0], "median": t_so[1]},
               "hip_over_sliced": t[0] / t_sl[0], "hip_over_sorted": t[0] / t_so[0],
               "share_identical_sliced": float((torch_sliced(block, vals) == got).float().mean()),
               "share_identical_sorted": float((torch_sorted(block, vals) == got).float().mean()),
               "note": "the timed call includes the host's check of val_ptr (a synchronising read of B + 1 entries)"}
        result["runs"].append(run)
        print(json.dumps(run), flush=True)

    def first_pass():
        return ColdStartReport(ds, train, test, cfg["topks"], group_view=[10, 30, 50, 100]).evaluate(model)

    setup = _wall(lambda: ColdStartReport(ds, train, test, cfg["topks"], group_view=[10, 30, 50, 100]), 1)
    whole = _wall(first_pass, max(1, args.reps // 2))
    rep = ColdStartReport(ds, train, test, cfg["topks"])
    result["report"] = {"cold_test_items": int(rep.items.size), "pairs": rep.num_pairs, "host_setup_s": setup[0],
                        "report_pass_with_setup_s": {"best": whole[0], "median": whole[1]},
                        "report_over_test_pass": (whole[0] - setup[0]) / test_pass[0], "table": first_pass()[1]}
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
