"""Cold-start users at the synthetic Tiktok shape:
  * the fold-in of 8192 test users from their training histories: the kernel alone (elimrec_segment_row_sum on resident lists,
    events around `--calls` launches), ops.segment_row_sum with its host checks, and the whole EliMRec.fold_in_users call (host
    checks, weights, upload, the sum, the projections, the overlay table);
  * the kernel's gathered GB/s (entries x 4 C bytes) beside the random-row gather rate MI355X_MICROARCH.md quotes for whole rows
    gathered into registers (5.5-5.8 TB/s beyond the Infinity Cache; 7.4-8.6 TB/s into LDS for 38-151 MB tables -- the regime of
    this measurement: the 78 MB item block is gathered in back-to-back launches and stays in the Infinity Cache);
  * the torch composition torch.sparse.mm(W_csr, Out[U:]) on the same inputs (an fp32 sum), and the share of its rows and of the
    kernel's rows within the float64 bound 2^-23 |want| + n 2^-50 sum |w x| of a float64 torch reference;
  * the whole report pass (NewUserReport.evaluate; a fresh report each time) against ONE evaluator test pass;
  * with --bench PARENT.json THIS.json: the result lines of `bench.py --gpus 1 --steps 300 --warmup 50` at the parent commit and at
    this one, copied into the record.
Best and median of `--reps`. Dev tool. On a shared machine run every GPU step under its own time limit, chained:

    timeout -k 10 600 python tools/newuser_time.py [--out profiles/newuser_tiktok.json] [--bench PARENT.json THIS.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from _timing import _events, _setup, _wall  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "newuser_tiktok.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--users", type=int, default=8192)
    ap.add_argument("--bench", nargs=2, metavar=("PARENT.json", "THIS.json"), default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from elimrec_amd import _lib, ops, reports
    from elimrec_amd.evaluator import NewUserReport
    cfg, ds, model = _setup()
    dev = torch.device("cuda:0")
    U, I, C = model.num_users, model.num_items, model.C
    model.predict_type = "TIE"
    train, test = ds.get_user_train_dict(), ds.get_user_test_dict()
    test_pass = _wall(lambda: model.test(), args.reps)
    result = {"shape": {"users": U, "items": I, "C": C}, "device": torch.cuda.get_device_name(0), "reps": args.reps, "calls": args.calls,
              "chunk": ops.FOLDIN_CHUNK, "evaluator_test_pass_s": {"best": test_pass[0], "median": test_pass[1]}}

    users = [u for u in test if len(train.get(u, []))][:args.users]
    hist = [list(train[u]) for u in users]
    Q = len(hist)
    whole = _wall(lambda: model.fold_in_users(hist), args.reps)
    new = model.fold_in_users(hist)
    ptr, flat = new.hist_ptr_host, new.hist_flat
    lens = np.diff(ptr)
    w = reports.fold_in_weights(str(cfg["adj_type"]), ptr, flat, reports.item_train_counts(train, I))
    Out = model._ws["Out"]
    out = torch.empty(Q, C, dtype=torch.float32, device=dev)
    w_t, rows_t, ptr_t = torch.from_numpy(w).to(dev), new.hist_items, new.hist_ptr
    lib = _lib.load()

    def kernel():
        _lib.check(lib.elimrec_segment_row_sum(Out.data_ptr(), U + I, C, Out.stride(0), U, ptr_t.data_ptr(), rows_t.data_ptr(), w_t.data_ptr(),
                                               Q, int(flat.size), out.data_ptr(), C, torch.cuda.current_stream().cuda_stream), "segment_row_sum")

    t_k = _events(kernel, args.calls, args.reps)
    t_op = _wall(lambda: ops.segment_row_sum(Out, ptr, flat.astype(np.int32), w, out, row_offset=U), args.reps)
    gathered = float(flat.size) * 4 * C
    # the torch composition: one CSR matrix [Q x I] of the weights times the item rows of Out
    seg = torch.repeat_interleave(torch.arange(Q, device=dev), torch.from_numpy(lens).to(dev))
    W_csr = torch.sparse_coo_tensor(torch.stack((seg, rows_t[:flat.size].long())), w_t, size=(Q, I)).coalesce().to_sparse_csr()
    items = Out[U:].contiguous()
    t_sp = _events(lambda: torch.sparse.mm(W_csr, items), args.calls, args.reps)
    got_sp = torch.sparse.mm(W_csr, items)
    kernel()
    # float64 reference on the device: index_add_ of the float64 products in list order
    share = {"kernel": 0, "torch_sparse_mm": 0}
    step = 1024
    for a in range(0, Q, step):
        b = min(Q, a + step)
        lo, hi = int(ptr[a]), int(ptr[b])
        prod = w_t[lo:hi].double()[:, None] * items[rows_t[lo:hi].long()].double()
        want = torch.zeros(b - a, C, dtype=torch.float64, device=dev).index_add_(0, seg[lo:hi] - a, prod)
        mag = torch.zeros(b - a, C, dtype=torch.float64, device=dev).index_add_(0, seg[lo:hi] - a, prod.abs())
        bound = 2.0 ** -23 * want.abs() + torch.from_numpy(lens[a:b]).to(dev).double()[:, None] * 2.0 ** -50 * mag
        share["kernel"] += int(((out[a:b].double() - want).abs() <= bound).all(1).sum())
        share["torch_sparse_mm"] += int(((got_sp[a:b].double() - want).abs() <= bound).all(1).sum())
    result["fold_in"] = {
        "users": Q, "entries": int(flat.size), "history_len": {"mean": float(lens.mean()), "median": float(np.median(lens)), "max": int(lens.max())},
        "kernel_s": {"best": t_k[0], "median": t_k[1]}, "kernel_gathered_GBps": gathered / t_k[0] * 1e-9,
        "guide_random_row_gather_GBps": {"registers_beyond_infinity_cache": [5500, 5800], "lds_38_to_151_MB_table": [7400, 8600]},
        "ops_segment_row_sum_with_host_checks_s": {"best": t_op[0], "median": t_op[1]},
        "fold_in_users_whole_call_s": {"best": whole[0], "median": whole[1]},
        "torch_sparse_mm_s": {"best": t_sp[0], "median": t_sp[1]}, "hip_over_torch": t_k[0] / t_sp[0],
        "share_rows_within_float64_bound": {k: v / float(Q) for k, v in share.items()},
        "note": "one workgroup per user: a history shorter than one chunk keeps one of the four waves busy"}
    print(json.dumps(result["fold_in"]), flush=True)

    ks = [int(k) for k in cfg["topks"]]

    def first_pass():
        rep = NewUserReport(ds, train, test, ks, group_view=[10, 30, 50, 100], metric=cfg["metric"])
        return rep.evaluate(model)

    setup = _wall(lambda: NewUserReport(ds, train, test, ks, group_view=[10, 30, 50, 100], metric=cfg["metric"]), 1)
    whole_rep = _wall(first_pass, max(1, args.reps // 2))
    result["report"] = {"users": len(NewUserReport(ds, train, test, ks).users), "host_setup_s": setup[0],
                        "report_pass_with_setup_s": {"best": whole_rep[0], "median": whole_rep[1]},
                        "report_over_test_pass": (whole_rep[0] - setup[0]) / test_pass[0], "table": first_pass()[1]}
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
