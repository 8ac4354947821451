"""The EASE baseline at the synthetic Tiktok shape (or, with --items N, over the N most popular items: the largest square that
fits), each part beside its yardstick on the same GPU:
  * the Gram build (ops.gram_counts), the inverse (ops.spd_inverse) and the ranking pass (ops.ease_topk over all test users);
  * the inverse's achieved float64 TFLOP/s -- n^3 operations: the upper block triangle, n / 64 pivot blocks, 2 x 64 per element and
    block -- beside the microarchitecture guide's peak (the guide states no float64 matrix figure; its FP32 matrix peak, 157.3
    TFLOPS, is recorded for scale) and the sweep's bytes (16 per element of the upper triangle and pivot block) per second;
  * the ranking pass's GB/s over the bytes of P it must read (sum over users of |history| x I x 8);
  * the inverse against torch.linalg.inv on the same float64 matrix (skipped with --no-torch-inv), with max|P - P_torch|;
  * the whole `ease` report pass (lists + table; the fit kept) and fit + report against ONE evaluator test pass;
  * with --bench PARENT.json THIS.json [...]: the result lines of bench.py at the parent commit and at this one, copied in.
The inverse runs once per clock (no warm-up repeat: it is seconds long). Dev tool. On a shared machine run every GPU step under its
own time limit:

    timeout -k 10 900 python tools/ease_time.py [--out profiles/ease_tiktok.json] [--items N] [--bench PARENT.json THIS.json ...]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from _timing import _events, _setup, _wall  # noqa: E402

GUIDE_FP32_MATRIX_PEAK_TFLOPS = 157.3


def once(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ease_tiktok.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--l2", type=float, default=500.0)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--items", type=int, default=0, help="time the kernels over the N most popular items only (0: the whole catalogue)")
    ap.add_argument("--no-torch-inv", action="store_true")
    ap.add_argument("--bench", nargs="+", metavar="JSON", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from elimrec_amd import ops
    from elimrec_amd.evaluator import BaselineReport
    cfg, ds, model = _setup()
    dev = torch.device("cuda:0")
    U, I = model.num_users, model.num_items
    model.predict_type = "TIE"
    train, test = ds.get_user_train_dict(), ds.get_user_test_dict()
    test_pass = _wall(lambda: model.test(), args.reps)
    result = {"shape": {"users": U, "items": I}, "device": torch.cuda.get_device_name(0), "l2": args.l2, "K": args.K,
              "block": ops.EASE_BLOCK, "evaluator_test_pass_s": {"best": test_pass[0], "median": test_pass[1]}}

    def dump():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")

    # the kernels alone, over the whole catalogue or its n most popular items (ids renumbered by popularity)
    n = I if not args.items else min(I, args.items)
    counts = np.bincount(np.concatenate([np.unique(v) for v in train.values()]), minlength=I)
    keep = np.argsort(-counts, kind="stable")[:n]
    new_id = np.full(I, -1, dtype=np.int64)
    new_id[keep] = np.arange(n)
    sub = {u: np.unique(new_id[np.asarray(v, dtype=np.int64)][new_id[np.asarray(v, dtype=np.int64)] >= 0]) for u, v in train.items()}
    index = ops.CooccurIndex.from_train(sub, U, n, "item", dev)
    G = torch.empty(n, n, dtype=torch.float64, device=dev)
    t_gram = _events(lambda: ops.gram_counts(index, args.l2, G), 1, args.reps)
    P = G.clone()
    ws = torch.empty(ops.spd_inverse_workspace(n), dtype=torch.uint8, device=dev)
    t_inv, pivot = once(lambda: ops.spd_inverse(P, ws))
    flops, blocks = float(n) ** 3, -(-n // ops.EASE_BLOCK)
    result["kernels"] = {"items": n, "whole_catalogue": n == I, "edges": index.n_edges, "matrix_bytes": 8 * n * n, "workspace_bytes": ws.numel(),
                         "gram_s": {"best": t_gram[0], "median": t_gram[1]}, "gram_GBps_over_matrix_bytes": 8 * n * n / t_gram[0] / 1e9,
                         "inverse_s": t_inv, "pivot_min": pivot, "inverse_flop": flops, "inverse_f64_TFLOPs": flops / t_inv / 1e12,
                         "guide_fp64_matrix_peak": None, "guide_fp32_matrix_peak_TFLOPs": GUIDE_FP32_MATRIX_PEAK_TFLOPS,
                         "inverse_sweep_bytes": 8.0 * n * n * blocks, "inverse_TBps": 8.0 * n * n * blocks / t_inv / 1e12}
    print(json.dumps(result["kernels"]), flush=True)
    dump()
    if not args.no_torch_inv:
        try:
            t_torch, Pt = once(lambda: torch.linalg.inv(G))
            result["kernels"]["torch_linalg_inv_s"] = t_torch
            result["kernels"]["hip_over_torch"] = t_inv / t_torch
            result["kernels"]["max_abs_diff_to_torch"] = float((P - Pt).abs().max().item())
            result["kernels"]["max_abs_P"] = float(P.abs().max().item())
            del Pt
        except RuntimeError as e:        # the library call needs the matrix several times over: out of memory is a result, too
            result["kernels"]["torch_linalg_inv_error"] = str(e).splitlines()[0][:200]
            torch.cuda.empty_cache()
        print(json.dumps({k: v for k, v in result["kernels"].items() if "torch" in k}), flush=True)
        dump()
    del G

    users = np.asarray(sorted(test), dtype=np.int64)
    hptr, hflat, hlen = ops.ragged([sub.get(int(u), np.zeros(0, dtype=np.int64)) for u in users], cast=int)
    hist = ops.HistoryIndex(hptr, hflat, dev, n_items=n)
    every = np.arange(users.size, dtype=np.int64)
    idx = torch.empty(users.size, args.K, dtype=torch.int32, device=dev)
    val = torch.empty(users.size, args.K, dtype=torch.float32, device=dev)
    tws = torch.empty(ops.ease_topk_workspace(users.size, n, args.K), dtype=torch.uint8, device=dev)
    t_rank = _events(lambda: ops.ease_topk(P, hist, every, args.K, idx, val, workspace=tws), 1, args.reps)
    must = float(hlen.sum()) * n * 8
    result["ranking"] = {"users": int(users.size), "history_entries": int(hlen.sum()), "s": {"best": t_rank[0], "median": t_rank[1]},
                         "bytes_of_P_read": must, "GBps": must / t_rank[0] / 1e9}
    print(json.dumps(result["ranking"]), flush=True)
    dump()
    del P, ws, tws

    # the fit and the report pass over the whole catalogue
    if n == I:
        t_fit, fit = once(lambda: model.fit_ease(args.l2))

        def report():
            return BaselineReport(ds, train, test, cfg["topks"], metric=cfg["metric"], sources=("ease",), group_view=[10, 30, 50, 100], l2=args.l2)
        setup = _wall(report, 1)
        whole = _wall(lambda: report().evaluate(model), max(1, args.reps // 2))
        result["report"] = {"fit_s": t_fit, "fit_bytes": fit.bytes, "host_setup_s": setup[0],
                            "report_pass_with_setup_s": {"best": whole[0], "median": whole[1]},
                            "report_over_test_pass": (whole[0] - setup[0]) / test_pass[0],
                            "fit_plus_report_over_test_pass": (t_fit + whole[0] - setup[0]) / test_pass[0], "table": report().evaluate(model)[1]}
        print(json.dumps(result["report"]), flush=True)
    if args.bench:
        lines = []
        for path in args.bench:
            with open(path) as f:
                lines.append(json.loads([ln for ln in f.read().splitlines() if ln.strip().startswith("{")][-1]))
        result["bench_gpus1_steps300_warmup50"] = {"order": [os.path.basename(p) for p in args.bench], "lines": lines}
    dump()


if __name__ == "__main__":
    main()
