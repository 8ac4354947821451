"""The embedding-geometry kernels at the Tiktok shape beside a torch composition of the same work: after three training steps, over
the 76 085 item rows and the 36 656 user rows of the fused block of the cached tables (d = 64),
  * the uniformity launch pair (ops.uniformity_sum_device: no read back, events around `--calls` calls) against the torch
    composition -- normalize, a blocked `@` over 8192-row blocks, exp, the strict-upper-triangle mask, a float64 sum -- on the same
    GPU; the algorithmic TFLOP/s (2 d flop per pair of the triangle) and the difference of the two log(S / pairs);
  * the Gram launch pair (ops.row_gram_device) against `Xn.double().T @ Xn.double()`;
  * the whole report pass (GeometryReport.evaluate with four user groups and three item bounds; a fresh report each time, then a second
    call on the same tables, which launches nothing) against ONE evaluator test pass (model.test());
  * with --bench PARENT.json THIS.json: the result lines of `bench.py --gpus 1 --steps 300 --warmup 50` at the parent commit and at
    this one, run beside each other, copied into the record (the step's code is untouched: the two agree within their spread).
Best and median of `--reps`. Dev tool. On a shared machine run every GPU step under its own time limit, chained:

    timeout -k 10 600 python tools/geometry_time.py [--out profiles/geometry_tiktok.json] [--bench PARENT.json THIS.json]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from _timing import _events, _setup, _wall  # noqa: E402

T_UNIFORMITY, BLOCK = 2.0, 8192


def torch_uniformity_sum(T, t):
    import torch
    from torch.nn import functional as F
    Xn = F.normalize(T, dim=1)
    n = Xn.shape[0]
    S = torch.zeros((), dtype=torch.float64, device=T.device)
    for a in range(0, n, BLOCK):
        for b in range(a, n, BLOCK):
            e = torch.exp(2.0 * t * (Xn[a:a + BLOCK] @ Xn[b:b + BLOCK].T - 1.0))
            if a == b:
                e = torch.triu(e, diagonal=1)
            S += e.sum(dtype=torch.float64)
    return S


def torch_gram(T):
    from torch.nn import functional as F
    Xn = F.normalize(T, dim=1).double()
    return Xn.T @ Xn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geometry_tiktok.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--bench", nargs=2, metavar=("PARENT.json", "THIS.json"), default=None)
    args = ap.parse_args()
    import torch
    from elimrec_amd import ops
    from elimrec_amd.evaluator import GeometryReport
    cfg, ds, model = _setup()
    dev = torch.device("cuda:0")
    U, I, d = model.num_users, model.num_items, model.latent_dim
    model.predict_type = "TIE"
    train, test = ds.get_user_train_dict(), ds.get_user_test_dict()
    test_pass = _wall(lambda: model.test(), args.reps)
    model._cached_tables("geometry_time needs")
    sqn = model._block_sqnorms(dev)
    result = {"shape": {"users": U, "items": I, "recdim": d, "test_users": len(test)}, "t": T_UNIFORMITY, "torch_block": BLOCK,
              "device": torch.cuda.get_device_name(0), "reps": args.reps, "calls": args.calls,
              "evaluator_test_pass_s": {"best": test_pass[0], "median": test_pass[1]}, "runs": []}
    for side in ("item", "user"):
        lo, n = model._side_rows(side)
        T, sq = model._ws["Y"][lo:lo + n, :d], sqn[lo:lo + n, 0]
        rows = torch.arange(n, dtype=torch.int32, device=dev)
        ws = torch.empty(max(ops.uniformity_workspace(n, d), ops.row_gram_workspace(n, d)), dtype=torch.uint8, device=dev)
        u_hip = _events(lambda: ops.uniformity_sum_device(T, sq, rows, T_UNIFORMITY, workspace=ws), args.calls, args.reps)
        u_ref = _events(lambda: torch_uniformity_sum(T, T_UNIFORMITY), max(1, args.calls // 2), args.reps)
        S, pairs, n_valid = ops.uniformity_sum(T, sq, rows, T_UNIFORMITY, workspace=ws)
        S_ref = float(torch_uniformity_sum(T, T_UNIFORMITY).item())
        g_hip = _events(lambda: ops.row_gram_device(T, sq, rows, workspace=ws), args.calls, args.reps)
        g_ref = _events(lambda: torch_gram(T), args.calls, args.reps)
        G = ops.row_gram(T, sq, rows, workspace=ws)[0]
        flop = 2.0 * d * (n * (n - 1) / 2)
        result["runs"].append({
            "side": side, "rows": n, "d": d, "pairs": pairs, "n_valid": n_valid,
            "uniformity_s": {"best": u_hip[0], "median": u_hip[1]}, "torch_uniformity_s": {"best": u_ref[0], "median": u_ref[1]},
            "uniformity_hip_over_torch": u_hip[0] / u_ref[0], "uniformity_algorithmic_tflops": flop / u_hip[0] / 1e12,
            "uniformity": ops.uniformity_value(S, pairs), "torch_uniformity": math.log(S_ref / (n * (n - 1) / 2)),
            "uniformity_minus_torch": ops.uniformity_value(S, pairs) - math.log(S_ref / (n * (n - 1) / 2)),
            "gram_s": {"best": g_hip[0], "median": g_hip[1]}, "torch_gram_s": {"best": g_ref[0], "median": g_ref[1]},
            "gram_hip_over_torch": g_hip[0] / g_ref[0], "gram_max_abs_diff_to_torch": float((G - torch_gram(T)).abs().max().item()),
        })
        print(json.dumps(result["runs"][-1]), flush=True)

    def first_pass():
        return GeometryReport(ds, train, test, group_view=[10, 30, 50, 100], item_group_view=[1, 4, 16], t=T_UNIFORMITY).evaluate(model)

    build = _wall(lambda: GeometryReport(ds, train, test, group_view=[10, 30, 50, 100], item_group_view=[1, 4, 16]), max(1, args.reps // 2))
    whole = _wall(first_pass, max(1, args.reps // 2))
    report = GeometryReport(ds, train, test, group_view=[10, 30, 50, 100], item_group_view=[1, 4, 16], t=T_UNIFORMITY)
    table = report.evaluate(model)[1]
    again = _wall(lambda: report.evaluate(model), args.reps)
    result["report"] = {"host_setup_s": {"best": build[0], "median": build[1]},
                        "report_pass_with_setup_s": {"best": whole[0], "median": whole[1]},
                        "report_pass_same_tables_s": {"best": again[0], "median": again[1]},
                        "report_over_test_pass": (whole[0] - build[0]) / test_pass[0], "table": table}
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
