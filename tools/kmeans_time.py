"""Spherical k-means at the Tiktok shape beside a torch composition of the same two steps: after three training steps, over the
76 085 item rows of the fused block of the cached tables (d = 64), for C = 16 and C = 256 centroids drawn as ops.spherical_kmeans
draws them,
  * the assign launch alone (ops.kmeans_assign without the read of `changed`: the C entry point, events around `--calls` calls)
    against `(normalize(T) @ normalize(Cen).T).argmax(1)` on the same GPU, and the share of identical assignments;
  * the update (two launches) against `index_add_` of the unit rows in float64 followed by the normalisation;
  * a whole run of 25 iterations (ops.spherical_kmeans, iters = 25: wall-clock, it reads one integer per iteration) against 25
    rounds of the torch composition;
  * the whole report pass (ClusterReport.evaluate: K = 10, 8 clusters, four user groups; the first call, which clusters, and a
    second one on the same tables, which does not) against ONE evaluator test pass (model.test());
  * with --bench PARENT.json THIS.json: the result lines of `bench.py --gpus 1 --steps 300 --warmup 50` at the parent commit and at
    this one, run beside each other, copied into the record (the step's code is untouched: the two agree within their spread).
Best and median of `--reps`. Dev tool.

    python tools/kmeans_time.py [--out profiles/kmeans_tiktok.json] [--bench PARENT.json THIS.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from _timing import _events, _setup, _wall  # noqa: E402

ITERS, SEED = 25, 2022


def torch_assign(T, cen):
    import torch
    from torch.nn import functional as F
    return (F.normalize(T, dim=1) @ F.normalize(cen, dim=1).T).argmax(1)


def torch_update(T, assign, C):
    import torch
    from torch.nn import functional as F
    sums = torch.zeros(C, T.shape[1], dtype=torch.float64, device=T.device)
    sums.index_add_(0, assign, F.normalize(T, dim=1).double())
    return F.normalize(sums, dim=1).float()


def torch_lloyd(T, cen, iters):
    for _ in range(iters):
        cen = torch_update(T, torch_assign(T, cen), cen.shape[0])
    return cen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_tiktok.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--bench", nargs=2, metavar=("PARENT.json", "THIS.json"), default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from elimrec_amd import _lib, ops
    from elimrec_amd.evaluator import ClusterReport
    cfg, ds, model = _setup()
    dev = torch.device("cuda:0")
    U, I, d = model.num_users, model.num_items, model.latent_dim
    model.predict_type = "TIE"
    train, test = ds.get_user_train_dict(), ds.get_user_test_dict()
    test_pass = _wall(lambda: model.test(), args.reps)
    model._cached_tables("kmeans_time needs")
    sqn = model._block_sqnorms(dev)
    T, sq = model._ws["Y"][U:U + I, :d], sqn[U:U + I, 0]
    result = {"shape": {"users": U, "items": I, "recdim": d, "test_users": len(test)}, "iters": ITERS, "seed": SEED,
              "device": torch.cuda.get_device_name(0), "reps": args.reps, "calls": args.calls,
              "evaluator_test_pass_s": {"best": test_pass[0], "median": test_pass[1]}, "runs": []}
    lib = _lib.load()
    for C in (16, 256):
        good = np.flatnonzero(np.isfinite(sq.cpu().numpy()) & (sq.cpu().numpy() > 0))
        rows = torch.from_numpy(good[np.random.default_rng(SEED).permutation(good.size)[:C]]).to(dev)
        cen, csq = T.index_select(0, rows).contiguous(), sq.index_select(0, rows).contiguous()
        assign = torch.empty(I, dtype=torch.int32, device=dev)
        cos = torch.empty(I, dtype=torch.float32, device=dev)
        changed = torch.empty(1, dtype=torch.int32, device=dev)
        ws = torch.empty(ops.kmeans_workspace(I, d, C), dtype=torch.uint8, device=dev)

        def hip_assign():
            _lib.check(lib.elimrec_kmeans_assign(T.data_ptr(), T.stride(0), I, d, sq.data_ptr(), sq.stride(0), cen.data_ptr(), csq.data_ptr(),
                                                 C, None, assign.data_ptr(), cos.data_ptr(), changed.data_ptr(), ops._stream()), "kmeans_assign")

        a_hip = _events(hip_assign, args.calls, args.reps)
        a_ref = _events(lambda: torch_assign(T, cen), args.calls, args.reps)
        same = float((torch_assign(T, cen) == assign.long()).float().mean().item())
        moved, moved_sq = cen.clone(), csq.clone()
        u_hip = _events(lambda: ops.kmeans_update(T, sq, assign, moved, moved_sq, workspace=ws), args.calls, args.reps)
        u_ref = _events(lambda: torch_update(T, assign.long().clamp(min=0), C), args.calls, args.reps)
        run = ops.spherical_kmeans(T, sq, C, iters=ITERS, seed=SEED)
        l_hip = _wall(lambda: ops.spherical_kmeans(T, sq, C, iters=ITERS, seed=SEED), args.reps)
        l_ref = _wall(lambda: torch_lloyd(T, cen, run.n_iter), max(1, args.reps // 2))
        result["runs"].append({
            "C": C, "rows": I, "d": d,
            "assign_s": {"best": a_hip[0], "median": a_hip[1]}, "torch_assign_s": {"best": a_ref[0], "median": a_ref[1]},
            "assign_hip_over_torch": a_hip[0] / a_ref[0], "share_of_identical_assignments": same,
            "update_s": {"best": u_hip[0], "median": u_hip[1]}, "torch_update_s": {"best": u_ref[0], "median": u_ref[1]},
            "update_hip_over_torch": u_hip[0] / u_ref[0],
            "lloyd_s": {"best": l_hip[0], "median": l_hip[1]}, "torch_lloyd_s": {"best": l_ref[0], "median": l_ref[1]},
            "lloyd_hip_over_torch": l_hip[0] / l_ref[0], "n_iter": run.n_iter, "converged": run.converged, "cohesion": run.cohesion,
        })
        print(json.dumps(result["runs"][-1]), flush=True)
    report = ClusterReport(ds, train, test, 10, n_clusters=8, group_view=[10, 30, 50, 100])

    def first_pass():
        report._clusters = None
        return report.evaluate(model)

    whole = _wall(first_pass, args.reps)
    again = _wall(lambda: report.evaluate(model), args.reps)
    result["report"] = {"K": report.top_k, "clusters": report.num_classes, "space": report.space,
                        "report_pass_with_clustering_s": {"best": whole[0], "median": whole[1]},
                        "report_pass_clusters_cached_s": {"best": again[0], "median": again[1]},
                        "report_over_test_pass": whole[0] / test_pass[0], "cached_report_over_test_pass": again[0] / test_pass[0],
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
