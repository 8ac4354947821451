"""The iALS baseline at the synthetic Tiktok shape, factors = 64, beside torch compositions of the same work:
  * one user half-sweep and one item half-sweep (the factors after two iterations of the fit): the Gram (ops.row_gram_device), the
    solve launch (elimrec_als_solve alone: events around `--calls` launches, no read back), the host part (ops.als_solve's wall
    time minus the launch: the checks, the upload of the ridge and the rows, the status read back) and the gathered TB/s of the
    launch (edges x d x 4 bytes / time);
  * the torch composition of a half-sweep: per block of rows an `index_add_` of the float64 outer products into [rows x d x d],
    `torch.linalg.cholesky`, `torch.cholesky_solve`;
  * the tail: the longest row solved alone against the whole launch -- does the most popular row pace its half-sweep?
  * ops.cross_topk over all test users at K = 10 and K = 50 against torch.topk(X[block] @ Y.T) with the train items masked;
  * the fit (15 iterations) and the whole `ials` report pass (lists + table; the fit kept) against ONE evaluator test pass;
  * with --bench PARENT.json THIS.json [PARENT2.json THIS2.json]: the result lines of `bench.py --gpus 1 --steps 300 --warmup 50`
    at the parent commit and at this one, copied into the record.
Best and median of `--reps`. Dev tool. On a shared machine run every GPU step under its own time limit, chained:

    timeout -k 10 600 python tools/ials_time.py [--out profiles/ials_tiktok.json] [--bench PARENT.json THIS.json ...]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from _timing import _events, _setup, _wall  # noqa: E402

OUTER_BYTES = 1 << 30        # the float64 outer products one index_add_ of the torch composition holds at most


def torch_half_sweep(ptr, nbr, F, A0, reg, conf, block_rows):
    """A half-sweep by torch: ptr (host int64), nbr (device int64), F float32, A0 / reg float64 on the device -> float32 [n x d]."""
    import numpy as np
    import torch
    n, d = ptr.size - 1, F.shape[1]
    out = torch.zeros(n, d, dtype=torch.float32, device=F.device)
    eye = torch.eye(d, dtype=torch.float64, device=F.device)
    per = max(1, OUTER_BYTES // (8 * d * d))
    for a in range(0, n, block_rows):
        b = min(n, a + block_rows)
        e0, e1 = int(ptr[a]), int(ptr[b])
        local = torch.from_numpy(np.repeat(np.arange(b - a, dtype=np.int64), np.diff(ptr[a:b + 1]))).to(F.device)
        S = torch.zeros(b - a, d, d, dtype=torch.float64, device=F.device)
        rhs = torch.zeros(b - a, d, dtype=torch.float64, device=F.device)
        for c0 in range(e0, e1, per):
            c1 = min(e1, c0 + per)
            f = F[nbr[c0:c1]].double()
            S.index_add_(0, local[c0 - e0:c1 - e0], f[:, :, None] * f[:, None, :])
            rhs.index_add_(0, local[c0 - e0:c1 - e0], f)
        A = A0[None] + reg[a:b, None, None] * eye[None] + conf * S
        x = torch.cholesky_solve(((1.0 + conf) * rhs)[:, :, None], torch.linalg.cholesky(A))[:, :, 0]
        out[a:b] = x.float()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ials_tiktok.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--bench", nargs="+", metavar="JSON", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from elimrec_amd import _lib, ops
    from elimrec_amd.evaluator import BaselineReport
    cfg, ds, model = _setup()
    dev = torch.device("cuda:0")
    U, I, d, conf, reg = model.num_users, model.num_items, 64, 1.0, 0.01
    model.predict_type = "TIE"
    train, test = ds.get_user_train_dict(), ds.get_user_test_dict()
    test_pass = _wall(lambda: model.test(), args.reps)
    warm = model.fit_ials(factors=d, iters=2)
    X, Y = warm.users, warm.items
    by_user, by_item = model._ials_graph(dev)
    result = {"shape": {"users": U, "items": I, "edges": by_user.n_edges}, "device": torch.cuda.get_device_name(0), "reps": args.reps,
              "calls": args.calls, "factors": d, "conf": conf, "reg": reg, "als_chunk": ops.ALS_CHUNK,
              "evaluator_test_pass_s": {"best": test_pass[0], "median": test_pass[1]}, "half_sweeps": {}}
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream

    for side, index, F, out in (("user", by_user, Y, torch.empty_like(X)), ("item", by_item, X, torch.empty_like(Y))):
        n, nf = index.n, index.n_fixed
        ones = torch.ones(nf, dtype=torch.float32, device=dev)
        every = torch.arange(nf, dtype=torch.int32, device=dev)
        A0 = ops.row_gram_device(F, ones, every)[0]
        t_gram = _events(lambda: ops.row_gram_device(F, ones, every), args.calls, args.reps)
        reg_host = np.full(n, reg)
        reg_dev = torch.from_numpy(reg_host).to(dev)
        status = torch.tensor([0, 2 ** 31 - 1], dtype=torch.int32, device=dev)

        def launch(rows):
            return lambda: lib.elimrec_als_solve(F.data_ptr(), F.stride(0), nf, d, A0.data_ptr(), index.ptr.data_ptr(), index.nbr.data_ptr(), n,
                                                 rows.data_ptr(), rows.numel(), reg_dev.data_ptr(), conf, out.data_ptr(), out.stride(0),
                                                 status.data_ptr(), stream)
        rows_all = torch.from_numpy(index.by_degree).to(dev)
        longest = int(index.by_degree[0])
        t_launch = _events(launch(rows_all), args.calls, args.reps)
        t_long = _events(launch(rows_all[:1].clone()), args.calls, args.reps)
        assert int(status[0].item()) == 0
        t_call = _wall(lambda: ops.als_solve(index, F, A0, reg_host, conf, out), args.reps)
        want = out.clone()
        ptr = index.ptr.cpu().numpy()
        nbr = index.nbr[:index.n_edges].long()
        block = 4096
        t_torch = _wall(lambda: torch_half_sweep(ptr, nbr, F, A0, reg_dev, conf, block), max(1, args.reps // 2))
        diff = float((torch_half_sweep(ptr, nbr, F, A0, reg_dev, conf, block) - want).abs().max().item())
        run = {"rows": n, "fixed_rows": nf, "edges": index.n_edges, "degree": {"mean": float(index.deg.mean()), "max": int(index.deg.max())},
               "gram_s": {"best": t_gram[0], "median": t_gram[1]}, "solve_launch_s": {"best": t_launch[0], "median": t_launch[1]},
               "als_solve_call_s": {"best": t_call[0], "median": t_call[1]}, "host_part_s": t_call[0] - t_launch[0],
               "gathered_TBps": index.n_edges * d * 4 / t_launch[0] / 1e12,
               "longest_row": {"row": longest, "degree": int(index.deg[longest]), "alone_s": {"best": t_long[0], "median": t_long[1]},
                               "share_of_launch": t_long[0] / t_launch[0]},
               "torch": {"block_rows": block, "s": {"best": t_torch[0], "median": t_torch[1]}, "hip_call_over_torch": t_call[0] / t_torch[0],
                         "max_abs_diff": diff}}
        result["half_sweeps"][side] = run
        print(json.dumps({side: run}), flush=True)

    # serving: all test users, the train items masked
    users = np.asarray(sorted(test), dtype=np.int64)
    ptr_e, flat_e, _ = ops.ragged([train.get(int(u), []) for u in users], cast=int)
    query = ops.CrossQuery(users, U, I, dev, ptr_e, flat_e)
    mask_rows = torch.from_numpy(np.repeat(np.arange(users.size, dtype=np.int64), np.diff(ptr_e))).to(dev)
    mask_cols = torch.from_numpy(flat_e.astype(np.int64)).to(dev)
    users_dev = torch.from_numpy(users).to(dev)
    block = max(1, (1 << 30) // (4 * I))

    def torch_topk(K):
        out = torch.empty(users.size, K, dtype=torch.int64, device=dev)
        for a in range(0, users.size, block):
            b = min(users.size, a + block)
            S = X[users_dev[a:b]] @ Y.T
            sel = (mask_rows >= a) & (mask_rows < b)
            S[mask_rows[sel] - a, mask_cols[sel]] = float("-inf")
            out[a:b] = torch.topk(S, K, dim=1)[1]
        return out

    result["cross_topk"] = []
    for K in (10, 50):
        idx = torch.empty(users.size, K, dtype=torch.int32, device=dev)
        val = torch.empty(users.size, K, dtype=torch.float32, device=dev)
        ws = torch.empty(ops.cosine_topk_workspace(users.size, I, K), dtype=torch.uint8, device=dev)
        t = _events(lambda: ops.cross_topk(X, None, Y, None, query, K, idx, val, workspace=ws), args.calls, args.reps)
        t_ref = _events(lambda: torch_topk(K), 1, max(1, args.reps // 2))
        same = float((torch_topk(K) == idx.long()).all(dim=1).float().mean().item())
        run = {"K": K, "users": int(users.size), "s": {"best": t[0], "median": t[1]}, "torch_s": {"best": t_ref[0], "median": t_ref[1]},
               "hip_over_torch": t[0] / t_ref[0], "share_identical_lists": same, "torch_block_users": block}
        result["cross_topk"].append(run)
        print(json.dumps(run), flush=True)

    # the fit and the report pass
    def fit():
        model.__dict__.pop("_ials", None)
        return model.fit_ials(factors=d, iters=15)
    t_fit = _wall(fit, 1)
    full = model.fit_ials(factors=d, iters=15)
    result["fit"] = {"iters": 15, "s": t_fit[0], "objective_first": float(full.objective[0]), "objective_last": float(full.objective[-1]),
                     "monotone": bool((np.diff(full.objective) <= 1e-9 * np.abs(full.objective[:-1])).all())}
    print(json.dumps(result["fit"]), flush=True)

    def report():
        return BaselineReport(ds, train, test, cfg["topks"], metric=cfg["metric"], sources=("ials",), group_view=[10, 30, 50, 100])

    setup = _wall(report, 1)
    whole = _wall(lambda: report().evaluate(model), max(1, args.reps // 2))
    result["report"] = {"host_setup_s": setup[0], "report_pass_with_setup_s": {"best": whole[0], "median": whole[1]},
                        "report_over_test_pass": (whole[0] - setup[0]) / test_pass[0],
                        "fit_plus_report_over_test_pass": (t_fit[0] + whole[0] - setup[0]) / test_pass[0], "table": report().evaluate(model)[1]}
    print(json.dumps(result["report"]), flush=True)
    if args.bench:
        lines = []
        for path in args.bench:
            with open(path) as f:
                lines.append(json.loads([ln for ln in f.read().splitlines() if ln.strip().startswith("{")][-1]))
        result["bench_gpus1_steps300_warmup50"] = {"order": [os.path.basename(p) for p in args.bench], "lines": lines}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
