"""The RP3beta neighbour lists at the synthetic Tiktok shape beside the kernel they were modelled on and a torch composition of the
same work: all 76 085 items as queries over the training graph, alpha = 1.0, beta = 0.6,
  * the launch (ops.walk_topk: no read back, events around `--calls` calls) at K = 50 against ops.cooccur_topk(measure="cosine") on
    the same rows -- the yardstick: the same walk with int32 counts where walk_topk carries int64 sums -- and both at K = 10;
  * the share of rows on the dense form; every row forced onto the dense form (K = 50);
  * the torch composition: a blocked `torch.sparse.mm` of the two weighted incidence matrices in float64, `to_dense`, the popularity
    penalty and a `topk`, over item blocks whose dense [block x I] float64 product fits 1 GiB, and the share of identical lists;
  * zero_votes and the power-of-two scale of EliMRec.neighbour_lists("rp3", 50) at the defaults;
  * the whole report pass (BaselineReport.evaluate, source rp3; a fresh report each time, the model's neighbour lists kept) against ONE
    evaluator test pass;
  * with --bench PARENT.json THIS.json: the result lines of `bench.py --gpus 1 --steps 300 --warmup 50` at the parent commit and at
    this one, copied into the record.
Best and median of `--reps`. Dev tool. On a shared machine run every GPU step under its own time limit, chained:

    timeout -k 10 600 python tools/walk_time.py [--out profiles/rp3_tiktok.json] [--bench PARENT.json THIS.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from _timing import _events, _setup, _wall  # noqa: E402


def torch_rp3_topk(P_ui, edge_item, edge_user, edge_w, q_ptr, penalty, K, block):
    """RP3beta lists by torch: P_ui [U x I] sparse float64 = deg(u)^-alpha on the edges; the same edges sorted by item (edge_item,
    edge_user int64, edge_w float64 = deg(item)^-alpha on the device, q_ptr on the host); penalty [I] float64 = deg^-beta -> idx
    int64 [I x K], -1 where fewer than K items are reached. Float sums: the last bit of a score is the library's."""
    import torch
    U, I = P_ui.shape
    out = torch.empty(I, K, dtype=torch.int64, device=P_ui.device)
    for a in range(0, I, block):
        b = min(a + block, I)
        e0, e1 = int(q_ptr[a]), int(q_ptr[b])
        P_iu = torch.sparse_coo_tensor(torch.stack([edge_item[e0:e1] - a, edge_user[e0:e1]]), edge_w[e0:e1], (b - a, U))
        S = torch.sparse.mm(P_iu, P_ui).to_dense()
        reached = S > 0
        S = S * penalty[None, :]
        S[~reached] = float("-inf")
        S[torch.arange(b - a, device=S.device), torch.arange(a, b, device=S.device)] = float("-inf")
        val, idx = torch.topk(S.float(), K, dim=1)
        out[a:b] = torch.where(torch.isinf(val), torch.full_like(idx, -1), idx)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rp3_tiktok.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--bench", nargs=2, metavar=("PARENT.json", "THIS.json"), default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from elimrec_amd import ops
    from elimrec_amd.evaluator import BaselineReport
    cfg, ds, model = _setup()
    dev = torch.device("cuda:0")
    U, I, alpha, beta = model.num_users, model.num_items, 1.0, 0.6
    model.predict_type = "TIE"
    train, test = ds.get_user_train_dict(), ds.get_user_test_dict()
    test_pass = _wall(lambda: model.test(), args.reps)
    index = model.cooccur_index("item")
    weights = ops.rp3_weights(index, alpha, beta)
    W = index.walk
    half = ops.WALK_SLOTS // 2
    in_lds = W <= half
    rows_all = np.arange(I, dtype=np.int64)
    result = {"shape": {"users": U, "items": I, "edges": index.n_edges}, "device": torch.cuda.get_device_name(0), "reps": args.reps,
              "calls": args.calls, "alpha": alpha, "beta": beta, "frac_bits": ops.WALK_FRAC_BITS,
              "evaluator_test_pass_s": {"best": test_pass[0], "median": test_pass[1]},
              "walk": {"mean": float(W.mean()), "max": int(W.max()), "rows_lds_form": int(in_lds.sum()), "rows_dense_form": int((~in_lds).sum()),
                       "share_rows_dense_form": float((~in_lds).mean()), "share_walk_dense_form": float(W[~in_lds].sum() / max(1, W.sum()))},
              "runs": []}
    print(json.dumps(result["walk"]), flush=True)

    def timed(kernel, K, lds=True):
        idx = torch.empty(I, K, dtype=torch.int32, device=dev)
        val = torch.empty(I, K, dtype=torch.float32, device=dev)
        n_dense = int((~in_lds).sum()) if lds else I
        if kernel == "walk_topk":
            ws = torch.zeros(max(16, ops.walk_workspace(n_dense, I)), dtype=torch.uint8, device=dev)
            call = lambda: ops.walk_topk(index, rows_all, K, weights, idx, val, lds=lds, workspace=ws)
        else:
            ws = torch.zeros(max(16, ops.cooccur_workspace(n_dense, I)), dtype=torch.uint8, device=dev)
            call = lambda: ops.cooccur_topk(index, rows_all, K, idx, val, measure="cosine", lds=lds, workspace=ws)
        t = _events(call, args.calls, args.reps)
        return {"kernel": kernel, "rows": I, "K": K, "lds": lds, "dense_rows": n_dense, "s": {"best": t[0], "median": t[1]}}, idx

    best = {}
    for kernel, K, lds in (("walk_topk", 50, True), ("cooccur_topk", 50, True), ("walk_topk", 10, True), ("cooccur_topk", 10, True),
                           ("walk_topk", 50, False), ("cooccur_topk", 50, False)):
        run, idx = timed(kernel, K, lds)
        result["runs"].append(run)
        best[(kernel, K, lds)] = run["s"]["best"]
        print(json.dumps(run), flush=True)
        if (kernel, K, lds) == ("walk_topk", 10, True):
            lists10 = idx.cpu().numpy()
    result["walk_over_cooccur"] = {"K50": best[("walk_topk", 50, True)] / best[("cooccur_topk", 50, True)],
                                   "K10": best[("walk_topk", 10, True)] / best[("cooccur_topk", 10, True)],
                                   "K50_all_dense": best[("walk_topk", 50, False)] / best[("cooccur_topk", 50, False)]}
    print(json.dumps(result["walk_over_cooccur"]), flush=True)
    # the torch composition
    q_ptr = index.q_ptr.cpu().numpy()
    edge_item = torch.from_numpy(np.repeat(np.arange(I, dtype=np.int64), np.diff(q_ptr))).to(dev)
    edge_user = index.q_nbr[:index.n_edges].long()
    power = lambda deg, p: torch.from_numpy(np.where(deg > 0, np.power(np.maximum(deg, 1).astype(np.float64), -p), 0.0)).to(dev)
    P_ui = torch.sparse_coo_tensor(torch.stack([edge_user, edge_item]), power(index.deg_other, alpha)[edge_user], (U, I)).coalesce()
    edge_w, penalty = power(index.deg, alpha)[edge_item], power(index.deg, beta)
    block = max(1, (1 << 30) // (8 * I))
    try:
        t_ref = _events(lambda: torch_rp3_topk(P_ui, edge_item, edge_user, edge_w, q_ptr, penalty, 10, block), 1, max(1, args.reps // 2))
        ref = torch_rp3_topk(P_ui, edge_item, edge_user, edge_w, q_ptr, penalty, 10, block).cpu().numpy()
        result["torch"] = {"K": 10, "block_items": block, "s": {"best": t_ref[0], "median": t_ref[1]},
                           "hip_over_torch": best[("walk_topk", 10, True)] / t_ref[0],
                           "share_identical_lists": float((ref == lists10).all(axis=1).mean()),
                           "note": "float64 sums in the library's order, rounded to fp32 before torch.topk, which orders equal scores as it "
                                   "likes: a differing list is a tie or a last bit"}
    except RuntimeError as e:                                 # (a torch build without the float64 sparse product: say so in the record)
        result["torch"] = {"K": 10, "block_items": block, "error": str(e).splitlines()[0]}
    print(json.dumps(result["torch"]), flush=True)
    # the lists as the vote takes them
    model.__dict__.pop("_knn_lists", None)
    build = _wall(lambda: (model.__dict__.pop("_knn_lists", None), model.neighbour_lists("rp3", 50, alpha=alpha, beta=beta)), 1)
    lists = model.neighbour_lists("rp3", 50, alpha=alpha, beta=beta)
    result["neighbour_lists"] = {"neighbours": 50, "build_s": build[0], "scale_exp": lists.scale_exp, "zero_votes": lists.zero_votes}
    print(json.dumps(result["neighbour_lists"]), flush=True)

    def report():
        return BaselineReport(ds, train, test, cfg["topks"], metric=cfg["metric"], sources=("rp3",), neighbours=50, alpha=alpha, beta=beta,
                              group_view=[10, 30, 50, 100])

    setup = _wall(report, 1)
    whole = _wall(lambda: report().evaluate(model), max(1, args.reps // 2))
    result["report"] = {"host_setup_s": setup[0], "report_pass_with_setup_s": {"best": whole[0], "median": whole[1]},
                        "report_over_test_pass": (whole[0] - setup[0]) / test_pass[0], "table": report().evaluate(model)[1]}
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
