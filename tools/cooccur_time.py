"""The co-interaction neighbours at the synthetic Tiktok shape beside a torch composition of the same work: all 76 085 items as
queries over the training graph,
  * the launch (ops.cooccur_topk: no read back, events around `--calls` calls) at K = 10 and 50 under `cosine`;
  * the distribution of W(q) and the share of rows each form takes; the rows of each form timed separately (K = 10), and every row
    forced onto the dense form;
  * the torch composition: a blocked `torch.sparse.mm(A^T_block, A)`, `to_dense`, the cosine score and a `topk`, over item blocks
    whose dense [block x I] float32 product fits 1 GiB, and the share of identical lists;
  * the whole report pass (CoNeighbourReport.evaluate, three item bounds; a fresh report each time) against ONE evaluator test pass;
  * with --bench PARENT.json THIS.json: the result lines of `bench.py --gpus 1 --steps 300 --warmup 50` at the parent commit and at
    this one, copied into the record.
Best and median of `--reps`. Dev tool. On a shared machine run every GPU step under its own time limit, chained:

    timeout -k 10 600 python tools/cooccur_time.py [--out profiles/cooccur_tiktok.json] [--bench PARENT.json THIS.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from _timing import _events, _setup, _wall  # noqa: E402


def torch_cooccur_topk(A, edge_item, edge_user, q_ptr, deg, K, block):
    """Cosine co-occurrence lists by torch: A [U x I] sparse float32; the same edges sorted by item (edge_item, edge_user int64 on
    the device, q_ptr on the host); deg [I] float64 -> idx int64 [I x K], -1 where fewer than K items share a user."""
    import torch
    U, I = A.shape
    out = torch.empty(I, K, dtype=torch.int64, device=A.device)
    for a in range(0, I, block):
        b = min(a + block, I)
        e0, e1 = int(q_ptr[a]), int(q_ptr[b])
        At = torch.sparse_coo_tensor(torch.stack([edge_item[e0:e1] - a, edge_user[e0:e1]]), torch.ones(e1 - e0, device=A.device), (b - a, U))
        C = torch.sparse.mm(At, A).to_dense()
        S = C.double() / torch.sqrt(deg[a:b, None] * deg[None, :]).clamp(min=1.0)
        S[C < 1] = float("-inf")
        S[torch.arange(b - a, device=A.device), torch.arange(a, b, device=A.device)] = float("-inf")
        val, idx = torch.topk(S, K, dim=1)
        out[a:b] = torch.where(torch.isinf(val), torch.full_like(idx, -1), idx)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cooccur_tiktok.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--bench", nargs=2, metavar=("PARENT.json", "THIS.json"), default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from elimrec_amd import ops
    from elimrec_amd.evaluator import CoNeighbourReport
    cfg, ds, model = _setup()
    dev = torch.device("cuda:0")
    U, I = model.num_users, model.num_items
    model.predict_type = "TIE"
    train = ds.get_user_train_dict()
    test_pass = _wall(lambda: model.test(), args.reps)
    build = _wall(lambda: ops.CooccurIndex.from_train(train, U, I, "item", dev), 1)
    index = model.cooccur_index("item")
    W = index.walk
    half = ops.COOCCUR_SLOTS // 2
    in_lds = W <= half
    rows_all = np.arange(I, dtype=np.int64)
    pct = [50, 90, 99, 99.9, 100]
    result = {"shape": {"users": U, "items": I, "edges": index.n_edges}, "device": torch.cuda.get_device_name(0), "reps": args.reps,
              "calls": args.calls, "slots": ops.COOCCUR_SLOTS, "groups": ops.COOCCUR_GROUPS,
              "index_build_s": build[0], "evaluator_test_pass_s": {"best": test_pass[0], "median": test_pass[1]},
              "walk": {"mean": float(W.mean()), "percentiles": {str(p): float(np.percentile(W, p)) for p in pct},
                       "rows_lds_form": int(in_lds.sum()), "rows_dense_form": int((~in_lds).sum()),
                       "share_rows_dense_form": float((~in_lds).mean()), "share_walk_dense_form": float(W[~in_lds].sum() / max(1, W.sum()))},
              "runs": []}
    print(json.dumps(result["walk"]), flush=True)

    def timed(rows, K, lds=True):
        Q = len(rows)
        idx = torch.empty(Q, K, dtype=torch.int32, device=dev)
        val = torch.empty(Q, K, dtype=torch.float32, device=dev)
        n_dense = int((W[rows] > half).sum()) if lds else Q
        ws = torch.zeros(max(16, ops.cooccur_workspace(n_dense, I)), dtype=torch.uint8, device=dev)
        t = _events(lambda: ops.cooccur_topk(index, rows, K, idx, val, measure="cosine", lds=lds, workspace=ws), args.calls, args.reps)
        return {"rows": Q, "K": K, "lds": lds, "dense_rows": n_dense, "s": {"best": t[0], "median": t[1]}}, idx

    for K in (10, 50):
        run, idx = timed(rows_all, K)
        run["what"] = "all items"
        result["runs"].append(run)
        print(json.dumps(run), flush=True)
        if K == 10:
            lists10 = idx.cpu().numpy()
    for what, rows, lds in (("the LDS form's rows", rows_all[in_lds], True), ("the dense form's rows", rows_all[~in_lds], True),
                            ("all items on the dense form", rows_all, False)):
        if len(rows):
            run, _ = timed(rows, 10, lds)
            run["what"] = what
            result["runs"].append(run)
            print(json.dumps(run), flush=True)
    # the torch composition
    q_ptr = index.q_ptr.cpu().numpy()
    edge_item = torch.from_numpy(np.repeat(np.arange(I, dtype=np.int64), np.diff(q_ptr))).to(dev)
    edge_user = index.q_nbr[:index.n_edges].long()
    A = torch.sparse_coo_tensor(torch.stack([edge_user, edge_item]), torch.ones(index.n_edges, device=dev), (U, I)).coalesce()
    deg = torch.from_numpy(index.deg.astype(np.float64)).to(dev)
    block = max(1, (1 << 30) // (4 * I))
    t_ref = _events(lambda: torch_cooccur_topk(A, edge_item, edge_user, q_ptr, deg, 10, block), 1, max(1, args.reps // 2))
    ref = torch_cooccur_topk(A, edge_item, edge_user, q_ptr, deg, 10, block).cpu().numpy()
    hip10 = result["runs"][0]["s"]["best"]
    result["torch"] = {"K": 10, "block_items": block, "s": {"best": t_ref[0], "median": t_ref[1]}, "hip_over_torch": hip10 / t_ref[0],
                       "share_identical_lists": float((ref == lists10).all(axis=1).mean()),
                       "note": "torch.topk orders equal scores as it likes: a differing list is a tie at the cut or within the list"}
    print(json.dumps(result["torch"]), flush=True)

    def first_pass():
        return CoNeighbourReport(ds, train, 10, item_group_view=[1, 4, 16]).evaluate(model)

    setup = _wall(lambda: CoNeighbourReport(ds, train, 10, item_group_view=[1, 4, 16]), 1)
    whole = _wall(first_pass, max(1, args.reps // 2))
    result["report"] = {"host_setup_s": setup[0], "report_pass_with_setup_s": {"best": whole[0], "median": whole[1]},
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
