"""The neighbour-vote recommender at the synthetic Tiktok shape beside a torch composition of the same work: the test users, the
co-interaction lists under `cosine` with Kn = 50 neighbours an item,
  * the launch (ops.neighbour_vote_topk: no read back, events around `--calls` calls) at K = 10 and 50;
  * the share of the users, and of the votes, each form takes; every row forced onto the dense form (K = 10);
  * the torch composition: per user block an `index_add_` of the votes into a dense [users x items] float32 block, the mask of the
    history's items and of the items nobody voted for, and a `topk`; the share of identical lists;
  * the whole report pass (BaselineReport.evaluate, source co; a fresh report each time, the model's neighbour lists kept) against ONE
    evaluator test pass;
  * with --bench PARENT.json THIS.json: the result lines of `bench.py --gpus 1 --steps 300 --warmup 50` at the parent commit and at
    this one, copied into the record.
Best and median of `--reps`. Dev tool. On a shared machine run every GPU step under its own time limit, chained:

    timeout -k 10 600 python tools/knn_recommend_time.py [--out profiles/knn_recommend_tiktok.json] [--bench PARENT.json THIS.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from _timing import _events, _setup, _wall  # noqa: E402


def torch_vote_topk(nbr_idx, nbr_val, hist_ptr, hist_items, users, K, block):
    """The votes by torch: nbr_idx int64 / nbr_val fp32 [I x Kn], the histories as CSR on the device -> idx int64 [B x K], -1 where
    fewer than K items are voted for. Float adds through index_add_: the bits may change from run to run."""
    import torch
    I, Kn = nbr_idx.shape
    dev = nbr_idx.device
    out = torch.empty(users.numel(), K, dtype=torch.int64, device=dev)
    lens = hist_ptr[1:] - hist_ptr[:-1]
    for a in range(0, users.numel(), block):
        u = users[a:a + block]
        n = lens[u]
        row = torch.repeat_interleave(torch.arange(u.numel(), device=dev), n)
        at = torch.repeat_interleave(hist_ptr[u] - (torch.cumsum(n, 0) - n), n) + torch.arange(int(n.sum()), device=dev)
        items = hist_items[at].long()
        to = (row[:, None] * I + nbr_idx[items].clamp(min=0)).reshape(-1)
        ok = (nbr_idx[items] >= 0).reshape(-1)
        S = torch.zeros(u.numel() * I, dtype=torch.float32, device=dev)
        C = torch.zeros(u.numel() * I, dtype=torch.float32, device=dev)
        S.index_add_(0, to[ok], nbr_val[items].reshape(-1)[ok])
        C.index_add_(0, to[ok], torch.ones_like(S[:1]).expand(int(ok.sum())))
        S[C < 1] = float("-inf")
        S[row * I + items] = float("-inf")
        val, idx = torch.topk(S.view(u.numel(), I), K, dim=1)
        out[a:a + block] = torch.where(torch.isinf(val), torch.full_like(idx, -1), idx)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_recommend_tiktok.json"))
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
    U, I, Kn = model.num_users, model.num_items, 50
    model.predict_type = "TIE"
    train, test = ds.get_user_train_dict(), ds.get_user_test_dict()
    test_pass = _wall(lambda: model.test(), args.reps)
    users = np.asarray(list(test.keys()), dtype=np.int64)

    def build_lists():
        model.__dict__.pop("_knn_lists", None)
        return model.neighbour_lists("co", Kn, "cosine")

    build = _wall(build_lists, 1)
    lists = model.neighbour_lists("co", Kn, "cosine")
    hptr, hflat, _ = ops.ragged([train.get(u, []) for u in range(U)], cast=int)
    hist = ops.HistoryIndex(hptr, hflat, dev, n_items=I)
    V = ops.vote_votes(lists, hist)[users]
    in_lds = V <= ops.VOTE_SLOTS // 2
    result = {"shape": {"users": U, "items": I, "test_users": int(users.size), "neighbours": Kn}, "device": torch.cuda.get_device_name(0),
              "reps": args.reps, "calls": args.calls, "slots": ops.VOTE_SLOTS, "groups": ops.VOTE_GROUPS,
              "neighbour_lists_build_s": build[0], "evaluator_test_pass_s": {"best": test_pass[0], "median": test_pass[1]},
              "votes": {"mean": float(V.mean()), "max": int(V.max()), "users_lds_form": int(in_lds.sum()), "users_dense_form": int((~in_lds).sum()),
                        "share_users_dense_form": float((~in_lds).mean()), "share_votes_dense_form": float(V[~in_lds].sum() / max(1, V.sum()))},
              "runs": []}
    print(json.dumps(result["votes"]), flush=True)

    def timed(K, lds=True):
        B = users.size
        idx = torch.empty(B, K, dtype=torch.int32, device=dev)
        val = torch.empty(B, K, dtype=torch.float32, device=dev)
        cnt = torch.empty(B, K, dtype=torch.int32, device=dev)
        n_dense = int((~in_lds).sum()) if lds else B
        ws = torch.zeros(max(16, ops.vote_workspace(n_dense, I)), dtype=torch.uint8, device=dev)
        t = _events(lambda: ops.neighbour_vote_topk(lists, hist, users, K, idx, val, cnt, lds=lds, workspace=ws), args.calls, args.reps)
        return {"users": int(B), "K": K, "lds": lds, "dense_rows": n_dense, "s": {"best": t[0], "median": t[1]}}, idx

    for K, lds, what in ((10, True, "the test users"), (50, True, "the test users"), (10, False, "every row on the dense form")):
        run, idx = timed(K, lds)
        run["what"] = what
        result["runs"].append(run)
        print(json.dumps(run), flush=True)
        if K == 10 and lds:
            lists10 = idx.cpu().numpy()
    block = max(1, (1 << 29) // (4 * I))
    tl, tv, tu = lists.idx.long(), lists.val, torch.from_numpy(users).to(dev)
    t_ref = _events(lambda: torch_vote_topk(tl, tv, hist.ptr, hist.items, tu, 10, block), 1, max(1, args.reps // 2))
    ref = torch_vote_topk(tl, tv, hist.ptr, hist.items, tu, 10, block).cpu().numpy()
    hip10 = result["runs"][0]["s"]["best"]
    result["torch"] = {"K": 10, "block_users": block, "s": {"best": t_ref[0], "median": t_ref[1]}, "hip_over_torch": hip10 / t_ref[0],
                       "share_identical_lists": float((ref == lists10).all(axis=1).mean()),
                       "note": "float adds in arrival order and torch.topk's order among equal scores: a differing list is a tie or a last bit"}
    print(json.dumps(result["torch"]), flush=True)

    def first_pass():
        return BaselineReport(ds, train, test, cfg["topks"], metric=cfg["metric"], neighbours=Kn, group_view=[10, 30, 50, 100]).evaluate(model)

    setup = _wall(lambda: BaselineReport(ds, train, test, cfg["topks"], metric=cfg["metric"], neighbours=Kn, group_view=[10, 30, 50, 100]), 1)
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
