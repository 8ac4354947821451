"""The list report at the Tiktok shape beside a torch composition of the same numbers: after three training steps, for K = 10 and
50 over ALL test users,
  * the pair-cosine launch alone (EliMRec.list_similarity_device over the users' top-K lists, all 1 + S spaces in one launch;
    events around `--calls` calls), and the exposure launch alone;
  * the whole report pass (ListReport.list_rows + evaluate: lists from predict_device, similarity, popularity, exposure, tables;
    wall-clock around a device synchronisation) against ONE evaluator test pass (model.test());
  * the yardstick: the same means from torch.bmm over gathered, normalised rows on the same GPU -- per space
    R = normalize(T[lists]) [B x K x d], G = bmm(R, R^T), (sum(G) - trace(G)) / (K (K - 1)) -- and the largest difference.
Best and median of `--reps`. Dev tool.

    python tools/lists_time.py [--out profiles/list_report_tiktok.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from _timing import _events, _setup, _wall  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "list_report_tiktok.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from elimrec_amd import ops
    from elimrec_amd.evaluator import ListReport
    cfg, ds, model = _setup()
    dev = "cuda:0"
    U, I, d, nb = model.num_users, model.num_items, model.latent_dim, 1 + model.S
    model.predict_type = "TIE"
    train, test = ds.get_user_train_dict(), ds.get_user_test_dict()
    test_pass = _wall(lambda: model.test(), args.reps)
    result = {"shape": {"users": U, "items": I, "recdim": d, "spaces": nb, "test_users": len(test)},
              "device": torch.cuda.get_device_name(0), "reps": args.reps, "calls": args.calls,
              "evaluator_test_pass_s": {"best": test_pass[0], "median": test_pass[1]}, "runs": []}
    for K in (10, 50):
        report = ListReport(ds, train, test, K, group_view=[10, 30, 50, 100], item_group_view=[1, 10, 100])
        rows, columns, lists, counts = report.list_rows(model)
        B = lists.shape[0]
        out = torch.empty(B, nb, dtype=torch.float32, device=dev)
        pair = _events(lambda: model.list_similarity_device(lists, out), args.calls, args.reps)
        expo = _events(lambda: ops.list_exposure(lists, counts), args.calls, args.reps)
        whole = _wall(lambda: report.evaluate(model), args.reps)
        Y = model._ws["Y"]
        ids = lists.clamp(min=0).long()

        def torch_means():
            cols = []
            for h in range(nb):
                R = F.normalize(Y[U:U + I, h * d:(h + 1) * d], dim=1)[ids]
                G = torch.bmm(R, R.transpose(1, 2))
                cols.append((G.sum(dim=(1, 2)) - G.diagonal(dim1=1, dim2=2).sum(dim=1)) / (K * (K - 1)))
            return torch.stack(cols, dim=1)
        ref = _events(torch_means, args.calls, args.reps)
        full = bool((lists >= 0).all())
        diff = float((torch_means() - out).abs().max().item()) if full else None
        result["runs"].append({
            "K": K, "lists": B, "columns": list(columns),
            "list_pair_cosine_s": {"best": pair[0], "median": pair[1]},
            "list_pair_cosine_gflops": 2.0 * B * nb * (K * (K - 1) / 2.0) * d / pair[0] * 1e-9,
            "list_pair_cosine_gather_gbs": B * K * nb * d * 4.0 / pair[0] * 1e-9,
            "list_exposure_s": {"best": expo[0], "median": expo[1]},
            "report_pass_s": {"best": whole[0], "median": whole[1]},
            "report_over_test_pass": whole[0] / test_pass[0],
            "torch_bmm_s": {"best": ref[0], "median": ref[1]},
            "hip_over_torch": pair[0] / ref[0],
            "max_abs_diff_to_torch": diff,
        })
        print(json.dumps(result["runs"][-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
