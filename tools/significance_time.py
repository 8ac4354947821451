"""The bootstrap at the Tiktok shape: after three training steps, the test users' TIE metric rows compacted to the shown columns,
the groups `all` + [10,30,50,100], R = 2000 and R = 10 000 replicates,
  * the launch alone (ops.bootstrap_means, csrc/bootstrap.hip; events around `--calls` calls), its draws per second (R x the
    listed rows) and the bytes of row reads per second (draws x C floats; the block fits the caches, this is not an HBM rate);
  * the yardstick: the same replicate means as torch ops on the same GPU -- per group torch.randint positions in replicate blocks
    whose [block x n_g x C] float64 gather stays within `--block_bytes`, an index into the group's rows, a mean (other draws, the
    same work) -- and, as a check of both, the largest distance between the two forms' standard errors in units of the standard
    error's own sampling error se / sqrt(2 R);
  * the whole report pass (SignificanceReport.evaluate: one evaluator scoring pass, the launch, the host summary) against one
    evaluator test pass.
Best and median of `--reps`. Dev tool.

    python tools/significance_time.py [--out profiles/significance_tiktok.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from _timing import _events, _setup, _wall  # noqa: E402


def torch_means(rows, ptr, group_rows, R, block_bytes, seed):
    """float64 [R x G x C]: bootstrap replicate means as torch ops (torch's generator: not the contract's draws)."""
    import torch
    gen = torch.Generator(device=rows.device)
    gen.manual_seed(seed)
    G, C = len(ptr) - 1, rows.shape[1]
    out = torch.full((R, G, C), float("nan"), dtype=torch.float64, device=rows.device)
    for g in range(G):
        n_g = int(ptr[g + 1] - ptr[g])
        if not n_g:
            continue
        mine = rows[group_rows[ptr[g]:ptr[g + 1]].long()].double()
        step = max(1, int(block_bytes) // (n_g * C * 8))
        for a in range(0, R, step):
            b = min(R, a + step)
            at = torch.randint(0, n_g, (b - a, n_g), device=rows.device, generator=gen)
            out[a:b, g] = mine[at].mean(dim=1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "significance_tiktok.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--block_bytes", type=int, default=1 << 30)
    args = ap.parse_args()
    import numpy as np
    import torch
    from elimrec_amd import ops
    from elimrec_amd.evaluator import SignificanceReport
    cfg, ds, model = _setup()
    dev = torch.device("cuda:0")
    model.predict_type = "TIE"
    train, test = ds.get_user_train_dict(), ds.get_user_test_dict()
    test_pass = _wall(lambda: model.test(), args.reps)
    view = [10, 30, 50, 100]
    result = {"shape": {"users": model.num_users, "items": model.num_items, "test_users": len(test)}, "group_view": view,
              "predict_type": "TIE", "device": torch.cuda.get_device_name(0), "reps": args.reps, "calls": args.calls,
              "torch_block_bytes": args.block_bytes, "evaluator_test_pass_s": {"best": test_pass[0], "median": test_pass[1]}, "runs": []}
    for R in (2000, 10000):
        report = SignificanceReport(ds, train, test, cfg["topks"], metric=cfg["metric"], group_view=view, replicates=R)
        rows, columns = report.metric_rows(model)
        index = report._resident(dev)["groups"]
        sizes = [int(s) for s in index.sizes]
        C = rows.shape[1]
        out = torch.empty(R, index.n_groups, C, dtype=torch.float64, device=dev)
        launch = _events(lambda: ops.bootstrap_means(rows, index, None, R, report.seed, out=out), args.calls, args.reps)
        draws = float(R) * float(sum(sizes))
        ptr = index.ptr.cpu().numpy()
        ref = _wall(lambda: torch_means(rows, ptr, index.rows, R, args.block_bytes, report.seed), max(1, args.reps // 2))
        want = torch_means(rows, ptr, index.rows, R, args.block_bytes, report.seed)
        se_hip, se_torch = out.std(dim=0), want.std(dim=0)
        z = ((se_hip - se_torch).abs() / (se_torch / np.sqrt(2.0 * R)).clamp(min=1e-300)).nan_to_num(0.0)
        whole = _wall(lambda: report.evaluate(model), args.reps)
        result["runs"].append({
            "R": R, "columns": list(columns), "group_labels": [x.strip() for x in report.group_labels], "group_sizes": sizes,
            "groups_in_lds": [ops.bootstrap_rows_in_lds(s, min(C, ops.BOOTSTRAP_MAX_COLUMNS)) for s in sizes],
            "bootstrap_means_s": {"best": launch[0], "median": launch[1]}, "draws": draws, "draws_per_s": draws / launch[0],
            "row_read_bytes_per_s": draws * C * 4.0 / launch[0],
            "torch_composition_s": {"best": ref[0], "median": ref[1]}, "hip_over_torch": launch[0] / ref[0],
            "largest_se_gap_in_se_sampling_errors": float(z.max().item()),
            "report_pass_s": {"best": whole[0], "median": whole[1]}, "report_over_test_pass": whole[0] / test_pass[0],
        })
        print(json.dumps(result["runs"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
