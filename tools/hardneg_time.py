"""Hard-negative sampling at the Tiktok shape: after three training steps, over one epoch's triplets (n = the training
interactions), for M = 8 and 64 candidates in the fused space,
  * the pick launch alone (EliMRec.hard_negatives_device, csrc/hardneg.hip; events around `--calls` calls) and the rate of the rows
    it gathers, n * M item rows + n user rows of d floats (TB/s; the table fits the caches, this is not an HBM rate);
  * the candidate draw (ops.sample_triplet_candidates) against the uniform draw (ops.sample_triplets);
  * the yardstick: the same picks as torch ops on the same GPU -- gather, F.normalize, bmm, argmax, in blocks of `--block`
    triplets -- and the share of triplets on which the two agree (they differ where scores tie within fp32 rounding);
  * one hard epoch's sampling (draw + pick + the one-column launch of the statistics, PairwiseSamplerV2.sample_epoch) against one
    uniform epoch's, and both against the epoch's training steps at 0.28 ms each for scale.
Best and median of `--reps`. Dev tool.

    python tools/hardneg_time.py [--out profiles/hardneg_tiktok.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from _timing import _events, _setup, _wall  # noqa: E402


def torch_pick(Y, U, I, d, users, cands, block):
    """argmax_j cos(Y[u], Y[U + cands[:, j]]) over the fused block as torch ops: int64 [n] columns."""
    import torch
    import torch.nn.functional as F
    out = []
    for a in range(0, users.numel(), block):
        u, c = users[a:a + block], cands[a:a + block].long()
        rows = F.normalize(Y[U:U + I, :d][c], dim=2)
        out.append(torch.bmm(rows, F.normalize(Y[:U, :d][u], dim=1)[:, :, None])[:, :, 0].argmax(dim=1))
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hardneg_tiktok.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--block", type=int, default=65536)
    args = ap.parse_args()
    import torch
    from elimrec_amd import PairwiseSamplerV2, ops
    cfg, ds, model = _setup()
    dev = "cuda:0"
    U, I, d = model.num_users, model.num_items, model.latent_dim
    uniform = PairwiseSamplerV2(ds, batch_size=2048, device=dev)
    uniform._to_device()
    n = uniform.num_trainings
    u, p, q = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(3))
    draw1 = _events(lambda: ops.sample_triplets(*uniform._dev, I, n, 2022, 1, u, p, q), args.calls, args.reps)
    epoch1 = _wall(uniform.sample_epoch, args.reps)
    result = {"shape": {"users": U, "items": I, "recdim": d, "triplets": n}, "space": "fused", "device": torch.cuda.get_device_name(0),
              "reps": args.reps, "calls": args.calls, "uniform_draw_s": {"best": draw1[0], "median": draw1[1]},
              "uniform_epoch_sampling_s": {"best": epoch1[0], "median": epoch1[1]}, "epoch_steps": len(uniform),
              "epoch_training_s_at_0.28ms": 0.28e-3 * len(uniform), "runs": []}
    model.hard_negatives_device(u[:1], torch.zeros(1, 1, dtype=torch.int32, device=dev))       # the tables, realised once
    Y = model._ws["Y"]
    for M in (8, 64):
        cands = torch.empty(n, M, dtype=torch.int32, device=dev)
        draw = _events(lambda: ops.sample_triplet_candidates(*uniform._dev, I, n, 2022, 1, M, u, p, cands), args.calls, args.reps)
        out = (torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, device=dev))
        pick = _events(lambda: model.hard_negatives_device(u, cands, "fused", *out), args.calls, args.reps)
        ref = _wall(lambda: torch_pick(Y, U, I, d, u, cands, args.block), max(1, args.reps // 2))
        same = float((torch_pick(Y, U, I, d, u, cands, args.block) == out[1].long()).float().mean().item())
        hard = PairwiseSamplerV2(ds, batch_size=2048, device=dev, neg_sampling="hard", neg_candidates=M, model=model)
        epoch = _wall(hard.sample_epoch, args.reps)
        result["runs"].append({
            "M": M, "d": d, "triplets": n,
            "pick_s": {"best": pick[0], "median": pick[1]},
            "pick_gathered_rows_tbs": (n * M + n) * d * 4.0 / pick[0] * 1e-12,
            "candidate_draw_s": {"best": draw[0], "median": draw[1]}, "candidate_draw_over_uniform_draw": draw[0] / draw1[0],
            "torch_pick_s": {"best": ref[0], "median": ref[1]}, "hip_over_torch": pick[0] / ref[0],
            "share_of_identical_picks": same,
            "hard_epoch_sampling_s": {"best": epoch[0], "median": epoch[1]}, "hard_over_uniform_epoch_sampling": epoch[0] / epoch1[0],
            "last_stats": hard.last_stats,
        })
        print(json.dumps(result["runs"][-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
