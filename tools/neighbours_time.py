"""Similar items at the Tiktok shape beside a torch composition of the same lists: after three training steps, for k = 10 and 50,
in the fused space and in the first head's space,
  * EliMRec.similar_items over ALL items (wall-clock around a device synchronisation, host lists and copies included);
  * the device call alone (neighbours_device with a checked NeighbourQuery built once; events around `--calls` calls) and the
    algorithmic 2 Q n d flops over it = the achieved fp32 MFMA TFLOP/s (the merge launch is inside the time);
  * the yardstick: the same lists from torch.topk(normalize(T[q_block]) @ normalize(T).T, k + 1) over 8192-query blocks on the same
    GPU (k + 1: the query itself is in its own list and is dropped on the host side of the comparison).
Best and median of `--reps`. Dev tool.

    python tools/neighbours_time.py [--out profiles/neighbours_tiktok.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from _timing import _events, _setup, _wall  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbours_tiktok.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from elimrec_amd import ops
    cfg, ds, model = _setup()
    dev = "cuda:0"
    U, I, d = model.num_users, model.num_items, model.latent_dim
    model.similar_items([0], 1)
    query = ops.NeighbourQuery(torch.arange(I, dtype=torch.int32), I, dev)
    all_items = list(range(I))
    result = {"shape": {"users": U, "items": I, "recdim": d}, "device": torch.cuda.get_device_name(0), "reps": args.reps,
              "calls": args.calls, "runs": []}
    for space in ("fused", model._mods[0]):
        h = model._neighbour_space(space)
        T = model._ws["Y"][U:U + I, h * d:(h + 1) * d]
        for k in (10, 50):
            idx = torch.empty(I, k, dtype=torch.int32, device=dev)
            val = torch.empty(I, k, dtype=torch.float32, device=dev)
            api = _wall(lambda: model.similar_items(all_items, k, space=space), args.reps)
            knn = _events(lambda: model.neighbours_device("item", None, k, space, idx, val, query=query), args.calls, args.reps)

            def torch_lists():
                Tn = F.normalize(T, dim=1)
                out = []
                for a in range(0, I, 8192):
                    out.append(torch.topk(Tn[a:a + 8192] @ Tn.t(), k + 1, dim=1))
                return out
            ref = _events(torch_lists, args.calls, args.reps)
            # agreement: the share of the HIP lists' ids that the torch lists hold (ties and fp32 order aside, 1.0)
            tl = torch.cat([x.indices for x in torch_lists()]).int()
            cnt = torch.empty(I, dtype=torch.int32, device=dev)
            pad = torch.cat([idx, torch.full((I, 1), -1, dtype=torch.int32, device=dev)], dim=1).contiguous()
            ops.list_overlap(pad, tl.contiguous(), cnt)
            flops = 2.0 * I * I * d
            result["runs"].append({
                "space": space, "k": k,
                "similar_items_s": {"best": api[0], "median": api[1]},
                "cosine_topk_s": {"best": knn[0], "median": knn[1]},
                "cosine_topk_tflops": flops / knn[0] * 1e-12,
                "torch_topk_blocks_s": {"best": ref[0], "median": ref[1]},
                "hip_over_torch": knn[0] / ref[0],
                "shared_ids": float(cnt.double().mean().item()) / k,
            })
            print(json.dumps(result["runs"][-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
