"""What the report timing tools share (effects_time, rank_time, neighbours_time, lists_time): the model after three training steps
at the benchmark's shape, and the two clocks."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _setup():
    import torch
    import bench
    from elimrec_amd import ColumnShardEngine, ColumnShardTrainer, FusedAdam, PairwiseSamplerV2
    cfg, ds, model = bench.build(None, "cuda:0")
    model = model.to("cuda:0")
    opt = FusedAdam(model.parameters(), lr=cfg["lr"], weight_decay=cfg["weight_decay"])
    tr = ColumnShardTrainer(ColumnShardEngine(model), opt)
    u, p, n = PairwiseSamplerV2(ds, batch_size=2048, device="cuda:0").sample_epoch()
    for i in range(3):
        tr.step(u[i * 2048:(i + 1) * 2048], p[i * 2048:(i + 1) * 2048], n[i * 2048:(i + 1) * 2048])
    torch.cuda.synchronize()
    return cfg, ds, model


def _wall(fn, reps):
    """Seconds per pass: (best, median) over `reps` runs, each ended by a device synchronisation."""
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts), sorted(ts)[len(ts) // 2]


def _events(fn, calls, reps):
    """Seconds per call: (best, median) over `reps` groups of `calls` launches between two events."""
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3 / calls)
    return min(ts), sorted(ts)[len(ts) // 2]
