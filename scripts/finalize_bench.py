"""Norm finalize launches back to back on one stream, replayed from a captured graph (no host time between them): time per
launch of the direct form on 64 / 128 / 256 threads per block against the pooled form (T2V_FINALIZE_DIRECT=0), for the
bottleneck's shape (64x64 map, 32 partials per channel) and a batch of two.  The tables of all settings must be the same bits.
Usage: finalize_bench.py [--launches 200] [--reps 5]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from text2video_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=200)
ap.add_argument("--reps", type=int, default=5)
a = ap.parse_args()
dev = torch.device("cuda:0")
ops.context()


def per_launch_us(desc, stats, batch):
    mr = torch.empty(desc.Cout, 2, device=dev)
    one = (lambda: ops.batch_norm_finalize(stats, desc, batch)) if batch > 1 else (lambda: ops.instance_norm_finalize(stats, desc, out=mr))
    table = one().clone()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        one()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            for _ in range(a.launches):
                one()
    best = float("inf")
    for _ in range(a.reps + 1):   # the first replay warms up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, 1e3 * e0.elapsed_time(e1) / a.launches)
    return best, table


for C, batch in ((1024, 1), (512, 1), (1024, 2)):
    desc = ops.conv_desc(64, 64, 32, C, 3, 1, 1, ops.PAD_REFLECT, algo=ops.ALGO_WINOGRAD_F4)
    n = ops.conv_stats_buffer(desc, dev).numel()
    stats = torch.randn(batch * n, generator=torch.Generator().manual_seed(1)).abs().to(dev)
    row, ref = [], None
    for mode in ("0", "64", "128", "256"):
        os.environ["T2V_FINALIZE_DIRECT"] = mode
        ops.reload_env()
        us, table = per_launch_us(desc, stats, batch)
        ref = table if ref is None else ref
        assert torch.equal(table.view(torch.int32), ref.view(torch.int32)), "T2V_FINALIZE_DIRECT=%s: other bits" % mode
        row.append("%s: %.2f us" % ("pooled" if mode == "0" else "direct/" + mode, us))
    print("C %4d, %d x 32 partials, per launch (best of %d replays of %d): %s" % (C, batch, a.reps, a.launches, "  ".join(row)))
