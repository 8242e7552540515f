"""fp32 polyphase (T2V_ALGO_POLYPHASE) against split polyphase (T2V_ALGO_POLYPHASE_BF16X2) on one MI355X, by the method of
scripts/measure_split_bf16.py: ONE process, the two forms alternating and warmed, the median of --rounds rounds with min and max
beside it, the core clock sampled during every timed loop.

  * per layer class: the four polyphase layer shapes of a 512x512 frame (each occurs twice: both encoders, both branches), and
    the 512 <-> 1024 pair at 512x320 and 512x680 -- the GEMM stage alone (stage 2), the input transform alone (stage 1) and the
    whole conv (stages 1 | 2 | 4), HIP events around loops of launches;
  * whole 512x512 frames with the flow branch in fp32, arith="bf16x2" (trunk) and arith_layers="trunk+stride2", one sequence
    and two in lock-step;
  * --parent TREE: TREE/bench.py against this tree's in alternating child processes (the default fp32 path).
    python scripts/measure_split_bf16_stride2.py --parent ../parent --out profiles/split_bf16_stride2_times.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import torch  # noqa: E402

import bench  # noqa: E402  (ClockSampler: the benchmark's own helper, read only)
import measure_split_bf16 as base  # noqa: E402  (frame_times, bench_fps, fmt)
from text2video_amd import ops  # noqa: E402
from text2video_amd.generator import GeneratorSpec, HipGenerator, Vid2VidModelG, synthetic_state_dict  # noqa: E402

# label, up, H, W (input map), Cin, Cout
LAYERS = [("512x512 down2 256 -> 512", False, 256, 256, 256, 512), ("512x512 down3 512 -> 1024", False, 128, 128, 512, 1024),
          ("512x512 up1 1024 -> 512", True, 64, 64, 1024, 512), ("512x512 up2 512 -> 256", True, 128, 128, 512, 256),
          ("512x320 down3 512 -> 1024", False, 128, 80, 512, 1024), ("512x320 up1 1024 -> 512", True, 64, 40, 1024, 512),
          ("512x680 down3 512 -> 1024", False, 128, 170, 512, 1024), ("512x680 up1 1024 -> 512", True, 64, 85, 1024, 512)]


def layer_times(dev, up, H, W, Cin, Cout, stages, launches, rounds, clocks):
    """us per launch of `stages` for ALGO_POLYPHASE and ALGO_POLYPHASE_BF16X2, alternating"""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, H, W, Cin, generator=g).to(dev)
    w = (torch.randn(*((Cin, Cout, 3, 3) if up else (Cout, Cin, 3, 3)), generator=g) * (9 * Cin) ** -0.5).to(dev)
    b = torch.zeros(Cout, device=dev)
    runs = {}
    for name, algo in (("fp32", ops.ALGO_POLYPHASE), ("bf16x2", ops.ALGO_POLYPHASE_BF16X2)):
        d = ops.conv_desc(H, W, Cin, Cout, 3, 2, 1, ops.PAD_ZERO, up, algo=algo)
        pu = ops.pack_conv_weight(w, d, Cin)
        ws = ops.winograd_batch_workspace(d, Cin, 1, dev)
        ho, wo = ops.conv_out_dims(d)
        y = torch.empty(1, ho, wo, Cout, device=dev)
        stats = ops.conv_stats_buffer(d, dev)
        ops.conv2d_winograd_batch(x, pu, b, d, ws, stats=stats, out=y, stages=7)
        runs[name] = lambda d=d, pu=pu, ws=ws, y=y, stats=stats: ops.conv2d_winograd_batch(x, pu, b, d, ws, stats=stats, out=y, stages=stages)
    res = {k: [] for k in runs}
    for fn in runs.values():
        for _ in range(launches):
            fn()
    torch.cuda.synchronize()
    samp = clocks.fork(0.01)
    with samp:
        for _ in range(rounds):
            for name, fn in runs.items():
                for _ in range(8):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(launches):
                    fn()
                e1.record()
                e1.synchronize()
                res[name].append(e0.elapsed_time(e1) * 1e3 / launches)
    return res, samp.mean_mhz()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--no-frames", action="store_true")
    ap.add_argument("--no-layers", action="store_true")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its bench.py against this tree's")
    ap.add_argument("--bench-rounds", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "measure_split_bf16_stride2.py needs a GPU"
    dev = torch.device("cuda:0")
    clocks = bench.ClockSampler(0)
    lines = ["split polyphase against fp32 polyphase, one process, alternating rounds; %s" % clocks.ident]

    def flush():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    if a.parent:
        res = {"parent": [], "this": []}
        trees = {"parent": os.path.abspath(a.parent), "this": ROOT}
        for r in range(a.bench_rounds):
            for k in (("parent", "this") if r % 2 == 0 else ("this", "parent")):      # who goes first alternates too
                res[k].append(base.bench_fps(trees[k], 62, a.warmup))
        lines.append("bench.py --gpus 1 --steps 62 --warmup %d (the default fp32 path), parent commit against this tree, alternating child "
                     "processes, the first of each round alternating" % a.warmup)
        for k, v in res.items():
            lines.append("    %-7s %s" % (k, base.fmt(v, "fps")))
        lines.append("    this / parent = %.3f" % (statistics.median(res["this"]) / statistics.median(res["parent"])))
        print("\n".join(lines[-4:]), flush=True)
        flush()
    if not a.no_layers:
        for label, up, H, W, Cin, Cout in LAYERS:
            for stages, sname in ((2, "GEMM stage"), (1, "input transform"), (7, "whole conv")):
                res, mhz = layer_times(dev, up, H, W, Cin, Cout, stages, a.launches, a.rounds, clocks)
                lines.append("%s on %dx%d, %s, sclk %s MHz" % (label, H, W, sname, mhz))
                for k, v in res.items():
                    lines.append("    %-7s %s" % (k, base.fmt(v, "us")))
                lines.append("    fp32 / bf16x2 = %.2f, ranges %s" % (statistics.median(res["fp32"]) / statistics.median(res["bf16x2"]),
                                                                    "apart" if max(res["bf16x2"]) < min(res["fp32"]) or max(res["fp32"]) < min(res["bf16x2"]) else "overlap"))
                print("\n".join(lines[-4:]), flush=True)
                flush()
    if not a.no_frames:
        spec = GeneratorSpec(ngf=128, n_downsample=3, n_blocks=9, no_flow=False, norm="batch")
        sd = synthetic_state_dict(spec, seed=1, flow_gain=0.1)
        models = {"fp32": Vid2VidModelG([HipGenerator(spec, dev).load_state_dict(sd)]),
                  "trunk": Vid2VidModelG([HipGenerator(spec, dev, arith="bf16x2").load_state_dict(sd)]),
                  "trunk+stride2": Vid2VidModelG([HipGenerator(spec, dev, arith="bf16x2", arith_layers="trunk+stride2").load_state_dict(sd)])}
        for batch in (1, 2):
            res, mhz = base.frame_times(models, dev, batch, a.frames, a.warmup, a.rounds, clocks)
            lines.append("512x512 frames, flow on, %d sequence%s in lock-step, sclk %s MHz" % (batch, "s" if batch > 1 else "", mhz))
            for k, v in res.items():
                lines.append("    %-13s %s per sequence" % (k, base.fmt(v, "fps")))
            lines.append("    trunk+stride2 / trunk = %.3f, trunk / fp32 = %.3f" % (
                statistics.median(res["trunk+stride2"]) / statistics.median(res["trunk"]),
                statistics.median(res["trunk"]) / statistics.median(res["fp32"])))
            print("\n".join(lines[-5:]), flush=True)
            flush()


if __name__ == "__main__":
    main()
