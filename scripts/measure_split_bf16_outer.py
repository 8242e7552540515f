"""The direct stride-2 / transposed 128 <-> 256 layers in fp32 (T2V_ALGO_DIRECT) against split-bf16 (T2V_ALGO_DIRECT_BF16X2) on one
MI355X, by the method of scripts/measure_split_bf16_stride2.py: ONE process, the forms alternating and warmed, the median of
--rounds rounds with min and max beside it, the core clock sampled during every timed loop.

  * per layer class (128 -> 256 and 256 -> 128 transposed at 512x512, 512x320, 512x680 and 1024x1024): the norm apply pass in
    front of the layer + the whole conv with bias and statistics partials, as the generator runs them -- fp32 apply + fp32 conv
    against split-emitting apply + split conv -- and the conv alone.  One extra row: the same layer forced to
    T2V_ALGO_POLYPHASE_BF16X2, which takes the pending norm in its input transform (no apply pass);
  * whole 512x512 frames with the flow branch in fp32, arith_layers="trunk+stride2" and arith_outer=True, one sequence and two
    in lock-step;
  * --parent TREE: TREE/bench.py against this tree's in alternating child processes (the default fp32 path).
    python scripts/measure_split_bf16_outer.py --parent ../parent --out profiles/split_bf16_outer_times.txt
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
LAYERS = [("512x512 down1 128 -> 256", False, 512, 512, 128, 256), ("512x512 up3 256 -> 128", True, 256, 256, 256, 128),
          ("512x320 down1 128 -> 256", False, 512, 320, 128, 256), ("512x320 up3 256 -> 128", True, 256, 160, 256, 128),
          ("512x680 down1 128 -> 256", False, 512, 680, 128, 256), ("512x680 up3 256 -> 128", True, 256, 340, 256, 128),
          ("1024x1024 down1 128 -> 256", False, 1024, 1024, 128, 256), ("1024x1024 up3 256 -> 128", True, 512, 512, 256, 128)]


def layer_runs(dev, up, H, W, Cin, Cout, with_apply):
    """{form: callable}: one launch sequence of the layer per form"""
    g = torch.Generator().manual_seed(1)
    raw = torch.randn(H, W, Cin, generator=g).to(dev)
    mr = torch.stack([torch.randn(Cin, generator=g) * 0.3, torch.rand(Cin, generator=g) + 0.5], -1).to(dev).contiguous()
    w = (torch.randn(*((Cin, Cout, 3, 3) if up else (Cout, Cin, 3, 3)), generator=g) * (9 * Cin) ** -0.5).to(dev)
    b = torch.zeros(Cout, device=dev)
    mk = lambda algo: ops.conv_desc(H, W, Cin, Cout, 3, 2, 1, ops.PAD_ZERO, up, algo=algo)
    d0, d6, d5 = mk(ops.ALGO_DIRECT), mk(ops.ALGO_DIRECT_BF16X2), mk(ops.ALGO_POLYPHASE_BF16X2)
    ho, wo = ops.conv_out_dims(d0)
    runs = {}
    xa, y0, st0, p0 = torch.empty_like(raw), torch.empty(ho, wo, Cout, device=dev), ops.conv_stats_buffer(d0, dev), ops.pack_conv_weight(w, d0, Cin)
    ops.instance_norm_apply(raw, mr, relu=True, out=xa)

    def fp32():
        if with_apply:
            ops.instance_norm_apply(raw, mr, relu=True, out=xa)
        ops.conv2d(xa, p0, b, d0, y_cs=Cout, stats=st0, out=y0)
    runs["fp32"] = fp32
    xp, y6, st6, p6 = torch.empty_like(raw), torch.empty(ho, wo, Cout, device=dev), ops.conv_stats_buffer(d6, dev), ops.pack_conv_weight(w, d6, Cin)
    ops.instance_norm_apply_bf16x2(raw, mr, relu=True, out=xp)

    def split():
        if with_apply:
            ops.instance_norm_apply_bf16x2(raw, mr, relu=True, out=xp)
        ops.conv2d_winograd(xp, p6, b, d6, stats=st6, out=y6, workspace=xp, stages=6)      # (6: the workspace holds the pairs)
    runs["bf16x2"] = split
    if with_apply and ops.polyphase_bf16x2_supported(d5, Cin):
        p5, ws5 = ops.pack_conv_weight(w, d5, Cin), ops.winograd_batch_workspace(d5, Cin, 1, dev)
        y5, st5, mr1 = torch.empty(1, ho, wo, Cout, device=dev), ops.conv_stats_buffer(d5, dev), mr.view(1, Cin, 2)
        runs["polyphase bf16x2"] = lambda: ops.conv2d_winograd_batch(raw.unsqueeze(0), p5, b, d5, ws5, stats=st5, out=y5, stages=7,
                                                                     mean_rstd=mr1, relu=1)
    return runs


def layer_times(runs, launches, rounds, clocks):
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
    assert torch.cuda.is_available(), "measure_split_bf16_outer.py needs a GPU"
    dev = torch.device("cuda:0")
    clocks = bench.ClockSampler(0)
    lines = ["split-bf16 direct stride-2 / transposed convs against fp32, one process, alternating rounds; %s" % clocks.ident]

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
            for with_apply, sname in ((True, "apply pass + whole conv"), (False, "whole conv alone")):
                res, mhz = layer_times(layer_runs(dev, up, H, W, Cin, Cout, with_apply), a.launches, a.rounds, clocks)
                lines.append("%s on %dx%d, %s, sclk %s MHz" % (label, H, W, sname, mhz))
                for k, v in res.items():
                    lines.append("    %-16s %s" % (k, base.fmt(v, "us")))
                apart = max(res["bf16x2"]) < min(res["fp32"]) or max(res["fp32"]) < min(res["bf16x2"])
                lines.append("    fp32 / bf16x2 = %.2f, ranges %s" % (statistics.median(res["fp32"]) / statistics.median(res["bf16x2"]),
                                                                    "apart" if apart else "overlap"))
                print("\n".join(lines[-(len(res) + 2):]), flush=True)
                flush()
                torch.cuda.empty_cache()
    if not a.no_frames:
        spec = GeneratorSpec(ngf=128, n_downsample=3, n_blocks=9, no_flow=False, norm="batch")
        sd = synthetic_state_dict(spec, seed=1, flow_gain=0.1)
        scope = dict(arith="bf16x2", arith_layers="trunk+stride2")
        models = {"fp32": Vid2VidModelG([HipGenerator(spec, dev).load_state_dict(sd)]),
                  "trunk+stride2": Vid2VidModelG([HipGenerator(spec, dev, **scope).load_state_dict(sd)]),
                  "arith_outer": Vid2VidModelG([HipGenerator(spec, dev, arith_outer=True, **scope).load_state_dict(sd)])}
        for batch in (1, 2):
            res, mhz = base.frame_times(models, dev, batch, a.frames, a.warmup, a.rounds, clocks)
            lines.append("512x512 frames, flow on, %d sequence%s in lock-step, sclk %s MHz" % (batch, "s" if batch > 1 else "", mhz))
            for k, v in res.items():
                lines.append("    %-13s %s per sequence" % (k, base.fmt(v, "fps")))
            lines.append("    arith_outer / trunk+stride2 = %.3f, trunk+stride2 / fp32 = %.3f" % (
                statistics.median(res["arith_outer"]) / statistics.median(res["trunk+stride2"]),
                statistics.median(res["trunk+stride2"]) / statistics.median(res["fp32"])))
            print("\n".join(lines[-5:]), flush=True)
            flush()


if __name__ == "__main__":
    main()
