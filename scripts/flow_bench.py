"""Time ops.optical_flow (t2v_optical_flow: dense coarse-to-fine Lucas-Kanade, the train step's --flow_ref lk) with HIP
events: per frame pair at 512x512, 512x680 and 1024x1024, default arguments.  One process; run it under a time limit:
    timeout -k 10 120 python scripts/flow_bench.py [--sizes 512x512,512x680,1024x1024] [--reps 200]
Prints the launch count the header's formula gives, levels * (iters + 1) + 1, to compare with a kernel trace."""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from bench import ClockSampler
from text2video_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="512x512,512x680,1024x1024", help="HxW, comma separated")
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--radius", type=int, default=3)
args = ap.parse_args()
dev = "cuda:0"
clock = ClockSampler(0, period=0.01)      # core clock from sysfs while each size's timed loop runs


def default_levels(h, w):
    n = 1
    while n < 6 and min((h + 1) // 2, (w + 1) // 2) >= 16:
        h, w, n = (h + 1) // 2, (w + 1) // 2, n + 1
    return n


for size in args.sizes.split(","):
    H, W = (int(v) for v in size.split("x"))
    rng = np.random.default_rng(0)
    # a smooth texture and the same texture two pixels further: a motion the estimator finds
    base = torch.from_numpy(rng.standard_normal((H // 8 + 2, W // 8 + 2, 3)).astype(np.float32)).permute(2, 0, 1)[None]
    big = torch.tanh(torch.nn.functional.interpolate(base, size=(H + 8, W + 8), mode="bicubic", align_corners=False))[0]
    cur = torch.zeros(H, W, 4, device=dev)
    prev = torch.zeros(H, W, 4, device=dev)
    cur[..., :3] = big[:, 4:4 + H, 4:4 + W].permute(1, 2, 0).to(dev)
    prev[..., :3] = big[:, 3:3 + H, 6:6 + W].permute(1, 2, 0).to(dev)
    out = torch.empty(H, W, 4, device=dev)
    for _ in range(10):
        ops.optical_flow(cur, prev, iters=args.iters, radius=args.radius, out=out)
    torch.cuda.synchronize()
    # per-call times from event pairs: median and spread, plus the back-to-back rate of the whole run
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    samp = clock.fork()
    with samp:
        t0.record()
        for a, b in evs:
            a.record()
            ops.optical_flow(cur, prev, iters=args.iters, radius=args.radius, out=out)
            b.record()
        t1.record()
        torch.cuda.synchronize()
    ms = np.array([a.elapsed_time(b) for a, b in evs])
    L = default_levels(H, W)
    f = out[..., :2]
    print("optical_flow %dx%d: levels %d, iters %d, radius %d, %d launches per call | per pair: median %.3f ms, p10 %.3f, p90 %.3f, "
          "back-to-back %.3f ms (%d calls) at %s MHz (%d clock samples) | mean flow (%.2f, %.2f) px"
          % (H, W, L, args.iters, args.radius, L * (args.iters + 1) + 1, np.median(ms), np.percentile(ms, 10),
             np.percentile(ms, 90), t0.elapsed_time(t1) / args.reps, args.reps, samp.mean_mhz(), len(samp.samples), f[..., 0].mean().item(), f[..., 1].mean().item()),
          flush=True)
