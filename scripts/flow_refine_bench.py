"""Time ops.optical_flow with and without its Horn-Schunck refinement (t2v_optical_flow_refined, libt2v_flow.so) with HIP
events, per frame pair, default arguments (64 Jacobi steps per level, alpha 0.2): the LK entry, then the refined entry with
1, 2, 4, 8 steps per launch and with the library's choice.  One process; run it under a time limit:
    timeout -k 10 120 python scripts/flow_refine_bench.py [--size 512x512] [--reps 100]
Prints the launch count the header's formula gives, levels * (iters + 2 + ceil(refine_iters / k)) + 1, with every row, and
checks that every form returned the same bits."""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from bench import ClockSampler
from text2video_amd import _flowlib, ops

ap = argparse.ArgumentParser()
ap.add_argument("--size", default="512x512", help="HxW")
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--refine_iters", type=int, default=64)
ap.add_argument("--library_choice", type=int, default=8, help="what iters_per_launch = 0 stands for (for the launch count)")
args = ap.parse_args()
dev = "cuda:0"
clock = ClockSampler(0, period=0.01)      # core clock from sysfs while each timed loop runs
H, W = (int(v) for v in args.size.split("x"))
L, n = 1, (H, W)
while L < 6 and min((n[0] + 1) // 2, (n[1] + 1) // 2) >= 16:
    n, L = ((n[0] + 1) // 2, (n[1] + 1) // 2), L + 1
rng = np.random.default_rng(0)
# a smooth texture and the same texture two pixels further: a motion the estimator finds
base = torch.from_numpy(rng.standard_normal((H // 8 + 2, W // 8 + 2, 3)).astype(np.float32)).permute(2, 0, 1)[None]
big = torch.tanh(torch.nn.functional.interpolate(base, size=(H + 8, W + 8), mode="bicubic", align_corners=False))[0]
cur = torch.zeros(H, W, 4, device=dev)
prev = torch.zeros(H, W, 4, device=dev)
cur[..., :3] = big[:, 4:4 + H, 4:4 + W].permute(1, 2, 0).to(dev)
prev[..., :3] = big[:, 3:3 + H, 6:6 + W].permute(1, 2, 0).to(dev)
out = torch.empty(H, W, 4, device=dev)
first = None
forms = [("lk", {})] + [("refined, %s" % ("library's choice" if k == 0 else "%d per launch" % k),
                         dict(refine_iters=args.refine_iters, iters_per_launch=k))
                        for k in (1, 2, 4, _flowlib.MAX_FUSED, 0)]
for name, kw in forms:
    for _ in range(10):
        ops.optical_flow(cur, prev, out=out, **kw)
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    samp = clock.fork()
    with samp:
        t0.record()
        for a, b in evs:
            a.record()
            ops.optical_flow(cur, prev, out=out, **kw)
            b.record()
        t1.record()
        torch.cuda.synchronize()
    ms = np.array([a.elapsed_time(b) for a, b in evs])
    if kw:
        k = kw["iters_per_launch"] or args.library_choice
        launches = L * (3 + 2 + -(-args.refine_iters // k)) + 1
        same = "first refined form" if first is None else ("bits equal" if torch.equal(first, out) else "BITS DIFFER")
        first = out.clone() if first is None else first
    else:
        launches, same = L * 4 + 1, "-"
    print("optical_flow %dx%d %-28s %3d launches | per pair: median %.3f ms, p10 %.3f, p90 %.3f, back-to-back %.3f ms (%d calls) "
          "at %s MHz (%d clock samples) | %s" % (H, W, name + ":", launches, np.median(ms), np.percentile(ms, 10),
                                                 np.percentile(ms, 90), t0.elapsed_time(t1) / args.reps, args.reps,
                                                 samp.mean_mhz(), len(samp.samples), same), flush=True)
