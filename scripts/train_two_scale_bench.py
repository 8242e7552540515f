"""Time Vid2VidTrainer.train_step with two spatial scales (--n_scales_spatial 2: G0 on the half-size level, the local
enhancer G1 on the frame) on one GPU: 1 sequence, 2 frames per chunk, 2-scale discriminator, --no_vgg, zero reference flow
(the setting of BASELINE configs[4]), in the frozen phase (--fix_global: G0 does not train, --niter_fix_global) or the joint
one.  One phase and one size per process.
Usage: train_two_scale_bench.py [--size 512] [--fix_global] [--iters 5] [--n_blocks_local 3]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from text2video_amd import train as T
from text2video_amd.options import TrainOptions

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=512, help="the finest scale's frame (G0 runs at half of it)")
ap.add_argument("--frames", type=int, default=2)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--n_blocks_local", type=int, default=3)
ap.add_argument("--fix_global", action="store_true", help="the frozen phase: only G1 trains")
args = ap.parse_args()
opt = TrainOptions().parse(["--name", "b", "--dataset_mode", "pose", "--input_nc", "3", "--openpose_only", "--num_D", "2",
                            "--max_frames_per_gpu", str(args.frames), "--n_scales_temporal", "0", "--no_first_img", "--no_vgg",
                            "--fineSize", str(args.size), "--n_scales_spatial", "2", "--n_blocks_local", str(args.n_blocks_local),
                            "--niter_fix_global", "1" if args.fix_global else "0"])
dev = "cuda:0"
H = W = args.size
F = args.frames
tr = T.Vid2VidTrainer(opt, dev, seed=1)
assert tr.two_scale and tr.fix_global == args.fix_global
rng = np.random.default_rng(0)
pose = torch.zeros(F, H, W, 12, device=dev)
pose[..., :9] = torch.from_numpy(np.where(rng.random((F, H, W, 1)) < 0.02, rng.uniform(-1, 1, (F, H, W, 9)), -1.0).astype(np.float32)).to(dev)
real = torch.zeros(F, H, W, 4, device=dev)
real[..., :3] = torch.tanh(torch.from_numpy(rng.standard_normal((F, H, W, 3)).astype(np.float32))).to(dev)
real_prev = torch.cat([real[1:], real[:1]], 0).contiguous()
# a running sequence: non-zero FIFOs on both scales (zero previous frames make the image encoders' norms 0/0)
prev = [torch.zeros(1, H >> s, W >> s, 8, device=dev) for s in (0, 1)]
for p in prev:
    p[..., :6] = torch.tanh(torch.from_numpy(rng.standard_normal(tuple(p.shape[:3]) + (6,)).astype(np.float32))).to(dev)


def step():
    return tr.train_step(pose, real, None, (prev[0].clone(), prev[1].clone()), real_prev=real_prev)[0]


step(); step(); torch.cuda.synchronize()
torch.cuda.reset_peak_memory_stats()
from bench import ClockSampler
clock = ClockSampler(0, period=0.01)      # core clock from sysfs during the timed steps
starts = []
with clock:
    for _ in range(args.iters):
        starts.append(time.perf_counter())
        losses = step()      # (ends in the losses' read-back: the distance between two starts is one step)
    torch.cuda.synchronize()
    starts.append(time.perf_counter())
per_step = np.diff(np.array(starts)) * 1e3
n0, n1 = (sum(p.numel() for p in g.parameters()) for g in (tr.G.G0, tr.G.G1))
print("two-scale train step %dx%d (G0 on %dx%d), %d frames, %s phase, ngf %d, %d local blocks: median %.1f ms/step (min %.1f, max %.1f of "
      "%d; %s MHz), peak mem %.2f GB; %.1f M of G0's %.1f M + G1's %.1f M weights train | %s"
      % (H, W, H // 2, W // 2, F, "frozen-G0" if args.fix_global else "joint", opt.ngf, args.n_blocks_local, np.median(per_step),
         per_step.min(), per_step.max(), len(per_step), clock.mean_mhz(), torch.cuda.max_memory_allocated() / 2**30,
         sum(p.numel() for p in tr.optG.params) / 1e6, n0 / 1e6, n1 / 1e6, " ".join("%s %.3f" % kv for kv in losses.items())))
