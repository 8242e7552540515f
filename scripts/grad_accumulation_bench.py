"""Figures of profiles/grad_accumulation.txt: a train step of K clips per rank (--batchSize above the number of ranks) at the
512 x 512 configs[4] trainer of bench.py's train block (2 frames, flow branch, 2-scale D + face D, --no_vgg), one rank, no
process group.  HIP events around synchronised work, after warm-up.  One process per figure; run each under a time limit:
    timeout -k 10 120 python scripts/grad_accumulation_bench.py fold
    timeout -k 10 180 python scripts/grad_accumulation_bench.py step --K 1 [--steps 10] [--tree OTHER_CHECKOUT]
fold: t2v_grad_fold over the trainer's real bucket sizes, every mode, with the bytes it moves per second.
step: ms per optimiser step (K micro-steps) and per clip, and the peak device memory.  --tree: import the package from another
checkout with its libraries built (K = 1 only: the parent commit beside this one, alternating the two in one call)."""
import argparse, os, sys

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["fold", "step"])
ap.add_argument("--K", type=int, default=1)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--tag", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
import numpy as np
import torch
from text2video_amd import ops
from text2video_amd import train as T
from text2video_amd.options import TrainOptions

dev, H, W, F = "cuda:0", 512, 512, 2
opt = TrainOptions().parse(["--name", "bench", "--dataset_mode", "pose", "--input_nc", "3", "--openpose_only", "--num_D", "2",
                            "--max_frames_per_gpu", str(F), "--n_scales_temporal", "0", "--no_first_img", "--fineSize", str(H),
                            "--no_vgg", "--add_face_disc", "--ngf", "128"])
tr = T.Vid2VidTrainer(opt, dev, seed=1)


def events(fn, reps):
    """ms of each of `reps` calls of fn, every call between two events, synchronised before the first and after the last"""
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    torch.cuda.synchronize()
    marks[0].record()
    for r in range(reps):
        fn()
        marks[r + 1].record()
    torch.cuda.synchronize()
    return [marks[r].elapsed_time(marks[r + 1]) for r in range(reps)]


if args.what == "fold":
    sizes = [hi - lo for b in (tr.bucketsG, tr.bucketsD) for lo, hi in b.bounds]
    total = sum(sizes)
    print("buckets of the 512x512 configs[4] trainer: %d, %.1f MB in all; t2v_grad_fold, median of 50 launches" % (len(sizes), 4e-6 * total))
    grad, acc = torch.randn(total, device=dev), torch.randn(total, device=dev)
    for name, mode, streams in (("OPEN", ops.GRAD_FOLD_OPEN, 2), ("ADD", ops.GRAD_FOLD_ADD, 3), ("CLOSE", ops.GRAD_FOLD_CLOSE, 3)):
        per, off = [], 0
        for n in sizes:
            g, a = grad[off:off + n], acc[off:off + n]
            off += n
            for _ in range(5):
                ops.grad_fold(g, a, mode, 0.5)
            per.append((n, float(np.median(events(lambda: ops.grad_fold(g, a, mode, 0.5), 50)))))
        by_size = {}
        for n, ms in per:
            by_size.setdefault(n, []).append(ms)
        all_ms = sum(ms for _, ms in per)
        print("%-5s all buckets %.3f ms, %.2f TB/s (%d x 4 B x n)" % (name, all_ms, streams * 4e-9 * total / all_ms, streams))
        for n in sorted(by_size):
            ms = float(np.median(by_size[n]))
            print("      n = %9d (%6.1f MB) x %2d: %7.1f us, %.2f TB/s" % (n, 4e-6 * n, len(by_size[n]), 1e3 * ms, streams * 4e-9 * n / ms))
    # every bucket once, back to back: 2 x 1.49 GB pass through the caches, as in a micro-step; and, on the same box in the
    # same process, both optimisers' steps as the trainer calls them (t2v_adam_step_multi: p, g, m, v read, p, m, v written)
    def all_buckets(mode):
        off = 0
        for n in sizes:
            ops.grad_fold(grad[off:off + n], acc[off:off + n], mode, 0.5)
            off += n
    for name, mode, streams in (("OPEN", ops.GRAD_FOLD_OPEN, 2), ("ADD", ops.GRAD_FOLD_ADD, 3), ("CLOSE", ops.GRAD_FOLD_CLOSE, 3)):
        all_buckets(mode)
        ms = float(np.median(events(lambda: all_buckets(mode), 10)))
        print("%-5s one pass over all buckets back to back: %.3f ms, %.2f TB/s (%d x 4 B x n; median of 10 passes)"
              % (name, ms, streams * 4e-9 * total / ms, streams))
    nparam = 0
    for b in (tr.bucketsG, tr.bucketsD):
        for p, sl in zip(b.params, b.slots):
            p.grad = sl.view
            nparam += p.numel()

    def adam():
        tr.optG.step()
        tr.optD.step()
    for _ in range(3):
        adam()
    ms = float(np.median(events(adam, 10)))
    print("Adam  optG.step() + optD.step() over %.1f MB of parameters: %.3f ms, %.2f TB/s (7 x 4 B x n; median of 10)"
          % (4e-6 * nparam, ms, 7 * 4e-9 * nparam / ms))
    sys.exit(0)

K = args.K
clips = []
for s in range(K):
    rng = np.random.default_rng(100 + s)
    pose = torch.zeros(F, H, W, 12, device=dev)
    pose[..., :9] = torch.from_numpy(np.where(rng.random((F, H, W, 1)) < 0.02, rng.uniform(-1, 1, (F, H, W, 9)), -1.0)
                                     .astype(np.float32)).to(dev)
    real = torch.zeros(F, H, W, 4, device=dev)
    real[..., :3] = torch.tanh(torch.from_numpy(rng.standard_normal((F, H, W, 3)).astype(np.float32))).to(dev)
    prev = torch.zeros(1, H, W, 8, device=dev)
    prev[..., :6] = torch.tanh(torch.from_numpy(rng.standard_normal((1, H, W, 6)).astype(np.float32))).to(dev)
    clips.append((pose, real, torch.cat([real[1:], real[:1]], 0).contiguous(), prev))
side = max(8, H // 32 * 8)
boxes = [(H // 8, H // 8 + side, (W - side) // 2, (W - side) // 2 + side)] * F


def step():
    for j, (pose, real, real_prev, prev) in enumerate(clips):
        kw = {"micro": (j, K)} if K > 1 else {}      # (K = 1: the call the parent commit takes as well)
        tr.train_step(pose, real, boxes, prev.clone(), real_prev=real_prev, **kw)


import contextlib, io
with contextlib.redirect_stdout(io.StringIO()):          # (the zero-reference-flow notice)
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ms = events(step, args.steps)
med = float(np.median(ms))
print("%sK = %d: %.2f ms per optimiser step, %.2f ms per clip (median of %d; min %.2f, max %.2f); peak memory %.2f GB"
      % (args.tag, K, med, med / K, args.steps, min(ms), max(ms), torch.cuda.max_memory_allocated() / 2**30))
