"""Real-data training: what the loader costs per optimiser step, and what --train_loader prefetch / --gpu_resize hide.

  --make DIR [--src 384x512] [--seqs 3] [--frames 60]
        write a recipe-sized dataset: DIR/train_openpose/<seq>/*.json + DIR/train_img/<seq>/*.jpg, the frames rendered from
        the golden key points (tests/golden/keypoints_fadg0) on a --src = WxH canvas over a noise background (JPEG decoding
        and the resize then cost what photographs cost)
  --dataroot DIR --run TREE [--extra "--train_loader prefetch --gpu_resize"] [--clips 6]
        TREE/vid2vid/train.py (this checkout: `.`; or another one, e.g. the parent commit) as a child process on the
        reference's recipe (--loadSize 544 --fineSize 512 --n_frames_total 12 --max_frames_per_gpu 2, full-width nets): the
        wall time of every clip as train.py reports it (loader + upload + all optimiser steps of the clip), the time per
        optimiser step over whole clips (first clip dropped: warm-up), the core clock sampled here while the child runs
  --dataroot DIR --floor [--clips 6]
        the same trainer stepping over the same clips held in device memory (no loader, no upload): the floor
  --kernel [--src 384x512]
        ops.resample_crop_normalize_u8 alone on a recipe clip (14 frames, 544-high resize, 512-high crop): device events
Every mode ends in one line starting with "RESULT" that a driver can append to profiles/train_loader_times.txt."""
import argparse
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--make", default=None)
ap.add_argument("--src", default="384x512")
ap.add_argument("--seqs", type=int, default=3)
ap.add_argument("--frames", type=int, default=60)
ap.add_argument("--dataroot", default=None)
ap.add_argument("--run", default=None)
ap.add_argument("--floor", action="store_true")
ap.add_argument("--kernel", action="store_true")
ap.add_argument("--extra", default="")
ap.add_argument("--clips", type=int, default=6)
ap.add_argument("--nThreads", type=int, default=4)
ap.add_argument("--tag", default="")
args = ap.parse_args()


def recipe(dataroot, ckpt):
    return ["--name", "loader_bench", "--dataroot", dataroot, "--checkpoints_dir", ckpt, "--dataset_mode", "pose", "--input_nc",
            "3", "--openpose_only", "--num_D", "2", "--resize_or_crop", "randomScaleHeight_and_scaledCrop", "--loadSize", "544",
            "--fineSize", "512", "--batchSize", "1", "--max_frames_per_gpu", "2", "--no_first_img", "--n_frames_total", "12",
            "--max_t_step", "4", "--add_face_disc", "--random_drop_prob", "0", "--vgg_random_init", "--niter_decay", "0",
            "--save_latest_freq", "1000000", "--save_epoch_freq", "1000000", "--nThreads", str(args.nThreads)]


def report(what, clip_ms, chunks_per_clip, mhz, more=""):
    import numpy as np
    ms = np.array(clip_ms[1:], float)          # the first clip carries the warm-up
    per_step = ms / chunks_per_clip
    print("RESULT %s%s: %d clips of %d optimiser steps after 1 warm-up clip: %.1f ms/step (median clip %.1f, min %.1f, max %.1f "
          "ms/step), clips %s ms, %s MHz%s" % (what, (" [" + args.tag + "]") if args.tag else "", len(ms), chunks_per_clip,
                                               ms.sum() / (len(ms) * chunks_per_clip), np.median(per_step), per_step.min(),
                                               per_step.max(), " ".join("%.0f" % v for v in clip_ms), mhz, more), flush=True)


if args.make:
    import shutil
    import numpy as np
    from PIL import Image
    from text2video_amd.keypoints import read_keypoints
    w, h = (int(v) for v in args.src.split("x"))
    gold = os.path.join(ROOT, "tests", "golden", "keypoints_fadg0")
    files = sorted(f for f in os.listdir(gold) if f.endswith(".json"))
    rng = np.random.default_rng(0)
    back = np.clip(rng.normal(128, 40, (h, w, 3)), 0, 255).astype(np.uint8)
    n = 0
    for s in range(args.seqs):
        seq = "seq%02d" % s
        os.makedirs(os.path.join(args.make, "train_openpose", seq), exist_ok=True)
        os.makedirs(os.path.join(args.make, "train_img", seq), exist_ok=True)
        for i in range(args.frames):
            f = files[(s * 7 + i) % len(files)]
            shutil.copyfile(os.path.join(gold, f), os.path.join(args.make, "train_openpose", seq, "%04d_keypoints.json" % i))
            m = read_keypoints(os.path.join(gold, f), (w, h))
            img = np.where(m.any(-1, keepdims=True), m, np.roll(back, 3 * i, 1))
            Image.fromarray(img).save(os.path.join(args.make, "train_img", seq, "%04d.jpg" % i), quality=90)
            n += 1
    print("wrote %d frames of %dx%d in %d sequences under %s" % (n, w, h, args.seqs, args.make))
    sys.exit(0)

if args.run:
    import tempfile
    import torch
    from bench import ClockSampler
    tree = os.path.abspath(args.run)
    n_seqs = len(os.listdir(os.path.join(args.dataroot, "train_openpose")))
    clock = ClockSampler(0, period=0.05)        # (sysfs only: this process runs nothing on the device)
    with tempfile.TemporaryDirectory() as ckpt:
        # an epoch is one clip per sequence: the run ends by itself after ceil(clips / sequences) epochs
        cmd = [sys.executable, os.path.join(tree, "vid2vid", "train.py")] + recipe(os.path.abspath(args.dataroot), ckpt) \
            + ["--niter", str(-(-args.clips // n_seqs))] + args.extra.split()
        with clock:
            r = subprocess.run(cmd, cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    clip_ms, chunks = [], 0
    for line in r.stdout.splitlines():
        m = re.match(r"\(iter \d+, epoch \d+, seq \S+, (\d+) frames .*?, (\d+) ms,", line)
        if m:
            clip_ms.append(float(m.group(2)))
            chunks = -(-int(m.group(1)) // 2)
    if r.returncode != 0 or len(clip_ms) < 2:
        sys.exit("train.py ended with status %d:\n%s" % (r.returncode, r.stdout[-3000:]))
    report("%s/vid2vid/train.py %s" % (args.run, args.extra or "(default loader)"), clip_ms, chunks, clock.mean_mhz())
    sys.exit(0)

import numpy as np
import torch
from bench import ClockSampler
from text2video_amd import ops

if args.kernel:
    from text2video_amd.pose_dataset import get_train_img_params
    from text2video_amd.options import TrainOptions
    w, h = (int(v) for v in args.src.split("x"))
    opt = TrainOptions().parse(recipe("none", "none"))
    rng = np.random.default_rng(0)
    prm = get_train_img_params(opt, (w, h), rng)
    prm["new_size"] = (int(round(544 * w / h / 4)) * 4, 544)          # the largest resize the recipe draws
    prm["crop_pos"] = (min(prm["crop_pos"][0], prm["new_size"][0] - prm["crop_size"][0]), 16)
    src = torch.from_numpy(rng.integers(0, 256, (14, h, w, 3), dtype=np.uint8)).cuda()
    out = torch.zeros(14, prm["crop_size"][1], prm["crop_size"][0], 4, device="cuda")
    for _ in range(3):
        ops.resample_crop_normalize_u8(src, prm["new_size"], prm["crop_pos"], prm["crop_size"], out=out)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(50)]
    clock = ClockSampler(0, period=0.01)
    with clock:
        for a, b in ev:
            a.record()
            ops.resample_crop_normalize_u8(src, prm["new_size"], prm["crop_pos"], prm["crop_size"], out=out)
            b.record()
        torch.cuda.synchronize()
    k = np.array([a.elapsed_time(b) for a, b in ev])
    mb = (src.numel() + out.numel() * 4) / 1e6
    print("RESULT resample kernel%s: 14 frames %dx%d -> %dx%d, crop %dx%d at %s, %d x %d taps: %.3f ms per clip (median of 50 single "
          "launches between events, min %.3f, max %.3f), %.1f MB read + written = %.0f GB/s, %s MHz"
          % ((" [" + args.tag + "]") if args.tag else "", w, h, prm["new_size"][0], prm["new_size"][1], prm["crop_size"][0],
             prm["crop_size"][1], prm["crop_pos"], ops.pillow_bicubic_taps(w, prm["new_size"][0]),
             ops.pillow_bicubic_taps(h, prm["new_size"][1]), np.median(k), k.min(), k.max(), mb, mb / np.median(k), clock.mean_mhz()))
    sys.exit(0)

from text2video_amd import train as T
from text2video_amd.options import TrainOptions
import tempfile

if not args.floor:
    sys.exit("one of --make, --run, --floor, --kernel")
opt = TrainOptions().parse(recipe(args.dataroot, tempfile.mkdtemp()))
clock = ClockSampler(0, period=0.01)

# ---- floor: the same clips, already on the device
from text2video_amd.pose_dataset import TrainPoseDataset
dev = "cuda:0"
torch.cuda.set_device(0)
trainer = T.Vid2VidTrainer(opt, dev)
ds = TrainPoseDataset(opt, seed=1000)
tG, F_ = opt.n_frames_G, opt.max_frames_per_gpu
clips = []
for i in range(args.clips):
    c = ds.sample(i)
    A = torch.from_numpy(c["A"]).to(dev)
    real_all = torch.zeros(A.shape[0], A.shape[1], A.shape[2], 4, device=dev)
    real_all[..., :3] = (torch.from_numpy(c["B"]).to(dev).float() / 255.0 - 0.5) / 0.5
    clips.append((c, A, real_all))
clip_ms, chunks = [], 0
with clock:
    for c, A, real_all in clips:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        T_, H, W = A.shape[0], A.shape[1], A.shape[2]
        prev, chunks = None, 0
        for c0 in range(tG - 1, T_, F_):
            fr = list(range(c0, min(c0 + F_, T_)))
            pose = torch.zeros(len(fr), H, W, 12, device=dev)
            for j, t in enumerate(fr):
                for f in range(tG):
                    ops.pose_u8_to_f32(A[t - tG + 1 + f], pose[j], 3 * f)
            box = T.get_face_region(c["A"][fr], opt.fineSize)
            losses, prev = trainer.train_step(pose, real_all[fr[0]:fr[-1] + 1], [box] * len(fr) if box is not None else None, prev,
                                              real_prev=real_all[fr[0] - 1:fr[-1]])
            chunks += 1
        torch.cuda.synchronize()
        clip_ms.append((time.perf_counter() - t0) * 1e3)
report("floor (clips in device memory)", clip_ms, chunks, clock.mean_mhz())
