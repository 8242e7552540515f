#!/usr/bin/env python
"""The step-time figures of profiles/train_display.txt: ms per optimiser step of the configs[4]-shaped train step (bench.py's
train_block geometry: 2 frames of 512x512, flow branch, 2-scale D + face D, --no_vgg; no gradient exchange), every step
timed by a host clock around step + device synchronise, one fresh process per figure:

    python scripts/train_display_step_time.py --tag off                                  # the step as it is
    python scripts/train_display_step_time.py --tag f100 --mode display --freq 100       # + TrainDisplay.show every 100 steps
    python scripts/train_display_step_time.py --tag parent --tree <checkout of another commit, built>

--tree: the checkout whose text2video_amd is measured (default: this one); --mode plain uses nothing a commit before
--display_web lacks.  Prints one line `STEPTIME {json}`."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--mode", default="plain")
ap.add_argument("--freq", type=int, default=100)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=6)
ap.add_argument("--ckpt", default=None, help="checkpoints_dir of the display (default: a temporary directory)")
ap.add_argument("--tag", required=True)
a = ap.parse_args()
if a.ckpt is None:
    import tempfile
    a.ckpt = tempfile.mkdtemp(prefix="train_display_")
sys.path.insert(0, os.path.abspath(a.tree))
import torch  # noqa: E402
from text2video_amd import train as T  # noqa: E402
from text2video_amd.options import TrainOptions  # noqa: E402
assert os.path.abspath(T.__file__).startswith(os.path.abspath(a.tree)), T.__file__

H = W = 512
F = 2
dev = torch.device("cuda:0")
argv = ["--name", "steptime_" + a.tag, "--checkpoints_dir", a.ckpt, "--dataset_mode", "pose", "--input_nc", "3", "--openpose_only",
        "--num_D", "2", "--max_frames_per_gpu", str(F), "--n_scales_temporal", "0", "--no_first_img", "--fineSize", str(H),
        "--no_vgg", "--add_face_disc", "--ngf", "128"]
if a.mode == "display":
    argv += ["--display_web", "--display_freq", str(a.freq)]
opt = TrainOptions().parse(argv)
tr = T.Vid2VidTrainer(opt, str(dev), seed=1)
display = None
if a.mode == "display":
    from text2video_amd.train_display import TrainDisplay
    display = TrainDisplay(opt)
    tr.keep_visuals = True
rng = np.random.default_rng(100)
pose = torch.zeros(F, H, W, 12, device=dev)
pose[..., :9] = torch.from_numpy(np.where(rng.random((F, H, W, 1)) < 0.02, rng.uniform(-1, 1, (F, H, W, 9)), -1.0).astype(np.float32)).to(dev)
real = torch.zeros(F, H, W, 4, device=dev)
real[..., :3] = torch.tanh(torch.from_numpy(rng.standard_normal((F, H, W, 3)).astype(np.float32))).to(dev)
real_prev = torch.cat([real[1:], real[:1]], 0).contiguous()
side = max(8, H // 32 * 8)
boxes = [(H // 8, H // 8 + side, (W - side) // 2, (W - side) // 2 + side)] * F
prev = torch.zeros(1, H, W, 8, device=dev)
prev[..., :6] = torch.tanh(torch.from_numpy(rng.standard_normal((1, H, W, 6)).astype(np.float32))).to(dev)

ms = []
for i in range(a.warmup + a.steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.train_step(pose, real, boxes, prev.clone(), real_prev=real_prev)
    k = i - a.warmup + 1
    shown = display is not None and k > 0 and k % a.freq == 0
    if shown:
        display.show(tr.visuals, 1, k)
    torch.cuda.synchronize()
    if i >= a.warmup:
        ms.append((1e3 * (time.perf_counter() - t0), shown))
if display is not None:
    display.close()
all_ms = np.array([m for m, _ in ms])
plain = np.array([m for m, s in ms if not s])
shown_ms = [round(m, 2) for m, s in ms if s]
res = {"tag": a.tag, "mode": a.mode, "freq": a.freq if a.mode == "display" else None, "steps": len(ms),
       "median_ms": round(float(np.median(all_ms)), 3), "mean_ms": round(float(all_ms.mean()), 3),
       "p05_ms": round(float(np.percentile(all_ms, 5)), 3), "p95_ms": round(float(np.percentile(all_ms, 95)), 3),
       "min_ms": round(float(all_ms.min()), 3), "max_ms": round(float(all_ms.max()), 3),
       "displays": len(shown_ms), "median_ms_of_displayed_steps": round(float(np.median(shown_ms)), 3) if shown_ms else None,
       "median_ms_of_other_steps": round(float(np.median(plain)), 3) if len(plain) else None}
if display is not None:
    web = os.path.join(a.ckpt, "steptime_" + a.tag, "web", "images")
    res["jpegs"] = len(os.listdir(web))
print("STEPTIME " + json.dumps(res), flush=True)
