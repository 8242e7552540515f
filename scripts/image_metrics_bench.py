#!/usr/bin/env python
"""The figures of profiles/image_metrics.txt, from one job on one GPU:

    python scripts/image_metrics_bench.py [--frames 170] [--out FILE]

1. ops.image_metrics (two launches) per 512x512 and 512x320 pair, with and without one 128x128 box: device events around
   back-to-back calls on one stream.
2. fps_loop of the `vid2vid/test.py` command on a two-sequence utterance at 512x320 (the reference's geometry), with and
   without --metrics, alternating, full-size generator on seeded weights.  The real frames are seeded noise JPEGs of 512x384
   (the worst case for the decoder threads: a camera frame of this size decodes faster).
3. The host work --metrics adds to the loop's thread per frame, alone.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden", "dataset_fadg0_l2", "test_openpose")


def kernel_times(emit):
    import torch
    from text2video_amd import ops
    rng = np.random.default_rng(0)
    for H, W in ((512, 512), (512, 320)):
        a = torch.from_numpy(rng.integers(0, 256, (H, W, 4), dtype=np.uint8)).cuda()
        b = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda()
        for boxes in ((), ((190, 318, 96, 224),)):
            out = torch.empty(1 + len(boxes), 4, dtype=torch.float64, device="cuda")
            for _ in range(50):
                ops.image_metrics(a, b, boxes, out=out)
            torch.cuda.synchronize()
            reps = []
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(500):
                    ops.image_metrics(a, b, boxes, out=out)
                e1.record()
                e1.synchronize()
                reps.append(e0.elapsed_time(e1) * 1000.0 / 500)
            emit("image_metrics %dx%d, %d box: %.1f us per call (two launches; 5 x 500 back-to-back calls: %s)"
                 % (H, W, len(boxes), sorted(reps)[2], " ".join("%.1f" % r for r in reps)))


def host_pieces(emit):
    """the host work --metrics adds per frame besides the decoder threads, alone on this host"""
    from text2video_amd import metrics as M
    from text2video_amd.keypoints import read_keypoints
    from text2video_amd.pose_dataset import central_crop_cols
    from PIL import Image
    src = os.path.join(GOLD, "tmp", sorted(os.listdir(os.path.join(GOLD, "tmp")))[2])
    m = np.asarray(Image.fromarray(read_keypoints(src, (512, 384))).resize((680, 512), Image.NEAREST))
    c0, c1 = central_crop_cols(680)
    m = np.ascontiguousarray(m[:, c0:c1])
    real, stage = np.random.default_rng(0).integers(0, 256, m.shape, dtype=np.uint8), np.empty_like(m)
    for what, fn in (("face_box(pose map)", lambda: M.face_box(m)), ("copy into the pinned stage", lambda: np.copyto(stage, real))):
        t0 = time.perf_counter()
        for _ in range(200):
            fn()
        emit("host, per 512x320 frame: %s %.3f ms" % (what, (time.perf_counter() - t0) * 5.0))


def make_dataset(work, frames):
    from PIL import Image
    root = os.path.join(work, "datasets", "fadg0")
    rng = np.random.default_rng(3)
    for seq, pat in (("tmp", "%04d.jpg"), ("tmp_smooth", "smooth_%04d.jpg")):
        src = sorted(os.listdir(os.path.join(GOLD, seq)))
        os.makedirs(os.path.join(root, "test_openpose", seq))
        os.makedirs(os.path.join(root, "test_img", seq))
        for i in range(frames):
            j = i % (2 * len(src) - 2)        # back and forth over the fixture's frames
            j = j if j < len(src) else 2 * len(src) - 2 - j
            shutil.copyfile(os.path.join(GOLD, seq, src[j]), os.path.join(root, "test_openpose", seq, "%05d.json" % i))
            Image.fromarray(rng.integers(0, 256, (384, 512, 3), dtype=np.uint8)).save(
                os.path.join(root, "test_img", seq, pat % i), quality=90)


def command_fps(emit, frames, rounds):
    work = tempfile.mkdtemp(prefix="t2v_metrics_bench_")
    try:
        make_dataset(work, frames)
        cmd = [sys.executable, os.path.join(ROOT, "vid2vid", "test.py"), "--name", "fadg0", "--dataroot", "datasets/fadg0",
               "--dataset_mode", "pose", "--input_nc", "3", "--resize_or_crop", "scaleHeight", "--loadSize", "512",
               "--openpose_only", "--how_many", "1200", "--no_first_img", "--random_drop_prob", "0", "--synthetic_weights", "1",
               "--timing_json", "timing.json"]
        fps = {False: [], True: []}
        for r in range(rounds):
            for metrics in (False, True):
                shutil.rmtree(os.path.join(work, "results"), ignore_errors=True)
                t0 = time.perf_counter()
                p = subprocess.run(cmd + (["--metrics"] if metrics else []), cwd=work, capture_output=True, text=True, timeout=300)
                if p.returncode != 0:
                    emit("FAILED (%d): %s" % (p.returncode, (p.stdout + p.stderr)[-1500:]))
                    return 1
                t = json.load(open(os.path.join(work, "timing.json")))
                fps[metrics].append(t["fps_loop"])
                emit("test.py %s round %d: %d frames, fps_loop %.1f, loop split %s, wall %.2f s%s"
                     % ("--metrics" if metrics else "plain    ", r, t["frames"], t["fps_loop"],
                        json.dumps(t["cold_start"]["loop_split"]), time.perf_counter() - t0,
                        (", summary tmp: " + json.dumps(t["metrics"]["tmp"])) if metrics and r == 0 else ""))
        emit("fps_loop median: plain %.1f, --metrics %.1f" % (sorted(fps[False])[len(fps[False]) // 2],
                                                             sorted(fps[True])[len(fps[True]) // 2]))
        return 0
    finally:
        shutil.rmtree(work, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=170, help="pose frames per sequence (two sequences)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    rc = command_fps(emit, args.frames, args.rounds)      # (before this process opens the GPU itself)
    if rc == 0:
        host_pieces(emit)
        kernel_times(emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
