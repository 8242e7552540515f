#!/usr/bin/env python
"""The figures of profiles/temporal_metrics.txt, from one job on one GPU:

    python scripts/temporal_metrics_bench.py [--frames 170] [--out FILE]

1. fps_loop of the `vid2vid/test.py` command on a two-sequence utterance at 512x320 (the reference's geometry), with
   --metrics and with --metrics_temporal, alternating, full-size generator on seeded weights, with the loop's host-time
   split.  The real frames are seeded noise JPEGs of 512x384 (the worst case for the decoder threads).
2. ops.temporal_metrics (two launches) per 512x512 and 512x320 pair of pairs, with and without one 128x128 box, and the
   three ops.optical_flow_u8 calls a frame of the loop enqueues: device events around back-to-back calls on one stream, with
   the core clock sampled while they run.
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from image_metrics_bench import make_dataset  # noqa: E402  (the same utterance as profiles/image_metrics.txt)


def _timed(torch, clock, fn, calls, reps=5):
    for _ in range(50):
        fn()
    torch.cuda.synchronize()
    out = []
    samp = clock.fork()
    with samp:
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1) * 1000.0 / calls)
    return out, samp


def kernel_times(emit):
    import torch
    from bench import ClockSampler
    from text2video_amd import ops
    clock = ClockSampler(0, period=0.01)
    emit("device: %s" % json.dumps(clock.ident))
    rng = np.random.default_rng(0)
    for H, W in ((512, 512), (512, 320)):
        # a smooth texture and the same texture moved by a few pixels, as bytes: motions the estimator finds
        ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)

        def tex(dx, dy, gain):
            g = 128 + gain * (np.sin((xs + dx) / 9.0) * np.cos((ys + dy) / 7.0) + 0.5 * np.sin((xs + dx + ys + dy) / 13.0))
            return np.clip(np.stack([g, 0.9 * g + 5, 0.8 * g + 20], -1) + rng.integers(-2, 3, (H, W, 3)), 0, 255).astype(np.uint8)
        b_cur, b_prev = torch.from_numpy(tex(0, 0, 60)).cuda(), torch.from_numpy(tex(1.5, -1.0, 60)).cuda()
        a4 = [np.concatenate([tex(dx, dy, 55), np.zeros((H, W, 1), np.uint8)], -1) for dx, dy in ((0, 0), (1.2, -1.3))]
        a_cur, a_prev = (torch.from_numpy(a).cuda() for a in a4)
        flows = [torch.empty(H, W, 4, device="cuda") for _ in range(3)]

        def three_flows():
            ops.optical_flow_u8(b_cur, b_prev, out=flows[0])
            ops.optical_flow_u8(b_prev, b_cur, out=flows[1])
            ops.optical_flow_u8(a_cur, a_prev, out=flows[2])
        reps, samp = _timed(torch, clock, three_flows, 100)
        emit("3 x optical_flow_u8 %dx%d (real t->t-1, real t-1->t, generated t->t-1): %.1f us (5 x 100 back-to-back triples: %s) "
             "at %s MHz (%d clock samples)" % (H, W, sorted(reps)[2], " ".join("%.1f" % r for r in reps), samp.mean_mhz(),
                                               len(samp.samples)))
        for boxes in ((), ((190, 318, 96, 224),)):
            out = torch.empty(1 + len(boxes), 6, dtype=torch.float64, device="cuda")

            def call():
                ops.temporal_metrics(a_cur, a_prev, b_cur, b_prev, flows[0], flows[1], flows[2], boxes, out=out)
            reps, samp = _timed(torch, clock, call, 500)
            row = out.cpu().numpy()[0]
            emit("temporal_metrics %dx%d, %d box: %.1f us per call (two launches; 5 x 500 back-to-back calls: %s) at %s MHz "
                 "(%d clock samples); frame summary %s"
                 % (H, W, len(boxes), sorted(reps)[2], " ".join("%.1f" % r for r in reps), samp.mean_mhz(), len(samp.samples),
                    json.dumps(ops.temporal_summary(row, H * W))))


def command_fps(emit, frames, rounds):
    work = tempfile.mkdtemp(prefix="t2v_temporal_bench_")
    try:
        make_dataset(work, frames)
        cmd = [sys.executable, os.path.join(ROOT, "vid2vid", "test.py"), "--name", "fadg0", "--dataroot", "datasets/fadg0",
               "--dataset_mode", "pose", "--input_nc", "3", "--resize_or_crop", "scaleHeight", "--loadSize", "512",
               "--openpose_only", "--how_many", "1200", "--no_first_img", "--random_drop_prob", "0", "--synthetic_weights", "1",
               "--timing_json", "timing.json"]
        fps = {"--metrics": [], "--metrics_temporal": []}
        for r in range(rounds):
            for flag in ("--metrics", "--metrics_temporal"):
                shutil.rmtree(os.path.join(work, "results"), ignore_errors=True)
                t0 = time.perf_counter()
                p = subprocess.run(cmd + [flag], cwd=work, capture_output=True, text=True, timeout=300)
                if p.returncode != 0:
                    emit("FAILED (%d): %s" % (p.returncode, (p.stdout + p.stderr)[-1500:]))
                    return 1
                t = json.load(open(os.path.join(work, "timing.json")))
                fps[flag].append(t["fps_loop"])
                emit("test.py %-18s round %d: %d frames, fps_loop %.1f, loop split %s, wall %.2f s%s"
                     % (flag, r, t["frames"], t["fps_loop"], json.dumps(t["cold_start"]["loop_split"]), time.perf_counter() - t0,
                        (", temporal summary tmp: " + json.dumps(t["metrics"]["tmp"]["temporal"]))
                        if flag == "--metrics_temporal" and r == 0 else ""))
        emit("fps_loop median: --metrics %.1f, --metrics_temporal %.1f"
             % tuple(sorted(fps[k])[len(fps[k]) // 2] for k in ("--metrics", "--metrics_temporal")))
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
        kernel_times(emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
