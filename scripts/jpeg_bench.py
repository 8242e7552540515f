#!/usr/bin/env python
"""The figures of profiles/jpeg_encode.txt, from one job on one GPU:

    python scripts/jpeg_bench.py [--frames 90] [--rounds 3] [--parent-root DIR] [--out FILE]

1. `vid2vid/test.py` on the one-sequence 512x320 dataset of scripts/e2e_bench.py (full-size generator, seeded weights), plain
   and with --gpu_jpeg, alternating: fps_loop, finish_s, d2h_s, jpeg_s, D2H bytes per frame (all from --timing_json) and the
   CPU seconds of the process and its children (user + system).  --parent-root DIR: the same command from another checkout
   (the parent commit, built) joins the alternation.
2. Scan bytes of a generated frame and of a pose map (the files of the last --gpu_jpeg run).
3. GPU time of one ops.jpeg_encode_u8 call at 512x512, 512x680 and 512x320 for 1, 2 and 4 images: device events around
   back-to-back calls on one stream, on a generated-frame-like image (smooth + noise) -- and per kernel from a run of its
   own under `rocprofv3 --kernel-trace --stats` (a fresh child process; skipped with a note where rocprofv3 is missing).
Every block carries the core clock sampled around it where sysfs shows one.
"""
import argparse
import csv
import glob
import json
import os
import resource
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GEOMETRIES = ((512, 512), (512, 680), (512, 320))
BATCHES = (1, 2, 4)


def sclk_mhz():
    """the current core clock of card 0 from sysfs (the line marked '*' of pp_dpm_sclk), or None"""
    for path in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk")):
        try:
            for line in open(path):
                if line.rstrip().endswith("*"):
                    return int(line.split(":")[1].strip().lower().replace("mhz", "").split()[0])
        except (OSError, ValueError, IndexError):
            continue
    return None


def frame_like(H, W, n, seed=0):
    """n uint8 [H,W,4] images with the statistics of a generated frame: smooth shapes plus a little noise"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for i in range(n):
        img = np.stack([127 + 90 * np.sin(xx / (23.0 + i) + c) * np.cos(yy / (31.0 + c)) for c in range(3)], -1)
        img = img + rng.normal(0.0, 4.0, (H, W, 3))
        out.append(np.concatenate([np.clip(np.rint(img), 0, 255).astype(np.uint8), np.zeros((H, W, 1), np.uint8)], -1))
    return np.stack(out)


def call_times(emit):
    import torch
    from text2video_amd import ops
    for H, W in GEOMETRIES:
        for n in BATCHES:
            x = torch.from_numpy(frame_like(H, W, n)).cuda()
            out = torch.empty(n, ops.jpeg_scan_capacity(H, W), dtype=torch.uint8, device="cuda")
            lengths = torch.empty(n, dtype=torch.int32, device="cuda")
            for _ in range(20):
                ops.jpeg_encode_u8(x, 75, out=out, lengths=lengths)
            torch.cuda.synchronize()
            reps, clk0 = [], sclk_mhz()
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(200):
                    ops.jpeg_encode_u8(x, 75, out=out, lengths=lengths)
                e1.record()
                e1.synchronize()
                reps.append(e0.elapsed_time(e1) * 1000.0 / 200)
            emit("jpeg_encode_u8 %dx%d x %d, quality 75: %.1f us per call (1 memset + 7 launches; 5 x 200 back-to-back calls: %s); "
                 "scan bytes %s; sclk %s -> %s MHz" % (H, W, n, sorted(reps)[2], " ".join("%.1f" % r for r in reps),
                                                        lengths.cpu().tolist(), clk0, sclk_mhz()))


def trace_worker(H, W, n, calls):
    """what the per-kernel run traces: `calls` encode calls of one configuration"""
    import torch
    from text2video_amd import ops
    x = torch.from_numpy(frame_like(H, W, n)).cuda()
    for _ in range(calls):
        ops.jpeg_encode_u8(x, 75)
    torch.cuda.synchronize()


def kernel_times(emit, scratch):
    prof = shutil.which("rocprofv3")
    if prof is None:
        emit("per-kernel times: not measured (no rocprofv3 on PATH)")
        return
    for H, W in GEOMETRIES:
        for n in BATCHES:
            d = os.path.join(scratch, "trace_%dx%dx%d" % (H, W, n))
            p = subprocess.run([prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "jpeg", "--",
                                sys.executable, os.path.abspath(__file__), "--trace-worker", str(H), str(W), str(n)],
                               capture_output=True, text=True, timeout=300)
            stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            if p.returncode != 0 or not stats:
                emit("per-kernel times %dx%d x %d: not measured (rocprofv3 exit %d: %s)" % (H, W, n, p.returncode, p.stderr[-300:]))
                return
            rows = [r for r in csv.DictReader(open(stats[0])) if "jpeg_" in r.get("Name", "")]
            parts = ["%s %.1f" % (r["Name"].split("jpeg_")[1].split("(")[0], float(r["AverageNs"]) / 1e3) for r in rows]
            total = sum(float(r["TotalDurationNs"]) for r in rows) / 1e3 / 100
            emit("kernels %dx%d x %d, avg us over 100 traced calls (scan_kernel runs twice per call): %s; sum per call %.1f us"
                 % (H, W, n, ", ".join(parts), total))


def make_dataset(work, frames):
    from PIL import Image
    from text2video_amd.keypoints import read_keypoints
    src = os.path.join(ROOT, "tests", "golden", "keypoints_fadg0")
    files = sorted(f for f in os.listdir(src) if f.startswith("sa1_"))
    root = os.path.join(work, "datasets", "fadg0")
    os.makedirs(os.path.join(root, "test_openpose", "tmp"))
    os.makedirs(os.path.join(root, "test_img", "tmp"))
    img = Image.fromarray(read_keypoints(os.path.join(src, files[0]), (512, 384)))
    for i in range(frames):
        shutil.copyfile(os.path.join(src, files[i % len(files)]), os.path.join(root, "test_openpose", "tmp", "%05d.json" % i))
        img.save(os.path.join(root, "test_img", "tmp", "%04d.jpg" % i))


def command_runs(emit, frames, rounds, parent_root, work):
    make_dataset(work, frames)
    base = ["--name", "fadg0", "--dataroot", "datasets/fadg0", "--dataset_mode", "pose", "--input_nc", "3", "--resize_or_crop",
            "scaleHeight", "--loadSize", "512", "--openpose_only", "--how_many", "1200", "--no_first_img", "--random_drop_prob",
            "0", "--synthetic_weights", "1", "--timing_json", "timing.json"]
    variants = [("plain     ", ROOT, []), ("--gpu_jpeg", ROOT, ["--gpu_jpeg"])]
    if parent_root:
        variants.append(("parent    ", parent_root, []))
    rows = {name: [] for name, _, _ in variants}
    for r in range(rounds):
        for name, root, extra in variants:
            shutil.rmtree(os.path.join(work, "results"), ignore_errors=True)
            clk0, ru0, t0 = sclk_mhz(), resource.getrusage(resource.RUSAGE_CHILDREN), time.perf_counter()
            p = subprocess.run([sys.executable, os.path.join(root, "vid2vid", "test.py")] + base + extra, cwd=work,
                               capture_output=True, text=True, timeout=600)
            wall, ru1 = time.perf_counter() - t0, resource.getrusage(resource.RUSAGE_CHILDREN)
            if p.returncode != 0:
                emit("FAILED %s (%d): %s" % (name, p.returncode, (p.stdout + p.stderr)[-1500:]))
                return 1
            t = json.load(open(os.path.join(work, "timing.json")))
            sp = t["cold_start"]["loop_split"]
            cpu = (ru1.ru_utime - ru0.ru_utime) + (ru1.ru_stime - ru0.ru_stime)
            rows[name].append((t["fps_loop"], sp["finish_s"], sp.get("d2h_s", 0.0), cpu))
            emit("test.py %s round %d: %d frames, fps_loop %.1f, finish_s %.3f, d2h_s %.4f, jpeg_s %s, second copies %s, D2H bytes per "
                 "frame %s, process CPU %.2f s, wall %.2f s, sclk %s -> %s MHz"
                 % (name, r, t["frames"], t["fps_loop"], sp["finish_s"], sp.get("d2h_s", 0.0), sp.get("jpeg_s", "-"),
                    sp.get("jpeg_second_copies", "-"), t["cold_start"].get("d2h_bytes_per_frame", "-"), cpu, wall, clk0, sclk_mhz()))
            if extra:
                sizes = {label: sorted(os.path.getsize(f) - 625 for f in glob.glob(os.path.join(
                    work, "results", "fadg0", "test_latest", "tmp", label + "_*.jpg"))) for label in ("fake_B", "real_A")}
    for name in rows:
        med = [sorted(v[i] for v in rows[name])[len(rows[name]) // 2] for i in range(4)]
        emit("median %s: fps_loop %.1f, finish_s %.3f, d2h_s %.4f, process CPU %.2f s" % ((name,) + tuple(med)))
    for label, v in sizes.items():
        emit("scan bytes, %s at 512x320 (seeded weights), quality 75: min %d, median %d, max %d" % (label, v[0], v[len(v) // 2], v[-1]))
    return 0


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--trace-worker":
        trace_worker(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), 100)
        return 0
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=90)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit to run the same command from")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    work = tempfile.mkdtemp(prefix="t2v_jpeg_bench_")
    try:
        rc = command_runs(emit, args.frames, args.rounds, args.parent_root, work)      # (before this process opens the GPU itself)
        if rc == 0:
            kernel_times(emit, work)
            call_times(emit)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
