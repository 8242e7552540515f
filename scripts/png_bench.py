#!/usr/bin/env python
"""The figures of profiles/png_encode.txt, from one job on one GPU:

    python scripts/png_bench.py [--frames 90] [--rounds 3] [--out FILE]

1. `vid2vid/test.py` on the one-sequence 512x320 dataset of scripts/jpeg_bench.py (full-size generator, seeded weights):
   plain, with --gpu_jpeg and with --frame_format png, alternating: fps_loop, finish_s, d2h_s, png_s / jpeg_s, D2H bytes per
   frame (all from --timing_json) and the file sizes of the PNG run.
2. GPU time of one ops.png_encode_u8 call at 512x512 and 512x680 for 1, 2 and 8 images: device events around back-to-back
   calls on one stream, on a generated-frame-like image (smooth + noise), the committed crop tiled, and a pose map -- and
   per kernel from a run of its own under `rocprofv3 --kernel-trace --stats` (a fresh child process; skipped with a note
   where rocprofv3 is missing).
3. The yardstick on this host's CPU: Pillow's Image.save(..., "PNG") at its default and at compress_level=1 on the same
   images, one core, and its file sizes beside the writer's.
Every GPU block carries the core clock sampled around it where sysfs shows one.
"""
import argparse
import csv
import glob
import io
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from jpeg_bench import frame_like, make_dataset, sclk_mhz      # noqa: E402

GEOMETRIES = ((512, 512), (512, 680))
BATCHES = (1, 2, 8)
LAUNCHES = "1 memset + 7 launches"


def images(kind, H, W, n):
    """n uint8 [H,W,4] images"""
    if kind == "frame-like":
        return frame_like(H, W, n)
    if kind == "crop tiled":
        import png_reference as R
        crop = R.make_image("crop", 128, 128)
        img = np.tile(crop, ((H + 127) // 128, (W + 127) // 128, 1))[:H, :W]
    else:
        m = np.load(os.path.join(ROOT, "tests", "golden", "pose_maps_fadg0.npz"))["maps"][0]
        img = np.tile(m, ((H + m.shape[0] - 1) // m.shape[0], (W + m.shape[1] - 1) // m.shape[1], 1))[:H, :W]
    img = np.concatenate([img, np.zeros((H, W, 1), np.uint8)], -1)
    return np.stack([np.roll(img, 7 * i, axis=1) for i in range(n)])


def pillow_times(emit, img, label):
    from PIL import Image
    im = Image.fromarray(np.ascontiguousarray(img[..., :3]))
    out = []
    for kw, name in (({}, "default"), ({"compress_level": 1}, "compress_level=1")):
        reps = []
        for _ in range(5):
            buf = io.BytesIO()
            t0 = time.perf_counter()
            im.save(buf, "PNG", **kw)
            reps.append((time.perf_counter() - t0) * 1e3)
        out.append("%s %.1f ms, %d bytes" % (name, sorted(reps)[2], len(buf.getvalue())))
    emit("Pillow Image.save(PNG), one core, %s: %s" % (label, "; ".join(out)))


def call_times(emit):
    import torch
    from text2video_amd import ops
    for H, W in GEOMETRIES:
        for kind in ("frame-like", "crop tiled", "pose map"):
            for n in BATCHES if kind == "frame-like" else (1,):
                host = images(kind, H, W, n)
                x = torch.from_numpy(host).cuda()
                out = torch.empty(n, ops.png_file_capacity(H, W), dtype=torch.uint8, device="cuda")
                lengths = torch.empty(n, dtype=torch.int32, device="cuda")
                for _ in range(20):
                    ops.png_encode_u8(x, out=out, lengths=lengths)
                torch.cuda.synchronize()
                reps, clk0 = [], sclk_mhz()
                for _ in range(5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(100):
                        ops.png_encode_u8(x, out=out, lengths=lengths)
                    e1.record()
                    e1.synchronize()
                    reps.append(e0.elapsed_time(e1) * 1000.0 / 100)
                emit("png_encode_u8 %dx%d x %d, %s: %.1f us per call (%s; 5 x 100 back-to-back calls: %s); file bytes %s; "
                     "sclk %s -> %s MHz" % (H, W, n, kind, sorted(reps)[2], LAUNCHES, " ".join("%.1f" % r for r in reps),
                                            lengths.cpu().tolist(), clk0, sclk_mhz()))
                if n == 1:
                    pillow_times(emit, host[0], "%dx%d %s" % (H, W, kind))


def trace_worker(H, W, n, calls):
    import torch
    from text2video_amd import ops
    x = torch.from_numpy(frame_like(H, W, n)).cuda()
    for _ in range(calls):
        ops.png_encode_u8(x)
    torch.cuda.synchronize()


def kernel_times(emit, scratch):
    prof = shutil.which("rocprofv3")
    if prof is None:
        emit("per-kernel times: not measured (no rocprofv3 on PATH)")
        return
    for H, W, n in ((512, 512, 1), (512, 512, 8), (512, 680, 1)):
        d = os.path.join(scratch, "trace_%dx%dx%d" % (H, W, n))
        p = subprocess.run([prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "png", "--",
                            sys.executable, os.path.abspath(__file__), "--trace-worker", str(H), str(W), str(n)],
                           capture_output=True, text=True, timeout=300)
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if p.returncode != 0 or not stats:
            emit("per-kernel times %dx%d x %d: not measured (rocprofv3 exit %d: %s)" % (H, W, n, p.returncode, p.stderr[-300:]))
            return
        rows = [r for r in csv.DictReader(open(stats[0])) if "png_" in r.get("Name", "")]
        parts = ["%s %.1f" % (r["Name"].split("png_")[1].split("(")[0], float(r["AverageNs"]) / 1e3) for r in rows]
        total = sum(float(r["TotalDurationNs"]) for r in rows) / 1e3 / 100
        emit("kernels %dx%d x %d, avg us over 100 traced calls: %s; sum per call %.1f us" % (H, W, n, ", ".join(parts), total))


def command_runs(emit, frames, rounds, work):
    make_dataset(work, frames)
    base = ["--name", "fadg0", "--dataroot", "datasets/fadg0", "--dataset_mode", "pose", "--input_nc", "3", "--resize_or_crop",
            "scaleHeight", "--loadSize", "512", "--openpose_only", "--how_many", "1200", "--no_first_img", "--random_drop_prob",
            "0", "--synthetic_weights", "1", "--timing_json", "timing.json"]
    variants = [("plain             ", []), ("--gpu_jpeg        ", ["--gpu_jpeg"]), ("--frame_format png", ["--frame_format", "png"])]
    rows = {name: [] for name, _ in variants}
    sizes = {}
    for r in range(rounds):
        for name, extra in variants:
            shutil.rmtree(os.path.join(work, "results"), ignore_errors=True)
            clk0, t0 = sclk_mhz(), time.perf_counter()
            p = subprocess.run([sys.executable, os.path.join(ROOT, "vid2vid", "test.py")] + base + extra, cwd=work,
                               capture_output=True, text=True, timeout=600)
            wall = time.perf_counter() - t0
            if p.returncode != 0:
                emit("FAILED %s (%d): %s" % (name, p.returncode, (p.stdout + p.stderr)[-1500:]))
                return 1
            t = json.load(open(os.path.join(work, "timing.json")))
            sp = t["cold_start"]["loop_split"]
            rows[name].append((t["fps_loop"], sp["finish_s"], sp.get("d2h_s", 0.0)))
            emit("test.py %s round %d: %d frames, fps_loop %.1f, finish_s %.3f, d2h_s %.4f, encode enqueue %s s, second copies %s, "
                 "D2H bytes per frame %s, wall %.2f s, sclk %s -> %s MHz"
                 % (name, r, t["frames"], t["fps_loop"], sp["finish_s"], sp.get("d2h_s", 0.0), sp.get("png_s", sp.get("jpeg_s", "-")),
                    sp.get("png_second_copies", sp.get("jpeg_second_copies", "-")), t["cold_start"].get("d2h_bytes_per_frame", "-"),
                    wall, clk0, sclk_mhz()))
            if "png" in extra:
                sizes = {label: sorted(os.path.getsize(f) for f in glob.glob(os.path.join(
                    work, "results", "fadg0", "test_latest", "tmp", label + "_*.png"))) for label in ("fake_B", "real_A")}
    for name in rows:
        med = [sorted(v[i] for v in rows[name])[len(rows[name]) // 2] for i in range(3)]
        emit("median %s: fps_loop %.1f, finish_s %.3f, d2h_s %.4f" % ((name,) + tuple(med)))
    for label, v in sizes.items():
        emit("file bytes, %s.png at 512x320 (seeded weights): min %d, median %d, max %d" % (label, v[0], v[len(v) // 2], v[-1]))
    return 0


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--trace-worker":
        trace_worker(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), 100)
        return 0
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=90)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    work = tempfile.mkdtemp(prefix="t2v_png_bench_")
    try:
        rc = command_runs(emit, args.frames, args.rounds, work)      # (before this process opens the GPU itself)
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
