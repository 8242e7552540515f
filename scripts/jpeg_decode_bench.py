#!/usr/bin/env python
"""The figures of profiles/jpeg_decode.txt, from one job on one GPU:

    python scripts/jpeg_decode_bench.py [--pairs 200] [--rounds 3] [--parent-root DIR] [--train [--train-rounds 3]] [--out FILE]

1. `python -m text2video_amd.evaluate` over --pairs pairs of 512x512 JPEG files (smooth-plus-noise frames, quality 75 against
   quality 95), alternating: this checkout without the flag, with --gpu_decode and, with --parent-root DIR, the same command
   from another built checkout (the parent commit).  Wall time and the CPU seconds of the child (user + system); the reports
   of the two commands of this checkout are compared.
2. --train: `train.py --train_loader prefetch --gpu_resize` with and without --gpu_decode by scripts/train_loader_bench.py's
   method (its --run mode, as child processes), alternating, on 384x512 and 1280x720 sources; process CPU seconds and the
   bytes a clip uploads either way.
3. GPU time of one ops.jpeg_decode_u8 call for 1 and 12 frames at quality 75 and 95: device events around 200 back-to-back
   calls on one stream -- and per kernel from a run of its own under `rocprofv3 --kernel-trace --stats` (a fresh child
   process; skipped with a note where rocprofv3 is missing).  Beside them Pillow's decode of the same files on one core.
Every block carries the core clock sampled around it where sysfs shows one.
"""
import argparse
import csv
import glob
import io
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
H = W = 512
CONFIGS = ((1, 75), (12, 75), (1, 95), (12, 95))


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


def frame_like(n, seed=0):
    """n uint8 [H,W,3] images with the statistics of a generated frame: smooth shapes plus a little noise"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for i in range(n):
        img = np.stack([127 + 90 * np.sin(xx / (23.0 + i) + c) * np.cos(yy / (31.0 + c)) for c in range(3)], -1)
        out.append(np.clip(np.rint(img + rng.normal(0.0, 4.0, (H, W, 3))), 0, 255).astype(np.uint8))
    return out


def files(n, quality, seed=0):
    from PIL import Image
    out = []
    for img in frame_like(n, seed):
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="JPEG", quality=quality)
        out.append(buf.getvalue())
    return out


def packed(n, quality):
    import torch
    from text2video_amd import jpeg_decode
    blobs = files(n, quality)
    (g,), refused = jpeg_decode.pack(blobs)
    assert not refused
    dev = g.host.to("cuda", non_blocking=True)
    dst = torch.empty(n, H, W, 3, dtype=torch.uint8, device="cuda")
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    return blobs, g, dev, dst, status


def call_times(emit):
    import torch
    from text2video_amd import jpeg_decode
    os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})      # Pillow's figure is one core's
    for n, q in CONFIGS:
        blobs, g, dev, dst, status = packed(n, q)
        for _ in range(20):
            jpeg_decode.decode_uploaded(g, dev, 3, dst=dst, status=status)
        torch.cuda.synchronize()
        exact = all(np.array_equal(dst[i].cpu().numpy(), jpeg_decode.pillow_rgb(b)) for i, b in enumerate(blobs))
        reps, clk0 = [], sclk_mhz()
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(200):
                jpeg_decode.decode_uploaded(g, dev, 3, dst=dst, status=status)
            e1.record()
            e1.synchronize()
            reps.append(e0.elapsed_time(e1) * 1000.0 / 200)
        t0 = time.perf_counter()
        for _ in range(5):
            for b in blobs:
                jpeg_decode.pillow_rgb(b)
        pil = (time.perf_counter() - t0) * 1e6 / 5
        emit("jpeg_decode_u8 %dx%d x %d, quality %d: %.1f us per call (1 memset + 8 launches; 5 x 200 back-to-back calls: %s); status %s, "
             "equal to Pillow %s; scan bytes %s, capacity %d; Pillow on one core: %.0f us for the same %d file(s); sclk %s -> %s MHz"
             % (H, W, n, q, sorted(reps)[2], " ".join("%.1f" % r for r in reps), sorted(set(status.cpu().tolist())), exact,
                g.lengths().tolist(), g.capacity, pil, n, clk0, sclk_mhz()))


def trace_worker(n, q, calls):
    """what the per-kernel run traces: `calls` decode calls of one configuration"""
    import torch
    from text2video_amd import jpeg_decode
    _, g, dev, dst, status = packed(n, q)
    for _ in range(calls):
        jpeg_decode.decode_uploaded(g, dev, 3, dst=dst, status=status)
    torch.cuda.synchronize()


def kernel_times(emit, scratch):
    prof = shutil.which("rocprofv3")
    if prof is None:
        emit("per-kernel times: not measured (no rocprofv3 on PATH)")
        return
    for n, q in CONFIGS:
        d = os.path.join(scratch, "trace_%d_%d" % (n, q))
        p = subprocess.run([prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "jpegdec", "--",
                            sys.executable, os.path.abspath(__file__), "--trace-worker", str(n), str(q)],
                           capture_output=True, text=True, timeout=300)
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if p.returncode != 0 or not stats:
            emit("per-kernel times x %d, quality %d: not measured (rocprofv3 exit %d: %s)" % (n, q, p.returncode, p.stderr[-300:]))
            return
        rows = [r for r in csv.DictReader(open(stats[0])) if "jpegdec_" in r.get("Name", "")]
        parts = ["%s %.1f" % (r["Name"].split("jpegdec_")[1].split("(")[0], float(r["AverageNs"]) / 1e3) for r in rows]
        total = sum(float(r["TotalDurationNs"]) for r in rows) / 1e3 / 100
        emit("kernels %dx%d x %d, quality %d, avg us over 100 traced calls (sync_kernel runs twice per call): %s; sum per call %.1f us"
             % (H, W, n, q, ", ".join(parts), total))


def evaluate_runs(emit, pairs, rounds, parent_root, work):
    from PIL import Image
    for d, q in (("a", 75), ("b", 95)):
        os.makedirs(os.path.join(work, d, "seq"))
        for i, img in enumerate(frame_like(pairs, seed=1)):
            Image.fromarray(img).save(os.path.join(work, d, "seq", "fake_B_%04d.jpg" % i), quality=q)
    variants = [("plain       ", ROOT, []), ("--gpu_decode", ROOT, ["--gpu_decode"])]
    if parent_root:
        variants.append(("parent      ", parent_root, []))
    rows, reports = {name: [] for name, _, _ in variants}, {}
    for r in range(rounds):
        for name, root, extra in variants:
            out = os.path.join(work, "report.json")
            clk0, ru0, t0 = sclk_mhz(), resource.getrusage(resource.RUSAGE_CHILDREN), time.perf_counter()
            p = subprocess.run([sys.executable, "-m", "text2video_amd.evaluate", os.path.join(work, "a"), os.path.join(work, "b"),
                                "--json", out] + extra, cwd=root, capture_output=True, text=True, timeout=600)
            wall, ru1 = time.perf_counter() - t0, resource.getrusage(resource.RUSAGE_CHILDREN)
            if p.returncode != 0:
                emit("FAILED evaluate %s (%d): %s" % (name, p.returncode, (p.stdout + p.stderr)[-1500:]))
                return 1
            cpu = (ru1.ru_utime - ru0.ru_utime) + (ru1.ru_stime - ru0.ru_stime)
            reports[name] = json.load(open(out))
            rows[name].append((wall, cpu))
            emit("evaluate %s round %d: %d pairs of %dx%d, wall %.2f s, process CPU %.2f s, psnr %.4f, sclk %s -> %s MHz%s"
                 % (name, r, reports[name]["overall"]["frames"], H, W, wall, cpu, reports[name]["overall"]["psnr"], clk0, sclk_mhz(),
                    (" [" + p.stderr.strip().splitlines()[-1] + "]") if p.stderr.strip() else ""))
    for name in rows:
        walls = sorted(v[0] for v in rows[name])
        emit("median %s: wall %.2f s (min %.2f, max %.2f), process CPU %.2f s" % (name, walls[len(walls) // 2], walls[0], walls[-1],
                                                                               sorted(v[1] for v in rows[name])[len(walls) // 2]))
    emit("reports of plain and --gpu_decode equal: %s" % (reports["plain       "] == reports["--gpu_decode"]))
    return 0


def train_runs(emit, rounds, work):
    from text2video_amd import jpeg
    bench = os.path.join(ROOT, "scripts", "train_loader_bench.py")
    for src in ("384x512", "1280x720"):
        data = os.path.join(work, "train_" + src)
        p = subprocess.run([sys.executable, bench, "--make", data, "--src", src], capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            emit("FAILED --make %s: %s" % (src, (p.stdout + p.stderr)[-800:]))
            return 1
        scans = [jpeg.parse(open(f, "rb").read()).scan_length for f in sorted(glob.glob(os.path.join(data, "train_img", "*", "*.jpg")))[:60]]
        w, h = (int(v) for v in src.split("x"))
        emit("H2D bytes per frame at %s: raw %d, compressed %.0f (mean scan %.0f + %d table and length bytes); per 14-frame clip %.2f MB "
             "against %.2f MB" % (src, h * w * 3, np.mean(scans) + jpeg.TABLE_BYTES + 4, np.mean(scans), jpeg.TABLE_BYTES + 4,
                                  14 * h * w * 3 / 1e6, 14 * (np.mean(scans) + jpeg.TABLE_BYTES + 4) / 1e6))
        for r in range(rounds):
            for name, extra in (("--gpu_resize             ", "--train_loader prefetch --gpu_resize"),
                                ("--gpu_resize --gpu_decode", "--train_loader prefetch --gpu_resize --gpu_decode")):
                ru0 = resource.getrusage(resource.RUSAGE_CHILDREN)
                p = subprocess.run([sys.executable, bench, "--dataroot", data, "--run", ROOT, "--extra", extra, "--clips", "5",
                                    "--tag", "%s round %d" % (src, r)], capture_output=True, text=True, timeout=900)
                ru1 = resource.getrusage(resource.RUSAGE_CHILDREN)
                cpu = (ru1.ru_utime - ru0.ru_utime) + (ru1.ru_stime - ru0.ru_stime)
                res = [line for line in p.stdout.splitlines() if line.startswith("RESULT")]
                if p.returncode != 0 or not res:
                    emit("FAILED train %s %s: %s" % (src, name, (p.stdout + p.stderr)[-1500:]))
                    return 1
                emit("train %s %s; process CPU %.1f s" % (name, res[-1][len("RESULT "):], cpu))
    return 0


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--trace-worker":
        trace_worker(int(sys.argv[2]), int(sys.argv[3]), 100)
        return 0
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit to run evaluate from")
    ap.add_argument("--train", action="store_true", help="also time train.py with and without --gpu_decode")
    ap.add_argument("--train-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    work = tempfile.mkdtemp(prefix="t2v_jpegdec_bench_")
    try:
        rc = evaluate_runs(emit, args.pairs, args.rounds, args.parent_root, work)      # (before this process opens the GPU itself)
        if rc == 0 and args.train:
            rc = train_runs(emit, args.train_rounds, work)
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
