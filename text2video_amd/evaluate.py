"""python -m text2video_amd.evaluate DIR_A DIR_B [--pattern 'fake_B_*'] [--temporal] [--gpu_decode] [--json OUT]

PSNR / SSIM / MAE between the image files of two result trees, paired by relative path: the picture-level answer to "what
does --arith bf16x2 do to my model" (the same test.py command run twice) and "epoch 20 against epoch 40".  The files are
decoded with Pillow and compared on the GPU by the kernel of `test.py --metrics` (ops.image_metrics, whole frame only).
Prints and (--json) writes one summary per sequence (= directory) and one overall.  Unpaired files and pairs of different
sizes are listed and make the exit status 1.

--gpu_decode reads the files as bytes and decodes the JPEG ones on the GPU, in batches (jpeg_decode.decode_files: Pillow's
bytes, so the report is the same value for value); files the decoder does not take -- other formats, progressive or grey
JPEGs, code streams that do not synchronise -- go through Pillow as without the flag.

--temporal adds the temporal-consistency figures of `test.py --metrics_temporal` (ops.optical_flow_u8 + ops.temporal_metrics):
within each directory, files that are consecutive in the sorted paired list form the pairs (t-1, t); A = DIR_A is read against
B = DIR_B, whose flows give the forward-backward mask.  Every summary gains a "temporal" entry, pooled over sums.
"""
import argparse
import fnmatch
import json
import os
import sys

IMG_EXT = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".tiff")


def list_images(root, pattern):
    """relative paths (posix separators) of the image files under `root` whose base name matches `pattern`"""
    out = []
    for d, _, files in os.walk(root):
        for f in files:
            if f.lower().endswith(IMG_EXT) and fnmatch.fnmatch(f, pattern):
                out.append(os.path.relpath(os.path.join(d, f), root).replace(os.sep, "/"))
    return sorted(out)


def pair_files(dir_a, dir_b, pattern="fake_B_*", by_stem=False):
    """-> (paired relative paths, only under dir_a, only under dir_b), each sorted.
    by_stem: files pair when their relative paths agree up to the extension (a tree of .png frames against one of .jpg
    frames); a pair is then the tuple (path under dir_a, path under dir_b).  Of several files of one tree with the same
    stem, the first in sorted order pairs and the others count as unpaired."""
    a, b = list_images(dir_a, pattern), list_images(dir_b, pattern)
    if by_stem:
        first_a, first_b = {}, {}
        for paths, first in ((a, first_a), (b, first_b)):
            for p in paths:
                first.setdefault(os.path.splitext(p)[0], p)
        return ([(first_a[k], first_b[k]) for k in sorted(first_a) if k in first_b],
                [p for p in a if first_a[os.path.splitext(p)[0]] != p or os.path.splitext(p)[0] not in first_b],
                [p for p in b if first_b[os.path.splitext(p)[0]] != p or os.path.splitext(p)[0] not in first_a])
    sa, sb = set(a), set(b)
    return [p for p in a if p in sb], [p for p in a if p not in sb], [p for p in b if p not in sa]


MIN_FLOW_SIDE = 8        # ops.optical_flow_u8 refuses smaller frames
DECODE_BATCH = 32        # pairs per jpeg_decode.decode_files call under --gpu_decode


def _decoded_pairs(pairs, dir_a, dir_b, device, gpu_decode, fallback):
    """pairs: [(path under dir_a, path under dir_b)].  yield (the path under dir_a, a, b): the two RGB images uint8 [H,W,3]
    of every pair -- host arrays from Pillow, or device tensors from the GPU decoder (`fallback` collects the files Pillow
    decoded for it)"""
    import numpy as np
    if not gpu_decode:
        from PIL import Image
        for rel, rel_b in pairs:
            with Image.open(os.path.join(dir_a, rel)) as im:
                a = np.array(im.convert("RGB"))
            with Image.open(os.path.join(dir_b, rel_b)) as im:
                b = np.array(im.convert("RGB"))
            yield rel, a, b
        return
    from . import jpeg_decode
    for at in range(0, len(pairs), DECODE_BATCH):
        batch = pairs[at:at + DECODE_BATCH]
        files = [os.path.join(dir_a, rel) for rel, _ in batch] + [os.path.join(dir_b, rel) for _, rel in batch]
        blobs = []
        for f in files:
            with open(f, "rb") as fh:
                blobs.append(fh.read())
        tensors, fell = jpeg_decode.decode_files(blobs, device)
        fallback.extend((files[i], reason) for i, reason in fell)
        for j, (rel, _) in enumerate(batch):
            yield rel, tensors[j], tensors[len(batch) + j]


def compare_trees(dir_a, dir_b, pattern="fake_B_*", device="cuda:0", temporal=False, gpu_decode=False, fallback=None,
                  temporal_flow="lk", pair_by_stem=False):
    """-> the report: {"definition", "overall", "sequences": {dir: summary}, "unpaired_a", "unpaired_b", "size_mismatch"};
    temporal: every summary gains "temporal" (metrics.pool_temporal over the directory's consecutive pairs), the report
    "temporal_definition", "temporal_flow" (the estimator: lk, or lkhs = ops.optical_flow_u8 with the Horn-Schunck refinement)
    and "temporal_skipped" (second files of pairs that changed size or are narrower than 8 pixels).
    gpu_decode: decode on the GPU (the same report); `fallback`, a list, receives (file, reason) of what Pillow decoded then;
    pair_by_stem: pair_files(by_stem=True) -- the report names a pair by its path under dir_a"""
    from ._xp import torch
    from . import metrics as M
    from . import ops
    pairs, only_a, only_b = pair_files(dir_a, dir_b, pattern, pair_by_stem)
    if not pair_by_stem:
        pairs = [(p, p) for p in pairs]
    flow_kw = ops.temporal_flow_kwargs(temporal_flow)
    per_seq, mismatch, pending = {}, [], []
    t_pending, t_skipped, last = [], [], None      # last: (directory, device a, device b) of the previous paired file
    for rel, a, b in _decoded_pairs(pairs, dir_a, dir_b, device, gpu_decode, [] if fallback is None else fallback):
        if tuple(a.shape) != tuple(b.shape):
            mismatch.append({"file": rel, "a": [a.shape[1], a.shape[0]], "b": [b.shape[1], b.shape[0]]})
            last = None
            continue
        da, db = (a, b) if gpu_decode else (torch.from_numpy(a).to(device), torch.from_numpy(b).to(device))
        row = ops.image_metrics(da, db)
        pending.append((rel, 3 * a.shape[0] * a.shape[1], row))
        if temporal:
            seq = os.path.dirname(rel) or "."
            if last is not None and last[0] == seq:
                if tuple(last[1].shape) != tuple(a.shape) or min(a.shape[:2]) < MIN_FLOW_SIDE:
                    t_skipped.append(rel)
                else:
                    pa, pb = last[1], last[2]
                    trow = ops.temporal_metrics(da, pa, db, pb, ops.optical_flow_u8(db, pb, **flow_kw),
                                                ops.optical_flow_u8(pb, db, **flow_kw), ops.optical_flow_u8(da, pa, **flow_kw))
                    t_pending.append((seq, a.shape[0] * a.shape[1], trow))
            last = (seq, da, db)
    for rel, n_values, row in pending:       # (the copies wait for the GPU once everything is enqueued)
        s = ops.metrics_summary(row.cpu().numpy()[0], n_values)
        per_seq.setdefault(os.path.dirname(rel) or ".", []).append((s, n_values))
    rep = {"definition": ops.METRICS_DEFINITION, "a": dir_a, "b": dir_b, "pattern": pattern,
           "overall": M._pooled([p for parts in per_seq.values() for p in parts]),
           "sequences": {seq: M._pooled(parts) for seq, parts in sorted(per_seq.items())},
           "unpaired_a": only_a, "unpaired_b": only_b, "size_mismatch": mismatch}
    if temporal:
        t_seq = {}
        for seq, n_pixels, trow in t_pending:
            t_seq.setdefault(seq, []).append((trow.cpu().numpy()[0], n_pixels))
        rep["overall"]["temporal"] = M.pool_temporal([p for parts in t_seq.values() for p in parts])
        for seq, summary in rep["sequences"].items():
            summary["temporal"] = M.pool_temporal(t_seq.get(seq, []))
        rep["temporal_definition"], rep["temporal_skipped"] = ops.temporal_definition(temporal_flow), t_skipped
        rep["temporal_flow"] = temporal_flow
    return rep


def _fmt(v, spec):
    return "none" if v is None else format(v, spec)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m text2video_amd.evaluate", description=__doc__.split("\n\n")[1])
    ap.add_argument("dir_a")
    ap.add_argument("dir_b")
    ap.add_argument("--pattern", default="fake_B_*", help="shell pattern the files' base names must match")
    ap.add_argument("--temporal", action="store_true", help="add warping error, tOF and the flicker term of consecutive files")
    ap.add_argument("--temporal_flow", default=None, choices=["lk", "lkhs"], help="with --temporal: the flow estimator, lk "
                    "(default) or lkhs = with the Horn-Schunck refinement; named in the report")
    ap.add_argument("--gpu_decode", action="store_true", help="decode the JPEG files on the GPU, in batches (the same report)")
    ap.add_argument("--pair_by_stem", action="store_true", help="pair files whose relative paths agree up to the extension: a "
                    "tree of .png frames (test.py --frame_format png) against one of .jpg frames")
    ap.add_argument("--json", default=None, metavar="OUT", help="write the report to this file")
    ap.add_argument("--gpu_ids", default="0")
    args = ap.parse_args(argv)
    for d in (args.dir_a, args.dir_b):
        if not os.path.isdir(d):
            ap.error("%s is not a directory" % d)
    if args.temporal_flow is not None and not args.temporal:
        ap.error("--temporal_flow %s: the estimator of --temporal, which is not given" % args.temporal_flow)
    if os.environ.get("T2V_LEAN", "1") != "0":
        from . import _xp
        _xp.use_lean()          # no torch needed for an allocator and a stream (honoured when torch is not loaded yet)
    fallback = []
    rep = compare_trees(args.dir_a, args.dir_b, args.pattern, "cuda:%d" % int(str(args.gpu_ids).split(",")[0]), args.temporal,
                        args.gpu_decode, fallback, **({"temporal_flow": args.temporal_flow} if args.temporal_flow else {}),
                        **({"pair_by_stem": True} if args.pair_by_stem else {}))
    if fallback:
        print("--gpu_decode: Pillow decoded %d file(s), the first: %s (%s)" % ((len(fallback),) + fallback[0]), file=sys.stderr)
    for seq, s in list(rep["sequences"].items()) + [("overall", rep["overall"])]:
        print("%-24s %4d frames  psnr %s dB  ssim %s  mae %s" % (seq, s["frames"], _fmt(s["psnr"], ".3f"), _fmt(s["ssim"], ".6f"),
                                                               _fmt(s["mae"], ".4f")))
        if args.temporal:
            t = s["temporal"]
            print("%-24s %4d pairs   warp_mse %s (real %s, valid %s)  tof %s px  tdiff_mse %s"
                  % ("", t["pairs"], _fmt(t["warp_mse"], ".3f"), _fmt(t["warp_mse_real"], ".3f"), _fmt(t["valid"], ".3f"),
                     _fmt(t["tof"], ".4f"), _fmt(t["tdiff_mse"], ".3f")))
    for key, what in (("unpaired_a", "only under %s" % args.dir_a), ("unpaired_b", "only under %s" % args.dir_b)):
        for f in rep[key]:
            print("unpaired (%s): %s" % (what, f), file=sys.stderr)
    for m in rep["size_mismatch"]:
        print("size mismatch: %s is %dx%d and %dx%d" % (m["file"], m["a"][0], m["a"][1], m["b"][0], m["b"][1]), file=sys.stderr)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rep, fh, indent=1, sort_keys=True)
            fh.write("\n")
    if not rep["overall"]["frames"] and not (rep["unpaired_a"] or rep["unpaired_b"] or rep["size_mismatch"]):
        print("no file matches %r under both directories" % args.pattern, file=sys.stderr)
        return 1
    return 1 if (rep["unpaired_a"] or rep["unpaired_b"] or rep["size_mismatch"]) else 0


if __name__ == "__main__":
    sys.exit(main())
