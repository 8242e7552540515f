"""Host side of `test.py --metrics` / `--metrics_temporal`: the real frames a sequence's generated frames are compared with,
and the summaries.

The comparison itself is one call of ops.image_metrics per frame on the GPU (t2v_image_metrics_u8); this module decodes the
real frames on threads ahead of the frame loop, keeps each sequence's rows in one device buffer that is copied to the host
once when the sequence ends, and turns the rows into metrics.json.  --metrics_temporal adds, per frame after a sequence's
first, three ops.optical_flow_u8 calls and one ops.temporal_metrics call on the pair (t-1, t).  Nothing here imports torch: the frame loop runs on
text2video_amd/leantorch.py as well.
"""
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import ops
from .keypoints import get_face_region
from .pose_dataset import _decode_frame, central_crop_cols, get_img_params

DECODE_THREADS = 4
DECODE_AHEAD = 16        # real frames decoded ahead of the loop (0.5 MB each at 512 x 320)


def real_frame_geometry(opt, size):
    """(new_size, crop box, (H, W)) of a real frame of `size` = (w, h): the BICUBIC resize to get_img_params and the
    central-column crop the pose map of the same frame gets"""
    new_w, new_h = get_img_params(opt, size)
    c0, c1 = (0, new_w) if opt.no_pose_crop else central_crop_cols(new_w)
    return (new_w, new_h), (c0, 0, c1, new_h), (new_h, c1 - c0)


class RealFrames:
    """The real frames of the dataset's items in the order the frame loop meets them, decoded DECODE_AHEAD ahead on
    DECODE_THREADS threads (Pillow releases the GIL while it decodes and resamples)."""

    def __init__(self, dataset, opt, n_lanes, limit=None):
        missing = sorted({seq for seq, _ in dataset.items if not dataset.img.get(seq)})
        if missing:
            raise ValueError("--metrics: no real frames for sequence(s) %s: it compares with <dataroot>/%s_img/<seq>/<frame>"
                             % (", ".join(missing), getattr(opt, "phase", "test")))
        plan = dataset.lane_plan(n_lanes, limit)
        steps = max((len(p) for p in plan), default=0)
        self.jobs = []        # (path, new_size, box, (H, W)) in the loop's order
        geo = {}
        for t in range(steps):
            for lane in plan:
                if t < len(lane):
                    seq, i = dataset.items[lane[t]]
                    if seq not in geo:
                        geo[seq] = real_frame_geometry(opt, dataset._size(seq))
                    self.jobs.append((dataset.img[seq][i],) + geo[seq])
        self.pool = ThreadPoolExecutor(max_workers=DECODE_THREADS)
        self.futures, self.next = {}, 0
        self._pump()

    @staticmethod
    def _decode(job):
        path, new_size, box, (h, w) = job
        out = np.empty((h, w, 3), np.uint8)
        _decode_frame(path, new_size, box, out)
        return out

    def _pump(self):
        while self.next < len(self.jobs) and len(self.futures) < DECODE_AHEAD:
            job = self.jobs[self.next]
            self.futures[job[0]] = self.pool.submit(self._decode, job)
            self.next += 1

    def get(self, path):
        """the decoded real frame [H,W,3] uint8 of the item named `path`"""
        fut = self.futures.pop(path, None)
        if fut is None:       # not within the window (an order the plan did not foresee): decode now
            job = next((j for j in self.jobs if j[0] == path), None)
            if job is None:
                raise ValueError("--metrics: no real frame for %s" % path)
            return self._decode(job)
        out = fut.result()
        self._pump()
        return out

    def close(self):
        for f in self.futures.values():
            f.cancel()
        self.pool.shutdown(wait=True)


class SequenceRows:
    """One sequence's rows on the device: two of ops.image_metrics per frame (the frame, its face box) and, with
    temporal=True, two of ops.temporal_metrics per frame after the first (--metrics_temporal).  Both kinds live in ONE buffer
    (`buf`: the [2n,4] picture rows, then the [2n,6] temporal rows), which goes to the host in one copy when the sequence ends."""

    def __init__(self, torch, seq, capacity, device, temporal=False, temporal_flow="lk"):
        self.seq, self.capacity, self.temporal = seq, capacity, bool(temporal)
        self.temporal_flow = temporal_flow                              # --temporal_flow: lk, or lkhs = the refined estimate
        self._flow_kw = ops.temporal_flow_kwargs(temporal_flow)
        n = 2 * capacity
        if self.temporal:
            self.buf = torch.empty(n * (4 + ops.TEMPORAL_COLUMNS), dtype=torch.float64, device=device)
            self.rows = self.buf.narrow(0, 0, n * 4).view(n, 4)
            self.trows = self.buf.narrow(0, n * 4, n * ops.TEMPORAL_COLUMNS).view(n, ops.TEMPORAL_COLUMNS)
        else:
            self.buf = self.rows = torch.empty(n, 4, dtype=torch.float64, device=device)
            self.trows = None
        self._torch = torch
        self.prev = None      # (generated bytes, real frame) of the sequence's previous frame, on the device
        self.flows = None     # the three flows of a pair, written anew for every pair (stream-ordered)
        self.frames = []      # (name, (H, W), face box or None)

    def compare(self, fake_u8, real_u8, name, face):
        """real_u8 must stay untouched until the NEXT frame of the sequence has been compared when temporal (the caller
        alternates between two buffers); fake_u8 is kept by reference"""
        if len(self.frames) >= self.capacity:
            raise RuntimeError("--metrics: sequence %s has more frames than its %d pose files" % (self.seq, self.capacity))
        boxes = [face] if face is not None else []
        ops.image_metrics(fake_u8, real_u8, boxes, out=self.rows, out_row=2 * len(self.frames))
        if self.temporal:
            if self.prev is not None and tuple(self.prev[0].shape[:2]) == tuple(fake_u8.shape[:2]):
                prev_fake, prev_real = self.prev
                if self.flows is None or tuple(self.flows[0].shape[:2]) != tuple(fake_u8.shape[:2]):
                    self.flows = [self._torch.empty(fake_u8.shape[0], fake_u8.shape[1], 4, dtype=self._torch.float32,
                                                    device=fake_u8.device) for _ in range(3)]
                fwd = ops.optical_flow_u8(real_u8, prev_real, out=self.flows[0], **self._flow_kw)        # real t -> t-1
                bwd = ops.optical_flow_u8(prev_real, real_u8, out=self.flows[1], **self._flow_kw)        # real t-1 -> t
                gen = ops.optical_flow_u8(fake_u8, prev_fake, out=self.flows[2], **self._flow_kw)        # generated t -> t-1
                ops.temporal_metrics(fake_u8, prev_fake, real_u8, prev_real, fwd, bwd, gen, boxes, out=self.trows,
                                     out_row=2 * len(self.frames))
            self.prev = (fake_u8, real_u8)
        self.frames.append((name, tuple(fake_u8.shape[:2]), face))

    def split_host(self, host):
        """the host copy of `buf` -> (picture rows [2n,4], temporal rows [2n,6] or None)"""
        n = 2 * self.capacity
        if not self.temporal:
            return host.reshape(n, 4), None
        flat = host.reshape(-1)
        return flat[:n * 4].reshape(n, 4), flat[n * 4:].reshape(n, ops.TEMPORAL_COLUMNS)


def face_box(pose_map_u8):
    """the face region of a frame (keypoints.get_face_region on its pose map, side from the frame height), or None when the
    map shows no face or the frame is too small to hold the box"""
    H, W = pose_map_u8.shape[:2]
    box = get_face_region(pose_map_u8, H)
    if box is None or box[0] < 0 or box[2] < 0 or box[1] > H or box[3] > W:
        return None
    return tuple(int(v) for v in box)


def _mean(values):
    values = [v for v in values if v is not None]
    return sum(values) / len(values) if values else None


def _pooled(parts):
    """parts: [(summary dict, n_values)] -> {frames, psnr of the pooled MSE, mean ssim, mean mae}"""
    import math
    n = sum(nv for _, nv in parts)
    sse = sum(s["mse"] * nv for s, nv in parts)
    return {"frames": len(parts), "psnr": None if not parts or sse == 0 else 10.0 * math.log10(255.0 * 255.0 * n / sse),
            "ssim": _mean([s["ssim"] for s, _ in parts]), "mae": _mean([s["mae"] for s, _ in parts])}


def pool_temporal(parts):
    """parts: [(row of ops.temporal_metrics, n_pixels)] -> the pooled figures, over SUMS (not a mean of ratios):
    sum sse / sum(3 n_valid), sum epe / sum n_flow, sum tdiff / sum(3 n_pixels), and `pairs`"""
    tot = [sum(float(r[i]) for r, _ in parts) for i in range(ops.TEMPORAL_COLUMNS)]
    out = ops.temporal_summary(tot, sum(n for _, n in parts))
    out["pairs"] = len(parts)
    return out


def summarise(frames, rows, trows=None, temporal_flow="lk"):
    """frames: [(name, (H, W), face box or None)]; rows: host array [2 * len(frames), 4]; trows: host array
    [2 * len(frames), 6] of the temporal rows (frame 0's are not read) or None -> the metrics.json document, whose
    "temporal_definition" names the flow estimator the rows were taken with (temporal_flow)"""
    out, whole, faces, t_whole, t_faces = [], [], [], [], []
    for j, (name, (H, W), face) in enumerate(frames):
        s = ops.metrics_summary(rows[2 * j], 3 * H * W)
        whole.append((s, 3 * H * W))
        entry = {"name": name, "psnr": s["psnr"], "ssim": s["ssim"], "mae": s["mae"], "face": None}
        if face is not None:
            nf = 3 * (face[1] - face[0]) * (face[3] - face[2])
            f = ops.metrics_summary(rows[2 * j + 1], nf)
            faces.append((f, nf))
            entry["face"] = {"psnr": f["psnr"], "ssim": f["ssim"], "mae": f["mae"], "box": list(face)}
        if trows is not None:
            entry["temporal"] = None
            if j > 0:
                t = ops.temporal_summary(trows[2 * j], H * W)
                t_whole.append((trows[2 * j], H * W))
                t["face"] = None
                if face is not None:
                    t["face"] = ops.temporal_summary(trows[2 * j + 1], nf // 3)
                    t_faces.append((trows[2 * j + 1], nf // 3))
                entry["temporal"] = t
        out.append(entry)
    summary = _pooled(whole)
    summary["face"] = _pooled(faces)
    doc = {"definition": ops.METRICS_DEFINITION, "summary": summary, "frames": out}
    if trows is not None:
        summary["temporal"] = pool_temporal(t_whole)
        summary["temporal"]["face"] = pool_temporal(t_faces)
        doc["temporal_definition"] = ops.temporal_definition(temporal_flow)
    return doc


def write_json(path, doc):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
