"""Host side of `test.py --metrics`: the real frames a sequence's generated frames are compared with, and the summaries.

The comparison itself is one call of ops.image_metrics per frame on the GPU (t2v_image_metrics_u8); this module decodes the
real frames on threads ahead of the frame loop, keeps each sequence's rows in one device buffer that is copied to the host
once when the sequence ends, and turns the rows into metrics.json.  Nothing here imports torch: the frame loop runs on
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
    """One sequence's rows of ops.image_metrics on the device: two per frame (the frame, its face box)."""

    def __init__(self, torch, seq, capacity, device):
        self.seq, self.capacity = seq, capacity
        self.rows = torch.empty(2 * capacity, 4, dtype=torch.float64, device=device)
        self.frames = []      # (name, (H, W), face box or None)

    def compare(self, fake_u8, real_u8, name, face):
        if len(self.frames) >= self.capacity:
            raise RuntimeError("--metrics: sequence %s has more frames than its %d pose files" % (self.seq, self.capacity))
        ops.image_metrics(fake_u8, real_u8, [face] if face is not None else [], out=self.rows, out_row=2 * len(self.frames))
        self.frames.append((name, tuple(fake_u8.shape[:2]), face))


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


def summarise(frames, rows):
    """frames: [(name, (H, W), face box or None)]; rows: host array [2 * len(frames), 4] -> the metrics.json document"""
    out, whole, faces = [], [], []
    for j, (name, (H, W), face) in enumerate(frames):
        s = ops.metrics_summary(rows[2 * j], 3 * H * W)
        whole.append((s, 3 * H * W))
        entry = {"name": name, "psnr": s["psnr"], "ssim": s["ssim"], "mae": s["mae"], "face": None}
        if face is not None:
            nf = 3 * (face[1] - face[0]) * (face[3] - face[2])
            f = ops.metrics_summary(rows[2 * j + 1], nf)
            faces.append((f, nf))
            entry["face"] = {"psnr": f["psnr"], "ssim": f["ssim"], "mae": f["mae"], "box": list(face)}
        out.append(entry)
    summary = _pooled(whole)
    summary["face"] = _pooled(faces)
    return {"definition": ops.METRICS_DEFINITION, "summary": summary, "frames": out}


def write_json(path, doc):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
