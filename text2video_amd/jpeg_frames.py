"""The frame loop's side of `test.py --gpu_jpeg`: batches of uint8 frames on the device -> finished JPEG files on the
host, without a host synchronisation of its own.

    enc = StepEncoder(H, W, nimg, quality, device)
    ... write frame i of the step into enc.image(i) (ops.tensor2im_u8(out=...), ops.jpeg_stage_u8) ...
    step = enc.encode()          # one ops.jpeg_encode_u8 call, then the D2H copies and an event: all asynchronous
    ... enqueue the next step ...
    files = enc.files(step)      # waits for the step's event; header + scan + EOI per image

What travels with the event: the int32 scan lengths and a first window of every scan, into one page-locked buffer.  A
window starts at jpeg_window_bytes(H, W) (a quarter byte per pixel).  A scan longer than its window is completed in
files() by a second copy from the step's device buffer: on a stream of its own (ops.side_stream -- the step's event has
been waited for, so the copy has nothing to be ordered against and does not queue behind the next step's work), and the
host waits for that copy alone.  The window of that image slot then grows to 5/4 of the length seen, for the steps encoded
from then on: slot i of a step is the same kind of picture every step (a sequence's generated frame, its pose map), so the
second copies stop after the first frames.  Windows never shrink and never exceed the scan capacity.
Device and host buffers form rings of three: files(step n) must run before encode() of step n + 3 (the frame loop calls
it before step n + 2 is enqueued).
"""
import time

import numpy as np

from ._xp import torch
from . import jpeg, ops

LENGTHS_BYTES = 256      # the head of a step's pinned buffer: the int32 scan lengths; the windows follow
RING = 3


def jpeg_window_bytes(H, W):
    return max(4096, (H * W // 4 + 255) // 256 * 256)


class Step:
    __slots__ = ("event", "slot", "host", "windows")

    def __init__(self, event, slot, host, windows):
        self.event, self.slot, self.host, self.windows = event, slot, host, windows


class StepEncoder:
    def __init__(self, H, W, nimg, quality=75, device="cuda:0", window=None):
        if not ops.jpeg_supported(H, W):
            raise ValueError("jpeg_frames: the encoder does not take %dx%d frames" % (H, W))
        if not 1 <= nimg <= LENGTHS_BYTES // 4:
            raise ValueError("jpeg_frames: %d images per step (1..%d)" % (nimg, LENGTHS_BYTES // 4))
        dev = torch.device(device)
        self.H, self.W, self.nimg, self.quality = H, W, nimg, int(quality)
        self.capacity = ops.jpeg_scan_capacity(H, W)
        self.windows = (min(int(window) if window is not None else jpeg_window_bytes(H, W), self.capacity),) * nimg
        self.header = jpeg.header(H, W, self.quality)
        self.batch = torch.empty(nimg, H, W, 4, dtype=torch.uint8, device=dev)
        self.workspace = torch.empty(ops.jpeg_workspace_bytes(H, W, nimg), dtype=torch.uint8, device=dev)
        self.out = [torch.empty(nimg, self.capacity, dtype=torch.uint8, device=dev) for _ in range(RING)]
        self.lengths = [torch.empty(nimg, dtype=torch.int32, device=dev) for _ in range(RING)]
        self.host = [None] * RING       # pinned, (re)allocated when the windows have grown
        self.steps = 0
        self.second_copies = 0          # scans that did not fit their window
        self.d2h_bytes = 0
        self.encode_s = self.d2h_s = 0.0      # host time spent enqueueing the encode calls / the copies

    def _encode(self, out, lengths):
        ops.jpeg_encode_u8(self.batch, self.quality, out=out, lengths=lengths, workspace=self.workspace)

    def _file(self, scan):
        return jpeg.file_bytes(self.header, scan)

    def image(self, i):
        """frame i of the step being assembled: a uint8 device view [H,W,4]"""
        return self.batch.narrow(0, i, 1).view(self.H, self.W, 4)

    def encode(self):
        slot = self.steps % RING
        self.steps += 1
        windows, need = self.windows, LENGTHS_BYTES + sum(self.windows)
        if self.host[slot] is None or self.host[slot].numel() < need:
            self.host[slot] = torch.empty(need, dtype=torch.uint8, pin_memory=True)
        out, lengths, host = self.out[slot], self.lengths[slot], self.host[slot]
        t0 = time.perf_counter()
        self._encode(out, lengths)
        t1 = time.perf_counter()
        ops.copy_bytes_to_host(host, 0, lengths, 0, 4 * self.nimg)
        o = LENGTHS_BYTES
        for i, w in enumerate(windows):
            ops.copy_bytes_to_host(host, o, out, i * self.capacity, w)
            o += w
        self.d2h_bytes += 4 * self.nimg + sum(windows)
        ev = torch.cuda.Event()
        ev.record()
        self.encode_s += t1 - t0
        self.d2h_s += time.perf_counter() - t1
        return Step(ev, slot, host, windows)

    def files(self, step):
        step.event.synchronize()
        buf = step.host.numpy()
        lengths = [int(n) for n in buf[:4 * self.nimg].view(np.int32)]
        rest = {}
        for i, n in enumerate(lengths):
            if n > self.capacity:      # (t2v_jpeg_scan_capacity bounds every scan)
                raise RuntimeError("jpeg_frames: a scan of %d bytes exceeds the capacity %d" % (n, self.capacity))
            w = step.windows[i]
            if n > w:
                side = ops.side_stream()
                rest[i] = torch.empty(n - w, dtype=torch.uint8, pin_memory=True)
                ops.copy_bytes_to_host(rest[i], 0, self.out[step.slot], i * self.capacity + w, n - w, stream=side)
                self.d2h_bytes += n - w
        if rest:
            ops.stream_synchronize(side)
            self.second_copies += len(rest)
            grown = list(self.windows)
            for i in rest:
                grown[i] = max(grown[i], min(self.capacity, (lengths[i] * 5 // 4 + 255) // 256 * 256))
            self.windows = tuple(grown)
        files, o = [], LENGTHS_BYTES
        for i, n in enumerate(lengths):
            w = step.windows[i]
            scan = buf[o:o + min(n, w)].tobytes()
            if i in rest:
                scan += rest[i].numpy().tobytes()
            files.append(self._file(scan))
            o += w
        return files
