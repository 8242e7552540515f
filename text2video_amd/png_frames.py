"""The frame loop's side of `test.py --frame_format png`: batches of uint8 frames on the device -> finished PNG files on
the host, without a host synchronisation of its own.  The ring of three, the lengths, the windows and the second-copy rule
are those of jpeg_frames.StepEncoder (its docstring has them); what differs is the encode call, that the device writes
the complete file (nothing is added on the host), the capacity (ops.png_file_capacity) and where a window starts: lossless
frames are larger, png_window_bytes(H, W) is one byte per pixel.
"""
from ._xp import torch
from . import ops
from .jpeg_frames import LENGTHS_BYTES, RING, StepEncoder as _JpegStepEncoder


def png_window_bytes(H, W):
    return max(4096, (H * W + 255) // 256 * 256)


class StepEncoder(_JpegStepEncoder):
    def __init__(self, H, W, nimg, device="cuda:0", window=None):
        if not ops.png_supported(H, W):
            raise ValueError("png_frames: the encoder does not take %dx%d frames" % (H, W))
        if not 1 <= nimg <= LENGTHS_BYTES // 4:
            raise ValueError("png_frames: %d images per step (1..%d)" % (nimg, LENGTHS_BYTES // 4))
        dev = torch.device(device)
        self.H, self.W, self.nimg = H, W, nimg
        self.capacity = ops.png_file_capacity(H, W)
        self.windows = (min(int(window) if window is not None else png_window_bytes(H, W), self.capacity),) * nimg
        self.batch = torch.empty(nimg, H, W, 4, dtype=torch.uint8, device=dev)
        self.workspace = torch.empty(ops.png_workspace_bytes(H, W, nimg), dtype=torch.uint8, device=dev)
        self.out = [torch.empty(nimg, self.capacity, dtype=torch.uint8, device=dev) for _ in range(RING)]
        self.lengths = [torch.empty(nimg, dtype=torch.int32, device=dev) for _ in range(RING)]
        self.host = [None] * RING
        self.steps = 0
        self.second_copies = 0
        self.d2h_bytes = 0
        self.encode_s = self.d2h_s = 0.0

    def _encode(self, out, lengths):
        ops.png_encode_u8(self.batch, out=out, lengths=lengths, workspace=self.workspace)

    def _file(self, data):
        return data
