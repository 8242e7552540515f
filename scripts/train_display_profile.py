#!/usr/bin/env python
"""The kernel figures of profiles/train_display.txt: ops.train_visuals on the display's own 8 panels at 512x512, scale 1,
30 calls, to be run under the profiler in a run of its own:

    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/train_display_profile.py

and the bytes one call reads and writes, computed from the shapes (printed as `BYTES ...`)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from text2video_amd import ops  # noqa: E402

H = W = 512
g = torch.Generator(device="cuda").manual_seed(0)
pose = torch.rand(H, W, 12, device="cuda", generator=g) * 2 - 1
fake, raw, real = (torch.rand(H, W, 4, device="cuda", generator=g) * 2 - 1 for _ in range(3))
fw = torch.randn(H, W, 4, device="cuda", generator=g)
flow_ref = torch.randn(H, W, 4, device="cuda", generator=g) * 3
conf = (torch.rand(H, W, device="cuda", generator=g) < 0.5).float()
panels = [(ops.VISUALS_IMAGE, pose, 6), (ops.VISUALS_IMAGE, fake, 0), (ops.VISUALS_IMAGE, raw, 0), (ops.VISUALS_IMAGE, real, 0),
          (ops.VISUALS_FLOW, fw, 0), (ops.VISUALS_UNIT, fw, 2), (ops.VISUALS_FLOW, flow_ref, 0), (ops.VISUALS_UNIT, conf, 0)]
out = torch.empty(8, H, W, 3, dtype=torch.uint8, device="cuda")
for _ in range(30):
    ops.train_visuals(panels, 1, out=out)
torch.cuda.synchronize()
px = H * W
needed = px * 4 * (3 * 4 + 2 + 1 + 2 + 1)            # the channels launch 2 reads
extent = px * 4 * (12 + 4 * 3 + 4 + 4 + 1)           # every tensor once, whole pixels (cache lines hold whole pixels)
minmax_needed, minmax_extent = px * 4 * 2 * 2, px * 4 * 4 * 2
print("BYTES render: reads %d B of channels (%d B of whole tensors), writes %d B; minmax: reads %d B of channels (%d B of whole "
      "tensors), writes %d B" % (needed, extent, out.numel(), minmax_needed, minmax_extent, 2 * 64 * 2 * 8), flush=True)
