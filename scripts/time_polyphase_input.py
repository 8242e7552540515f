"""us per launch of the fp32 polyphase input transform (stage 1: polyphase_input_kernel<UP, NORM>) of the tree given by --root, plain
and with a pending norm, at the four polyphase layer shapes of a 512x512 frame.  Run it on a built checkout of the parent commit
and on this tree in alternating processes to compare the two builds of the kernel:
    python scripts/time_polyphase_input.py --root ../parent; python scripts/time_polyphase_input.py --root ."""
import argparse, os, statistics, sys
ap = argparse.ArgumentParser(); ap.add_argument("--root", required=True); a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
import torch
import text2video_amd
from text2video_amd import ops
print("tree:", os.path.dirname(os.path.abspath(text2video_amd.__file__)))
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(1)
for label, up, H, W, C, Cout in (("up1 1024->512 64x64", True, 64, 64, 1024, 512), ("up2 512->256 128x128", True, 128, 128, 512, 256),
                                 ("down2 256->512 256x256", False, 256, 256, 256, 512), ("down3 512->1024 128x128", False, 128, 128, 512, 1024)):
    x = torch.randn(1, H, W, C, generator=g).to(dev)
    d = ops.conv_desc(H, W, C, Cout, 3, 2, 1, ops.PAD_ZERO, up, algo=ops.ALGO_POLYPHASE)
    ws = ops.winograd_batch_workspace(d, C, 1, dev)
    ho, wo = ops.conv_out_dims(d)
    y = torch.empty(1, ho, wo, Cout, device=dev)
    pu = torch.zeros(81 * Cout * C, device=dev)
    mr = torch.stack([torch.randn(1, C, generator=g) * 0.5, torch.rand(1, C, generator=g) + 0.5], -1).to(dev).contiguous()
    gm, bt = torch.randn(C, generator=g).to(dev), torch.randn(C, generator=g).to(dev)
    for mode, kw in (("plain", {}), ("norm", dict(mean_rstd=mr, relu=1)), ("norm+affine", dict(mean_rstd=mr, gamma=gm, beta=bt, relu=1))):
        fn = lambda: ops.conv2d_winograd_batch(x, pu, None, d, ws, out=y, stages=1, **kw)
        for _ in range(50): fn()
        torch.cuda.synchronize()
        res = []
        for _ in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(100): fn()
            e1.record(); e1.synchronize()
            res.append(e0.elapsed_time(e1) * 10.0)
        print("%-26s %-12s median %7.2f us (min %.2f, max %.2f)" % (label, mode, statistics.median(res), min(res), max(res)), flush=True)
