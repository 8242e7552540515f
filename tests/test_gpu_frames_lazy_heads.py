"""Whole frames with the norms applied by their consumers (default) against the stand-alone apply passes (T2V_CHAIN_LAZY=0),
each in a fresh child process: the heads that normalise the raw decoder output in LDS, the one-pass encoder join and the
input transform of the encoder sum shared by both branches must leave every output -- frames, and img_feat / flow_feat where a
caller asks for them -- bit for bit what the apply form computes.

Configurations (config-2 generator: ngf 128, 3 down layers, 9 blocks; local enhancer ngf 64, 3 blocks):
  flow and no-flow 512x512 single-scale, flow 512x320 (ragged tile grids) as a lock-step batch of 2, two-scale 512x512
  (global generator at 256x256 + local enhancer) with and without flow, the global generator's feature maps themselves, and a
  512x512 flow frame of the instance-norm generator (no gamma / beta: the plain forms of the head's norm stage and of the join).

Launch counts per 512x512 flow frame, from torch.profiler in the child: the parent form runs 12 inorm_apply_kernel launches,
4 winograd4_input_kernel<0> and add_kernel at the join.  The default form drops four apply passes (two in front of the heads,
the two that close the encoder chains), one input transform and the add; the join runs as ONE launch of inorm_apply_kernel
with its second operand (no new kernel): 12 - 4 = 8 apply passes + that launch = 9 launches of the kernel.  That the ninth is
the join, and that nothing else was added, is pinned by the frame's total of library launches: 203 = the parent's 208 minus
four apply passes, the add and one input transform, plus the join."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import json, os, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
out_dir = sys.argv[2]
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import kernel_variants as kv
from text2video_amd.generator import GeneratorSpec, HipGenerator, Recurrence, Vid2VidModelG, synthetic_state_dict

dev = torch.device("cuda:0")
results, counts = {}, {}


def window(H, W, seed):
    rng = np.random.default_rng(seed)
    win = torch.zeros(H, W, 12)
    win[..., :9] = torch.from_numpy(np.where(rng.random((H, W, 1)) < 0.02, rng.uniform(-1, 1, (H, W, 9)), -1.0).astype(np.float32))
    return win.to(dev)


def frames(model, H, W, nseq, name, nframes=3, profile_last=False):
    wins = [window(H, W, 11 + q) for q in range(nseq)]
    states = [Recurrence() for _ in range(nseq)]
    for t in range(nframes):
        if profile_last and t == nframes - 1:
            torch.cuda.synchronize()
            with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
                outs = model.inference_nhwc_batch(wins, states)
                torch.cuda.synchronize()
            c = {}
            for e in prof.events():
                if "t2v::" in e.name:
                    n = kv.normalise(e.name)
                    c[n] = c.get(n, 0) + 1
            counts[name] = c
        else:
            outs = model.inference_nhwc_batch(wins, states)
        for q, o in enumerate(outs):
            results["%s.f%d.s%d" % (name, t, q)] = o.cpu().numpy()


for flow in (True, False):
    tag = "flow" if flow else "noflow"
    spec = GeneratorSpec(ngf=128, n_downsample=3, n_blocks=9, no_flow=not flow, norm="batch")
    g0 = HipGenerator(spec, dev).load_state_dict(synthetic_state_dict(spec, 1, flow_gain=0.1))
    frames(Vid2VidModelG([g0]), 512, 512, 1, tag + "_512x512", profile_last=True)
    if flow:
        frames(Vid2VidModelG([g0]), 512, 320, 2, "flow_512x320_batch2")
    spec1 = GeneratorSpec(ngf=64, n_blocks=3, no_flow=not flow, norm="batch", is_local=True, scale=1)
    g1 = HipGenerator(spec1, dev).load_state_dict(synthetic_state_dict(spec1, 2, flow_gain=0.1))
    frames(Vid2VidModelG([g0, g1]), 512, 512, 1, tag + "_two_scale_512x512")
    # the global generator's feature maps as a caller of the two-scale path receives them
    pose, prev = window(256, 256, 5), torch.zeros(256, 256, 8, device=dev)
    prev[..., :6] = torch.tanh(torch.randn(256, 256, 6, generator=torch.Generator().manual_seed(3))).to(dev)
    want = ("out", "img_feat", "flow_feat") if flow else ("out", "img_feat")
    for k, v in g0.forward(pose, prev, want=want).items():
        results["%s_feat_256x256.%s" % (tag, k)] = v.cpu().numpy()
    del g0, g1
    torch.cuda.empty_cache()

# norm="instance": no gamma / beta -- the plain forms of the head's norm stage and of the join inside whole frames
spec = GeneratorSpec(ngf=128, n_downsample=3, n_blocks=9, no_flow=False, norm="instance")
gi = HipGenerator(spec, dev).load_state_dict(synthetic_state_dict(spec, 4, flow_gain=0.1))
frames(Vid2VidModelG([gi]), 512, 512, 1, "flow_instance_norm_512x512", profile_last=True)
del gi

np.savez(os.path.join(out_dir, "outputs.npz"), **results)
json.dump(counts, open(os.path.join(out_dir, "counts.json"), "w"))
print("child ok: %d arrays" % len(results))
'''


def _run_child(tmp_path, name, lazy_env):
    out = tmp_path / name
    out.mkdir()
    script = tmp_path / (name + "_child.py")
    script.write_text(CHILD)
    env = {k: v for k, v in os.environ.items() if k != "T2V_CHAIN_LAZY"}
    if lazy_env is not None:
        env["T2V_CHAIN_LAZY"] = lazy_env
    p = subprocess.run([sys.executable, str(script), ROOT, str(out)], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, "child %s failed (%d):\n%s\n%s" % (name, p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    return dict(np.load(str(out / "outputs.npz"))), json.load(open(str(out / "counts.json")))


def _count(c, prefix):
    return sum(v for k, v in c.items() if k == prefix or k.startswith(prefix + "<"))


def test_frames_bit_equal_to_the_apply_form_and_launch_counts(tmp_path):
    lazy, lazy_counts = _run_child(tmp_path, "lazy", None)
    plain, plain_counts = _run_child(tmp_path, "apply", "0")
    assert sorted(lazy) == sorted(plain) and len(lazy) >= 20
    for k in sorted(lazy):
        a, b = lazy[k], plain[k]
        assert a.shape == b.shape and np.isfinite(a).all(), k
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), "%s: %d values differ, max |d| %.3g" % (
            k, (a.view(np.int32) != b.view(np.int32)).sum(), np.abs(a - b).max())
    for k in ("flow_feat_256x256.img_feat", "flow_feat_256x256.flow_feat", "noflow_feat_256x256.img_feat"):
        assert k in lazy and lazy[k].min() >= 0.0 and lazy[k].max() > 0.0, "%s must be the normalised (ReLU) map" % k

    c, p = lazy_counts["flow_512x512"], plain_counts["flow_512x512"]
    print("flow 512x512 launches per frame, default / T2V_CHAIN_LAZY=0: inorm_apply %d / %d, winograd4_input<0> %d / %d, add %d / %d,"
          " head %d / %d, all %d / %d" % (_count(c, "t2v::inorm_apply_kernel"), _count(p, "t2v::inorm_apply_kernel"),
                                          c.get("t2v::winograd4_input_kernel<0,true>", 0), p.get("t2v::winograd4_input_kernel<0,true>", 0),
                                          _count(c, "t2v::add_kernel"), _count(p, "t2v::add_kernel"),
                                          _count(c, "t2v::conv_head7x7_strip_kernel"), _count(p, "t2v::conv_head7x7_strip_kernel"),
                                          sum(c.values()), sum(p.values())))
    # 12 - 4 = 8 apply passes + the join, which is one more launch of the same kernel (module docstring)
    assert _count(c, "t2v::inorm_apply_kernel") == 8 + 1, c
    assert c.get("t2v::winograd4_input_kernel<0,true>", 0) == 3, c
    assert _count(c, "t2v::add_kernel") == 0, c
    assert _count(c, "t2v::conv_head7x7_strip_kernel") == 2, c
    assert _count(p, "t2v::add_kernel") == 1 and _count(p, "t2v::conv_head7x7_strip_kernel") == 2, p
    # the whole frame: 203 kernel launches -- the parent's 208 of this profiled frame (12 apply, 4 plain input transforms, the
    # add) minus 4 apply passes, the add and one transform, plus the join; any other added launch would show here
    assert sum(c.values()) == 203, (sum(c.values()), c)
    # the instance-norm frame takes the same sequence (the join and the heads without gamma / beta)
    i = lazy_counts["flow_instance_norm_512x512"]
    assert _count(i, "t2v::inorm_apply_kernel") == 9 and _count(i, "t2v::add_kernel") == 0, i
    assert i.get("t2v::winograd4_input_kernel<0,true>", 0) == 3 and sum(i.values()) == 203, (sum(i.values()), i)
    # no flow: 9 apply passes in the parent form; one head, the two chain closings -> the join: 9 - 3 + 1
    n = lazy_counts["noflow_512x512"]
    assert _count(n, "t2v::inorm_apply_kernel") == 7 and _count(n, "t2v::add_kernel") == 0, n
    assert n.get("t2v::winograd4_input_kernel<0,true>", 0) == 3, n
