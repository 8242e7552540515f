"""Digest of whole train steps, to compare two trees (a commit and its parent) bit for bit on one GPU.

For every case and switch setting one line:
    <case> <switches> losses=<SHA-256 over float.hex of every loss of every step> state=<SHA-256 over the bytes of every
    parameter and BatchNorm running statistic of G, D, D_f and D_T* after the last step, as Vid2VidTrainer.save writes them>
Two runs agree on a line exactly when every loss and every weight they computed is the same.

Usage: train_step_digest.py [--root TREE] [--cases a,b,c,d] [--switches all|default]
  a: 128x128, ngf 32, flow branch, two D scales, face D; 3 steps
  b: 128x128, ngf 64 (the kept input transforms, the fixed-grid GEMMs forced: T2V_WINO_GEMM_SK=2); 3 steps
  c: 64x64, two temporal D scales; 5 steps, the fourth begins a new sequence (prev=None: its first frame is raw-only, the
     flow branch's collected weight gradients are flushed)
  d: 64x64, two spatial scales (G0 + the local enhancer G1; the state digest covers both files); 3 steps, the third begins a
     new sequence
Case a also runs with each of the train step's A/B switches set to its other value, case d also pass by pass
(T2V_D_BATCHED=0)."""
import argparse
import hashlib
import os
import sys
import tempfile

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the tree to import")
ap.add_argument("--cases", default="a,b,c,d")
ap.add_argument("--switches", default="all", choices=["all", "default"])
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import numpy as np      # noqa: E402
import torch            # noqa: E402
from text2video_amd import ops, train as T      # noqa: E402
from text2video_amd.options import TrainOptions      # noqa: E402

print("train_step_digest: text2video_amd from %s" % os.path.dirname(os.path.abspath(T.__file__)), file=sys.stderr)

COMMON = ["--name", "t", "--dataset_mode", "pose", "--input_nc", "3", "--openpose_only", "--max_frames_per_gpu", "2", "--no_first_img"]
CASES = {
    "a": dict(size=128, seed=5, rng=33, steps=3, face=True, env={}, new_sequence_at=None,
              argv=["--ngf", "32", "--n_downsample_G", "2", "--n_blocks", "3", "--num_D", "2", "--ndf", "16", "--no_vgg",
                    "--n_scales_temporal", "0", "--add_face_disc"]),
    "b": dict(size=128, seed=9, rng=8, steps=3, face=False, env={"T2V_WINO_GEMM_SK": "2"}, new_sequence_at=None,
              argv=["--ngf", "64", "--n_downsample_G", "1", "--n_blocks", "2", "--num_D", "1", "--ndf", "16", "--no_vgg",
                    "--n_scales_temporal", "0"]),
    "c": dict(size=64, seed=0, rng=0, steps=5, face=False, env={}, new_sequence_at=3,
              argv=["--ngf", "16", "--n_blocks", "2", "--num_D", "1", "--fineSize", "64", "--n_scales_temporal", "2", "--no_vgg"]),
    "d": dict(size=64, seed=3, rng=4, steps=3, face=False, env={}, new_sequence_at=2,
              argv=["--ngf", "16", "--n_blocks", "2", "--n_downsample_G", "2", "--num_D", "2", "--ndf", "16", "--no_vgg",
                    "--fineSize", "64", "--loadSize", "64", "--n_scales_temporal", "0", "--n_scales_spatial", "2",
                    "--n_blocks_local", "1"]),
}
PASS_BY_PASS = {"T2V_D_BATCHED": "0"}
SWITCHES = [{}, {"T2V_GRAD_DIRECT": "0"}, {"T2V_WGRAD_STREAM": "0", "T2V_PACK_PREFETCH": "0"}, {"T2V_WGRAD_BATCH": "0"},
            {"T2V_WGRAD_PAIR": "0"}, {"T2V_WGRAD_KEEP_V": "0"}, PASS_BY_PASS, {"T2V_D_BWD_STREAM": "1"}]


def run(name, case, switches, ckpt):
    env = dict(case["env"], **switches)
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    ops.reload_env()
    try:
        S = case["size"]
        opt = TrainOptions().parse(COMMON + case["argv"] + ["--checkpoints_dir", ckpt])
        rng = np.random.default_rng(case["rng"])
        tr = T.Vid2VidTrainer(opt, "cuda:0", seed=case["seed"])
        h_loss = hashlib.sha256()
        prev = None
        for step in range(case["steps"]):
            pose = torch.zeros(2, S, S, 12, device="cuda:0")
            pose[..., :9] = torch.from_numpy(rng.uniform(-1, 1, (2, S, S, 9)).astype(np.float32)).cuda()
            real = torch.zeros(2, S, S, 4, device="cuda:0")
            real[..., :3] = torch.tanh(torch.from_numpy(rng.standard_normal((2, S, S, 3)).astype(np.float32))).cuda()
            real_prev = torch.cat([real[1:], real[:1]], 0).contiguous()
            if step == case["new_sequence_at"]:
                prev, real_prev = None, None
            losses, prev = tr.train_step(pose, real, [(16, 80, 32, 96)] * 2 if case["face"] else None, prev, real_prev=real_prev)
            for k in sorted(losses):
                h_loss.update(("%d %s %s\n" % (step, k, float(losses[k]).hex())).encode())
        torch.cuda.synchronize()
        ops.check_async_errors()
        tr.save("digest")
        h_state = hashlib.sha256()
        d = os.path.join(ckpt, opt.name)
        for f in sorted(os.listdir(d)):
            if f.startswith("digest_net_"):
                sd = torch.load(os.path.join(d, f), map_location="cpu")
                for k in sorted(sd):
                    h_state.update(k.encode())
                    h_state.update(sd[k].contiguous().numpy().tobytes())
                os.remove(os.path.join(d, f))
        tag = ",".join("%s=%s" % kv for kv in sorted(switches.items())) or "default"
        print("%s %s losses=%s state=%s" % (name, tag, h_loss.hexdigest(), h_state.hexdigest()), flush=True)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        ops.reload_env()


with tempfile.TemporaryDirectory() as ckpt:
    for name in args.cases.split(","):
        for switches in {"a": SWITCHES, "d": [{}, PASS_BY_PASS]}.get(name, [{}]) if args.switches == "all" else [{}]:
            run(name, CASES[name], switches, ckpt)
