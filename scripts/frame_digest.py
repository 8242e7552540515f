"""Digest of whole generator frames, to compare two trees (a commit and its parent) bit for bit on one GPU.

For every case and switch setting one line:
    <case> <switches> ws=<t2v_generator_workspace_bytes_batch per net> layers=<SHA-256 over the per-layer (algo,
    t2v_conv_stats_floats) list> algos=<the layers' algorithms, run-length coded> out=<SHA-256 over the bytes of every output
    of three consecutive frames: out, and img_feat / flow_feat where the case asks for them>
Two runs agree on a line exactly when the plan and every value they computed are the same.

Usage: frame_digest.py [--root TREE] [--cases a,b,...] [--sizes_only]
  --sizes_only stops before anything touches the device (ws, layers and algos only).
  a: global generator (ngf 128, 3 down layers, 9 blocks), flow, norm=batch, 192x192: F(4x4) lazy chains, the 256->512 down and
     512->256 up layers polyphase (144 tiles), both halo-tile heads
  b: the same, no flow, norm=instance (no gamma / beta; one branch)
  c: a at 192x128, a lock-step batch of 3; sequence 2 starts one frame late (use_raw_only differs across the batch).  (At
     this size the chains are F(2x2,3x3) and no layer is polyphase: 96 tiles; the heads still take a pending norm.)
  d: two-scale: the global generator at 96x96 + a local enhancer (ngf 64, 3 blocks) at 192x192, flow, batch 2
  e: a's generator called directly with want=(out, img_feat, flow_feat)
  f: ngf 16, 2 down layers, 2 blocks, 64x64: no polyphase layer, no lazy chain, implicit-GEMM heads -- nothing is ever pending
  g: c at 192x192: the staggered batch of 3 through a's F(4x4) lazy chains, polyphase layers and one-pass join
Case a also runs with each frame-path switch set to its other value, once with arith="bf16x2" and once with
arith_layers="trunk+stride2" on top of it."""
import argparse
import ctypes
import hashlib
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the tree to import")
ap.add_argument("--cases", default="a,e,g,c,d,b,f")
ap.add_argument("--sizes_only", action="store_true")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import numpy as np      # noqa: E402
import torch            # noqa: E402
import text2video_amd   # noqa: E402
from text2video_amd import _lib, ops      # noqa: E402
from text2video_amd.generator import (GeneratorSpec, HipGenerator, Recurrence, Vid2VidModelG, _gen_desc,      # noqa: E402
                                      synthetic_state_dict)

print("frame_digest: text2video_amd from %s" % os.path.dirname(os.path.abspath(text2video_amd.__file__)), file=sys.stderr)

GLOBAL = dict(ngf=128, n_downsample=3, n_blocks=9)
# name -> (nets [(spec, seed, downscale of the frame this net sees)], H, W, sequences, kind)
CASES = {
    "a": ([(GeneratorSpec(no_flow=False, norm="batch", **GLOBAL), 1, 1)], 192, 192, 1, "frames"),
    "b": ([(GeneratorSpec(no_flow=True, norm="instance", **GLOBAL), 4, 1)], 192, 192, 1, "frames"),
    "c": ([(GeneratorSpec(no_flow=False, norm="batch", **GLOBAL), 1, 1)], 192, 128, 3, "staggered"),
    "d": ([(GeneratorSpec(no_flow=False, norm="batch", **GLOBAL), 1, 2),
           (GeneratorSpec(ngf=64, n_blocks=3, no_flow=False, norm="batch", is_local=True, scale=1), 2, 1)], 192, 192, 2, "frames"),
    "e": ([(GeneratorSpec(no_flow=False, norm="batch", **GLOBAL), 1, 1)], 192, 192, 1, "features"),
    "g": ([(GeneratorSpec(no_flow=False, norm="batch", **GLOBAL), 1, 1)], 192, 192, 3, "staggered"),
    "f": ([(GeneratorSpec(ngf=16, n_downsample=2, n_blocks=2, no_flow=False, norm="batch"), 6, 1)], 64, 64, 1, "frames"),
}
SWITCHES = [{}, {"T2V_CHAIN_LAZY": "0"}, {"T2V_STREAMS": "1"}, {"T2V_STREAMS": "2"}, {"T2V_FINALIZE_DIRECT": "0"},
            {"T2V_CONV_ALGO": "1"}, {"T2V_CONV_ALGO": "2"}, {"arith": "bf16x2"}, {"arith": "bf16x2", "arith_layers": "trunk+stride2"}]


def plan(nets, H, W, nseq, conv_algo):
    """(workspace bytes per net, digest of the layer list, the algorithms run-length coded) -- host code only"""
    lib = _lib.load()
    ws, h, algos = [], hashlib.sha256(), []
    for spec, _, down in nets:
        gd = _gen_desc(spec, H // down, W // down, conv_algo)
        ws.append(lib.t2v_generator_workspace_bytes_batch(ctypes.byref(gd), nseq))
        for i in range(lib.t2v_generator_num_layers(ctypes.byref(gd))):
            cd, xcs = _lib.ConvDesc(), ctypes.c_int()
            _lib.check(lib.t2v_generator_layer_desc(ctypes.byref(gd), i, ctypes.byref(cd), ctypes.byref(xcs)), "layer_desc")
            h.update(("%d %d %d\n" % (i, cd.algo, lib.t2v_conv_stats_floats(ctypes.byref(cd)))).encode())
            if algos and algos[-1][0] == cd.algo:
                algos[-1][1] += 1
            else:
                algos.append([cd.algo, 1])
        algos.append(["|", 1])
    code = ".".join("%s" % a if n == 1 else "%s*%d" % (a, n) for a, n in algos[:-1]).replace(".|.", "/")
    return ",".join(str(w) for w in ws), h.hexdigest()[:16], code


def window(H, W, seed, dev):
    rng = np.random.default_rng(seed)
    win = torch.zeros(H, W, 12)
    win[..., :9] = torch.from_numpy(np.where(rng.random((H, W, 1)) < 0.02, rng.uniform(-1, 1, (H, W, 9)), -1.0).astype(np.float32))
    return win.to(dev)


_gens = {}      # (spec, seed, T2V_CONV_ALGO, arith) -> HipGenerator: the cases share the packed weights of one selection


def generator(spec, seed, arith, dev):
    arith, layers = arith      # (arith, arith_layers)
    pack = (os.environ.get("T2V_CONV_ALGO", "0"), arith, layers)
    if any(k[2:] != pack for k in _gens):      # another algorithm selection: those weights are not needed again
        _gens.clear()
        torch.cuda.empty_cache()
    key = (repr(spec), seed) + pack
    if key not in _gens:
        _gens[key] = HipGenerator(spec, dev, arith=arith, arith_layers=layers).load_state_dict(synthetic_state_dict(spec, seed, flow_gain=0.1))
    return _gens[key]


def outputs(nets, H, W, nseq, kind, arith):
    dev = torch.device("cuda:0")
    gens = [generator(spec, seed, arith, dev) for spec, seed, _ in nets]
    h = hashlib.sha256()
    if kind == "features":
        prev = torch.zeros(H, W, 8, device=dev)
        prev[..., :6] = torch.tanh(torch.randn(H, W, 6, generator=torch.Generator().manual_seed(3))).to(dev)
        for t in range(3):
            res = gens[0].forward(window(H, W, 5 + t, dev), prev, want=("out", "img_feat", "flow_feat"))
            for k in ("out", "img_feat", "flow_feat"):
                h.update(res[k].cpu().numpy().tobytes())
            prev[..., :3] = prev[..., 3:6]
            prev[..., 3:6] = res["out"][..., :3]
    else:
        model = Vid2VidModelG(gens)
        wins = [window(H, W, 11 + q, dev) for q in range(nseq)]
        states = [Recurrence() for _ in range(nseq)]
        if kind == "staggered":     # the last sequence joins one frame late
            model.inference_nhwc_batch(wins[:-1], states[:-1])
        for t in range(3):
            for o in model.inference_nhwc_batch(wins, states):
                h.update(o.cpu().numpy().tobytes())
    torch.cuda.synchronize()
    ops.check_async_errors()
    return h.hexdigest()


def run(name, switches):
    nets, H, W, nseq, kind = CASES[name]
    env = {k: v for k, v in switches.items() if k.startswith("T2V_")}
    arith, layers = switches.get("arith", "fp32"), switches.get("arith_layers", "trunk")
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    ops.reload_env()
    try:
        conv_algo = int(os.environ.get("T2V_CONV_ALGO", "0"))
        if arith == "bf16x2":
            conv_algo = _lib.CONV_ALGO_BF16X2_STRIDE2 if layers == "trunk+stride2" else _lib.CONV_ALGO_BF16X2
        line = "%s %s ws=%s layers=%s algos=%s" % ((name, ",".join("%s=%s" % kv for kv in sorted(switches.items())) or "default")
                                                  + plan(nets, H, W, nseq, conv_algo))
        if not args.sizes_only:
            line += " out=%s" % outputs(nets, H, W, nseq, kind, (arith, layers))
        print(line, flush=True)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        ops.reload_env()


# (the settings that select other algorithms, and so pack other weights, come last)
names = args.cases.split(",")
for name in names:
    for switches in (SWITCHES[:5] if name == "a" else [{}]):
        run(name, switches)
for switches in (SWITCHES[5:] if "a" in names else []):
    run("a", switches)
