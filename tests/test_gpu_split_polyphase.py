"""T2V_ALGO_POLYPHASE_BF16X2 on the GPU (text2video_amd/csrc/polyphase_split.hip, winograd_split.hip): the split-emitting
transforms bit for bit against `split` of what the fp32 polyphase kernels store, the 81-position GEMM stage against the float64
emulation of its own planes (tests/split_reference.py), the whole conv against the float64 layer, the refusals of every gradient
entry, and the generator with arith="bf16x2", arith_layers="trunk+stride2" against the float64 oracle and the trunk-only frame.
A missing symbol or a refused algo fails; nothing skips."""
import copy
import ctypes
import glob
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import kernel_variants as kv
import split_polyphase_reference as spr
import split_reference as sr

pytestmark = pytest.mark.gpu
NAN = float("nan")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _dev():
    assert torch.cuda.is_available(), "GPU test without a GPU"
    return torch.device("cuda:0")


def _rand(g, *shape, scale=1.0, offset=0.0):
    return torch.randn(*shape, generator=g) * scale + offset


def _descs(ops, H, W, Cin, Cout, up):
    mk = lambda algo: ops.conv_desc(H, W, Cin, Cout, 3, 2, 1, ops.PAD_ZERO, up, algo=algo)
    return mk(ops.ALGO_POLYPHASE), mk(ops.ALGO_POLYPHASE_BF16X2)


def _planes(buf, *shape):
    """the first 2 * prod(shape) bf16 of an fp32 buffer as int16 [2, *shape]"""
    n = int(np.prod(shape))
    return buf.view(torch.int16)[:2 * n].view(2, *shape)


def _weight(g, Cin, Cout, up):
    return _rand(g, *((Cin, Cout, 3, 3) if up else (Cout, Cin, 3, 3)), scale=(9 * Cin) ** -0.5)


# up, H, W, C, real tiles, Tt
INPUT_MAPS = [(False, 16, 24, 32, 6, 64), (False, 36, 44, 64, 30, 64), (False, 80, 88, 32, 110, 128),
              (True, 7, 9, 32, 6, 64), (True, 44, 48, 64, 132, 192)]


@pytest.mark.parametrize("mode", ["plain", "relu", "relu_affine"])
@pytest.mark.parametrize("up,H,W,C,T_want,Tt_want", INPUT_MAPS)
def test_input_transform_planes_are_the_split_of_the_fp32_transform(up, H, W, C, T_want, Tt_want, mode):
    from text2video_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(3)
    d3, d5 = _descs(ops, H, W, C, 128, up)
    T, Tt, _, _, Ho, Wo = spr.geometry(H, W, up)
    assert (T, Tt) == (T_want, Tt_want)
    x = _rand(g, 1, H, W, C, offset=0.25).to(dev)
    lazy = {}
    if mode != "plain":
        lazy["mean_rstd"] = torch.stack([_rand(g, 1, C, scale=0.5, offset=0.3), torch.rand(1, C, generator=g) + 0.5], -1).to(dev).contiguous()
        lazy["relu"] = 1
        if mode == "relu_affine":
            lazy["gamma"], lazy["beta"] = _rand(g, C, scale=0.5, offset=1.0).to(dev), _rand(g, C, scale=0.5, offset=0.2).to(dev)
    out = []
    for d in (d3, d5):
        ws = ops.winograd_batch_workspace(d, C, 1, dev).fill_(NAN)
        y = torch.empty(1, Ho, Wo, 128, device=dev)
        pu = torch.zeros(81 * 128 * C, device=dev)       # stage 1 does not read the weights
        ops.conv2d_winograd_batch(x, pu, None, d, ws, out=y, stages=1, **lazy)
        torch.cuda.synchronize()
        out.append(ws)
    ws3, ws5 = out
    assert ws3.numel() == ws5.numel()
    V = ws3[:81 * Tt * C].view(81, Tt, C)
    assert torch.isfinite(V).all() and V[:, :T].abs().max().item() > 0.1
    want = sr.split_planes_i16(V)
    got = _planes(ws5, 81, Tt, C)
    bad = (got != want)
    assert not bad.any(), "%d of %d plane elements differ, first at [plane, pos, row, c] %s" % (
        int(bad.sum()), bad.numel(), [int(i) for i in torch.nonzero(bad)[0]])
    assert (got[:, :, T:] == 0).all()                    # padding rows: zeros in both planes
    assert torch.isnan(ws5[81 * Tt * C:]).all(), "the stage wrote behind V"


@pytest.mark.parametrize("up,Cin,Cout", [(False, 64, 128), (True, 96, 256)], ids=["conv2d", "convtranspose2d"])
def test_packed_weight_planes_are_the_split_of_the_fp32_packing(up, Cin, Cout):
    from text2video_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(4)
    d3, d5 = _descs(ops, 16, 16, Cin, Cout, up)
    w = _weight(g, Cin, Cout, up).to(dev)
    u3, u5 = ops.pack_conv_weight(w, d3, Cin), ops.pack_conv_weight(w, d5, Cin)
    assert u3.numel() == u5.numel() == 81 * Cout * Cin
    assert u3.abs().max().item() > 0.01
    assert torch.equal(_planes(u5, 81, Cout, Cin), sr.split_planes_i16(u3.view(81, Cout, Cin)))


GEMM_MAPS = [(False, 16, 24, 64), (False, 80, 88, 128), (True, 44, 48, 192)]     # up, H, W, Tt


@pytest.mark.parametrize("K", [32, 64, 96, 160])        # 1, 2, 3 and 5 stages on the 3-slot ring
@pytest.mark.parametrize("up,H,W,Tt_want", GEMM_MAPS)
def test_gemm_stage_against_the_emulation_of_its_own_planes(up, H, W, Tt_want, K):
    """(the float64 emulation and its bounds are evaluated on the device: 81 positions of up to 192 x 256 x 160)"""
    from text2video_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(5)
    T, Tt, _, _, Ho, Wo = spr.geometry(H, W, up)
    assert Tt == Tt_want
    x = _rand(g, 1, H, W, K, offset=0.25).to(dev)
    for Cout in (128, 256):
        _, d5 = _descs(ops, H, W, K, Cout, up)
        pu = ops.pack_conv_weight(_weight(g, K, Cout, up).to(dev), d5, K)
        ws = ops.winograd_batch_workspace(d5, K, 1, dev).fill_(NAN)
        y = torch.empty(1, Ho, Wo, Cout, device=dev)
        ops.conv2d_winograd_batch(x, pu, None, d5, ws, out=y, stages=1)
        nv, nm = 81 * Tt * K, 81 * Tt * Cout
        M = ws[nv:nv + nm].view(81, Tt, Cout)
        ops.conv2d_winograd_batch(x, pu, None, d5, ws, out=y, stages=2)
        torch.cuda.synchronize()
        first = M.clone()
        M.fill_(NAN)
        ops.conv2d_winograd_batch(x, pu, None, d5, ws, out=y, stages=2)
        torch.cuda.synchronize()
        assert torch.equal(first, M), "two launches differ"
        assert torch.isfinite(M).all(), "every row of M, padding included, is written"
        ah, al = sr.planes_to_float(_planes(ws, 81, Tt, K)[:, :, :T])
        bh, bl = sr.planes_to_float(_planes(pu, 81, Cout, K))
        ref = sr.split_gemm64(ah, al, bh, bl)
        bnd = sr.split_gemm_bound(ah, al, bh, bl, K)
        ratio = (M[:, :T].double() - ref).abs() / bnd
        worst = ratio.max().item()
        rr = sr.rms(M[:, :T].double() - ref) / sr.split_gemm_rms_bound(ah, al, bh, bl, K)
        print("K %d Cout %d %s %dx%d: worst |M - emulation| / bound %.3g; rms(M - emulation) / rms bound, worst position %.3g"
              % (K, Cout, "up" if up else "down", H, W, worst, rr.max().item()))
        assert ref.abs().max().item() > 0.1
        assert worst <= 1.0, "worst ratio %.3g at [pos, row, n] %s" % (worst, [int(i) for i in torch.nonzero(ratio == ratio.max())[0]])
        assert rr.max().item() <= 1.0, "rms ratio %.3g at position %d" % (rr.max().item(), int(rr.argmax()))
        assert (M[:, T:] == 0).all(), "padding tile rows of V are zeros, so are theirs of M"
        assert torch.isnan(ws[nv + nm:]).all(), "the stage wrote behind M"


@pytest.mark.parametrize("up,H,W", [(False, 32, 32), (True, 20, 20)], ids=["down", "up"])
def test_whole_conv_against_float64(up, H, W):
    """t2v_conv2d_forward_winograd with algo 5, bias and statistics partials, within the fp32 polyphase pipeline's bound
    composed with the split term (split_polyphase_reference.split_pipeline_bound)."""
    from text2video_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(6)
    Cin, Cout = 64, 128
    _, d5 = _descs(ops, H, W, Cin, Cout, up)
    x = _rand(g, H, W, Cin, offset=0.25)
    w, b = _weight(g, Cin, Cout, up), _rand(g, Cout, scale=0.1)
    pu = ops.pack_conv_weight(w.to(dev), d5, Cin)
    stats = torch.full_like(ops.conv_stats_buffer(d5, dev), NAN)
    y = ops.conv2d_winograd(x.to(dev), pu, b.to(dev), d5, stats=stats)
    torch.cuda.synchronize()
    ref = spr.conv64(x, w, b, up)
    bnd = spr.split_pipeline_bound(x, w, b, up)
    got = y.cpu().double()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    ratio = (got - ref).abs() / bnd
    print("whole conv (%s): worst |y - f64| / bound %.3g, max |y - f64| %.3g, rms error %.3g of the output's rms"
          % ("up" if up else "down", ratio.max().item(), (got - ref).abs().max().item(),
             (got - ref).pow(2).mean().sqrt().item() / ref.pow(2).mean().sqrt().item()))
    assert ratio.max().item() <= 1.0
    mr = ops.instance_norm_finalize(stats, d5).view(-1, 2).double().cpu()
    parts = stats.numel() // (2 * Cout)
    m_, s_, e_m, e_s = kv.stats_bounds(ref.permute(2, 0, 1), bnd.permute(2, 0, 1), parts)
    assert ((mr[:, 0] - m_).abs() <= e_m).all() and ((mr[:, 1] - s_).abs() <= e_s).all()


@pytest.mark.parametrize("up", [False, True], ids=["down", "up"])
def test_gradient_entries_refuse_the_split_form(up):
    """algo 5 into each weight-gradient, packing-for-gradients and unpack entry: T2V_ERR_INVALID, a message that names the form,
    nothing launched"""
    from text2video_amd import ops
    dev = _dev()
    c = ops.context(dev)
    lib, h, s = c.lib, c.handle, ops._stream()
    _, d = _descs(ops, 16, 16, 128, 128, up)
    buf = torch.zeros(1 << 20, device=dev)
    p = ctypes.c_void_p(buf.data_ptr())
    D = ctypes.byref(d)
    calls = {
        "backward_weight": lambda: lib.t2v_conv2d_backward_weight(h, s, D, 1, p, 128, p, 128, p, 0, p),
        "backward_weight_strided": lambda: lib.t2v_conv2d_backward_weight_strided(h, s, D, 1, p, 128, 4096, p, 128, 4096, p, 0, p),
        "backward_weight_winograd": lambda: lib.t2v_conv2d_backward_weight_winograd(h, s, D, 1, p, 128, p, 128, p, 0, p),
        "backward_weight_winograd_stages": lambda: lib.t2v_conv2d_backward_weight_winograd_stages(h, s, D, 1, 0, 1, p, 128, p, 128, p, 0, p, 3),
        "backward_weight_winograd_dy_norm": lambda: lib.t2v_conv2d_backward_weight_winograd_dy_norm(h, s, D, 1, 0, 128, p, p, p, None, None, 1, p, p),
        "forward_winograd_keep_v": lambda: lib.t2v_conv2d_forward_winograd_keep_v(h, s, D, p, 128, p, p, p, 128, None, p, p, 1, 0),
        "backward_data_winograd": lambda: lib.t2v_conv2d_backward_data_winograd(h, s, D, 1, 0, p, 128, p, p, p),
        "backward_data_winograd_fw": lambda: lib.t2v_conv2d_backward_data_winograd_fw(h, s, D, 1, 0, p, 128, p, p, p),
        "pack_weight_transposed": lambda: lib.t2v_conv_pack_weight_transposed(h, s, D, 128, p, p),
        "pack_weight_adjoint": lambda: lib.t2v_conv_pack_weight_adjoint(h, s, D, 128, p, p),
        "unpack_weight": lambda: lib.t2v_conv_unpack_weight(h, s, D, 128, p, p),
    }
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        for name, call in calls.items():
            assert call() == -1, name
            msg = lib.t2v_last_error().decode()
            assert "T2V_ALGO_POLYPHASE_BF16X2" in msg and "algo 5" in msg, (name, msg)
        torch.cuda.synchronize()
    ran = [e.name for e in prof.events() if "t2v::" in e.name]
    assert not ran, ran
    assert not buf.any()


def _pose_seq(n, H, W, seed):
    rng = np.random.default_rng(seed)
    a = -np.ones((n, 3, H, W), np.float32)
    m = rng.random((n, 1, H, W)) < 0.02
    return torch.from_numpy(np.where(m, rng.uniform(-1, 1, size=(n, 3, H, W)).astype(np.float32), a))


def _layer_descs(spec, H, W, conv_algo):
    from text2video_amd import _lib
    from text2video_amd.generator import _gen_desc
    gd = _gen_desc(spec, H, W, conv_algo)
    lib = _lib.load()
    out = []
    for i in range(lib.t2v_generator_num_layers(ctypes.byref(gd))):
        cd, xcs = _lib.ConvDesc(), ctypes.c_int()
        assert lib.t2v_generator_layer_desc(ctypes.byref(gd), i, ctypes.byref(cd), ctypes.byref(xcs)) == 0
        out.append(cd)
    return out


@pytest.fixture
def exact_device_oracle():
    """oracle/generator_ref.py evaluated on the GPU by ATen's native kernels + rocBLAS in exact fp64 (no MIOpen), the setting
    tests/test_gpu_device_oracle.py shows to be the CPU oracle where the CPU is affordable"""
    old = (torch.backends.cudnn.enabled, torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32)
    torch.backends.cudnn.enabled = False
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cudnn.enabled, torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = old


def test_generator_trunk_and_stride2_against_the_float64_oracle(exact_device_oracle):
    """384 x 384, ngf 64, n_downsample 3, 2 blocks, flow on: four polyphase layers (two 256 -> 512 on 96 x 96, two 512 -> 256
    transposed on 48 x 48) and eight F(4x4,3x3) trunk convs; two consecutive frames, every path fed the oracle's previous
    frames.  The trunk+stride2 frame stays below the project's 1e-3 parity bar and within twice the trunk-only frame's
    deviation from float64 measured in the same run (the allowance tests/test_gpu_split_bf16.py gives a max-over-map
    statistic: RATIO_ALLOWED = 2 x measured).

    Measured on the MI355X (profiles/split_bf16_stride2_accuracy.txt): max |frame - f64| 6.6e-5 fp32, 2.67e-4 trunk-only,
    3.87e-4 trunk+stride2 (1.45 x trunk-only)."""
    from oracle.generator_ref import CompositeGenerator, Vid2VidInferenceRef
    from text2video_amd import _lib, ops
    from text2video_amd.generator import GeneratorSpec, HipGenerator, Recurrence, Vid2VidModelG, synthetic_state_dict
    dev = "cuda:0"
    H = W = 384
    spec = GeneratorSpec(ngf=64, n_downsample=3, n_blocks=2, no_flow=False, norm="batch")
    descs = _layer_descs(spec, H, W, _lib.CONV_ALGO_BF16X2_STRIDE2)
    s2 = [cd.algo for cd in descs if cd.kH == 3 and cd.stride == 2 and cd.Cin >= 256 and cd.Cout >= 256]
    trunk = [cd.algo for cd in descs if cd.kH == 3 and cd.stride == 1 and not cd.transposed]
    assert s2 == [ops.ALGO_POLYPHASE_BF16X2] * 4, s2
    assert len(trunk) == 8 and set(trunk) == {ops.ALGO_WINOGRAD_F4_BF16X2}, trunk
    assert [cd.algo for cd in descs].count(ops.ALGO_POLYPHASE_BF16X2) == 4
    sd = synthetic_state_dict(spec, 1, "vid2vid", flow_gain=0.1)
    net = CompositeGenerator(spec.input_nc, 3, spec.prev_nc, spec.ngf, spec.n_downsample, spec.n_blocks, spec.no_flow, spec.norm)
    net.load_state_dict(sd, strict=False)
    ref64 = Vid2VidInferenceRef([copy.deepcopy(net).double().to(dev)])
    hip32 = Vid2VidModelG([HipGenerator(spec, dev).load_state_dict(sd)])
    hipx2 = Vid2VidModelG([HipGenerator(spec, dev, arith="bf16x2").load_state_dict(sd)])
    hips2 = Vid2VidModelG([HipGenerator(spec, dev, arith="bf16x2", arith_layers="trunk+stride2").load_state_dict(sd)])
    assert (hip32.nets[0].conv_algo, hipx2.nets[0].conv_algo, hips2.nets[0].conv_algo) == (0, 3, 4)
    poses = _pose_seq(4, H, W, seed=9)
    e32 = ex2 = es2 = dx = 0.0
    for t in range(2, 4):
        A = poses[t - 2:t + 1].unsqueeze(0)
        if ref64.fake_B_prev is not None:
            for m in (hip32, hipx2, hips2):
                m.load_prev([p.float() for p in ref64.fake_B_prev])
        truth = ref64.inference(A.double().to(dev)).cpu()
        y32 = hip32.inference(A.to(dev))[0].cpu().double()
        yx2 = hipx2.inference(A.to(dev))[0].cpu().double()
        ys2 = hips2.inference(A.to(dev))[0].cpu().double()
        e32 = max(e32, (y32 - truth).abs().max().item())
        ex2 = max(ex2, (yx2 - truth).abs().max().item())
        es2 = max(es2, (ys2 - truth).abs().max().item())
        dx = max(dx, (ys2 - yx2).abs().max().item())
    print("generator 384x384: max |fp32 - f64| %.3e, max |trunk - f64| %.3e, max |trunk+stride2 - f64| %.3e (ratio to trunk-only "
          "%.3g, allowed 2), max |trunk+stride2 - trunk| %.3e" % (e32, ex2, es2, es2 / ex2, dx))
    assert truth.abs().max().item() > 0.05 and truth.std().item() > 0.01
    assert dx > 0.0, "the trunk+stride2 frame is the trunk-only frame bit for bit: the mode did not engage"
    assert es2 < 1e-3
    assert es2 <= 2 * ex2
    # two sequences in lock-step: each one's frame is the single-sequence frame, bit for bit, in this mode too
    wins = [ops.nchw_to_nhwc(poses[t:t + 3].reshape(9, H, W).contiguous().cuda()) for t in (0, 1)]
    alone = [hips2.inference_nhwc_batch([w], [Recurrence()])[0].clone() for w in wins]
    both = hips2.inference_nhwc_batch(wins, [Recurrence(), Recurrence()])
    assert all(torch.equal(a, b) for a, b in zip(alone, both))


def _make_dataset(tmp):
    from PIL import Image
    from text2video_amd.keypoints import read_keypoints
    root = os.path.join(tmp, "vid2vid", "datasets", "fadg0")
    for seq, pat in (("tmp", "%04d.jpg"), ("tmp_smooth", "smooth_%04d.jpg")):
        src = os.path.join(GOLD, "dataset_fadg0_l2", "test_openpose", seq)
        os.makedirs(os.path.join(root, "test_openpose", seq))
        os.makedirs(os.path.join(root, "test_img", seq))
        for i, f in enumerate(sorted(os.listdir(src))):
            shutil.copyfile(os.path.join(src, f), os.path.join(root, "test_openpose", seq, f))
            Image.fromarray(read_keypoints(os.path.join(src, f), (512, 384))).save(os.path.join(root, "test_img", seq, pat % i))
    return os.path.join(tmp, "vid2vid")


# the command line of the test below (after vid2vid/test.py); tests/golden/split_bf16_cli_parent_digest.json records it too
CLI_ARGS = ["--name", "fadg0", "--dataroot", "datasets/fadg0", "--dataset_mode", "pose", "--input_nc", "3", "--resize_or_crop",
            "scaleHeight", "--loadSize", "512", "--openpose_only", "--how_many", "1200", "--no_first_img", "--random_drop_prob", "0",
            "--synthetic_weights", "1", "--ngf", "64", "--n_blocks", "2"]


def test_command_line_arith_layers(tmp_path):
    """vid2vid/test.py --arith bf16x2 --arith_layers trunk+stride2 on the fixture dataset at 512 x 320 with ngf 64 (its
    256 <-> 512 layers are polyphase there: 160 tiles): all frames written, and not the bytes of --arith bf16x2 alone; and
    --arith bf16x2 alone writes the parent commit's bytes: tests/golden/split_bf16_cli_parent_digest.json holds the SHA-256 of
    the 8 frames the parent commit's build wrote for this command line, taken in the job that took this tree's."""
    import hashlib
    import json
    from text2video_amd import _lib, ops
    from text2video_amd.model import generator_specs
    from text2video_amd.options import TestOptions
    # the layer list of the generator these flags build (the options the runs below parse, the frames' 512 x 320)
    opt = TestOptions().parse(CLI_ARGS + ["--arith", "bf16x2", "--arith_layers", "trunk+stride2"])
    specs = generator_specs(opt)
    assert len(specs) == 1 and (opt.arith, opt.arith_layers) == ("bf16x2", "trunk+stride2")
    algos = [cd.algo for cd in _layer_descs(specs[0], 512, 320, _lib.CONV_ALGO_BF16X2_STRIDE2)]
    assert algos.count(ops.ALGO_POLYPHASE_BF16X2) == 3 and ops.ALGO_WINOGRAD_F4_BF16X2 in algos, algos
    assert ops.ALGO_POLYPHASE not in algos
    work = _make_dataset(str(tmp_path))
    base = [sys.executable, os.path.join(ROOT, "vid2vid", "test.py")] + CLI_ARGS
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="0")
    res = os.path.join(work, "results", "fadg0", "test_latest")

    def run(extra):
        shutil.rmtree(os.path.join(work, "results"), ignore_errors=True)
        r = subprocess.run(base + extra, cwd=work, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        files = sorted(glob.glob(os.path.join(res, "*", "fake_B_*.jpg")))
        return r, {os.path.relpath(f, res): open(f, "rb").read() for f in files}

    _, x2 = run(["--arith", "bf16x2"])
    assert len(x2) == 8
    with open(os.path.join(GOLD, "split_bf16_cli_parent_digest.json")) as fh:
        parent = json.load(fh)
    assert parent["args"] == CLI_ARGS + ["--arith", "bf16x2"] and len(parent["sha256"]) == 8
    got = {k: hashlib.sha256(v).hexdigest() for k, v in x2.items()}
    assert got == parent["sha256"], "--arith bf16x2 alone no longer writes the parent commit's frames: %s" % sorted(
        k for k in got if got[k] != parent["sha256"].get(k))
    _, s2 = run(["--arith", "bf16x2", "--arith_layers", "trunk+stride2"])
    assert sorted(s2) == sorted(x2)
    assert s2 != x2, "--arith_layers trunk+stride2 wrote the trunk-only frames byte for byte: the flag did not reach the generator"
    from PIL import Image
    import io
    a = np.asarray(Image.open(io.BytesIO(s2["tmp/fake_B_0003.jpg"])))
    assert a.shape == (512, 320, 3) and a.std() > 1.0
    r = subprocess.run(base + ["--arith_layers", "trunk+stride2"], cwd=work, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "--arith bf16x2" in r.stderr, r.stderr[-2000:]
