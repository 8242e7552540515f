"""T2V_ALGO_WINOGRAD_F4_BF16X2 on the GPU (text2video_amd/csrc/winograd_split.hip): the split-emitting transforms bit for bit
against `split` of what the fp32 kernels store, the GEMM stage against the float64 emulation of its own planes
(tests/split_reference.py), the whole conv against a float64 conv, the refusals of every gradient entry, and the generator
with arith="bf16x2" against the float64 oracle and the fp32 frame.  A missing symbol or a refused algo fails; nothing skips."""
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
import torch.nn.functional as F

import kernel_variants as kv
import split_reference as sr

pytestmark = pytest.mark.gpu
NAN = float("nan")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

# max |bf16x2 - f64| / max |fp32 - f64| of the generator test below, measured on the first MI355X run of this test (frames 1
# and 2; profiles/split_bf16_accuracy.txt), and what the test allows: twice that (max-over-map on a 160 x 160 frame is noisy)
RATIO_MEASURED = 6.91
RATIO_ALLOWED = 2 * RATIO_MEASURED


def _dev():
    assert torch.cuda.is_available(), "GPU test without a GPU"
    return torch.device("cuda:0")


def _rand(g, *shape, scale=1.0, offset=0.0):
    return torch.randn(*shape, generator=g) * scale + offset


def _descs(ops, H, W, Cin, Cout, pad=1, reflect=True):
    mk = lambda algo: ops.conv_desc(H, W, Cin, Cout, 3, 1, pad, ops.PAD_REFLECT if reflect else ops.PAD_ZERO, algo=algo)
    return mk(ops.ALGO_WINOGRAD_F4), mk(ops.ALGO_WINOGRAD_F4_BF16X2)


def _tiles(H, W, nimg, pad=1):
    T = -(-(H + 2 * pad - 2) // 4) * -(-(W + 2 * pad - 2) // 4)
    return T, kv.pad_tiles(nimg * T)


def _planes(buf, *shape):
    """the first 2 * prod(shape) bf16 of an fp32 buffer as int16 [2, *shape]"""
    n = int(np.prod(shape))
    return buf.view(torch.int16)[:2 * n].view(2, *shape)


@pytest.mark.parametrize("nimg", [1, 2])
@pytest.mark.parametrize("mode", ["plain", "relu", "relu_affine", "res"])
@pytest.mark.parametrize("H,W,C,Tt_want", [(10, 14, 32, 64), (37, 42, 64, 128), (10, 14, 1024, 64)])
def test_input_transform_planes_are_the_split_of_the_fp32_transform(H, W, C, Tt_want, mode, nimg):
    """(the 1024-channel case takes the channel-slice grid that both kernels have for C % 1024 == 0)"""
    from text2video_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(3)
    d2, d4 = _descs(ops, H, W, C, 128)
    T, Tt = _tiles(H, W, nimg)
    assert Tt == (Tt_want if nimg == 1 else kv.pad_tiles(2 * T))
    x = _rand(g, nimg, H, W, C, offset=0.25).to(dev)
    lazy = {}
    if mode != "plain":
        lazy["mean_rstd"] = torch.stack([_rand(g, nimg, C, scale=0.5, offset=0.3), torch.rand(nimg, C, generator=g) + 0.5], -1).to(dev).contiguous()
        lazy["relu"] = int(mode != "res")
        if mode != "relu":
            lazy["gamma"], lazy["beta"] = _rand(g, C, scale=0.5, offset=1.0).to(dev), _rand(g, C, scale=0.5, offset=0.2).to(dev)
        if mode == "res":
            lazy["res"] = _rand(g, nimg, H, W, C).to(dev)
    out = []
    for d in (d2, d4):
        ws = ops.winograd_batch_workspace(d, C, nimg, dev).fill_(NAN)
        y = torch.empty(nimg, H, W, 128, device=dev)
        kw = dict(lazy)
        if mode == "res":
            kw["xout"] = torch.full_like(x, NAN)
        pu = torch.zeros(36 * 128 * C, device=dev)       # stage 1 does not read the weights
        ops.conv2d_winograd_batch(x, pu, None, d, ws, out=y, stages=1, **kw)
        torch.cuda.synchronize()
        out.append((ws, kw.get("xout")))
    (ws2, xo2), (ws4, xo4) = out
    assert ws2.numel() == ws4.numel()
    V = ws2[:36 * Tt * C].view(36, Tt, C)
    assert torch.isfinite(V).all()
    want = sr.split_planes_i16(V)
    got = _planes(ws4, 36, Tt, C)
    bad = (got != want)
    assert not bad.any(), "%d of %d plane elements differ, first at [plane, pos, row, c] %s" % (
        int(bad.sum()), bad.numel(), [int(i) for i in torch.nonzero(bad)[0]])
    assert (got[:, :, nimg * T:] == 0).all()             # padding rows: zeros in both planes
    # the stage wrote nothing behind V
    assert torch.isnan(ws4[36 * Tt * C:]).all()
    if mode == "res":
        assert torch.equal(xo2, xo4) and torch.isfinite(xo4).all()


@pytest.mark.parametrize("Cin,Cout", [(64, 128), (96, 256)])
def test_packed_weight_planes_are_the_split_of_the_fp32_packing(Cin, Cout):
    from text2video_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(4)
    d2, d4 = _descs(ops, 16, 16, Cin, Cout)
    w = _rand(g, Cout, Cin, 3, 3, scale=(9 * Cin) ** -0.5).to(dev)
    u2, u4 = ops.pack_conv_weight(w, d2, Cin), ops.pack_conv_weight(w, d4, Cin)
    assert u2.numel() == u4.numel() == 36 * Cout * Cin
    assert torch.equal(_planes(u4, 36, Cout, Cin), sr.split_planes_i16(u2.view(36, Cout, Cin)))


GEMM_MAPS = [(8, 8, 1, 64), (40, 40, 1, 128), (64, 40, 1, 192), (40, 40, 2, 256)]     # H, W, nimg, Tt


@pytest.mark.parametrize("K", [32, 64, 96, 160])        # 1, 2, 3 and 5 stages on the 3-slot ring
@pytest.mark.parametrize("H,W,nimg,Tt_want", GEMM_MAPS)
def test_gemm_stage_against_the_emulation_of_its_own_planes(H, W, nimg, Tt_want, K):
    from text2video_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(5)
    T, Tt = _tiles(H, W, nimg)
    assert Tt == Tt_want
    rows = nimg * T
    x = _rand(g, nimg, H, W, K, offset=0.25).to(dev)
    for Cout in (128, 256):
        _, d4 = _descs(ops, H, W, K, Cout)
        w = _rand(g, Cout, K, 3, 3, scale=(9 * K) ** -0.5).to(dev)
        pu = ops.pack_conv_weight(w, d4, K)
        ws = ops.winograd_batch_workspace(d4, K, nimg, dev).fill_(NAN)
        y = torch.empty(nimg, H, W, Cout, device=dev)
        ops.conv2d_winograd_batch(x, pu, None, d4, ws, out=y, stages=1)
        nv, nm = 36 * Tt * K, 36 * Tt * Cout
        M = ws[nv:nv + nm].view(36, Tt, Cout)
        ops.conv2d_winograd_batch(x, pu, None, d4, ws, out=y, stages=2)
        torch.cuda.synchronize()
        first = M.clone()
        M.fill_(NAN)
        ops.conv2d_winograd_batch(x, pu, None, d4, ws, out=y, stages=2)
        torch.cuda.synchronize()
        assert torch.equal(first, M), "two launches differ"
        assert torch.isfinite(M).all(), "every row of M, padding included, is written"
        ah, al = sr.planes_to_float(_planes(ws, 36, Tt, K)[:, :, :rows])
        bh, bl = sr.planes_to_float(_planes(pu, 36, Cout, K))
        ref = sr.split_gemm64(ah, al, bh, bl)
        bnd = sr.split_gemm_bound(ah, al, bh, bl, K)
        ratio = (M[:, :rows].double() - ref).abs() / bnd
        worst = ratio.max().item()
        print("K %d Cout %d map %dx%dx%d: worst |M - emulation| / bound %.3g" % (K, Cout, nimg, H, W, worst))
        # the typical case, per position: rms of the deviation within sqrt(3K) 2^-24 rms of the absolute sum -- the check that
        # sees a missing or misplaced lo plane at every K (tests/test_cpu_split_bf16.py)
        rr = sr.rms(M[:, :rows].double() - ref) / sr.split_gemm_rms_bound(ah, al, bh, bl, K)
        print("    rms(M - emulation) / rms bound, worst position %.3g" % rr.max().item())
        assert worst <= 1.0, "worst ratio %.3g at [pos, row, n] %s" % (worst, [int(i) for i in torch.nonzero(ratio == ratio.max())[0]])
        assert rr.max().item() <= 1.0, "rms ratio %.3g at position %d" % (rr.max().item(), int(rr.argmax()))
        assert torch.isnan(ws[nv + nm:]).all(), "the stage wrote behind M"


@pytest.mark.parametrize("reflect", [True, False])
def test_whole_conv_against_float64(reflect):
    """t2v_conv2d_forward_winograd with algo 4: reflect pad 1 and zero pad 1, bias and statistics partials, within the fp32
    pipeline's bounds composed with the split term (split_reference.split_pipeline_bound)."""
    from text2video_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(6)
    H, W, Cin, Cout = 40, 40, 64, 128
    _, d4 = _descs(ops, H, W, Cin, Cout, reflect=reflect)
    x = _rand(g, H, W, Cin, offset=0.25)
    w, b = _rand(g, Cout, Cin, 3, 3, scale=(9 * Cin) ** -0.5), _rand(g, Cout, scale=0.1)
    pu = ops.pack_conv_weight(w.to(dev), d4, Cin)
    stats = torch.full_like(ops.conv_stats_buffer(d4, dev), NAN)
    y = ops.conv2d_winograd(x.to(dev), pu, b.to(dev), d4, stats=stats)
    torch.cuda.synchronize()
    xp = x.double().permute(2, 0, 1)[None]
    xp = F.pad(xp, (1,) * 4, mode="reflect") if reflect else F.pad(xp, (1,) * 4)
    ref = F.conv2d(xp, w.double(), b.double())[0].permute(1, 2, 0)
    bnd = sr.split_pipeline_bound(x, w, b, 1, reflect)
    got = y.cpu().double()
    assert torch.isfinite(got).all()
    ratio = (got - ref).abs() / bnd
    print("whole conv (reflect %s): worst |y - f64| / bound %.3g, max |y - f64| %.3g" % (reflect, ratio.max().item(), (got - ref).abs().max().item()))
    assert ratio.max().item() <= 1.0
    mr = ops.instance_norm_finalize(stats, d4).view(-1, 2).double().cpu()
    parts = stats.numel() // (2 * Cout)
    m_, s_, e_m, e_s = kv.stats_bounds(ref.permute(2, 0, 1), bnd.permute(2, 0, 1), parts)
    assert ((mr[:, 0] - m_).abs() <= e_m).all() and ((mr[:, 1] - s_).abs() <= e_s).all()


def test_gradient_entries_refuse_the_split_form():
    """algo 4 into each backward, weight-gradient and data-gradient entry: T2V_ERR_INVALID, a message that names the form,
    nothing launched"""
    from text2video_amd import ops
    dev = _dev()
    c = ops.context(dev)
    lib, h, s = c.lib, c.handle, ops._stream()
    _, d = _descs(ops, 16, 16, 128, 128)
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
            assert "BF16X2" in msg and "algo 4" in msg, (name, msg)
        torch.cuda.synchronize()
    ran = [e.name for e in prof.events() if "t2v::" in e.name]
    assert not ran, ran
    assert not buf.any()


def _pose_seq(n, H, W, seed):
    rng = np.random.default_rng(seed)
    a = -np.ones((n, 3, H, W), np.float32)
    m = rng.random((n, 1, H, W)) < 0.02
    return torch.from_numpy(np.where(m, rng.uniform(-1, 1, size=(n, 3, H, W)).astype(np.float32), a))


def test_generator_bf16x2_against_the_float64_oracle_and_the_fp32_frame():
    """160 x 160, n_downsample 2, ngf 32: a 40 x 40 bottleneck of 128 channels, the smallest square one whose ResnetBlock convs
    take F(4x4,3x3); 2 blocks, flow on, two consecutive frames (both paths fed the oracle's previous frames).  The bf16x2 frame
    stays below the project's 1e-3 parity bar, and its deviation from float64 within RATIO_ALLOWED of the fp32 frame's."""
    from oracle.generator_ref import CompositeGenerator, Vid2VidInferenceRef
    from text2video_amd import _lib, ops
    from text2video_amd.generator import GeneratorSpec, HipGenerator, Recurrence, Vid2VidModelG, _gen_desc, synthetic_state_dict
    H = W = 160
    spec = GeneratorSpec(ngf=32, n_downsample=2, n_blocks=2, no_flow=False, norm="batch")
    gd = _gen_desc(spec, H, W, _lib.CONV_ALGO_BF16X2)
    lib = _lib.load()
    algos = []
    for i in range(lib.t2v_generator_num_layers(ctypes.byref(gd))):
        cd, xcs = _lib.ConvDesc(), ctypes.c_int()
        assert lib.t2v_generator_layer_desc(ctypes.byref(gd), i, ctypes.byref(cd), ctypes.byref(xcs)) == 0
        if cd.kH == 3 and cd.stride == 1 and not cd.transposed:
            algos.append(cd.algo)
    assert algos and set(algos) == {ops.ALGO_WINOGRAD_F4_BF16X2}, algos
    sd = synthetic_state_dict(spec, 1, "vid2vid", flow_gain=0.1)
    net = CompositeGenerator(spec.input_nc, 3, spec.prev_nc, spec.ngf, spec.n_downsample, spec.n_blocks, spec.no_flow, spec.norm)
    net.load_state_dict(sd, strict=False)
    ref64 = Vid2VidInferenceRef([copy.deepcopy(net).double()])
    hip32 = Vid2VidModelG([HipGenerator(spec, "cuda:0").load_state_dict(sd)])
    hipx2 = Vid2VidModelG([HipGenerator(spec, "cuda:0", arith="bf16x2").load_state_dict(sd)])
    assert hipx2.nets[0].conv_algo == _lib.CONV_ALGO_BF16X2 and hip32.nets[0].conv_algo == 0
    poses = _pose_seq(4, H, W, seed=9)
    e32 = ex2 = dx = 0.0
    for t in range(2, 4):
        A = poses[t - 2:t + 1].unsqueeze(0)
        if ref64.fake_B_prev is not None:
            for m in (hip32, hipx2):
                m.load_prev([p.float() for p in ref64.fake_B_prev])
        truth = ref64.inference(A.double())
        y32 = hip32.inference(A.to("cuda:0"))[0].cpu().double()
        yx2 = hipx2.inference(A.to("cuda:0"))[0].cpu().double()
        e32 = max(e32, (y32 - truth).abs().max().item())
        ex2 = max(ex2, (yx2 - truth).abs().max().item())
        dx = max(dx, (yx2 - y32).abs().max().item())
    ratio = ex2 / e32
    print("generator 160x160: max |fp32 - f64| %.3e, max |bf16x2 - f64| %.3e, ratio %.3g (allowed %.3g), max |bf16x2 - fp32| %.3e"
          % (e32, ex2, ratio, RATIO_ALLOWED, dx))
    assert ex2 < 1e-3
    assert dx > 0.0, "the bf16x2 frame is the fp32 frame bit for bit: the mode did not engage"
    assert ratio <= RATIO_ALLOWED
    # two sequences in lock-step: each one's frame is the single-sequence frame, bit for bit, in this mode too
    wins = [ops.nchw_to_nhwc(poses[t:t + 3].reshape(9, H, W).contiguous().cuda()) for t in (0, 1)]
    alone = [hipx2.inference_nhwc_batch([w], [Recurrence()])[0].clone() for w in wins]
    both = hipx2.inference_nhwc_batch(wins, [Recurrence(), Recurrence()])
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


def test_command_line_arith_and_fp16(tmp_path):
    """vid2vid/test.py --arith bf16x2 writes its frames; --fp16 alone stays accepted and ignored: the frames of no flag, byte
    for byte, and a warning that names the mode that exists"""
    work = _make_dataset(str(tmp_path))
    base = [sys.executable, os.path.join(ROOT, "vid2vid", "test.py"), "--name", "fadg0", "--dataroot", "datasets/fadg0",
            "--dataset_mode", "pose", "--input_nc", "3", "--resize_or_crop", "scaleHeight", "--loadSize", "512",
            "--openpose_only", "--how_many", "1200", "--no_first_img", "--random_drop_prob", "0",
            "--synthetic_weights", "1", "--ngf", "32", "--n_blocks", "3"]
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="0")
    res = os.path.join(work, "results", "fadg0", "test_latest")

    def run(extra):
        shutil.rmtree(os.path.join(work, "results"), ignore_errors=True)
        r = subprocess.run(base + extra, cwd=work, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        files = sorted(glob.glob(os.path.join(res, "*", "fake_B_*.jpg")))
        return r, {os.path.relpath(f, res): open(f, "rb").read() for f in files}

    _, plain = run([])
    assert len(plain) == 8
    r16, fp16 = run(["--fp16"])
    assert fp16 == plain and "--arith bf16x2" in r16.stderr
    _, x2 = run(["--arith", "bf16x2"])
    assert sorted(x2) == sorted(plain)
    assert x2 != plain, "--arith bf16x2 wrote the fp32 frames byte for byte: the flag did not reach the generator"
    from PIL import Image
    import io
    a = np.asarray(Image.open(io.BytesIO(x2["tmp/fake_B_0003.jpg"])))
    assert a.shape == (512, 320, 3) and a.std() > 1.0
