"""T2V_ALGO_DIRECT_BF16X2 on the GPU (text2video_amd/csrc/conv_igemm_split.hip = libt2v_split.so, reached through libt2v_hip.so):
the packed weights and the split-emitting passes bit for bit against the pair layout of what the fp32 kernels store, the conv
against the float64 emulation of its own operands and against the exact layer (tests/split_direct_reference.py), zero padding
exactly, the refusals of every gradient entry, and the generator with arith_outer=True against the float64 oracle.
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
import split_direct_reference as sdr
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
    return mk(ops.ALGO_DIRECT), mk(ops.ALGO_DIRECT_BF16X2)


def _weight(g, Cin, Cout, up):
    return _rand(g, *((Cin, Cout, 3, 3) if up else (Cout, Cin, 3, 3)), scale=(9 * Cin) ** -0.5)


def _i32(t):
    return t.contiguous().view(torch.int32).cpu()


@pytest.mark.parametrize("up", [False, True], ids=["conv2d", "convtranspose2d"])
@pytest.mark.parametrize("Cin,Cout", [(64, 128), (96, 256)])
def test_packed_weights_are_the_pair_layout_of_the_fp32_packing(up, Cin, Cout):
    from text2video_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(4)
    d0, d6 = _descs(ops, 16, 16, Cin, Cout, up)
    w = _weight(g, Cin, Cout, up).to(dev)
    p0, p6 = ops.pack_conv_weight(w, d0, Cin), ops.pack_conv_weight(w, d6, Cin)
    assert p0.numel() == p6.numel() == Cout * 9 * Cin and p0.abs().max().item() > 0.01
    assert torch.equal(_i32(p6), sdr.pairs_i32(p0.cpu()))


APPLY_MAPS = [(10, 14, 32), (37, 42, 128)]


@pytest.mark.parametrize("mode", ["plain", "relu", "relu_affine"])
@pytest.mark.parametrize("H,W,C", APPLY_MAPS)
def test_split_emitting_apply_pass_is_the_pair_layout_of_the_fp32_pass(H, W, C, mode):
    from text2video_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(3)
    x = _rand(g, H, W, C, offset=0.25).to(dev)
    mr = torch.stack([_rand(g, C, scale=0.5, offset=0.3), torch.rand(C, generator=g) + 0.5], -1).to(dev).contiguous()
    kw = {"relu": mode != "plain"}
    if mode == "relu_affine":
        kw["gamma"], kw["beta"] = _rand(g, C, scale=0.5, offset=1.0).to(dev), _rand(g, C, scale=0.5, offset=0.2).to(dev)
    y32 = ops.instance_norm_apply(x, mr, **kw)
    buf = torch.full((H * W * C + 64,), NAN, device=dev)
    ops.instance_norm_apply_bf16x2(x, mr, out=buf[:H * W * C].view(H, W, C), **kw)
    torch.cuda.synchronize()
    assert y32.abs().max().item() > 0.5 and (mode == "plain" or (y32 == 0).any())
    want = sdr.pairs_i32(y32.cpu())
    assert torch.equal(_i32(buf[:H * W * C]).view(H, W, C), want)
    assert torch.isnan(buf[H * W * C:]).all(), "the pass wrote behind the map"
    inplace = x.clone()                                   # y == x: the generator's form
    ops.instance_norm_apply_bf16x2(inplace, mr, out=inplace, **kw)
    assert torch.equal(_i32(inplace), want)


@pytest.mark.parametrize("H,W,C", APPLY_MAPS)
def test_split_pass_of_the_single_layer_entry(H, W, C):
    """stage 1 of t2v_conv2d_forward_winograd_stages with algo 6: the workspace receives the pair layout of x, nothing else"""
    from text2video_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(8)
    He, We = H + H % 2, W + W % 2
    _, d6 = _descs(ops, He, We, C, 128, False)
    x = _rand(g, He, We, C, offset=0.25).to(dev)
    n = He * We * C
    assert ops.winograd_workspace(d6, C, dev).numel() == n
    ws = torch.full((n + 64,), NAN, device=dev)
    y = torch.full((He // 2, We // 2, 128), NAN, device=dev)
    ops.conv2d_winograd(x, torch.zeros(128 * 9 * C, device=dev), None, d6, out=y, workspace=ws, stages=1)
    torch.cuda.synchronize()
    assert torch.equal(_i32(ws[:n]).view(He, We, C), sdr.pairs_i32(x.cpu()))
    assert torch.isnan(ws[n:]).all() and torch.isnan(y).all()


# up, H, W, Cin, Cout
CONV_SHAPES = [(False, 2, 2, 32, 128),          # one output pixel
               (False, 20, 28, 32, 128),        # M = 140: one whole tile + a ragged one, 9 stages
               (False, 16, 24, 96, 256),        # 27 stages, two N tiles
               (False, 64, 64, 128, 256),       # the real channel counts, 36 stages
               (True, 1, 1, 32, 128),           # phase runs of 1, 2, 2, 4 stages: shorter than the ring
               (True, 7, 5, 64, 128),           # odd map, ragged phase grid
               (True, 20, 20, 96, 256),
               (True, 32, 32, 256, 128)]        # the real channel counts
_IDS = ["%s_%dx%d_%d_%d" % ("up" if s[0] else "down", s[1], s[2], s[3], s[4]) for s in CONV_SHAPES]


@pytest.mark.parametrize("up,H,W,Cin,Cout", CONV_SHAPES, ids=_IDS)
def test_conv_against_the_emulation_of_its_own_operands(up, H, W, Cin, Cout):
    """no bias, no statistics: every output within split_gemm_bound of the float64 sum of the three products of the operands
    the kernel read (the workspace's pairs; the weights' pairs are split(w) by the packing test), the rms of the deviation
    within split_gemm_rms_bound per group of outputs with one K"""
    from text2video_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(5)
    _, d6 = _descs(ops, H, W, Cin, Cout, up)
    x, w = _rand(g, H, W, Cin, offset=0.25), _weight(g, Cin, Cout, up)
    pw = ops.pack_conv_weight(w.to(dev), d6, Cin)
    ws = ops.winograd_workspace(d6, Cin, dev).fill_(NAN)
    y = ops.conv2d_winograd(x.to(dev), pw, None, d6, workspace=ws)
    torch.cuda.synchronize()
    xh, xl = sdr.unpairs(ws.cpu(), H, W, Cin)
    assert torch.equal(xh, sr.split(x)[0]) and torch.equal(xl, sr.split(x)[1])
    wh, wl = sr.split(w)
    zero = torch.zeros(Cout)
    ref = sdr.conv64(xh, wh, zero, up) + sdr.conv64(xh, wl, zero, up) + sdr.conv64(xl, wh, zero, up)
    got = y.cpu().double()
    assert got.shape == ref.shape and torch.isfinite(got).all() and ref.abs().max().item() > 0.1
    ratio = (got - ref).abs() / sdr.split_gemm_bound(xh, xl, wh, wl, up)
    rr = max((got - ref)[m].pow(2).mean().sqrt().item() / b for m, b in sdr.split_gemm_rms_bound(xh, xl, wh, wl, up))
    print("%s %dx%d %d -> %d: worst |y - emulation| / bound %.3g; rms(y - emulation) / rms bound, worst group %.3g"
          % ("up" if up else "down", H, W, Cin, Cout, ratio.max().item(), rr))
    assert ratio.max().item() <= 1.0, [int(i) for i in torch.nonzero(ratio == ratio.max())[0]]
    assert rr <= 1.0


@pytest.mark.parametrize("up,H,W,Cin,Cout", [s for s in CONV_SHAPES if s[1] <= 28], ids=[i for s, i in zip(CONV_SHAPES, _IDS) if s[1] <= 28])
def test_zero_padding_is_exact_on_ones(up, H, W, Cin, Cout):
    """x = 1, w = 1: every output is (taps in range) x Cin, integers that bf16 and the fp32 accumulators hold exactly"""
    from text2video_amd import ops
    dev = _dev()
    _, d6 = _descs(ops, H, W, Cin, Cout, up)
    w = torch.ones(*((Cin, Cout, 3, 3) if up else (Cout, Cin, 3, 3)), device=dev)
    y = ops.conv2d_winograd(torch.ones(H, W, Cin, device=dev), ops.pack_conv_weight(w, d6, Cin), None, d6)
    want = (sdr.taps_in_range(H, W, up) * Cin).float()[..., None].expand(-1, -1, Cout)
    assert torch.equal(y.cpu(), want)


@pytest.mark.parametrize("up,H,W,Cin,Cout", [CONV_SHAPES[1], CONV_SHAPES[3], CONV_SHAPES[5], CONV_SHAPES[7]],
                         ids=[_IDS[1], _IDS[3], _IDS[5], _IDS[7]])
def test_whole_conv_against_float64(up, H, W, Cin, Cout):
    """bias and statistics partials: within split_direct_bound of the exact layer, (mean, rstd) within the bounds that follow
    from it, and two calls bit-identical"""
    from text2video_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(6)
    _, d6 = _descs(ops, H, W, Cin, Cout, up)
    x, w, b = _rand(g, H, W, Cin, offset=0.25), _weight(g, Cin, Cout, up), _rand(g, Cout, scale=0.1)
    pw = ops.pack_conv_weight(w.to(dev), d6, Cin)
    stats = torch.full_like(ops.conv_stats_buffer(d6, dev), NAN)
    y = ops.conv2d_winograd(x.to(dev), pw, b.to(dev), d6, stats=stats)
    stats2 = torch.full_like(stats, NAN)
    y2 = ops.conv2d_winograd(x.to(dev), pw, b.to(dev), d6, stats=stats2)
    torch.cuda.synchronize()
    assert torch.equal(y, y2) and torch.equal(stats, stats2), "two calls differ"
    ref, bnd = sdr.conv64(x, w, b, up), sdr.split_direct_bound(x, w, b, up)
    got = y.cpu().double()
    assert got.shape == ref.shape and torch.isfinite(got).all() and torch.isfinite(stats).all()
    ratio = (got - ref).abs() / bnd
    print("whole conv (%s %dx%d %d -> %d): worst |y - f64| / bound %.3g, max |y - f64| %.3g, rms error %.3g of the output's rms"
          % ("up" if up else "down", H, W, Cin, Cout, ratio.max().item(), (got - ref).abs().max().item(),
             (got - ref).pow(2).mean().sqrt().item() / ref.pow(2).mean().sqrt().item()))
    assert ratio.max().item() <= 1.0
    mr = ops.instance_norm_finalize(stats, d6).view(-1, 2).double().cpu()
    parts = stats.numel() // (2 * Cout)
    m_, s_, e_m, e_s = kv.stats_bounds(ref.permute(2, 0, 1), bnd.permute(2, 0, 1), parts)
    assert ((mr[:, 0] - m_).abs() <= e_m).all() and ((mr[:, 1] - s_).abs() <= e_s).all()


@pytest.mark.parametrize("up", [False, True], ids=["down", "up"])
def test_gradient_entries_refuse_the_split_form(up):
    """algo 6 into each weight-gradient, packing-for-gradients and unpack entry: T2V_ERR_INVALID, a message that names the form,
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
            assert "T2V_ALGO_DIRECT_BF16X2" in msg and "algo 6" in msg, (name, msg)
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


@pytest.mark.parametrize("H,W", [(64, 64), (96, 80)])
def test_generator_outer_scope_against_the_float64_oracle(exact_device_oracle, H, W):
    """ngf 128, one down-sampling level, 2 blocks, flow on: conv_algo 5 puts algo 6 on the 128 -> 256 layer of both encoders and
    on the 256 -> 128 transposed layer of both branches (each behind a one-block chain whose closing apply pass stores the
    pair layout); two consecutive frames, every path fed the oracle's previous frames.  The arith_outer frame stays below the
    1e-3 parity bar and within twice the trunk+stride2 frame's deviation from float64 measured in the same run (the
    allowance the split-bf16 generator tests give a max-over-map statistic).  
    Measured on the MI355X (profiles/split_bf16_outer_accuracy.txt): max |frame - f64| at 64 x 64 3.3e-5 fp32, 3.33e-4
    trunk+stride2, 3.40e-4 arith_outer (1.02 x); at 96 x 80 4.1e-5, 4.61e-4, 4.55e-4 (0.99 x)."""
    from oracle.generator_ref import CompositeGenerator, Vid2VidInferenceRef
    from text2video_amd import _lib, ops
    from text2video_amd.generator import GeneratorSpec, HipGenerator, Recurrence, Vid2VidModelG, synthetic_state_dict
    dev = "cuda:0"
    spec = GeneratorSpec(ngf=128, n_downsample=1, n_blocks=2, no_flow=False, norm="batch")
    descs = _layer_descs(spec, H, W, _lib.CONV_ALGO_BF16X2_OUTER)
    down = [cd.algo for cd in descs if cd.kH == 3 and cd.stride == 2 and not cd.transposed]
    upl = [cd.algo for cd in descs if cd.kH == 3 and cd.stride == 2 and cd.transposed]
    assert down == [ops.ALGO_DIRECT_BF16X2] * 2 and upl == [ops.ALGO_DIRECT_BF16X2] * 2, (down, upl)
    sd = synthetic_state_dict(spec, 1, "vid2vid", flow_gain=0.1)
    net = CompositeGenerator(spec.input_nc, 3, spec.prev_nc, spec.ngf, spec.n_downsample, spec.n_blocks, spec.no_flow, spec.norm)
    net.load_state_dict(sd, strict=False)
    ref64 = Vid2VidInferenceRef([copy.deepcopy(net).double().to(dev)])
    hip32 = Vid2VidModelG([HipGenerator(spec, dev).load_state_dict(sd)])
    hips2 = Vid2VidModelG([HipGenerator(spec, dev, arith="bf16x2", arith_layers="trunk+stride2").load_state_dict(sd)])
    hipo = Vid2VidModelG([HipGenerator(spec, dev, arith="bf16x2", arith_layers="trunk+stride2", arith_outer=True).load_state_dict(sd)])
    assert (hip32.nets[0].conv_algo, hips2.nets[0].conv_algo, hipo.nets[0].conv_algo) == (0, 4, 5)
    poses = _pose_seq(4, H, W, seed=9)
    e32 = es2 = eo = dx = 0.0
    for t in range(2, 4):
        A = poses[t - 2:t + 1].unsqueeze(0)
        if ref64.fake_B_prev is not None:
            for m in (hip32, hips2, hipo):
                m.load_prev([p.float() for p in ref64.fake_B_prev])
        truth = ref64.inference(A.double().to(dev)).cpu()
        y32 = hip32.inference(A.to(dev))[0].cpu().double()
        ys2 = hips2.inference(A.to(dev))[0].cpu().double()
        yo = hipo.inference(A.to(dev))[0].cpu().double()
        e32 = max(e32, (y32 - truth).abs().max().item())
        es2 = max(es2, (ys2 - truth).abs().max().item())
        eo = max(eo, (yo - truth).abs().max().item())
        dx = max(dx, (yo - ys2).abs().max().item())
    line = ("generator %dx%d: max |fp32 - f64| %.3e, max |trunk+stride2 - f64| %.3e, max |arith_outer - f64| %.3e (ratio to "
            "trunk+stride2 %.3g, allowed 2), max |arith_outer - trunk+stride2| %.3e" % (H, W, e32, es2, eo, eo / es2, dx))
    print(line)
    assert truth.abs().max().item() > 0.05 and truth.std().item() > 0.01
    assert dx > 0.0, "the arith_outer frame is the trunk+stride2 frame bit for bit: the scope did not engage"
    assert eo < 1e-3
    assert eo <= 2 * es2
    # two sequences in lock-step: each one's frame is the single-sequence frame, bit for bit, in this scope too
    wins = [ops.nchw_to_nhwc(poses[t:t + 3].reshape(9, H, W).contiguous().cuda()) for t in (0, 1)]
    alone = [hipo.inference_nhwc_batch([w], [Recurrence()])[0].clone() for w in wins]
    both = hipo.inference_nhwc_batch(wins, [Recurrence(), Recurrence()])
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


CLI_ARGS = ["--name", "fadg0", "--dataroot", "datasets/fadg0", "--dataset_mode", "pose", "--input_nc", "3", "--resize_or_crop",
            "scaleHeight", "--loadSize", "128", "--openpose_only", "--how_many", "1200", "--no_first_img", "--random_drop_prob", "0",
            "--synthetic_weights", "1", "--ngf", "128", "--n_downsample_G", "1", "--n_blocks", "2"]
SCOPE = ["--arith", "bf16x2", "--arith_layers", "trunk+stride2"]


def test_command_line_arith_outer(tmp_path):
    """vid2vid/test.py --arith bf16x2 --arith_layers trunk+stride2 --arith_outer on the fixture dataset with synthetic weights at
    128 x 80: all frames written, for the generator whose layer list carries the form (the frames differ from the scope below
    it by ~1e-4, less than a byte of the JPEG: that the scope engages is the generator test's `dx > 0`)"""
    from text2video_amd import _lib, ops
    from text2video_amd.model import generator_specs
    from text2video_amd.options import TestOptions
    opt = TestOptions().parse(CLI_ARGS + SCOPE + ["--arith_outer"])
    specs = generator_specs(opt)
    assert len(specs) == 1 and opt.arith_outer is True
    work = _make_dataset(str(tmp_path))
    base = [sys.executable, os.path.join(ROOT, "vid2vid", "test.py")] + CLI_ARGS
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="0")
    res = os.path.join(work, "results", "fadg0", "test_latest")

    def run(extra):
        shutil.rmtree(os.path.join(work, "results"), ignore_errors=True)
        r = subprocess.run(base + extra, cwd=work, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        files = sorted(glob.glob(os.path.join(res, "*", "fake_B_*.jpg")))
        return {os.path.relpath(f, res): open(f, "rb").read() for f in files}

    s2 = run(SCOPE)
    outer = run(SCOPE + ["--arith_outer"])
    assert len(s2) == 8 and sorted(outer) == sorted(s2)
    from PIL import Image
    import io
    a = np.asarray(Image.open(io.BytesIO(outer["tmp/fake_B_0003.jpg"])))
    H, W = a.shape[:2]
    algos = [cd.algo for cd in _layer_descs(specs[0], H, W, _lib.CONV_ALGO_BF16X2_OUTER)]
    # (--openpose_only: no flow branch, so the 128 -> 256 layer of both encoders and the one decoder's 256 -> 128)
    assert specs[0].no_flow and algos.count(ops.ALGO_DIRECT_BF16X2) == 3 and a.std() > 1.0, (algos, a.shape)
    r = subprocess.run(base + ["--arith", "bf16x2", "--arith_outer"], cwd=work, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "--arith_layers trunk+stride2" in r.stderr, r.stderr[-2000:]
