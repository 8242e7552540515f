"""T2V_ALGO_WINOGRAD_F4_BF16X2 (ABI 22) without a GPU: the host-side planning of the split-bf16 form, and the float64
emulation of its arithmetic (tests/split_reference.py) -- how far it is from the exact product, and that the bound the GPU
tests hold the GEMM kernel to sees the faults such a kernel can have."""
import ctypes

import pytest
import torch

import kernel_variants as kv
import split_reference as sr


def _desc(H, W, Cin, Cout, k=3, stride=1, pad=1, pad_mode=None, algo=4):
    from text2video_amd import _lib
    pad_mode = _lib.PAD_REFLECT if pad_mode is None else pad_mode
    return _lib.ConvDesc(H, W, Cin, Cout, k, k, stride, pad, pad_mode, 0, _lib.ACT_NONE, 1.0, 0, algo)


def test_abi_and_planning(lib_built):
    from text2video_amd import _lib
    lib = lib_built
    assert lib.t2v_abi_version() == 22 == _lib.ABI_VERSION
    assert _lib.ALGO_WINOGRAD_F4_BF16X2 == 4
    ok = lambda d: lib.t2v_conv_winograd_bf16x2_supported(ctypes.byref(d), d.Cin)
    assert ok(_desc(64, 64, 1024, 1024)) == 1 and ok(_desc(16, 16, 64, 128)) == 1
    assert ok(_desc(64, 64, 1024, 64)) == 0                                   # Cout % 128
    assert ok(_desc(64, 64, 24, 128)) == 0                                    # Cin % 32
    assert ok(_desc(64, 64, 128, 128, stride=2, pad_mode=_lib.PAD_ZERO)) == 0
    assert ok(_desc(64, 64, 128, 128, k=5, pad=2)) == 0
    # the mask of the fp32 forms is what it was
    assert lib.t2v_conv_winograd_supported(ctypes.byref(_desc(64, 64, 1024, 1024)), 1024) == 3
    for H, W, Cin, Cout in ((64, 64, 1024, 1024), (16, 16, 64, 128), (64, 40, 256, 128), (37, 42, 64, 256)):
        d4, d2 = _desc(H, W, Cin, Cout), _desc(H, W, Cin, Cout, algo=_lib.ALGO_WINOGRAD_F4)
        for nimg in (1, 2, 3):
            n4 = lib.t2v_conv_winograd_batch_workspace_floats(ctypes.byref(d4), Cin, nimg)
            assert n4 > 0 and n4 == lib.t2v_conv_winograd_batch_workspace_floats(ctypes.byref(d2), Cin, nimg)
        assert lib.t2v_conv_winograd_workspace_floats(ctypes.byref(d4), Cin) == \
            lib.t2v_conv_winograd_workspace_floats(ctypes.byref(d2), Cin) > 0
        assert lib.t2v_conv_packed_weight_floats(ctypes.byref(d4), Cin) == \
            lib.t2v_conv_packed_weight_floats(ctypes.byref(d2), Cin) == 36 * Cout * Cin
        assert lib.t2v_conv_stats_floats(ctypes.byref(d4)) == lib.t2v_conv_stats_floats(ctypes.byref(d2)) > 0
        assert lib.t2v_conv_winograd_gemm_form(ctypes.byref(d4), 1) == 8
    # a shape the form does not take has no sizes
    bad = _desc(64, 64, 1024, 64)
    assert lib.t2v_conv_winograd_workspace_floats(ctypes.byref(bad), 1024) == 0
    assert lib.t2v_conv_packed_weight_floats(ctypes.byref(bad), 1024) == 0
    # training is fp32: the backward queries turn the descriptor away, and the library never proposes the form
    d = _desc(64, 64, 1024, 1024)
    assert lib.t2v_conv_backward_weight_winograd_supported(ctypes.byref(d), 1024, 1024) == 0
    assert lib.t2v_conv_backward_data_winograd_supported(ctypes.byref(d), 1024, 1024) == 0
    assert lib.t2v_conv_backward_data_winograd_takes_forward_weights(ctypes.byref(d), 1024, 1024) == 0
    assert lib.t2v_conv_backward_weight_strided_supported(ctypes.byref(d), 1024, 1024) == 0
    assert lib.t2v_conv_backward_weight_winograd_workspace_floats(ctypes.byref(d), 1024, 1) == 0
    assert lib.t2v_conv_backward_weight_workspace_floats(ctypes.byref(d), 1024, 1) == 0
    for cap in range(0, 5):
        assert lib.t2v_conv_best_algo(ctypes.byref(d), 1024, cap) != 4


def _layer_algos(lib, spec, H, W, conv_algo):
    from text2video_amd import _lib
    from text2video_amd.generator import _gen_desc
    gd = _gen_desc(spec, H, W, conv_algo)
    n = lib.t2v_generator_num_layers(ctypes.byref(gd))
    assert n > 0
    out = []
    for i in range(n):
        cd, xcs = _lib.ConvDesc(), ctypes.c_int()
        assert lib.t2v_generator_layer_desc(ctypes.byref(gd), i, ctypes.byref(cd), ctypes.byref(xcs)) == 0
        out.append((cd.algo, cd.Cout, cd.kH, cd.stride))
    return out, lib.t2v_generator_workspace_bytes(ctypes.byref(gd)), lib.t2v_generator_workspace_bytes_batch(ctypes.byref(gd), 2)


@pytest.mark.parametrize("ngf,nd,H,W", [(32, 2, 160, 160), (16, 2, 160, 160), (128, 3, 512, 512), (32, 3, 64, 64), (128, 3, 512, 320)])
def test_layer_desc_selects_the_split_form_on_the_f4_trunk(lib_built, ngf, nd, H, W):
    """conv_algo 3 reports algo 4 exactly where conv_algo 0 reports F(4x4,3x3) and Cout % 128 == 0, and what 0 reports
    everywhere else; the workspace byte counts do not change."""
    from text2video_amd import _lib
    from text2video_amd.generator import GeneratorSpec
    spec = GeneratorSpec(ngf=ngf, n_downsample=nd, n_blocks=4, no_flow=False, norm="batch")
    a0, ws0, ws0b = _layer_algos(lib_built, spec, H, W, 0)
    a3, ws3, ws3b = _layer_algos(lib_built, spec, H, W, 3)
    assert len(a0) == len(a3)
    want = [(4 if (a == _lib.ALGO_WINOGRAD_F4 and cout % 128 == 0) else a) for a, cout, _, _ in a0]
    assert [a for a, _, _, _ in a3] == want
    assert (ws0, ws0b) == (ws3, ws3b) and ws0 > 0
    if (ngf, H) in ((32, 160), (128, 512)):
        assert 4 in want, "this geometry's ResnetBlock convs take F(4x4,3x3) on >= 128 channels"
    else:
        assert 4 not in want


def _operands(K, T=96, N=64, seed=0):
    g = torch.Generator().manual_seed(seed + K)
    a = torch.randn(1, T, K, generator=g)
    b = torch.randn(1, N, K, generator=g) * K ** -0.5
    return a, b


@pytest.mark.parametrize("K", [32, 64, 256, 1024])
def test_emulation_is_within_the_split_term_of_the_exact_product(K):
    a, b = _operands(K)
    (ah, al), (bh, bl) = sr.split(a), sr.split(b)
    # the definition: the subtraction is exact and the two terms carry >= 16 mantissa bits
    assert torch.equal((a - ah).double(), a.double() - ah.double())
    assert ((a.double() - ah.double() - al.double()).abs() <= 2.0 ** -17 * a.double().abs()).all()
    emu = sr.split_gemm64(ah, al, bh, bl)
    exact = sr.bmm_t(a, b)
    mag = sr.bmm_t(a.abs(), b.abs())
    ratio = ((emu - exact).abs() / mag).max().item() / 2.0 ** -18
    print("K = %d: worst |emulation - exact| / (|a| . |b|^T) = %.3g * 2^-18" % (K, ratio))
    assert ratio <= 3.5


def _faults(K):
    a, b = _operands(K, seed=7)
    (ah, al), (bh, bl) = sr.split(a), sr.split(b)
    keep = K - 32
    return (ah, al, bh, bl), sr.split_gemm64(ah, al, bh, bl), {
        "one product dropped": sr.split_gemm64(ah, al, bh, bl, drop="product"),
        "hi / lo planes swapped": sr.split_gemm64(al, ah, bh, bl),
        "last K stage dropped": sr.split_gemm64(ah[..., :keep], al[..., :keep], bh[..., :keep], bl[..., :keep])}


def test_gemm_bound_sees_injected_faults():
    """one product dropped, the hi / lo planes swapped, the last K stage dropped: a 25th percentile of |fault| / bound >= 10
    and a 10th percentile >= 2, the criterion of the fp32 kernels' sensitivity tests.

    Asserted at K = 32 for all three faults and at every K of the GPU cases for the dropped stage.  The two plane faults are
    a random sum of K terms of 2^-9 |a||b| (growing as sqrt(K)), the bound is the worst-case linear-depth one over 3K terms
    (growing as K * K): their ratio falls as K^-1.5 -- 25th percentiles of 12, 4.4, 2.4 and 1.1 at K = 32, 64, 96, 160 -- so
    beyond one stage the per-element bound alone does not tell a missing lo product from rounding; the rms bound of the same
    GPU test does, at every K (test_gemm_rms_bound_sees_the_plane_faults_at_every_k).  The figures for every K are printed."""
    rows = []
    for K in (32, 64, 96, 160):
        planes, ref, faults = _faults(K)
        bnd = sr.split_gemm_bound(*planes, K)
        for what, f in faults.items():
            r = ((f - ref).abs() / bnd).flatten()
            rows.append((K, what, r.quantile(0.10).item(), r.quantile(0.25).item()))
    lines = ["K %4d %-26s 10th pct %9.3g, 25th pct %9.3g" % t for t in rows]
    print("\n".join(lines))
    asserted = [(t, ln) for t, ln in zip(rows, lines) if t[0] == 32 or t[1] == "last K stage dropped"]
    assert len(asserted) == 6
    weak = [ln for t, ln in asserted if t[3] < 10 or t[2] < 2]
    assert not weak, "faults too close to the bound:\n" + "\n".join(weak)


@pytest.mark.parametrize("K", [32, 64, 96, 160])
def test_gemm_rms_bound_sees_the_plane_faults_at_every_k(K):
    """split_gemm_rms_bound, the typical-case check of the GPU GEMM test: each of the three faults is at least 10 x the bound
    at every K the GPU cases run (a missing or misplaced lo plane is ~2^-10 of a sum that grows as sqrt(K), the bound
    sqrt(3K) * 2^-24 of the absolute sum)."""
    planes, ref, faults = _faults(K)
    bnd = sr.split_gemm_rms_bound(*planes, K)
    for what, f in faults.items():
        r = (sr.rms(f - ref) / bnd).min().item()
        print("K %4d %-26s rms(fault) / rms bound %9.3g" % (K, what, r))
        assert r >= 10, what


def test_split_planes_round_trip():
    v = torch.randn(3, 5, 8) * 3
    p = sr.split_planes_i16(v)
    hi, lo = sr.planes_to_float(p)
    assert torch.equal(hi, v.bfloat16().float()) and torch.equal(lo, (v - hi).bfloat16().float())


def test_generator_arith_argument_is_validated(monkeypatch):
    from text2video_amd import generator
    assert generator.ARITHS == ("fp32", "bf16x2")
    import inspect
    assert inspect.signature(generator.HipGenerator.__init__).parameters["arith"].default == "fp32"
    # the mode has one switch: neither conv_algo=3 without arith nor the environment turns it on behind `arith`'s back (the
    # checks come before anything touches the GPU)
    spec = generator.GeneratorSpec(ngf=32, n_downsample=2, n_blocks=2, no_flow=False, norm="batch")
    with pytest.raises(ValueError, match="arith='bf16x2'"):
        generator.HipGenerator(spec, "cuda:0", conv_algo=3)
    monkeypatch.setenv("T2V_CONV_ALGO", "3")
    with pytest.raises(ValueError, match="T2V_CONV_ALGO=3"):
        generator.HipGenerator(spec, "cuda:0")
    with pytest.raises(ValueError, match="one of"):
        generator.HipGenerator(spec, "cuda:0", arith="fp16")
