"""T2V_ALGO_DIRECT_BF16X2 without a GPU: the support predicate's truth table, the generator's selection under
t2v_gen_desc.conv_algo 5, the arguments that switch the scope on, and the float64 restatement of the arithmetic
(tests/split_direct_reference.py) against the exact layer and against an injected fault."""
import ctypes
import inspect

import pytest
import torch

import split_direct_reference as sdr
import split_reference as sr


def _desc(H, W, Cin, Cout, transposed=False, k=3, stride=2, pad=1, pad_mode=None, act=None, output_padding=None, algo=6):
    from text2video_amd import _lib
    pad_mode = _lib.PAD_ZERO if pad_mode is None else pad_mode
    act = _lib.ACT_NONE if act is None else act
    output_padding = int(transposed) if output_padding is None else output_padding
    return _lib.ConvDesc(H, W, Cin, Cout, k, k, stride, pad, pad_mode, int(transposed), act, 1.0, output_padding, algo)


# the frame's own layers: 128 -> 256 on 512 x 512, 256 -> 128 transposed on 256 x 256, the 512 x 320 and 512 x 680 maps
GOOD = [(512, 512, 128, 256, False), (256, 256, 256, 128, True), (512, 320, 128, 256, False), (256, 160, 256, 128, True),
        (512, 680, 128, 256, False), (256, 340, 256, 128, True), (2, 2, 32, 128, False), (1, 1, 32, 128, True)]


def test_predicate_truth_table(lib_built):
    from text2video_amd import _lib, ops
    lib = lib_built
    assert lib.t2v_abi_version() == 22 == _lib.ABI_VERSION
    assert _lib.ALGO_DIRECT_BF16X2 == 6 == ops.ALGO_DIRECT_BF16X2 and _lib.CONV_ALGO_BF16X2_OUTER == 5
    ok = lambda d, x_cs=None: lib.t2v_conv_direct_bf16x2_supported(ctypes.byref(d), d.Cin if x_cs is None else x_cs)
    for H, W, Cin, Cout, tr in GOOD:
        assert ok(_desc(H, W, Cin, Cout, tr)) == 1, (H, W, Cin, Cout, tr)
        assert ops.direct_bf16x2_supported(_desc(H, W, Cin, Cout, tr, algo=0))           # d->algo is ignored
    assert ok(_desc(64, 64, 128, 128, k=7, pad=3)) == 0                                  # 3x3 only
    assert ok(_desc(64, 64, 128, 128, stride=1)) == 0                                    # stride 2
    assert ok(_desc(64, 64, 128, 128, pad=0)) == 0                                       # pad 1
    assert ok(_desc(64, 64, 128, 128, pad_mode=_lib.PAD_REFLECT)) == 0                   # zero padding
    assert ok(_desc(64, 64, 128, 128, act=_lib.ACT_TANH)) == 0                           # no activation
    assert ok(_desc(64, 64, 128, 128), x_cs=132) == 0                                    # x_cs == Cin
    assert ok(_desc(64, 64, 24, 128)) == 0 and ok(_desc(64, 64, 48, 128), x_cs=48) == 0  # Cin % 32
    assert ok(_desc(64, 64, 128, 64)) == 0 and ok(_desc(64, 64, 128, 192)) == 0          # Cout % 128
    assert ok(_desc(63, 64, 128, 128)) == 0 and ok(_desc(64, 62 + 1, 128, 128)) == 0     # an odd map under a down conv
    assert ok(_desc(63, 65, 128, 128, True)) == 1                                        # (a transposed conv takes any map)
    assert ok(_desc(64, 64, 128, 128, True, output_padding=0)) == 0                      # output_padding 1
    assert ok(_desc(0, 64, 128, 128, True)) == 0                                         # H, W >= 1
    # the size limit: a map or a weight block of 0x7fff0000 bytes or more
    assert ok(_desc(2048, 2048, 128, 128)) == 0 and 2048 * 2048 * 128 * 4 >= 0x7fff0000  # the input map
    assert ok(_desc(1024, 1024, 128, 128)) == 1
    assert ok(_desc(2, 2, 8192, 8192)) == 0 and 9 * 8192 * 8192 * 4 >= 0x7fff0000        # the weight block
    assert ok(_desc(2, 2, 8192, 8192, True)) == 1 and 4 * 8192 * 8192 * 4 < 0x7fff0000   # (four taps at most per phase)
    assert ok(_desc(1024, 1024, 32, 512, True)) == 0                                     # the output map
    # the sizes are the direct form's; the workspace holds the split of x
    for H, W, Cin, Cout, tr in GOOD:
        d6, d0 = _desc(H, W, Cin, Cout, tr), _desc(H, W, Cin, Cout, tr, algo=0)
        B6, B0 = ctypes.byref(d6), ctypes.byref(d0)
        assert lib.t2v_conv_packed_weight_floats(B6, Cin) == lib.t2v_conv_packed_weight_floats(B0, Cin) > 0
        assert lib.t2v_conv_winograd_workspace_floats(B6, Cin) == H * W * Cin
        assert lib.t2v_conv_winograd_batch_workspace_floats(B6, Cin, 1) == H * W * Cin
        assert lib.t2v_conv_winograd_batch_workspace_floats(B6, Cin, 2) == 0
        Ho, Wo = (2 * H, 2 * W) if tr else (H // 2, W // 2)
        per_phase = -(-((Ho // 2) * (Wo // 2) if tr else Ho * Wo) // 128)
        assert lib.t2v_conv_stats_floats(B6) == (4 if tr else 1) * per_phase * Cout * 2       # one partial per 128 x 128 tile row
    bad = _desc(64, 64, 128, 64)
    assert lib.t2v_conv_winograd_workspace_floats(ctypes.byref(bad), 128) == 0
    assert lib.t2v_conv_packed_weight_floats(ctypes.byref(bad), 128) == 0


def test_the_library_never_proposes_the_form_and_gradient_queries_turn_it_away(lib_built):
    lib = lib_built
    for H, W, Cin, Cout, tr in GOOD:
        d = _desc(H, W, Cin, Cout, tr)
        D = ctypes.byref(d)
        for cap in range(0, 8):
            assert lib.t2v_conv_best_algo(D, Cin, cap) != 6
        assert lib.t2v_conv_backward_weight_winograd_supported(D, Cin, Cout) == 0
        assert lib.t2v_conv_backward_data_winograd_supported(D, Cin, Cout) == 0
        assert lib.t2v_conv_backward_data_winograd_takes_forward_weights(D, Cin, Cout) == 0
        assert lib.t2v_conv_backward_weight_strided_supported(D, Cin, Cout) == 0
        assert lib.t2v_conv_backward_weight_winograd_workspace_floats(D, Cin, 1) == 0
        assert lib.t2v_conv_backward_weight_workspace_floats(D, Cin, 1) == 0


def _layers(lib, spec, H, W, conv_algo):
    from text2video_amd import _lib
    from text2video_amd.generator import _gen_desc
    gd = _gen_desc(spec, H, W, conv_algo)
    n = lib.t2v_generator_num_layers(ctypes.byref(gd))
    assert n > 0
    out = []
    for i in range(n):
        cd, xcs = _lib.ConvDesc(), ctypes.c_int()
        assert lib.t2v_generator_layer_desc(ctypes.byref(gd), i, ctypes.byref(cd), ctypes.byref(xcs)) == 0
        out.append(cd)
    return out, lib.t2v_generator_workspace_bytes(ctypes.byref(gd))


@pytest.mark.parametrize("ngf,nd,nb,H,W,count", [(128, 3, 9, 512, 512, 4), (128, 3, 4, 512, 320, 4), (128, 3, 4, 512, 680, 4),
                                                  (128, 1, 2, 64, 64, 4), (128, 1, 2, 96, 80, 4), (128, 1, 1, 64, 64, 2),
                                                  (64, 3, 2, 384, 384, 4), (32, 2, 4, 160, 160, 0)])
def test_conv_algo_5_adds_the_direct_stride2_layers(lib_built, ngf, nd, nb, H, W, count):
    """conv_algo 5 reports algo 6 only on layers where 4 reports T2V_ALGO_DIRECT with stride 2, and what 4 reports everywhere
    else, and only on the measured classes (both channel counts >= 128: ngf 64's 64 -> 128 and ngf 32's layers stay fp32);
    algo 6 appears under neither 0, 3 nor 4; the workspace does not grow.  (128, 1, 1): no ResnetBlock between the
    encoder sum and the decoders, which both branches read -- those two layers stay fp32.)"""
    from text2video_amd.generator import GeneratorSpec
    spec = GeneratorSpec(ngf=ngf, n_downsample=nd, n_blocks=nb, no_flow=False, norm="batch")
    by = {ca: _layers(lib_built, spec, H, W, ca) for ca in (0, 3, 4, 5)}
    a4, a5 = [cd.algo for cd in by[4][0]], [cd.algo for cd in by[5][0]]
    assert len(a4) == len(a5)
    for cd4, x4, x5 in zip(by[4][0], a4, a5):
        if x5 == 6:
            assert x4 == 0 and cd4.kH == 3 and cd4.stride == 2 and cd4.Cin % 32 == 0 and cd4.Cout % 128 == 0
            assert cd4.Cin >= 128 and cd4.Cout >= 128          # the measured classes only (64 -> 128 stays fp32)
        else:
            assert x5 == x4
    assert a5.count(6) == count
    for ca in (0, 3, 4):
        assert 6 not in [cd.algo for cd in by[ca][0]]
    assert 0 < by[5][1] <= by[4][1] == by[0][1]


def test_generator_arguments_are_validated(monkeypatch):
    from text2video_amd import generator
    assert inspect.signature(generator.HipGenerator.__init__).parameters["arith_outer"].default is False
    spec = generator.GeneratorSpec(ngf=32, n_downsample=2, n_blocks=2, no_flow=False, norm="batch")
    # (every check comes before anything touches the GPU)
    with pytest.raises(ValueError, match="arith_outer=True extends"):
        generator.HipGenerator(spec, "cuda:0", arith_outer=True)
    with pytest.raises(ValueError, match="arith_outer=True extends"):
        generator.HipGenerator(spec, "cuda:0", arith="bf16x2", arith_outer=True)            # the trunk-only scope
    with pytest.raises(ValueError, match="conv_algo=5"):
        generator.HipGenerator(spec, "cuda:0", conv_algo=5)
    with pytest.raises(ValueError, match="conv_algo=5"):
        generator.HipGenerator(spec, "cuda:0", arith="bf16x2", arith_layers="trunk+stride2", conv_algo=5)
    with pytest.raises(ValueError, match="conv_algo=4"):
        generator.HipGenerator(spec, "cuda:0", arith="bf16x2", arith_layers="trunk+stride2", arith_outer=True, conv_algo=4)
    monkeypatch.setenv("T2V_CONV_ALGO", "5")
    with pytest.raises(ValueError, match="T2V_CONV_ALGO=5"):
        generator.HipGenerator(spec, "cuda:0")


FULL = ["--arith", "bf16x2", "--arith_layers", "trunk+stride2", "--arith_outer"]


def test_command_line_flag_needs_the_scope_below_it(capsys):
    from text2video_amd.options import TestOptions, TrainOptions
    opt = TestOptions().parse(FULL)
    assert (opt.arith, opt.arith_layers, opt.arith_outer) == ("bf16x2", "trunk+stride2", True)
    assert TestOptions().parse(FULL[:4]).arith_outer is False and TestOptions().parse([]).arith_outer is False
    for argv in (["--arith_outer"], ["--arith", "bf16x2", "--arith_outer"], ["--arith", "bf16x2", "--arith_layers", "trunk", "--arith_outer"]):
        with pytest.raises(SystemExit):
            TestOptions().parse(argv)
        assert "--arith bf16x2 --arith_layers trunk+stride2" in capsys.readouterr().err
    for argv in (["--arith_outer"], FULL):
        with pytest.raises(SystemExit):
            TrainOptions().parse(argv)
    assert "--arith_outer" in capsys.readouterr().err


def test_resident_server_key_carries_the_flag():
    from text2video_amd import resident
    from text2video_amd.options import TestOptions
    a = TestOptions().parse(FULL[:4] + ["--synthetic_weights", "1"])
    b = TestOptions().parse(FULL + ["--synthetic_weights", "1"])
    assert resident.model_key(a) != resident.model_key(b)


def _layer(up, H, W, Cin, Cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(H, W, Cin, generator=g) + 0.25
    w = torch.randn(*((Cin, Cout, 3, 3) if up else (Cout, Cin, 3, 3)), generator=g) * (9 * Cin) ** -0.5
    b = torch.randn(Cout, generator=g) * 0.1
    return x, w, b


def test_pair_layout_round_trip():
    v = torch.randn(3, 5, 8) * 3
    p = sdr.pairs_i32(v)
    assert p.dtype == torch.int32 and p.shape == v.shape
    hi, lo = sdr.unpairs(p, 3, 5, 8)
    assert torch.equal(hi, v.bfloat16().float()) and torch.equal(lo, (v - hi).bfloat16().float())
    # dword 0 of a pair: hi[c] in the low half, hi[c + 1] in the high half
    h16 = v.bfloat16().view(torch.int16).int() & 0xffff
    assert torch.equal(p[..., 0] & 0xffff, h16[..., 0]) and torch.equal((p[..., 0] >> 16) & 0xffff, h16[..., 1])


@pytest.mark.parametrize("up,H,W,Cin,Cout", [(False, 16, 24, 128, 256), (True, 8, 12, 256, 128)], ids=["down", "up"])
def test_emulation_is_within_the_split_direct_bound(lib_built, up, H, W, Cin, Cout):
    """N(0.25, 1) data, fan-in-scaled weights: the float64 restatement of the split conv against the exact layer stays within
    split_direct_bound.  It runs no kernel; what it asks of the build is that the form it restates exists and takes these
    shapes.  The figures are printed: 4.43e-6 (down) and 4.33e-6 (up) of the output's rms."""
    assert lib_built.t2v_conv_direct_bf16x2_supported(ctypes.byref(_desc(H, W, Cin, Cout, up)), Cin) == 1
    x, w, b = _layer(up, H, W, Cin, Cout, 21)
    ref, emu, bnd = sdr.conv64(x, w, b, up), sdr.split_conv64(x, w, b, up), sdr.split_direct_bound(x, w, b, up)
    err = (emu - ref).abs()
    rel = (emu - ref).pow(2).mean().sqrt().item() / ref.pow(2).mean().sqrt().item()
    print("%s %d -> %d on %d x %d: rms error %.3g of the output's rms, max error %.3g, worst error / bound %.3g"
          % ("up" if up else "down", Cin, Cout, H, W, rel, err.max().item(), (err / bnd).max().item()))
    assert ref.shape == emu.shape == bnd.shape and ref.abs().max().item() > 0.5
    assert (err <= bnd).all()
    assert rel > 1e-7          # the split is what the error is made of


@pytest.mark.parametrize("up,H,W,Cin,Cout", [(False, 16, 24, 32, 128), (False, 16, 24, 128, 128), (True, 8, 12, 64, 128),
                                             (True, 8, 12, 256, 128)])
def test_rms_bound_sees_a_dropped_product(up, H, W, Cin, Cout):
    """an emulation with xl * wh left out is at least 10 x split_gemm_rms_bound away from the full one, in every group of
    outputs with one K (the map; each sub-pixel phase): the GPU test's rms check can see a missing product"""
    x, w, b = _layer(up, H, W, Cin, Cout, 7)
    (xh, xl), (wh, wl) = sr.split(x), sr.split(w)
    full, fault = sdr.split_conv64(x, w, b, up), sdr.split_conv64(x, w, b, up, drop="product")
    for mask, bnd in sdr.split_gemm_rms_bound(xh, xl, wh, wl, up):
        r = (fault - full)[mask].pow(2).mean().sqrt().item() / bnd
        print("%s Cin %d, %d outputs: rms(fault) / rms bound %.3g" % ("up" if up else "down", Cin, int(mask.sum()) * Cout, r))
        assert r >= 10
