"""T2V_ALGO_POLYPHASE_BF16X2 without a GPU: the host-side planning of the split-bf16 polyphase form, the generator's selection
under t2v_gen_desc.conv_algo 4, the arguments that switch the mode on, and the float64 emulation of the arithmetic
(tests/split_polyphase_reference.py) against the exact layer."""
import ctypes

import pytest
import torch

import split_polyphase_reference as spr


def _desc(H, W, Cin, Cout, transposed=False, stride=2, pad=1, pad_mode=None, algo=5):
    from text2video_amd import _lib
    pad_mode = _lib.PAD_ZERO if pad_mode is None else pad_mode
    return _lib.ConvDesc(H, W, Cin, Cout, 3, 3, stride, pad, pad_mode, int(transposed), _lib.ACT_NONE, 1.0, int(transposed), algo)


GOOD = [(128, 128, 512, 1024, False), (64, 64, 1024, 512, True), (16, 24, 32, 128, False), (128, 170, 512, 1024, False)]


def test_planning(lib_built):
    from text2video_amd import _lib, ops
    lib = lib_built
    assert lib.t2v_abi_version() == 22 == _lib.ABI_VERSION
    assert _lib.ALGO_POLYPHASE_BF16X2 == 5 == ops.ALGO_POLYPHASE_BF16X2 and _lib.CONV_ALGO_BF16X2_STRIDE2 == 4
    ok = lambda d, x_cs=None: lib.t2v_conv_polyphase_bf16x2_supported(ctypes.byref(d), d.Cin if x_cs is None else x_cs)
    for H, W, Cin, Cout, tr in GOOD:
        assert ok(_desc(H, W, Cin, Cout, tr)) == 1, (H, W, Cin, Cout, tr)
        assert ops.polyphase_bf16x2_supported(_desc(H, W, Cin, Cout, tr, algo=0))       # d->algo is ignored
    assert ok(_desc(64, 64, 128, 128, stride=1)) == 0
    assert ok(_desc(64, 64, 128, 128, pad_mode=_lib.PAD_REFLECT)) == 0
    assert ok(_desc(64, 64, 24, 128)) == 0                                       # Cin % 32
    assert ok(_desc(64, 64, 128, 64)) == 0                                       # Cout % 128
    assert ok(_desc(64, 64, 128, 128), x_cs=132) == 0                            # x_cs != Cin
    assert ok(_desc(63, 64, 128, 128)) == 0                                      # odd H on a down conv
    assert ok(_desc(63, 64, 128, 128, True)) == 1                                # (a transposed conv takes any map)
    # every size is T2V_ALGO_POLYPHASE's: the planes are the bytes of the fp32 tensors
    for H, W, Cin, Cout, tr in GOOD:
        d5, d3 = _desc(H, W, Cin, Cout, tr), _desc(H, W, Cin, Cout, tr, algo=_lib.ALGO_POLYPHASE)
        B5, B3 = ctypes.byref(d5), ctypes.byref(d3)
        assert lib.t2v_conv_packed_weight_floats(B5, Cin) == lib.t2v_conv_packed_weight_floats(B3, Cin) == 81 * Cout * Cin
        assert lib.t2v_conv_winograd_workspace_floats(B5, Cin) == lib.t2v_conv_winograd_workspace_floats(B3, Cin) > 0
        assert lib.t2v_conv_winograd_batch_workspace_floats(B5, Cin, 1) == lib.t2v_conv_winograd_batch_workspace_floats(B3, Cin, 1) > 0
        assert lib.t2v_conv_winograd_batch_workspace_floats(B5, Cin, 2) == lib.t2v_conv_winograd_batch_workspace_floats(B3, Cin, 2) == 0
        assert lib.t2v_conv_stats_floats(B5) == lib.t2v_conv_stats_floats(B3) > 0
    bad = _desc(64, 64, 128, 64)
    assert lib.t2v_conv_winograd_workspace_floats(ctypes.byref(bad), 128) == 0
    assert lib.t2v_conv_packed_weight_floats(ctypes.byref(bad), 128) == 0
    # training is fp32: the gradient-side queries turn the descriptor away, and the library never proposes the form
    for H, W, Cin, Cout, tr in GOOD:
        d = _desc(H, W, Cin, Cout, tr)
        D = ctypes.byref(d)
        assert lib.t2v_conv_backward_weight_winograd_supported(D, Cin, Cout) == 0
        assert lib.t2v_conv_backward_data_winograd_supported(D, Cin, Cout) == 0
        assert lib.t2v_conv_backward_data_winograd_takes_forward_weights(D, Cin, Cout) == 0
        assert lib.t2v_conv_backward_weight_strided_supported(D, Cin, Cout) == 0
        assert lib.t2v_conv_backward_weight_winograd_workspace_floats(D, Cin, 1) == 0
        assert lib.t2v_conv_backward_weight_workspace_floats(D, Cin, 1) == 0
        for cap in range(0, 6):
            assert lib.t2v_conv_best_algo(D, Cin, cap) != 5


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
        out.append(cd.algo)
    return out, lib.t2v_generator_workspace_bytes(ctypes.byref(gd)), lib.t2v_generator_workspace_bytes_batch(ctypes.byref(gd), 2)


@pytest.mark.parametrize("ngf,nd,nb,H,W,count", [(128, 3, 4, 512, 512, 8), (128, 3, 4, 512, 320, 8), (128, 3, 4, 512, 680, 8),
                                                  (64, 3, 2, 384, 384, 4), (32, 2, 4, 160, 160, 0)])
def test_conv_algo_4_selects_the_split_form_on_the_polyphase_layers(lib_built, ngf, nd, nb, H, W, count):
    """conv_algo 4 reports algo 5 exactly where conv_algo 0 reports T2V_ALGO_POLYPHASE, algo 4 exactly where conv_algo 3 does,
    and what 0 reports everywhere else; the workspace byte counts are those of 0"""
    from text2video_amd.generator import GeneratorSpec
    spec = GeneratorSpec(ngf=ngf, n_downsample=nd, n_blocks=nb, no_flow=False, norm="batch")
    a0, ws0, ws0b = _layer_algos(lib_built, spec, H, W, 0)
    a3, ws3, ws3b = _layer_algos(lib_built, spec, H, W, 3)
    a4, ws4, ws4b = _layer_algos(lib_built, spec, H, W, 4)
    assert len(a0) == len(a3) == len(a4)
    want = [5 if z == 3 else (4 if t == 4 else z) for z, t in zip(a0, a3)]
    assert a4 == want
    assert a4.count(5) == a0.count(3) == count
    assert 5 not in a3 and 5 not in a0 and 4 not in a0
    assert (ws0, ws0b) == (ws4, ws4b) == (ws3, ws3b) and ws0 > 0


def test_generator_arguments_are_validated(monkeypatch):
    from text2video_amd import generator
    import inspect
    assert generator.ARITH_LAYERS == ("trunk", "trunk+stride2")
    assert inspect.signature(generator.HipGenerator.__init__).parameters["arith_layers"].default == "trunk"
    spec = generator.GeneratorSpec(ngf=32, n_downsample=2, n_blocks=2, no_flow=False, norm="batch")
    # (every check comes before anything touches the GPU)
    with pytest.raises(ValueError, match="arith_layers='all': one of"):
        generator.HipGenerator(spec, "cuda:0", arith="bf16x2", arith_layers="all")
    with pytest.raises(ValueError, match="arith='bf16x2'"):
        generator.HipGenerator(spec, "cuda:0", arith_layers="trunk+stride2")
    with pytest.raises(ValueError, match="conv_algo=4"):
        generator.HipGenerator(spec, "cuda:0", conv_algo=4)
    with pytest.raises(ValueError, match="conv_algo=4"):
        generator.HipGenerator(spec, "cuda:0", arith="bf16x2", conv_algo=4)      # the trunk-only scope does not take 4
    monkeypatch.setenv("T2V_CONV_ALGO", "4")
    with pytest.raises(ValueError, match="T2V_CONV_ALGO=4"):
        generator.HipGenerator(spec, "cuda:0")


def test_command_line_scope_needs_the_mode(capsys):
    from text2video_amd.options import TestOptions, TrainOptions
    opt = TestOptions().parse(["--arith", "bf16x2", "--arith_layers", "trunk+stride2"])
    assert (opt.arith, opt.arith_layers) == ("bf16x2", "trunk+stride2")
    assert TestOptions().parse(["--arith", "bf16x2"]).arith_layers == "trunk"
    assert TestOptions().parse([]).arith_layers == "trunk"
    for argv in (["--arith_layers", "trunk+stride2"], ["--arith_layers", "trunk"], ["--arith", "fp32", "--arith_layers", "trunk+stride2"]):
        with pytest.raises(SystemExit):
            TestOptions().parse(argv)
        assert "--arith bf16x2" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        TestOptions().parse(["--arith", "bf16x2", "--arith_layers", "stride2"])
    with pytest.raises(SystemExit):
        TrainOptions().parse(["--arith_layers", "trunk+stride2"])


def test_resident_server_key_carries_the_scope():
    from text2video_amd import resident
    from text2video_amd.options import TestOptions
    a = TestOptions().parse(["--arith", "bf16x2", "--synthetic_weights", "1"])
    b = TestOptions().parse(["--arith", "bf16x2", "--arith_layers", "trunk+stride2", "--synthetic_weights", "1"])
    assert resident.model_key(a) != resident.model_key(b)


@pytest.mark.parametrize("up,H,W,Cin,Cout", [(False, 16, 24, 256, 512), (True, 8, 12, 256, 128)], ids=["down", "up"])
def test_emulation_is_within_the_split_pipeline_bound(lib_built, up, H, W, Cin, Cout):
    """A record of the arithmetic more than a check of the library: N(0,1) data, fan-in-scaled weights, the float64 emulation
    of the split polyphase conv against the exact layer.  It runs no kernel; what it asks of the build is that the form it
    emulates exists and takes these shapes (algo 5, t2v_conv_polyphase_bf16x2_supported).  The worst-case bound the GPU
    test holds the kernels to (split_pipeline_bound) is ~1000 x above this typical-case error (worst error / bound 0.0011
    down, 0.016 up), so the figures that say something are the printed ones: 1.67e-5 (down) and 1.59e-5 (up) of the output's
    rms, max error 9.0e-5 and 7.7e-5 -- recorded, not asserted: the bound stays the derived one."""
    from text2video_amd import _lib
    assert _lib.ALGO_POLYPHASE_BF16X2 == 5
    assert lib_built.t2v_conv_polyphase_bf16x2_supported(ctypes.byref(_desc(H, W, Cin, Cout, up)), Cin) == 1
    g = torch.Generator().manual_seed(21)
    x = torch.randn(H, W, Cin, generator=g)
    w = torch.randn(*((Cin, Cout, 3, 3) if up else (Cout, Cin, 3, 3)), generator=g) * (9 * Cin) ** -0.5
    b = torch.randn(Cout, generator=g) * 0.1
    ref = spr.conv64(x, w, b, up)
    emu = spr.split_conv64(x, w, b, up)
    bnd = spr.split_pipeline_bound(x, w, b, up)
    err = (emu - ref).abs()
    rel = (emu - ref).pow(2).mean().sqrt().item() / ref.pow(2).mean().sqrt().item()
    print("%s %d -> %d on %d x %d: rms error %.3g of the output's rms, max error %.3g, worst error / bound %.3g"
          % ("up" if up else "down", Cin, Cout, H, W, rel, err.max().item(), (err / bnd).max().item()))
    assert ref.shape == emu.shape == bnd.shape and ref.abs().max().item() > 0.5
    assert (err <= bnd).all()
    # the split is what the error is made of: the fp32-operand pipeline in the same float64 arithmetic is two orders closer
    assert rel > 1e-6
