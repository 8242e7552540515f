"""Operator-level Python surface over libt2v_hip.so.

Mirrors the reference's operator interface for the hot path -- the torch.nn.functional calls the
vid2vid generator makes on torch 0.4.1 ($SP/torch/nn/functional.py: conv2d, conv_transpose2d,
instance_norm:1258, grid_sample:2046, pad(reflect):2169, avg_pool2d) -- but on NHWC fp32 device
tensors and with the fusions the HIP kernels implement.  PyTorch is used only as the device
allocator / stream provider; every computation below is a call through the C ABI.
"""
import ctypes

from ._xp import torch     # the real torch, or leantorch under vid2vid/test.py's torch-free frame loop

from . import _flowlib, _gradfoldlib, _lib
from ._lib import (ACT_FLOW_W, ACT_LRELU, ACT_NONE, ACT_TANH, ALGO_DIRECT, ALGO_WINOGRAD,  # noqa: F401
                   ALGO_DIRECT_BF16X2, ALGO_POLYPHASE, ALGO_POLYPHASE_BF16X2, ALGO_WINOGRAD_F4, ALGO_WINOGRAD_F4_BF16X2, PAD_REFLECT, PAD_ZERO, VISUALS_FLOW, VISUALS_IMAGE, VISUALS_MAX_PANELS,
                   VISUALS_UNIT, ConvDesc, check)

_contexts = {}


def context(device=None):
    """Per-device t2v context (created lazily; requires a visible gfx950 GPU)."""
    if not torch.cuda.is_available():
        raise RuntimeError("text2video_amd: no HIP device visible; the frame-synthesis path has no CPU fallback")
    dev = torch.cuda.current_device() if device is None else torch.device(device).index or 0
    c = _contexts.get(dev)
    if c is None:
        with torch.cuda.device(dev):
            c = _lib.Context(dev)
        _contexts[dev] = c
    return c


def reload_env():
    """The library reads its T2V_* switches once (t2v_create); a process that changes one afterwards (tests, A/B runs)
    calls this."""
    _lib.load().t2v_reload_env()


def check_async_errors():
    """Raise if a kernel of an EARLIER launch reported an error it could only report after the fact (a fixed-grid
    accumulator hand-over that timed out: that launch's output holds NaNs).  Call after synchronising."""
    check(_lib.load().t2v_check_async_errors(), "check_async_errors")


def set_overlap_hint(on):
    """Tell the library that this thread runs a second stream beside the launches it issues (returns the previous value);
    t2v_generator_forward does it for its own two-stream frames -- bench.py uses it to time the kernel those frames run.
    on == 2: the second stream carries fixed-grid GEMMs of its own (the train step's weight gradients): the whole-tile
    fixed-grid GEMM and the Winograd-domain weight gradient launch ONE block per CU, so that the two streams' launches are
    resident side by side (include/t2v.h, t2v_set_overlap_hint)."""
    return int(_lib.load().t2v_set_overlap_hint(2 if on == 2 else (1 if on else 0)))


def fixed_grid_enabled():
    return bool(_lib.load().t2v_fixed_grid_enabled())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _chk(t, name):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError("%s must be a contiguous fp32 device tensor" % name)


def round_up(v, m):
    return (v + m - 1) // m * m


def conv_desc(H, W, Cin, Cout, k, stride=1, pad=0, pad_mode=PAD_ZERO, transposed=False, act=ACT_NONE,
              act_scale=1.0, output_padding=None, algo=0):
    if output_padding is None:
        output_padding = 1 if transposed else 0     # the generator's ConvTranspose2d(k3,s2,p1,op1)
    return ConvDesc(H, W, Cin, Cout, k, k, stride, pad, pad_mode, int(transposed), act, act_scale, output_padding,
                    algo)


def winograd_supported(desc, x_cs=None, algo=None):
    """True when `desc` can run as the Winograd variant `algo` (default: desc.algo, or F(2x2,3x3) for a direct desc)."""
    x_cs = round_up(desc.Cin, 4) if x_cs is None else x_cs
    algo = (desc.algo or ALGO_WINOGRAD) if algo is None else algo
    if algo == ALGO_WINOGRAD_F4_BF16X2:
        return bool(_lib.load().t2v_conv_winograd_bf16x2_supported(ctypes.byref(desc), x_cs))
    mask = _lib.load().t2v_conv_winograd_supported(ctypes.byref(desc), x_cs)
    return bool(mask & (2 if algo == ALGO_WINOGRAD_F4 else 1))


def polyphase_supported(desc, x_cs=None):
    """True when `desc` (a stride-2 3x3 conv or its transposed counterpart) can run as ALGO_POLYPHASE (include/t2v.h)."""
    x_cs = round_up(desc.Cin, 4) if x_cs is None else x_cs
    return bool(_lib.load().t2v_conv_polyphase_supported(ctypes.byref(desc), x_cs) & 1)


def polyphase_bf16x2_supported(desc, x_cs=None):
    """True when `desc` can run as ALGO_POLYPHASE_BF16X2: ALGO_POLYPHASE with its 81 GEMMs in split-bf16 arithmetic (forward
    only; V and the packed weight then hold two bf16 planes in the fp32 tensors' bytes)"""
    x_cs = round_up(desc.Cin, 4) if x_cs is None else x_cs
    return bool(_lib.load().t2v_conv_polyphase_bf16x2_supported(ctypes.byref(desc), x_cs))


def direct_bf16x2_supported(desc, x_cs=None):
    """True when `desc` (a 3x3 stride-2 conv or its transposed counterpart) can run as ALGO_DIRECT_BF16X2: the direct form with
    its contraction in split-bf16 arithmetic (forward only; the input map and the packed weight then hold, in place of every
    fp32 channel pair, its two bf16 terms)"""
    x_cs = round_up(desc.Cin, 4) if x_cs is None else x_cs
    return bool(_lib.load().t2v_conv_direct_bf16x2_supported(ctypes.byref(desc), x_cs))


def polyphase_pays(desc, x_cs=None):
    """... and the library's own rule selects it for this shape (the faster form: both channel counts >= 256)"""
    x_cs = round_up(desc.Cin, 4) if x_cs is None else x_cs
    return bool(_lib.load().t2v_conv_polyphase_supported(ctypes.byref(desc), x_cs) & 2)


def best_conv_algo(desc, x_cs=None, cap=0):
    """ALGO_* the library would pick for `desc` (fewest GEMM rows; generator.hip uses the same rule)."""
    x_cs = round_up(desc.Cin, 4) if x_cs is None else x_cs
    return _lib.load().t2v_conv_best_algo(ctypes.byref(desc), x_cs, cap)


def conv2d_auto(x, packed_w, bias, desc, y_cs=None, stats=None, out=None):
    """conv2d or conv2d_winograd, whichever desc.algo (and the weight packing that goes with it) says."""
    if desc.algo in (ALGO_WINOGRAD, ALGO_WINOGRAD_F4, ALGO_WINOGRAD_F4_BF16X2, ALGO_POLYPHASE, ALGO_POLYPHASE_BF16X2,
                     ALGO_DIRECT_BF16X2):
        assert y_cs is None or y_cs == desc.Cout
        return conv2d_winograd(x, packed_w, bias, desc, stats=stats, out=out)
    return conv2d(x, packed_w, bias, desc, y_cs=y_cs, stats=stats, out=out)


def with_algo(desc, algo):
    """copy of a conv descriptor with another algorithm"""
    return ConvDesc(desc.H, desc.W, desc.Cin, desc.Cout, desc.kH, desc.kW, desc.stride, desc.pad, desc.pad_mode,
                    desc.transposed, desc.act, desc.act_scale, desc.output_padding, algo)


GEMM_FORMS = {0: "conv_igemm_kernel<64x64 tiles, one block per tile>", 1: "conv_igemm_kernel<128x128 tiles, one block per tile>",
              2: "wino_gemm_sk_kernel<128x128 tiles on a fixed grid of 2 blocks per CU>",
              3: "wino_gemm_sk_kernel<192x64 tiles on a fixed grid of 2 blocks per CU>",
              4: "wino_gemm_sk_kernel<160x128 tiles on a fixed grid of 1 block per CU>",
              5: "wino_gemm_skr_kernel<ragged 128/96/64/32 x 128 tiles on a fixed grid of 2 blocks per CU>",
              6: "wino_gemm_sk_kernel<256x128 tiles on a fixed grid of 1 block per CU>",
              7: "wino_gemm_skt_kernel<ragged 96..192 x 128 tiles on a fixed grid of 1 block per CU>",
              8: "wino_split_gemm_kernel<128x128 tiles, one block per tile, split-bf16 on the bf16 matrix cores>"}


def winograd_gemm_form(desc, nimg=1):
    """name of the kernel form the F(4x4,3x3) GEMM stage of `desc` takes for `nimg` images per launch"""
    return GEMM_FORMS.get(_lib.load().t2v_conv_winograd_gemm_form(ctypes.byref(desc), nimg), "?")


def winograd_tile_rows(desc):
    """GEMM rows one image contributes per F(4x4,3x3) transform position (tile count, padded)"""
    return _lib.load().t2v_conv_winograd_tile_rows(ctypes.byref(desc))


def winograd_workspace(desc, x_cs, device):
    n = _lib.load().t2v_conv_winograd_workspace_floats(ctypes.byref(desc), x_cs)
    if n == 0:
        raise RuntimeError("winograd_workspace: shape not supported")
    return torch.empty(n, dtype=torch.float32, device=device)


def conv2d_winograd(x, packed_u, bias, desc, stats=None, out=None, workspace=None, stages=7, keep_v=None):
    """3x3 stride-1 reflect-pad-1 conv through Winograd (desc.algo: ALGO_WINOGRAD F(2x2,3x3) | ALGO_WINOGRAD_F4 F(4x4,3x3) |
    ALGO_WINOGRAD_F4_BF16X2, F(4x4,3x3) with split-bf16 GEMMs: V and the packed weight then hold two bf16 planes).
    stages: bit mask 1 = input transform, 2 = batched GEMM, 4 = output transform (all by default).
    ALGO_DIRECT_BF16X2 (a stride-2 / transposed layer) runs here as well: stage 1 splits x into the workspace, 2 | 4 is the conv.
    keep_v = (wgrad_ws, batch, slot): the input transform lands in that slot of the Winograd-domain weight gradient's workspace
    (backward_weight_winograd_workspace) and stays there for the backward pass (conv2d_backward_weight_winograd_dy)."""
    c = context()
    _chk(x, "x")
    x_cs = x.shape[-1]
    ws = workspace if workspace is not None else winograd_workspace(desc, x_cs, x.device)
    ho, wo = conv_out_dims(desc)
    y = out if out is not None else torch.empty(ho, wo, desc.Cout, dtype=torch.float32, device=x.device)
    if keep_v is not None:
        assert stages == 7
        wg, batch, slot = keep_v
        check(c.lib.t2v_conv2d_forward_winograd_keep_v(c.handle, _stream(), ctypes.byref(desc), _p(x), x_cs, _p(packed_u), _p(bias),
                                                       _p(y), desc.Cout, _p(stats), _p(ws), _p(wg), batch, slot),
              "conv2d_forward_winograd_keep_v")
        return y
    check(c.lib.t2v_conv2d_forward_winograd_stages(c.handle, _stream(), ctypes.byref(desc), _p(x), x_cs, _p(packed_u),
                                                   _p(bias), _p(y), desc.Cout, _p(stats), _p(ws), stages),
          "conv2d_forward_winograd")
    return y


def winograd_batch_workspace(desc, x_cs, nimg, device):
    """workspace of conv2d_winograd_batch: V and M of `nimg` packed F(4x4,3x3) images ([36][pad(nimg*T)][C]), then the
    fixed-grid GEMM's hand-over scratch"""
    n = _lib.load().t2v_conv_winograd_batch_workspace_floats(ctypes.byref(desc), x_cs, nimg)
    if n == 0:
        raise RuntimeError("winograd_batch_workspace: shape not supported")
    return torch.empty(n, dtype=torch.float32, device=device)


def conv2d_winograd_batch(x, packed_u, bias, desc, workspace, stats=None, out=None, stages=7, mean_rstd=None, gamma=None,
                          beta=None, relu=0, res=None, xout=None):
    """The generator's forms of a Winograd / polyphase conv (t2v_conv2d_forward_winograd_batch_stages): x [nimg,H,W,Cin]
    packed into one tile list (F(4x4) only for nimg > 1; workspace: winograd_batch_workspace), and with mean_rstd
    ([nimg*Cin*2]) the previous layer's norm applied in the input transform -- relu 1: relu(norm(x)); F(4x4) relu 0 with
    res and xout ([nimg,H,W,Cin]): norm(x) + res, also written to xout.  Returns y [nimg,Ho,Wo,Cout]."""
    c = context()
    if x.dim() == 3:
        x = x.unsqueeze(0)
    _chk(x, "x")
    nimg, x_cs = x.shape[0], x.shape[-1]
    ho, wo = conv_out_dims(desc)
    y = out if out is not None else torch.empty(nimg, ho, wo, desc.Cout, dtype=torch.float32, device=x.device)
    check(c.lib.t2v_conv2d_forward_winograd_batch_stages(c.handle, _stream(), ctypes.byref(desc), nimg, _p(x), x_cs,
                                                         x[0].numel(), _p(packed_u), _p(bias), _p(y), desc.Cout, _p(stats),
                                                         _p(workspace), stages, _p(mean_rstd), _p(gamma), _p(beta), int(relu),
                                                         _p(res), _p(xout)),
          "conv2d_forward_winograd_batch_stages")
    return y


def conv_out_dims(desc):
    h, w = ctypes.c_int(), ctypes.c_int()
    check(_lib.load().t2v_conv_out_dims(ctypes.byref(desc), ctypes.byref(h), ctypes.byref(w)), "conv_out_dims")
    return h.value, w.value


def pack_conv_weight(weight, desc, x_cs=None, adjoint=False):
    """weight: torch layout ([Cout,Cin,kH,kW], or [Cin,Cout,3,3] if desc.transposed) on the device.
    adjoint=True: `desc` is the data-gradient conv of a stride-1 layer and `weight` that layer's FORWARD weight
    ([desc.Cin, desc.Cout, k, k]); flip and transpose happen inside the packing kernel."""
    c = context()
    _chk(weight, "weight")
    x_cs = round_up(desc.Cin, 4) if x_cs is None else x_cs
    n = c.lib.t2v_conv_packed_weight_floats(ctypes.byref(desc), x_cs)
    if n == 0:
        raise RuntimeError("pack_conv_weight: %s" % c.lib.t2v_last_error().decode())
    packed = torch.empty(n, dtype=torch.float32, device=weight.device)
    fn = c.lib.t2v_conv_pack_weight_adjoint if adjoint else c.lib.t2v_conv_pack_weight
    check(fn(c.handle, _stream(), ctypes.byref(desc), x_cs, _p(weight), _p(packed)), "conv_pack_weight")
    return packed


def conv_stats_buffer(desc, device):
    n = _lib.load().t2v_conv_stats_floats(ctypes.byref(desc))
    return torch.empty(max(n, 1), dtype=torch.float32, device=device)


def conv2d(x, packed_w, bias, desc, y_cs=None, stats=None, out=None):
    """x: [H,W,x_cs] NHWC.  Returns y [Hout,Wout,y_cs].  Reflection padding, bias, the head
    activation and (if `stats` is given) the instance-norm partial statistics are fused."""
    c = context()
    _chk(x, "x")
    x_cs = x.shape[-1]
    ho, wo = conv_out_dims(desc)
    y_cs = round_up(desc.Cout, 4) if y_cs is None else y_cs
    y = out if out is not None else torch.empty(ho, wo, y_cs, dtype=torch.float32, device=x.device)
    check(c.lib.t2v_conv2d_forward(c.handle, _stream(), ctypes.byref(desc), _p(x), x_cs, _p(packed_w), _p(bias),
                                   _p(y), y_cs, _p(stats)), "conv2d_forward")
    return y


def conv2d_head_norm(x, packed_w, bias, desc, mean_rstd, gamma=None, beta=None, relu=True, y_cs=None, out=None):  # relu: must be on
    """A 7x7 head on the RAW output x [H,W,x_cs] of the conv before it: the kernel applies that layer's norm ((mean, rstd)
    from instance_norm_finalize, gamma / beta, ReLU) to its halo planes.  Same bits as instance_norm_apply + conv2d."""
    c = context()
    _chk(x, "x")
    _chk(mean_rstd, "mean_rstd")
    x_cs = x.shape[-1]
    ho, wo = conv_out_dims(desc)
    y_cs = round_up(desc.Cout, 4) if y_cs is None else y_cs
    y = out if out is not None else torch.empty(ho, wo, y_cs, dtype=torch.float32, device=x.device)
    check(c.lib.t2v_conv2d_forward_head_norm(c.handle, _stream(), ctypes.byref(desc), _p(x), x_cs, _p(packed_w), _p(bias),
                                             _p(y), y_cs, _p(mean_rstd), _p(gamma), _p(beta), int(relu)),
          "conv2d_forward_head_norm")
    return y


def conv2d_batch(x, packed_w, bias, desc, y_cs=None, stats=None, out=None):
    """conv2d for a batch x: [B,H,W,x_cs] in ONE launch (direct algorithm) -> y [B,Hout,Wout,y_cs]; `stats` holds B
    consecutive per-image partial blocks (conv_stats_buffer(desc).numel() floats each).  Every image's result is
    conv2d's, bit for bit."""
    c = context()
    _chk(x, "x")
    B, x_cs = x.shape[0], x.shape[-1]
    ho, wo = conv_out_dims(desc)
    y_cs = round_up(desc.Cout, 4) if y_cs is None else y_cs
    y = out if out is not None else torch.empty(B, ho, wo, y_cs, dtype=torch.float32, device=x.device)
    if out is not None:
        _chk(out, "out")
    check(c.lib.t2v_conv2d_forward_batch(c.handle, _stream(), ctypes.byref(desc), B, _p(x), x_cs, _p(packed_w), _p(bias),
                                         _p(y), y_cs, _p(stats)), "conv2d_forward_batch")
    return y


def conv2d_auto_batch(x, packed_w, bias, desc, y_cs=None, stats=None, out=None):
    """conv2d_auto over a batch [B,...]: one launch for the direct algorithm, image by
    image for the Winograd forms (their batches go through the generator's own batched path).  stats: B consecutive blocks."""
    B = x.shape[0]
    if out is None:
        ho, wo = conv_out_dims(desc)
        out = torch.empty(B, ho, wo, round_up(desc.Cout, 4) if y_cs is None else y_cs, dtype=torch.float32, device=x.device)
    if desc.algo == ALGO_DIRECT and B > 1 and x.is_contiguous() and out.is_contiguous() and \
            (stats is None or stats.is_contiguous()):
        return conv2d_batch(x, packed_w, bias, desc, y_cs=y_cs, stats=stats, out=out)
    n = stats.numel() // B if stats is not None else 0
    for i in range(B):
        conv2d_auto(x[i], packed_w, bias, desc, y_cs=y_cs, stats=stats[i * n:(i + 1) * n] if stats is not None else None, out=out[i])
    return out


def norm_finalize_scratch(desc, device):
    """the scratch buffer instance_norm_finalize / batch_norm_finalize take as scratch= (t2v_norm_finalize_scratch_doubles)"""
    return torch.empty(_lib.load().t2v_norm_finalize_scratch_doubles(ctypes.byref(desc)), dtype=torch.float64, device=device)


def _finalize_scratch(c, desc, batch, stats, eps, mr, running, scratch):
    """t2v_batch_norm_finalize_scratch: a launch of >= 2048 partials pools them in groups through `scratch` (float64)"""
    if not (scratch.is_cuda and scratch.dtype == torch.float64 and scratch.is_contiguous()):
        raise ValueError("scratch must be a contiguous float64 device tensor")
    rm, rv, momentum, times = running if running is not None else (None, None, 0.0, 0)
    check(c.lib.t2v_batch_norm_finalize_scratch(c.handle, _stream(), ctypes.byref(desc), int(batch), _p(stats), eps, _p(mr), _p(rm),
                                                _p(rv), momentum, int(times), _p(scratch), scratch.numel()),
          "batch_norm_finalize_scratch")
    return mr


def instance_norm_finalize(stats, desc, eps=1e-5, out=None, running=None, scratch=None):
    """running = (running_mean, running_var, momentum, times): BatchNorm2d(train)'s running statistics (a batch of one) are
    moved `times` times by these statistics in the same launch (t2v_batch_norm_finalize_running).  scratch: a float64 device
    tensor of norm_finalize_scratch()'s size, see t2v_batch_norm_finalize_scratch."""
    c = context()
    mr = out if out is not None else torch.empty(desc.Cout, 2, dtype=torch.float32, device=stats.device)
    if scratch is not None:
        return _finalize_scratch(c, desc, 1, stats, eps, mr, running, scratch)
    if running is not None:
        rm, rv, momentum, times = running
        check(c.lib.t2v_batch_norm_finalize_running(c.handle, _stream(), ctypes.byref(desc), 1, _p(stats), eps, _p(mr), _p(rm), _p(rv),
                                                    momentum, int(times)), "batch_norm_finalize_running")
        return mr
    check(c.lib.t2v_instance_norm_finalize(c.handle, _stream(), ctypes.byref(desc), _p(stats), eps, _p(mr)),
          "instance_norm_finalize")
    return mr


def _numel(t, n, name):
    """the size contract of an elementwise entry, checked before the library sees a pointer"""
    if t is not None and t.numel() != n:
        raise ValueError("%s holds %d values, the call needs %d" % (name, t.numel(), n))


def instance_norm_apply(x, mean_rstd, gamma=None, beta=None, res1=None, res2=None, relu=False, out=None, nimg=None):
    """nimg: x, res1, res2 and the result are nimg images [nimg, ..., C] back to back, mean_rstd their nimg tables [nimg, C, 2]
    (t2v_instance_norm_apply_batch: one launch); gamma / beta are shared"""
    c = context()
    _chk(x, "x")
    C = x.shape[-1]
    if nimg is not None:
        nimg = int(nimg)
        if nimg < 1 or x.numel() % (nimg * C) != 0 or x.numel() == 0:
            raise ValueError("x does not hold nimg = %d images of C = %d channels" % (nimg, C))
        if C % 4 != 0:
            raise ValueError("C = %d must be a multiple of 4" % C)
        if (gamma is None) != (beta is None):
            raise ValueError("gamma and beta must both be given or both None")
        npix = x.numel() // (nimg * C)
        y = out if out is not None else torch.empty_like(x)
        for t, name in ((mean_rstd, "mean_rstd"), (gamma, "gamma"), (beta, "beta"), (res1, "res1"), (res2, "res2"), (y, "out")):
            if t is not None:
                _chk(t, name)
        _numel(mean_rstd, nimg * 2 * C, "mean_rstd")
        _numel(gamma, C, "gamma")
        _numel(beta, C, "beta")
        _numel(res1, x.numel(), "res1")
        _numel(res2, x.numel(), "res2")
        _numel(y, x.numel(), "out")
        check(c.lib.t2v_instance_norm_apply_batch(c.handle, _stream(), _p(x), _p(mean_rstd), _p(gamma), _p(beta), _p(res1),
                                                  _p(res2), _p(y), npix, C, int(relu), nimg), "instance_norm_apply_batch")
        return y
    npix = x.numel() // C
    y = out if out is not None else torch.empty_like(x)
    check(c.lib.t2v_instance_norm_apply(c.handle, _stream(), _p(x), _p(mean_rstd), _p(gamma), _p(beta), _p(res1),
                                        _p(res2), _p(y), npix, C, int(relu)), "instance_norm_apply")
    return y


def instance_norm_apply_bf16x2(x, mean_rstd, gamma=None, beta=None, relu=False, out=None):
    """instance_norm_apply with the split store (t2v_instance_norm_apply_bf16x2): the result holds, in the 8 bytes of every
    channel pair, the dwords {hi.x, hi.y | lo.x, lo.y} an ALGO_DIRECT_BF16X2 layer reads; out may be x."""
    c = context()
    _chk(x, "x")
    C = x.shape[-1]
    y = out if out is not None else torch.empty_like(x)
    check(c.lib.t2v_instance_norm_apply_bf16x2(c.handle, _stream(), _p(x), _p(mean_rstd), _p(gamma), _p(beta), _p(y),
                                               x.numel() // C, C, int(relu)), "instance_norm_apply_bf16x2")
    return y


def instance_norm_join(a, b, nimg=1, out=None):
    """The encoder join (t2v_instance_norm_join): (norm_a(a_y) + a_res) + (norm_b(b_y) + b_res) in one launch.  a, b: tuples
    (y, mean_rstd, gamma | None, beta | None, res); y and res [nimg, ..., C], mean_rstd [nimg, C, 2]."""
    c = context()
    ya = a[0]
    _chk(ya, "a.y")
    C = ya.shape[-1]
    nimg = int(nimg)
    if C % 4 != 0:
        raise ValueError("C = %d must be a multiple of 4" % C)
    if nimg < 1 or ya.numel() == 0 or ya.numel() % (nimg * C) != 0:
        raise ValueError("a.y does not hold nimg = %d images of C = %d channels" % (nimg, C))
    n = ya.numel()
    y = out if out is not None else torch.empty_like(ya)
    _chk(y, "out")
    _numel(y, n, "out")
    for side, tag in ((a, "a"), (b, "b")):
        sy, mr, ga, be, res = side
        if sy is None or mr is None or res is None:
            raise ValueError("%s: y, mean_rstd and res are required" % tag)
        if (ga is None) != (be is None):
            raise ValueError("%s: gamma and beta must both be given or both None" % tag)
        for t, name in ((sy, "y"), (mr, "mean_rstd"), (ga, "gamma"), (be, "beta"), (res, "res")):
            if t is not None:
                _chk(t, tag + "." + name)
        _numel(sy, n, tag + ".y")
        _numel(res, n, tag + ".res")
        _numel(mr, nimg * 2 * C, tag + ".mean_rstd")
        _numel(ga, C, tag + ".gamma")
        _numel(be, C, tag + ".beta")
    check(c.lib.t2v_instance_norm_join(c.handle, _stream(), _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), _p(a[4]), _p(b[0]),
                                       _p(b[1]), _p(b[2]), _p(b[3]), _p(b[4]), _p(y), n // (nimg * C), C, nimg),
          "instance_norm_join")
    return y


def add(a, b, out=None):
    """a + b (t2v_add); numel a multiple of 4"""
    c = context()
    _chk(a, "a")
    _chk(b, "b")
    n = a.numel()
    if n == 0 or n % 4 != 0:
        raise ValueError("n = %d must be a positive multiple of 4" % n)
    y = out if out is not None else torch.empty_like(a)
    _chk(y, "out")
    _numel(b, n, "b")
    _numel(y, n, "out")
    check(c.lib.t2v_add(c.handle, _stream(), _p(a), _p(b), _p(y), n), "add")
    return y


def conv_norm_act(x, packed_w, bias, desc, gamma=None, beta=None, relu=True, res1=None, res2=None, eps=1e-5):
    """[ReflPad,] Conv, InstanceNorm(+affine), [ReLU], [+res]: one conv launch + finalize + apply."""
    stats = conv_stats_buffer(desc, x.device)
    y = conv2d(x, packed_w, bias, desc, y_cs=desc.Cout, stats=stats)
    mr = instance_norm_finalize(stats, desc, eps)
    return instance_norm_apply(y, mr, gamma, beta, res1, res2, relu, out=y)


def flow_warp_composite(raw, fw, prev, prev_c0, want_warp=False, out=None):
    """raw,fw: [H,W,4]; prev: [H,W,prev_cs] (3 channels from prev_c0).  out = raw*w + warp*(1-w)."""
    c = context()
    H, W = raw.shape[0], raw.shape[1]
    out = torch.empty_like(raw) if out is None else out
    warp = torch.empty_like(raw) if want_warp else None
    check(c.lib.t2v_flow_warp_composite(c.handle, _stream(), _p(raw), _p(fw), _p(prev), prev.shape[-1], prev_c0,
                                        _p(out), _p(warp), H, W), "flow_warp_composite")
    return (out, warp) if want_warp else out


def flow_warp(fw, img, c0=0, out=None):
    """resample(img[..., c0:c0+3], flow): fw [H,W,4] (flow_x, flow_y in pixels; channel 2 ignored) -> [H,W,4]."""
    c = context()
    H, W = fw.shape[0], fw.shape[1]
    out = torch.empty(H, W, 4, dtype=torch.float32, device=fw.device) if out is None else out
    check(c.lib.t2v_flow_warp_composite(c.handle, _stream(), None, _p(fw), _p(img), img.shape[-1], c0, None, _p(out),
                                        H, W), "flow_warp")
    return out


def flow_warp_composite_backward(d_out, d_warp, raw, fw, prev, prev_c0, want_d_prev=False):
    """Adjoint of flow_warp_composite / flow_warp.  d_out, d_warp: [H,W,4] or None (not both); raw may be None when
    d_out is.  Returns (d_raw | None, d_fw [H,W,4] = (d flow_x, d flow_y, d weight, 0), d_prev | None)."""
    c = context()
    H, W = fw.shape[0], fw.shape[1]
    d_raw = torch.empty_like(fw) if d_out is not None else None
    d_fw = torch.empty_like(fw)
    d_prev = torch.zeros_like(prev) if want_d_prev else None
    check(c.lib.t2v_flow_warp_composite_backward(c.handle, _stream(), _p(d_out), _p(d_warp), _p(raw), _p(fw), _p(prev),
                                                 prev.shape[-1], prev_c0, _p(d_raw), _p(d_fw), _p(d_prev), H, W),
          "flow_warp_composite_backward")
    return d_raw, d_fw, d_prev


_flow_workspaces = {}      # (device, H, W, levels, refined) -> workspace of optical_flow
FLOW_ALPHA = 0.2           # the smoothness weight and the Jacobi steps per level the documents' figures were taken with
FLOW_REFINE_ITERS = 64
TEMPORAL_FLOWS = ("lk", "lkhs")


def optical_flow_workspace(H, W, levels=None, device=None, refined=False):
    """A workspace optical_flow accepts for this geometry (one call at a time may use it); refined: one that a call with
    refine_iters > 0 accepts as well (t2v_optical_flow_refined_workspace_floats)."""
    n = int((_flowlib.load().t2v_optical_flow_refined_workspace_floats if refined
             else _lib.load().t2v_optical_flow_workspace_floats)(H, W, int(levels or 0)))
    if n == 0:
        raise ValueError("optical_flow: unsupported size %d x %d or level count %r" % (H, W, levels))
    return torch.empty(n, dtype=torch.float32, device=device)


def _flow_workspace(c, name, like, H, W, levels, refined, workspace, strict):
    """the workspace a flow call hands the library: the caller's (checked), the cached one of the geometry, or -- for a shape
    the library refuses -- any pointer (it says so itself: nothing is launched, the pointer is not read)"""
    lv = int(levels or 0)
    need = (_flowlib.load().t2v_optical_flow_refined_workspace_floats if refined
            else c.lib.t2v_optical_flow_workspace_floats)(H, W, lv)
    if workspace is None:
        key = (like.device, H, W, lv, bool(refined))
        workspace = _flow_workspaces.get(key)
        if workspace is None and need:
            workspace = _flow_workspaces[key] = optical_flow_workspace(H, W, levels, like.device, refined)
    elif strict and not (workspace.is_cuda and workspace.dtype == torch.float32 and workspace.is_contiguous()):
        raise ValueError("%s: workspace must be a contiguous fp32 device tensor of the stated size" % name)
    elif workspace.numel() < need:
        raise ValueError("%s: workspace %s" % (name, "must be a contiguous fp32 device tensor of the stated size" if strict
                                               else "too small"))
    return like if workspace is None else workspace


def optical_flow(cur, prev, cur_c0=0, prev_c0=0, levels=None, iters=3, radius=3, lam=1e-3, out=None, workspace=None,
                 refine_iters=0, alpha=FLOW_ALPHA, iters_per_launch=0):
    """Dense optical flow from cur to prev (t2v_optical_flow: coarse-to-fine iterative Lucas-Kanade on the grey images):
    cur [H,W,cs], prev [H,W,cs'] NHWC, three channels from cur_c0 / prev_c0 -> [H,W,4] = (u, v, 0, 0) in pixels with
    cur(x, y) ~ prev(x + u, y + v), the flow flow_warp takes.  levels None: the default rule (include/t2v.h).  The
    workspace is cached per geometry when none is given (calls on one stream follow each other, so they may share it).
    refine_iters > 0: t2v_optical_flow_refined (libt2v_flow.so, include/t2v_flow_refine.h) -- every level's LK estimate goes through that many Horn-Schunck Jacobi
    steps with smoothness weight alpha, which fills textureless regions; iters_per_launch (0: the library's choice) never
    changes the result.  refine_iters = 0 (the default) is the LK entry itself."""
    c = context()
    _chk(cur, "cur")
    _chk(prev, "prev")
    H, W = cur.shape[0], cur.shape[1]
    if cur.dim() != 3 or prev.dim() != 3 or prev.shape[:2] != cur.shape[:2]:
        raise ValueError("optical_flow: cur and prev must be [H,W,C] of one size")
    lv = int(levels or 0)
    refined = int(refine_iters) != 0 or int(iters_per_launch) != 0 or float(alpha) != FLOW_ALPHA
    workspace = _flow_workspace(c, "optical_flow", cur, H, W, levels, int(refine_iters) > 0, workspace, False)
    out = torch.empty(H, W, 4, dtype=torch.float32, device=cur.device) if out is None else out
    if refined:
        check(_flowlib.load().t2v_optical_flow_refined(c.handle, _stream(), _p(cur), cur.shape[-1], cur_c0, _p(prev), prev.shape[-1],
                                             prev_c0, H, W, lv, int(iters), int(radius), float(lam), float(alpha),
                                             int(refine_iters), int(iters_per_launch), _p(workspace), _p(out)), "optical_flow")
    else:
        check(c.lib.t2v_optical_flow(c.handle, _stream(), _p(cur), cur.shape[-1], cur_c0, _p(prev), prev.shape[-1], prev_c0,
                                     H, W, lv, int(iters), int(radius), float(lam), _p(workspace), _p(out)), "optical_flow")
    return out


def optical_flow_u8(cur, prev, levels=None, iters=3, radius=3, lam=1e-3, out=None, workspace=None, refine_iters=0,
                    alpha=FLOW_ALPHA, iters_per_launch=0):
    """optical_flow on the delivered bytes (t2v_optical_flow_u8): cur, prev uint8 device images [H,W,3 or 4] (channels 0..2,
    the stride chosen per image) -> [H,W,4] = (u, v, 0, 0), bit for bit optical_flow on the fp32 images pose_u8_to_f32 makes
    of the same bytes.  Workspace, level rule, refinement arguments and refusals as optical_flow; the flows are finite."""
    c = context()
    for t, name in ((cur, "cur"), (prev, "prev")):
        if not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == 3):
            raise ValueError("optical_flow_u8: %s must be a contiguous uint8 device tensor [H,W,cs]" % name)
    H, W = cur.shape[0], cur.shape[1]
    if tuple(prev.shape[:2]) != (H, W):
        raise ValueError("optical_flow_u8: cur and prev must be [H,W,C] of one size")
    lv = int(levels or 0)
    refined = int(refine_iters) != 0 or int(iters_per_launch) != 0 or float(alpha) != FLOW_ALPHA
    workspace = _flow_workspace(c, "optical_flow_u8", cur, H, W, levels, int(refine_iters) > 0, workspace, True)
    out = torch.empty(H, W, 4, dtype=torch.float32, device=cur.device) if out is None else out
    _chk(out, "out")
    if tuple(out.shape) != (H, W, 4):
        raise ValueError("optical_flow_u8: out must be [H,W,4]")
    if refined:
        check(_flowlib.load().t2v_optical_flow_refined_u8(c.handle, _stream(), _p(cur), cur.shape[2], _p(prev), prev.shape[2], H, W, lv,
                                                int(iters), int(radius), float(lam), float(alpha), int(refine_iters),
                                                int(iters_per_launch), _p(workspace), _p(out)), "optical_flow_u8")
    else:
        check(c.lib.t2v_optical_flow_u8(c.handle, _stream(), _p(cur), cur.shape[2], _p(prev), prev.shape[2], H, W, lv, int(iters),
                                        int(radius), float(lam), _p(workspace), _p(out)), "optical_flow_u8")
    return out


def temporal_flow_kwargs(choice):
    """--temporal_flow {lk, lkhs} -> the refinement arguments of the optical_flow_u8 calls behind the temporal metrics"""
    if choice not in TEMPORAL_FLOWS:
        raise ValueError("temporal flow %r: one of %s" % (choice, ", ".join(TEMPORAL_FLOWS)))
    return dict(refine_iters=FLOW_REFINE_ITERS, alpha=FLOW_ALPHA) if choice == "lkhs" else {}


def avgpool3x3s2(x):
    """AvgPool2d(3, 2, 1, count_include_pad=False) on [H,W,C]."""
    c = context()
    _chk(x, "x")
    H, W, C = x.shape
    y = torch.empty((H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1, C, dtype=torch.float32, device=x.device)
    check(c.lib.t2v_avgpool3x3s2(c.handle, _stream(), _p(x), _p(y), H, W, C), "avgpool3x3s2")
    return y


def nchw_to_nhwc(x, cs=None, out=None):
    """[C,H,W] -> [H,W,cs] (extra channels zero)."""
    c = context()
    _chk(x, "x")
    C, H, W = x.shape
    cs = round_up(C, 4) if cs is None else cs
    y = out if out is not None else torch.empty(H, W, cs, dtype=torch.float32, device=x.device)
    check(c.lib.t2v_nchw_to_nhwc(c.handle, _stream(), _p(x), _p(y), C, H, W, cs), "nchw_to_nhwc")
    return y


def nhwc_to_nchw(x, C=None):
    """[H,W,cs] -> [C,H,W]."""
    c = context()
    _chk(x, "x")
    H, W, cs = x.shape
    C = cs if C is None else C
    y = torch.empty(C, H, W, dtype=torch.float32, device=x.device)
    check(c.lib.t2v_nhwc_to_nchw(c.handle, _stream(), _p(x), _p(y), C, H, W, cs), "nhwc_to_nchw")
    return y


def pose_u8_to_f32(src_u8, dst, c0):
    """uint8 [H,W,3] pose map -> channels [c0,c0+3) of dst [H,W,cs] as (v/255-0.5)/0.5."""
    c = context()
    H, W, _ = src_u8.shape
    check(c.lib.t2v_pose_u8_to_f32(c.handle, _stream(), _p(src_u8), _p(dst), H * W, dst.shape[-1], c0),
          "pose_u8_to_f32")
    return dst


def _bicubic(x):
    """Pillow's bicubic_filter (a = -0.5), evaluated in its operation order"""
    import numpy as np
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0,
                    np.where(x < 2.0, (((x - 5.0) * x + 8.0) * x - 4.0) * a, 0.0))


def pillow_bicubic_tables(in_size, out_size):
    """The tap table of Pillow's 8-bit BICUBIC resampler along one axis (precompute_coeffs + normalize_coeffs_8bpc of
    Resample.c, in float64): -> (first [out] int32, count [out] int32, coef [out, ksize] int32 scaled by 2^22, zero past
    count).  An axis that keeps its size gets the identity table (one tap of 2^22): Pillow skips that pass, and the
    bicubic coefficients at scale 1 are not the identity."""
    import numpy as np
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("pillow_bicubic_tables: sizes must be positive")
    if in_size == out_size:
        return (np.arange(out_size, dtype=np.int32), np.ones(out_size, np.int32),
                np.full((out_size, 1), 1 << 22, np.int32))
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(np.ceil(support)) * 2 + 1
    c = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    first = np.maximum(0, np.trunc(c - support + 0.5).astype(np.int64))
    end = np.minimum(in_size, np.trunc(c + support + 0.5).astype(np.int64))
    count = end - first
    j = np.arange(ksize, dtype=np.int64)[None, :]
    w = _bicubic((j + first[:, None] - c[:, None] + 0.5) * (1.0 / fs))
    w = np.where(j < count[:, None], w, 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]              # a left-to-right sum, as the C loop's (np.sum adds pairwise)
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    coef = np.trunc(np.where(w < 0, -0.5, 0.5) + w * float(1 << 22)).astype(np.int32)
    return first.astype(np.int32), count.astype(np.int32), np.ascontiguousarray(coef)


def pillow_bicubic_taps(in_size, out_size):
    """ksize of pillow_bicubic_tables(in_size, out_size): what t2v_resample_crop_normalize_u8's limit is stated in"""
    import math
    return 1 if in_size == out_size else 2 * math.ceil(2.0 * max(in_size / out_size, 1.0)) + 1


RESAMPLE_MAX_TAPS = _lib.RESAMPLE_MAX_TAPS      # T2V_RESAMPLE_MAX_TAPS (include/t2v.h)
_resample_tables = {}       # (device, in, out) -> (first, count, coef) on the device


def resample_tables_device(in_size, out_size, device):
    """pillow_bicubic_tables(in, out) as int32 device tensors, cached per (device, in, out)"""
    key = (str(device), int(in_size), int(out_size))
    t = _resample_tables.get(key)
    if t is None:
        if len(_resample_tables) > 256:            # random scales: a few dozen geometries per dataset
            _resample_tables.clear()
        t = _resample_tables[key] = tuple(torch.from_numpy(a).to(device) for a in pillow_bicubic_tables(in_size, out_size))
    return t


def resample_crop_normalize_u8(src_u8, new_size, crop_pos, crop_size, out=None, c0=0, x_tables=None, y_tables=None):
    """Image.resize(new_size, BICUBIC) of T uint8 frames [T,h,w,3] on the device, cropped to crop_size = (w, h) at
    crop_pos = (x, y) and normalised as (v/255-0.5)/0.5 into channels [c0, c0+3) of out [T,crop_h,crop_w,cs] (default: a
    new [..., 4] tensor whose pad channel is zero); the other channels of `out` keep their values.  One launch
    (t2v_resample_crop_normalize_u8), bit-equal to Pillow + crop + the torch expression.  x_tables / y_tables: (first,
    count, coef) int32 device tensors instead of Pillow's bicubic ones.  A geometry over the tap limit raises (status
    T2V_ERR_INVALID, nothing launched)."""
    c = context()
    if not (src_u8.is_cuda and src_u8.dtype == torch.uint8 and src_u8.is_contiguous() and src_u8.dim() == 4
            and src_u8.shape[-1] == 3):
        raise ValueError("src_u8 must be a contiguous uint8 device tensor [T,h,w,3]")
    T, h, w, _ = src_u8.shape
    (nw, nh), (cx, cy), (cw, ch) = new_size, crop_pos, crop_size
    xt = x_tables if x_tables is not None else resample_tables_device(w, nw, src_u8.device)
    yt = y_tables if y_tables is not None else resample_tables_device(h, nh, src_u8.device)
    if xt[0].numel() != nw or yt[0].numel() != nh:
        raise ValueError("resample_crop_normalize_u8: the tables do not cover new_size")
    if out is None:
        out = torch.zeros(T, ch, cw, 4, dtype=torch.float32, device=src_u8.device)
    _chk(out, "out")
    if tuple(out.shape[:3]) != (T, ch, cw):
        raise ValueError("resample_crop_normalize_u8: out must be [T,crop_h,crop_w,cs]")
    check(c.lib.t2v_resample_crop_normalize_u8(c.handle, _stream(), _p(src_u8), T, h, w, _p(xt[0]), _p(xt[1]), _p(xt[2]),
                                               xt[2].shape[1], nw, _p(yt[0]), _p(yt[1]), _p(yt[2]), yt[2].shape[1], nh,
                                               int(cx), int(cy), int(cw), int(ch), _p(out), out.shape[-1], int(c0)),
          "resample_crop_normalize_u8")
    return out


def tensor2im_u8(x, out=None):
    """util.tensor2im on the device: uint8 of (x+1)/2*255, same layout.  out: a contiguous uint8 device tensor of x's
    element count to write instead (e.g. one image of a batch for jpeg_encode_u8)."""
    c = context()
    _chk(x, "x")
    if out is None:
        out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    elif not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == x.numel()):
        raise ValueError("tensor2im_u8: out must be a contiguous uint8 device tensor of %d elements" % x.numel())
    check(c.lib.t2v_tensor2im_u8(c.handle, _stream(), _p(x), _p(out), x.numel()), "tensor2im_u8")
    return out


# ----------------------------------------------------------------------------------------------------------------------
# JPEG encoding (libt2v_jpeg.so, include/t2v_jpeg.h; the host part of the file: text2video_amd/jpeg.py)
# ----------------------------------------------------------------------------------------------------------------------
_jpeg_workspace = {}      # device -> uint8 workspace of t2v_jpeg_encode_u8 (grown on demand; uses are stream-ordered)


def _jpeg():
    from . import _jpeglib
    return _jpeglib


def jpeg_supported(H, W):
    """whether jpeg_encode_u8 takes H x W images (t2v_jpeg_supported)"""
    return bool(_jpeg().load().t2v_jpeg_supported(int(H), int(W)))


def jpeg_scan_capacity(H, W):
    """bytes no scan of an H x W image exceeds (t2v_jpeg_scan_capacity; 0: a geometry jpeg_encode_u8 refuses)"""
    return int(_jpeg().load().t2v_jpeg_scan_capacity(int(H), int(W)))


def jpeg_workspace_bytes(H, W, nimg):
    """bytes of workspace jpeg_encode_u8 needs for nimg H x W images (0: a call it refuses)"""
    return int(_jpeg().load().t2v_jpeg_workspace_bytes(int(H), int(W), int(nimg)))


def jpeg_stage_u8(src, dst, lut=None):
    """Copy the uint8 device image src [H,W,3|4] into dst [H,W,3|4] (another channel stride allowed), channels 0..2 through
    the 256-entry byte map `lut` (bytes / uint8 array on the host; None: unchanged); a fourth channel of dst is written
    as 0 (t2v_jpeg_stage_u8).  One launch; returns dst."""
    J = _jpeg()
    context()
    for t, name in ((src, "src"), (dst, "dst")):
        if not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == 3 and t.shape[2] in (3, 4)):
            raise ValueError("jpeg_stage_u8: %s must be a contiguous uint8 device tensor [H,W,3|4]" % name)
    if tuple(src.shape[:2]) != tuple(dst.shape[:2]):
        raise ValueError("jpeg_stage_u8: src is %dx%d, dst is %dx%d" % (src.shape[0], src.shape[1], dst.shape[0], dst.shape[1]))
    host_lut = None
    if lut is not None:
        lut = bytes(bytearray(lut))
        if len(lut) != 256:
            raise ValueError("jpeg_stage_u8: lut must hold 256 bytes")
        host_lut = ctypes.cast(ctypes.c_char_p(lut), ctypes.c_void_p)
    J.check(J.load().t2v_jpeg_stage_u8(_stream(), _p(src), src.shape[2], _p(dst), dst.shape[2], src.shape[0] * src.shape[1],
                                       host_lut), "stage_u8")
    return dst


def jpeg_encode_u8(images, quality=75, out=None, lengths=None, workspace=None):
    """The entropy-coded JPEG scans of uint8 device images (t2v_jpeg_encode_u8, include/t2v_jpeg.h): images is a contiguous
    uint8 device tensor [N,H,W,3|4] or [H,W,3|4] (R, G, B in channels 0..2), quality the IJG quality 1..100.
    -> (out, lengths): out a uint8 device tensor [N, capacity] whose row i starts with image i's scan, lengths an int32
    device tensor [N] of the scans' byte lengths.  jpeg.file_bytes(jpeg.header(H, W, quality), scan) is the file Pillow's
    Image.save(format="JPEG", quality=quality) writes.
    out: that tensor to write instead, any capacity >= 1 per row: a scan longer than the row is reported through
    lengths[i] > capacity, its first `capacity` bytes are valid and nothing behind them is written (default: rows of
    jpeg_scan_capacity(H, W) bytes, which every scan fits).  lengths: an int32 device tensor [N] to write instead.
    workspace: a uint8 device tensor of at least jpeg_workspace_bytes(H, W, N) bytes, 256-byte aligned (default: one kept
    per device).  One memset and seven launches on the current stream, no host synchronisation; an unsupported geometry
    (jpeg_supported) or an argument that does not fit raises with nothing launched."""
    J = _jpeg()
    context()
    if not (images.is_cuda and images.dtype == torch.uint8 and images.is_contiguous() and images.dim() in (3, 4)
            and images.shape[-1] in (3, 4)):
        raise ValueError("jpeg_encode_u8: images must be a contiguous uint8 device tensor [N,H,W,3|4] or [H,W,3|4]")
    N = images.shape[0] if images.dim() == 4 else 1
    H, W, cs = (int(v) for v in images.shape[-3:])
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError("jpeg_encode_u8: quality %d is not in 1..100" % quality)
    if not jpeg_supported(H, W):
        raise ValueError("jpeg_encode_u8: %dx%d is outside %d..%d per dimension" % (H, W, J.MIN_DIM, J.MAX_DIM))
    if not 1 <= N <= J.MAX_IMAGES:
        raise ValueError("jpeg_encode_u8: %d images (1..%d per call)" % (N, J.MAX_IMAGES))
    dev = images.device
    if out is None:
        out = torch.empty(N, jpeg_scan_capacity(H, W), dtype=torch.uint8, device=dev)
    if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.dim() == 2 and out.shape[0] == N
            and out.shape[1] >= 1):
        raise ValueError("jpeg_encode_u8: out must be a contiguous uint8 device tensor [%d, capacity]" % N)
    if lengths is None:
        lengths = torch.empty(N, dtype=torch.int32, device=dev)
    if not (lengths.is_cuda and lengths.dtype == torch.int32 and lengths.is_contiguous() and lengths.numel() == N):
        raise ValueError("jpeg_encode_u8: lengths must be a contiguous int32 device tensor [%d]" % N)
    need = jpeg_workspace_bytes(H, W, N)
    if workspace is None:
        workspace = _jpeg_workspace.get(str(dev))
        if workspace is None or workspace.numel() < need:
            workspace = _jpeg_workspace[str(dev)] = torch.empty(need, dtype=torch.uint8, device=dev)
    elif not (workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.is_contiguous()):
        raise ValueError("jpeg_encode_u8: workspace must be a contiguous uint8 device tensor")
    if workspace.numel() < need or workspace.data_ptr() % 256:
        raise ValueError("jpeg_encode_u8: workspace holds %d bytes at an address that is %d mod 256; %d images of %dx%d need "
                         "%d aligned bytes" % (workspace.numel(), workspace.data_ptr() % 256, N, H, W, need))
    J.check(J.load().t2v_jpeg_encode_u8(_stream(), _p(images), cs, H, W, N, quality, _p(workspace), _p(out), out.shape[1],
                                        _p(lengths)), "encode_u8")
    return out, lengths


# ----------------------------------------------------------------------------------------------------------------------
# PNG encoding (libt2v_png.so, include/t2v_png.h): complete files, nothing is added on the host
# ----------------------------------------------------------------------------------------------------------------------
_png_workspace = {}      # device -> uint8 workspace of t2v_png_encode_u8 (grown on demand; uses are stream-ordered)


def _png():
    from . import _pnglib
    return _pnglib


def png_supported(H, W):
    """whether png_encode_u8 takes H x W images (t2v_png_supported)"""
    return bool(_png().load().t2v_png_supported(int(H), int(W)))


def png_file_capacity(H, W):
    """bytes no file of an H x W image exceeds (t2v_png_file_capacity; 0: a geometry png_encode_u8 refuses)"""
    return int(_png().load().t2v_png_file_capacity(int(H), int(W)))


def png_workspace_bytes(H, W, nimg):
    """bytes of workspace png_encode_u8 needs for nimg H x W images (0: a call it refuses)"""
    return int(_png().load().t2v_png_workspace_bytes(int(H), int(W), int(nimg)))


def png_encode_u8(images, out=None, lengths=None, workspace=None):
    """Lossless PNG files of uint8 device images (t2v_png_encode_u8, include/t2v_png.h): images is a contiguous uint8
    device tensor [N,H,W,3|4] or [H,W,3|4] (R, G, B in channels 0..2; a fourth channel is ignored).
    -> (out, lengths): out a uint8 device tensor [N, capacity] whose row i starts with image i's complete file (signature
    ... IEND), lengths an int32 device tensor [N] of the files' byte lengths.
    out: that tensor to write instead, any capacity >= 1 per row: a file longer than the row is reported through
    lengths[i] > capacity, its first `capacity` bytes are valid and nothing behind them is written (default: rows of
    png_file_capacity(H, W) bytes, which every file fits).  lengths: an int32 device tensor [N] to write instead.
    workspace: a uint8 device tensor of at least png_workspace_bytes(H, W, N) bytes, 256-byte aligned (default: one kept
    per device).  One memset and seven launches on the current stream, no host synchronisation; an unsupported geometry
    (png_supported) or an argument that does not fit raises with nothing launched."""
    P = _png()
    context()
    if not (images.is_cuda and images.dtype == torch.uint8 and images.is_contiguous() and images.dim() in (3, 4)
            and images.shape[-1] in (3, 4)):
        raise ValueError("png_encode_u8: images must be a contiguous uint8 device tensor [N,H,W,3|4] or [H,W,3|4]")
    N = images.shape[0] if images.dim() == 4 else 1
    H, W, cs = (int(v) for v in images.shape[-3:])
    if not png_supported(H, W):
        raise ValueError("png_encode_u8: %dx%d is outside %d..%d per dimension" % (H, W, P.MIN_DIM, P.MAX_DIM))
    if not 1 <= N <= P.MAX_IMAGES:
        raise ValueError("png_encode_u8: %d images (1..%d per call)" % (N, P.MAX_IMAGES))
    dev = images.device
    if out is None:
        out = torch.empty(N, png_file_capacity(H, W), dtype=torch.uint8, device=dev)
    if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.dim() == 2 and out.shape[0] == N
            and out.shape[1] >= 1):
        raise ValueError("png_encode_u8: out must be a contiguous uint8 device tensor [%d, capacity]" % N)
    if lengths is None:
        lengths = torch.empty(N, dtype=torch.int32, device=dev)
    if not (lengths.is_cuda and lengths.dtype == torch.int32 and lengths.is_contiguous() and lengths.numel() == N):
        raise ValueError("png_encode_u8: lengths must be a contiguous int32 device tensor [%d]" % N)
    need = png_workspace_bytes(H, W, N)
    if workspace is None:
        workspace = _png_workspace.get(str(dev))
        if workspace is None or workspace.numel() < need:
            workspace = _png_workspace[str(dev)] = torch.empty(need, dtype=torch.uint8, device=dev)
    elif not (workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.is_contiguous()):
        raise ValueError("png_encode_u8: workspace must be a contiguous uint8 device tensor")
    if workspace.numel() < need or workspace.data_ptr() % 256:
        raise ValueError("png_encode_u8: workspace holds %d bytes at an address that is %d mod 256; %d images of %dx%d need "
                         "%d aligned bytes" % (workspace.numel(), workspace.data_ptr() % 256, N, H, W, need))
    P.check(P.load().t2v_png_encode_u8(_stream(), _p(images), cs, H, W, N, _p(workspace), _p(out), out.shape[1], _p(lengths)),
            "encode_u8")
    return out, lengths


# ----------------------------------------------------------------------------------------------------------------------
# JPEG decoding (libt2v_jpegdec.so, include/t2v_jpeg_decode.h; the host part: text2video_amd/jpeg.py parse())
# ----------------------------------------------------------------------------------------------------------------------
_jpegdec_workspace = {}      # device -> uint8 workspace of t2v_jpegdec_decode_u8 (grown on demand; uses are stream-ordered)


def _jpegdec():
    from . import _jpegdeclib
    return _jpegdeclib


def jpeg_decode_supported(H, W, sampling):
    """whether jpeg_decode_u8 takes H x W images of this sampling (t2v_jpegdec_supported)"""
    return bool(_jpegdec().load().t2v_jpegdec_supported(int(H), int(W), int(sampling)))


def jpeg_decode_workspace_bytes(H, W, sampling, nimg, scan_capacity):
    """bytes of workspace jpeg_decode_u8 needs (0: a call it refuses)"""
    return int(_jpegdec().load().t2v_jpegdec_workspace_bytes(int(H), int(W), int(sampling), int(nimg), int(scan_capacity)))


def jpeg_decode_u8(scans, scan_capacity, lengths, tables, H, W, sampling, nimg, dst=None, dst_cs=3, status=None, workspace=None):
    """Decode nimg JPEG scans of one geometry on the current stream (t2v_jpegdec_decode_u8, include/t2v_jpeg_decode.h).
    scans, lengths, tables: contiguous device tensors of nimg * scan_capacity, nimg * 4 and nimg * jpeg.TABLE_BYTES bytes
    (any dtype: byte views of one uploaded buffer are fine): the entropy-coded bytes of every file, their uint32 lengths and
    the table blobs jpeg.parse() made; sampling is Pillow's `subsampling` number.
    -> (dst, status): dst a uint8 device tensor [nimg,H,W,dst_cs] (channel 3, if any, 0) holding what Pillow's
    Image.open(...).convert("RGB") gives, status an int32 device tensor [nimg]: 0, or bits _jpegdeclib.NOT_CONVERGED /
    CORRUPT for an image whose dst slot is then unspecified.  One memset and eight launches, no host synchronisation; an
    unsupported geometry or an argument that does not fit raises with nothing launched."""
    D = _jpegdec()
    context()
    H, W, sampling, nimg, cap, dst_cs = int(H), int(W), int(sampling), int(nimg), int(scan_capacity), int(dst_cs)
    if not jpeg_decode_supported(H, W, sampling):
        raise ValueError("jpeg_decode_u8: %dx%d, sampling %d is outside %d..%d per dimension, sampling 0..2"
                         % (H, W, sampling, D.MIN_DIM, D.MAX_DIM))
    if not 1 <= nimg <= D.MAX_IMAGES:
        raise ValueError("jpeg_decode_u8: %d images (1..%d per call)" % (nimg, D.MAX_IMAGES))
    if dst_cs not in (3, 4):
        raise ValueError("jpeg_decode_u8: dst_cs %d (3 or 4)" % dst_cs)

    def size(t):      # (torch: a property; leantorch: a method)
        n = t.nbytes
        return n() if callable(n) else n
    for t, name, need in ((scans, "scans", nimg * cap), (lengths, "lengths", nimg * 4), (tables, "tables", nimg * D.load().t2v_jpegdec_table_bytes())):
        if not (t.is_cuda and t.is_contiguous() and size(t) == need):
            raise ValueError("jpeg_decode_u8: %s must be a contiguous device tensor of %d bytes" % (name, need))
    dev = scans.device
    if dst is None:
        dst = torch.empty(nimg, H, W, dst_cs, dtype=torch.uint8, device=dev)
    if not (dst.is_cuda and dst.dtype == torch.uint8 and dst.is_contiguous() and tuple(dst.shape) == (nimg, H, W, dst_cs)):
        raise ValueError("jpeg_decode_u8: dst must be a contiguous uint8 device tensor [%d,%d,%d,%d]" % (nimg, H, W, dst_cs))
    if status is None:
        status = torch.empty(nimg, dtype=torch.int32, device=dev)
    if not (status.is_cuda and status.dtype == torch.int32 and status.is_contiguous() and status.numel() == nimg):
        raise ValueError("jpeg_decode_u8: status must be a contiguous int32 device tensor [%d]" % nimg)
    need = jpeg_decode_workspace_bytes(H, W, sampling, nimg, cap)
    if need == 0:
        raise ValueError("jpeg_decode_u8: scan_capacity %d (a multiple of 16, 16..2^28)" % cap)
    if workspace is None:
        workspace = _jpegdec_workspace.get(str(dev))
        if workspace is None or workspace.numel() < need:
            workspace = _jpegdec_workspace[str(dev)] = torch.empty(need, dtype=torch.uint8, device=dev)
    elif not (workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.is_contiguous()):
        raise ValueError("jpeg_decode_u8: workspace must be a contiguous uint8 device tensor")
    if workspace.numel() < need or workspace.data_ptr() % 256:
        raise ValueError("jpeg_decode_u8: workspace holds %d bytes at an address that is %d mod 256; %d images of %dx%d need "
                         "%d aligned bytes" % (workspace.numel(), workspace.data_ptr() % 256, nimg, H, W, need))
    D.check(D.load().t2v_jpegdec_decode_u8(_stream(), _p(scans), cap, _p(lengths), _p(tables), H, W, sampling, nimg, _p(workspace),
                                           _p(dst), dst_cs, _p(status)), "decode_u8")
    return dst, status


_side_streams = {}      # device -> a stream of the library's own beside the current one (created on first use)


def side_stream():
    """A second stream on the current device (t2v_stream_create: non-blocking), for a copy that must not queue behind the
    work the current stream already holds.  The caller orders it against that work itself (an event it has waited for)."""
    c = context()
    h = _side_streams.get(c.device)
    if h is None:
        p = ctypes.c_void_p()
        check(c.lib.t2v_stream_create(c.handle, ctypes.byref(p)), "stream_create")
        h = _side_streams[c.device] = p.value
    return h


def stream_synchronize(stream):
    """wait on the host for a stream side_stream() returned"""
    c = context()
    check(c.lib.t2v_stream_synchronize(c.handle, ctypes.c_void_p(stream)), "stream_synchronize")


def copy_bytes_to_host(dst_pinned, dst_offset, src, src_offset, nbytes, stream=None):
    """Asynchronous D2H copy of nbytes bytes on the current stream (or on `stream`, a side_stream()): from byte src_offset of
    the device tensor src to byte dst_offset of the page-locked host tensor dst_pinned (both contiguous).  Parts of tensors,
    which neither tensor provider's copy_ does without building views."""
    c = context()

    def size(t):      # (torch: a property; leantorch: a method)
        n = t.nbytes
        return n() if callable(n) else n
    if not (0 <= src_offset and 0 <= dst_offset and 0 <= nbytes and src_offset + nbytes <= size(src)
            and dst_offset + nbytes <= size(dst_pinned)):
        raise ValueError("copy_bytes_to_host: %d bytes from offset %d to offset %d do not fit" % (nbytes, src_offset, dst_offset))
    if nbytes:
        check(c.lib.t2v_memcpy(c.handle, _stream() if stream is None else ctypes.c_void_p(stream),
                               ctypes.c_void_p(dst_pinned.data_ptr() + dst_offset),
                               ctypes.c_void_p(src.data_ptr() + src_offset), nbytes, _lib.COPY_D2H), "memcpy d2h")


METRICS_MAX_BOXES, METRICS_MAX_SIDE = _lib.METRICS_MAX_BOXES, _lib.METRICS_MAX_SIDE      # the library's limits (include/t2v.h)
_metrics_scratch = {}      # device -> float64 scratch of t2v_image_metrics_u8 (grown on demand; uses are stream-ordered)
METRICS_DEFINITION = ("psnr = 10 log10(255^2 / mse) and mae over the pixels' 3 channels; ssim = mean SSIM index (Wang et al. "
                      "2004: 11x11 Gaussian window, sigma 1.5, K1 0.01, K2 0.03, L 255, per channel on the 8-bit values, "
                      "float64) over the window positions wholly inside the region")


def image_metrics_scratch_doubles(H, W, nbox=0):
    """doubles of scratch t2v_image_metrics_u8 needs for an H x W pair with nbox boxes (0: a shape the call refuses)"""
    return int(_lib.load().t2v_image_metrics_scratch_doubles(int(H), int(W), int(nbox)))


def image_metrics(a, b, boxes=(), out=None, out_row=0, scratch=None):
    """The sums PSNR / MAE / SSIM are formed from (t2v_image_metrics_u8, include/t2v.h), of two uint8 device images
    [H,W,3 or 4] (channels 0..2 compared) over the whole frame (row 0) and over boxes = [(y0, y1, x0, x1), ...] (half-open,
    at most 3; rows 1..): a float64 device tensor [1+nbox, 4] of rows {sse, sad, ssim_sum, ssim_n} -- see metrics_summary.
    out: a float64 device tensor [R, 4] to write rows [out_row, out_row + 1 + nbox) of instead (its other rows keep their
    values; returned as it is).  scratch: a float64 device tensor of at least image_metrics_scratch_doubles(H, W, nbox)
    elements (default: one kept per device).  Two launches, no host synchronisation; a refused call (status
    T2V_ERR_INVALID) or a scratch / out that is too small raises with nothing launched."""
    c = context()
    for t, name in ((a, "a"), (b, "b")):
        if not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == 3):
            raise ValueError("image_metrics: %s must be a contiguous uint8 device tensor [H,W,cs]" % name)
    H, W = a.shape[0], a.shape[1]
    if tuple(b.shape[:2]) != (H, W):
        raise ValueError("image_metrics: a is %dx%d, b is %dx%d" % (H, W, b.shape[0], b.shape[1]))
    boxes = [tuple(int(v) for v in bx) for bx in boxes]
    if any(len(bx) != 4 for bx in boxes):
        raise ValueError("image_metrics: a box is (y0, y1, x0, x1)")
    nbox = len(boxes)
    if out is None:
        out, out_row = torch.empty(1 + nbox, 4, dtype=torch.float64, device=a.device), 0
    if not (out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.dim() == 2 and out.shape[1] == 4
            and 0 <= out_row and out_row + 1 + nbox <= out.shape[0]):
        raise ValueError("image_metrics: out must be a contiguous float64 device tensor [R,4] with rows [%d, %d)"
                         % (out_row, out_row + 1 + nbox))
    need = image_metrics_scratch_doubles(H, W, nbox)
    if scratch is None:
        scratch = _metrics_scratch.get(str(a.device))
        if need and (scratch is None or scratch.numel() < need):
            scratch = _metrics_scratch[str(a.device)] = torch.empty(max(need, 4096), dtype=torch.float64, device=a.device)
    elif not (scratch.is_cuda and scratch.dtype == torch.float64 and scratch.is_contiguous()):
        raise ValueError("image_metrics: scratch must be a contiguous float64 device tensor")
    if need and scratch.numel() < need:
        raise ValueError("image_metrics: scratch holds %d doubles, %dx%d with %d boxes needs %d" % (scratch.numel(), H, W, nbox, need))
    host_boxes = (ctypes.c_int32 * (4 * nbox))(*[v for bx in boxes for v in bx]) if nbox else None
    check(c.lib.t2v_image_metrics_u8(c.handle, _stream(), _p(a), a.shape[2], _p(b), b.shape[2], H, W, host_boxes, nbox,
                                     _p(scratch), ctypes.c_void_p(out.data_ptr() + out_row * 32)), "image_metrics_u8")
    return out


def metrics_summary(row, n_values):
    """Host helper: one row {sse, sad, ssim_sum, ssim_n} of image_metrics over n_values compared values (pixels x 3)
    -> {"mse", "mae", "psnr", "ssim"}; psnr = 10 log10(255^2 / mse), None for identical regions (sse == 0);
    ssim = ssim_sum / ssim_n, None for a region narrower than the 11x11 window (ssim_n == 0)."""
    import math
    sse, sad, ssim_sum, ssim_n = (float(v) for v in row)
    mse = sse / n_values
    return {"mse": mse, "mae": sad / n_values, "psnr": None if sse == 0 else 10.0 * math.log10(255.0 * 255.0 / mse),
            "ssim": None if ssim_n == 0 else ssim_sum / ssim_n}


TEMPORAL_DEFINITION = ("warp_mse = mean squared error (8-bit units) between frame t and frame t-1 warped by the REAL pair's flow, "
                       "over pixels passing the forward-backward check |f+b|^2 <= 0.01(|f|^2+|b|^2)+0.5 (valid = their share); "
                       "warp_mse_real = the same on the real pair (the floor); tof = mean endpoint error in px between the "
                       "generated pair's flow and the real pair's; tdiff_mse = mean ((a_t - a_t-1) - (b_t - b_t-1))^2; flows: "
                       "ops.optical_flow_u8 (coarse-to-fine Lucas-Kanade), float64 sums")


def temporal_definition(flow="lk"):
    """TEMPORAL_DEFINITION with the flow estimator of the choice named (lk: the text as it is)"""
    if flow == "lk":
        return TEMPORAL_DEFINITION
    temporal_flow_kwargs(flow)
    return TEMPORAL_DEFINITION.replace("(coarse-to-fine Lucas-Kanade)", "with refine_iters=%d, alpha=%g (coarse-to-fine Lucas-Kanade "
                                       "refined by Horn-Schunck steps at every level: --temporal_flow lkhs)"
                                       % (FLOW_REFINE_ITERS, FLOW_ALPHA))


TEMPORAL_COLUMNS = 6       # n_valid, warp_sse_a, warp_sse_b, n_flow, epe_sum, tdiff_sse


def temporal_metrics_scratch_doubles(H, W, nbox=0):
    """doubles of scratch t2v_temporal_metrics_u8 needs for H x W frames with nbox boxes (0: a shape the call refuses)"""
    return int(_lib.load().t2v_temporal_metrics_scratch_doubles(int(H), int(W), int(nbox)))


def temporal_metrics(a_cur, a_prev, b_cur, b_prev, flow_fwd, flow_bwd, flow_a=None, boxes=(), out=None, out_row=0, scratch=None):
    """The sums the temporal-consistency figures are formed from (t2v_temporal_metrics_u8, include/t2v.h): a_cur, a_prev
    (generated, frames t and t-1) and b_cur, b_prev (real) are uint8 device images [H,W,3 or 4]; flow_fwd = the flow from
    b_cur to b_prev, flow_bwd = from b_prev to b_cur, flow_a = from a_cur to a_prev or None, fp32 [H,W,4] as optical_flow
    writes them.  -> a float64 device tensor [1+nbox, 6] of rows {n_valid, warp_sse_a, warp_sse_b, n_flow, epe_sum,
    tdiff_sse} over the whole frame (row 0) and boxes = [(y0, y1, x0, x1), ...] (at most 3) -- see temporal_summary.
    out / out_row / scratch: as image_metrics (rows of 6; temporal_metrics_scratch_doubles).  Two launches, no host
    synchronisation; a refused call or a scratch / out that is too small raises with nothing launched."""
    c = context()
    H, W = a_cur.shape[0], a_cur.shape[1]
    for t, name in ((a_cur, "a_cur"), (a_prev, "a_prev"), (b_cur, "b_cur"), (b_prev, "b_prev")):
        if not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == 3):
            raise ValueError("temporal_metrics: %s must be a contiguous uint8 device tensor [H,W,cs]" % name)
        if tuple(t.shape[:2]) != (H, W):
            raise ValueError("temporal_metrics: a_cur is %dx%d, %s is %dx%d" % (H, W, name, t.shape[0], t.shape[1]))
    for t, name in ((flow_fwd, "flow_fwd"), (flow_bwd, "flow_bwd"), (flow_a, "flow_a")):
        if t is None and name == "flow_a":
            continue
        if t is None or not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (H, W, 4)):
            raise ValueError("temporal_metrics: %s must be a contiguous fp32 device tensor [%d,%d,4]" % (name, H, W))
    boxes = [tuple(int(v) for v in bx) for bx in boxes]
    if any(len(bx) != 4 for bx in boxes):
        raise ValueError("temporal_metrics: a box is (y0, y1, x0, x1)")
    nbox = len(boxes)
    if out is None:
        out, out_row = torch.empty(1 + nbox, TEMPORAL_COLUMNS, dtype=torch.float64, device=a_cur.device), 0
    if not (out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.dim() == 2
            and out.shape[1] == TEMPORAL_COLUMNS and 0 <= out_row and out_row + 1 + nbox <= out.shape[0]):
        raise ValueError("temporal_metrics: out must be a contiguous float64 device tensor [R,6] with rows [%d, %d)"
                         % (out_row, out_row + 1 + nbox))
    need = temporal_metrics_scratch_doubles(H, W, nbox)
    if scratch is None:
        scratch = _metrics_scratch.get(str(a_cur.device))
        if need and (scratch is None or scratch.numel() < need):
            scratch = _metrics_scratch[str(a_cur.device)] = torch.empty(max(need, 4096), dtype=torch.float64, device=a_cur.device)
    elif not (scratch.is_cuda and scratch.dtype == torch.float64 and scratch.is_contiguous()):
        raise ValueError("temporal_metrics: scratch must be a contiguous float64 device tensor")
    if need and scratch.numel() < need:
        raise ValueError("temporal_metrics: scratch holds %d doubles, %dx%d with %d boxes needs %d"
                         % (scratch.numel(), H, W, nbox, need))
    host_boxes = (ctypes.c_int32 * (4 * nbox))(*[v for bx in boxes for v in bx]) if nbox else None
    check(c.lib.t2v_temporal_metrics_u8(c.handle, _stream(), _p(a_cur), a_cur.shape[2], _p(a_prev), a_prev.shape[2], _p(b_cur),
                                        b_cur.shape[2], _p(b_prev), b_prev.shape[2], _p(flow_fwd), _p(flow_bwd), _p(flow_a), H, W,
                                        host_boxes, nbox, _p(scratch),
                                        ctypes.c_void_p(out.data_ptr() + out_row * 8 * TEMPORAL_COLUMNS)), "temporal_metrics_u8")
    return out


def temporal_summary(row, n_pixels):
    """Host helper: one row {n_valid, warp_sse_a, warp_sse_b, n_flow, epe_sum, tdiff_sse} of temporal_metrics over a region of
    n_pixels pixels -> {"warp_mse": warp_sse_a / (3 n_valid), "warp_mse_real": warp_sse_b / (3 n_valid), "valid": n_valid /
    n_pixels, "tof": epe_sum / n_flow (px), "tdiff_mse": tdiff_sse / (3 n_pixels)}, in 8-bit units squared; None wherever a
    denominator is 0."""
    n_valid, sse_a, sse_b, n_flow, epe, tdiff = (float(v) for v in row)
    return {"warp_mse": sse_a / (3.0 * n_valid) if n_valid else None,
            "warp_mse_real": sse_b / (3.0 * n_valid) if n_valid else None,
            "valid": n_valid / n_pixels if n_pixels else None,
            "tof": epe / n_flow if n_flow else None,
            "tdiff_mse": tdiff / (3.0 * n_pixels) if n_pixels else None}


_VISUALS_CHANNELS = {VISUALS_IMAGE: 3, VISUALS_UNIT: 1, VISUALS_FLOW: 2}


def train_visuals_scratch_doubles(H, W, npanels):
    """doubles of scratch t2v_train_visuals_u8 needs for npanels panels of H x W (0: a shape the call refuses)"""
    return int(_lib.load().t2v_train_visuals_scratch_doubles(int(H), int(W), int(npanels)))


def train_visuals(panels, scale=1, out=None, scratch=None):
    """The pictures of one training frame (t2v_train_visuals_u8, include/t2v.h): panels = [(kind, tensor [H,W,cs], c0), ...],
    at most 8, every tensor a contiguous fp32 device tensor of the same H x W (a [H,W] tensor counts as cs 1), read from
    channel c0 on; kind = VISUALS_IMAGE (3 channels: tensor2im_u8's bytes), VISUALS_UNIT (1 channel in [0,1] as grey) or
    VISUALS_FLOW (2 channels u, v in pixels: hue = direction, brightness = the panel's min-max-normalised magnitude).
    -> a uint8 device tensor [n, H/scale, W/scale, 3]; scale in (1, 2, 4) averages scale x scale blocks of bytes.
    out: that tensor to write instead; scratch: a float64 device tensor of at least train_visuals_scratch_doubles(H, W, n)
    elements (default: one kept per device).  Two launches on the current stream, no host synchronisation; a refused call
    (status T2V_ERR_INVALID) or a scratch / out that does not fit raises with nothing launched."""
    c = context()
    panels = [(int(kind), t, int(c0)) for kind, t, c0 in panels]
    n = len(panels)
    if n == 0:
        raise ValueError("train_visuals: no panel")
    for i, (kind, t, c0) in enumerate(panels):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() in (2, 3)):
            raise ValueError("train_visuals: panel %d must be a contiguous fp32 device tensor [H,W,cs]" % i)
        if kind not in _VISUALS_CHANNELS:
            raise ValueError("train_visuals: panel %d has the unknown kind %d" % (i, kind))
    H, W = panels[0][1].shape[0], panels[0][1].shape[1]
    for i, (kind, t, c0) in enumerate(panels):
        if tuple(t.shape[:2]) != (H, W):
            raise ValueError("train_visuals: panel 0 is %dx%d, panel %d is %dx%d" % (H, W, i, t.shape[0], t.shape[1]))
    scale = int(scale)
    dev = panels[0][1].device
    if out is None:
        if scale not in (1, 2, 4) or H % scale or W % scale:
            raise ValueError("train_visuals: scale must be 1, 2 or 4 and divide %dx%d (got %d)" % (H, W, scale))
        out = torch.empty(n, H // scale, W // scale, 3, dtype=torch.uint8, device=dev)
    if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
                                and out.numel() >= n * (H // max(1, scale)) * (W // max(1, scale)) * 3):
        raise ValueError("train_visuals: out must be a contiguous uint8 device tensor [%d,H/scale,W/scale,3]" % n)
    need = train_visuals_scratch_doubles(H, W, n)
    if scratch is None:
        scratch = _metrics_scratch.get(str(dev))
        if scratch is None or scratch.numel() < need:
            scratch = _metrics_scratch[str(dev)] = torch.empty(max(need, 4096), dtype=torch.float64, device=dev)
    elif not (scratch.is_cuda and scratch.dtype == torch.float64 and scratch.is_contiguous()):
        raise ValueError("train_visuals: scratch must be a contiguous float64 device tensor")
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for _, t, _ in panels])
    ints = (ctypes.c_int32 * (3 * n))(*[v for kind, t, c0 in panels for v in (kind, c0, t.shape[2] if t.dim() == 3 else 1)])
    # (too many panels, a bad scale, channels outside the stride, a scratch that is too small: the library refuses)
    check(c.lib.t2v_train_visuals_u8(c.handle, _stream(), ptrs, ints, n, H, W, scale, _p(scratch), scratch.numel(), _p(out)),
          "train_visuals_u8")
    return out


def copy_channels(src, src_c0, dst, dst_c0, nc):
    c = context()
    npix = src.numel() // src.shape[-1]
    check(c.lib.t2v_copy_channels(c.handle, _stream(), _p(src), src.shape[-1], src_c0, _p(dst), dst.shape[-1],
                                  dst_c0, nc, npix), "copy_channels")
    return dst


# ------------------------------------------------------------------------------------------------
# train-step pieces
# ------------------------------------------------------------------------------------------------
def batch_norm_finalize(stats, desc, batch, eps=1e-5, running=None, scratch=None):
    """BatchNorm2d(train) statistics over a batch: `stats` holds `batch` consecutive per-image
    partial blocks written by conv2d(..., stats=stats[b * n : (b + 1) * n]).  running, scratch: as instance_norm_finalize."""
    c = context()
    mr = torch.empty(desc.Cout, 2, dtype=torch.float32, device=stats.device)
    if scratch is not None:
        return _finalize_scratch(c, desc, batch, stats, eps, mr, running, scratch)
    if running is not None:
        rm, rv, momentum, times = running
        check(c.lib.t2v_batch_norm_finalize_running(c.handle, _stream(), ctypes.byref(desc), batch, _p(stats), eps, _p(mr), _p(rm),
                                                    _p(rv), momentum, int(times)), "batch_norm_finalize_running")
        return mr
    check(c.lib.t2v_batch_norm_finalize(c.handle, _stream(), ctypes.byref(desc), batch, _p(stats), eps, _p(mr)),
          "batch_norm_finalize")
    return mr


def batch_norm_update_running(mean_rstd, running_mean, running_var, n, momentum=0.1, eps=1e-5):
    """BatchNorm2d's running statistics, updated in place from a finalize call's (mean, rstd) table over n values per
    channel ($SP/torch/nn/modules/batchnorm.py:57-64: exponential average with `momentum`, unbiased variance)."""
    c = context()
    check(c.lib.t2v_batch_norm_update_running(c.handle, _stream(), _p(mean_rstd), _p(running_mean), _p(running_var), int(n),
                                              running_mean.numel(), momentum, eps), "batch_norm_update_running")


_scratch = {}


def _reduce_scratch(device):
    s = _scratch.get(device)
    if s is None:
        s = _scratch[device] = torch.empty(2048, dtype=torch.float32, device=device)
    return s


def sum_sq_diff_const(x, c0):
    """sum((x - c0)^2) as a 1-element device tensor (LSGAN MSE numerator)."""
    c = context()
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    check(c.lib.t2v_sum_sq_diff_const(c.handle, _stream(), _p(x), float(c0), x.numel(), _p(_reduce_scratch(x.device)),
                                      _p(out)), "sum_sq_diff_const")
    return out


def sum_abs_diff(a, b):
    """sum(|a - b|) as a 1-element device tensor (L1 feature-matching numerator)."""
    c = context()
    assert a.shape == b.shape
    out = torch.empty(1, dtype=torch.float32, device=a.device)
    check(c.lib.t2v_sum_abs_diff(c.handle, _stream(), _p(a), _p(b), a.numel(), _p(_reduce_scratch(a.device)), _p(out)),
          "sum_abs_diff")
    return out


def sum_abs_diff_masked(a, b, mask, c0, C):
    """sum over pixels and the channels [c0, c0+C) of mask[pix] * |a - b| ([..., cs] tensors; b / mask may be None)."""
    c = context()
    cs = a.shape[-1]
    out = torch.empty(1, dtype=torch.float32, device=a.device)
    check(c.lib.t2v_sum_abs_diff_masked(c.handle, _stream(), _p(a), _p(b), _p(mask), a.numel() // cs, c0, C, cs,
                                        _p(_reduce_scratch(a.device)), _p(out)), "sum_abs_diff_masked")
    return out


def sum_abs_diff_masked_backward(a, b, mask, c0, C, scale):
    c = context()
    cs = a.shape[-1]
    da = torch.empty_like(a)
    check(c.lib.t2v_sum_abs_diff_masked_backward(c.handle, _stream(), _p(a), _p(b), _p(mask), float(scale),
                                                 a.numel() // cs, c0, C, cs, _p(da)), "sum_abs_diff_masked_backward")
    return da


def loss_terms(term_ptrs, term_ints, term_floats, chunk_term, chunk_off, term_chunk0, nterms, nchunks, chunk, partials, out):
    """all scalar loss terms of a step (values and gradient seeds) in one launch: t2v_loss_terms (include/t2v.h)"""
    c = context()
    check(c.lib.t2v_loss_terms(c.handle, _stream(), _p(term_ptrs), _p(term_ints), _p(term_floats), _p(chunk_term), _p(chunk_off),
                               _p(term_chunk0), int(nterms), int(nchunks), int(chunk), _p(partials), _p(out)), "loss_terms")
    return out


def adam_step(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step):
    """In-place fused Adam update of one flat fp32 tensor (torch.optim.Adam.step semantics)."""
    c = context()
    check(c.lib.t2v_adam_step(c.handle, _stream(), _p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(),
                              lr, beta1, beta2, eps, int(step)), "adam_step")
    return param


def adam_step_multi(ptrs, nelem, step_size, chunk_tensor, chunk_off, chunk, beta1, beta2, eps):
    """One launch over many tensors (tables are device tensors: ptrs int64 [T,4], nelem int64 [T], step_size float32
    [T], chunk_tensor int32 [NC], chunk_off int64 [NC])."""
    c = context()
    check(c.lib.t2v_adam_step_multi(c.handle, _stream(), _p(ptrs), _p(nelem), _p(step_size), _p(chunk_tensor), _p(chunk_off),
                                    chunk_tensor.numel(), int(chunk), beta1, beta2, eps), "adam_step_multi")


def conv2d_backward_weight(x, dy, desc, accumulate_into=None):
    """Weight gradient in the PACKED layout.  x: [B,H,W,x_cs], dy: [B,Hout,Wout,dy_cs] (or 3-D, B=1)."""
    c = context()
    if x.dim() == 3:
        x, dy = x.unsqueeze(0), dy.unsqueeze(0)
    _chk(x, "x")
    _chk(dy, "dy")
    B, x_cs, dy_cs = x.shape[0], x.shape[-1], dy.shape[-1]
    n = c.lib.t2v_conv_packed_weight_floats(ctypes.byref(desc), x_cs)
    # (every real entry of the packed gradient is written -- by the kernel, its in-kernel combine or the reduce pass)
    dw = accumulate_into if accumulate_into is not None else torch.empty(n, dtype=torch.float32, device=x.device)
    nws = c.lib.t2v_conv_backward_weight_workspace_floats(ctypes.byref(desc), x_cs, B)
    ws = torch.empty(nws, dtype=torch.float32, device=x.device) if nws else None
    check(c.lib.t2v_conv2d_backward_weight(c.handle, _stream(), ctypes.byref(desc), B, _p(x), x_cs, _p(dy), dy_cs,
                                           _p(dw), int(accumulate_into is not None), _p(ws)), "conv2d_backward_weight")
    return dw


def backward_weight_strided_supported(desc, x_cs, dy_cs):
    return bool(_lib.load().t2v_conv_backward_weight_strided_supported(ctypes.byref(desc), x_cs, dy_cs))


def conv2d_backward_weight_pair(x0, dy0, x1, dy1, desc, accumulate_into=None):
    """packed dW of the two images x0 / x1 ([H,W,x_cs] each, in buffers of their own) and their output gradients in ONE
    launch (t2v_conv2d_backward_weight_strided): what conv2d_backward_weight computes on torch.stack of them, bit for bit."""
    c = context()
    for t, n in ((x0, "x0"), (x1, "x1"), (dy0, "dy0"), (dy1, "dy1")):
        _chk(t, n)
    assert x0.shape == x1.shape and dy0.shape == dy1.shape and x0.dim() == 3
    x_cs, dy_cs = x0.shape[-1], dy0.shape[-1]
    n = c.lib.t2v_conv_packed_weight_floats(ctypes.byref(desc), x_cs)
    dw = accumulate_into if accumulate_into is not None else torch.empty(n, dtype=torch.float32, device=x0.device)
    nws = c.lib.t2v_conv_backward_weight_workspace_floats(ctypes.byref(desc), x_cs, 2)
    ws = torch.empty(max(nws, 1), dtype=torch.float32, device=x0.device)
    xs, ys = (x1.data_ptr() - x0.data_ptr()) // 4, (dy1.data_ptr() - dy0.data_ptr()) // 4
    if xs == 0 or ys == 0:
        raise ValueError("conv2d_backward_weight_pair: the two images share a buffer")
    check(c.lib.t2v_conv2d_backward_weight_strided(c.handle, _stream(), ctypes.byref(desc), 2, _p(x0), x_cs, xs, _p(dy0), dy_cs, ys,
                                                   _p(dw), int(accumulate_into is not None), _p(ws)), "conv2d_backward_weight_strided")
    return dw


def backward_weight_winograd_supported(desc, x_cs, dy_cs):
    return bool(_lib.load().t2v_conv_backward_weight_winograd_supported(ctypes.byref(desc), x_cs, dy_cs))


def conv2d_backward_weight_winograd(x, dy, desc, accumulate_into=None, out=None):
    """Weight gradient of a 3x3 stride-1 conv through the Winograd domain (F(4x4,3x3)), TORCH layout
    [Cout,Cin,3,3].  x: [B,H,W,Cin], dy: [B,Ho,Wo,Cout] (or 3-D, B=1)."""
    c = context()
    if x.dim() == 3:
        x, dy = x.unsqueeze(0), dy.unsqueeze(0)
    _chk(x, "x")
    _chk(dy, "dy")
    B, x_cs, dy_cs = x.shape[0], x.shape[-1], dy.shape[-1]
    dw = accumulate_into if accumulate_into is not None else out if out is not None else \
        torch.empty(desc.Cout, desc.Cin, 3, 3, dtype=torch.float32, device=x.device)
    nws = c.lib.t2v_conv_backward_weight_winograd_workspace_floats(ctypes.byref(desc), x_cs, B)
    if nws == 0:
        raise RuntimeError("conv2d_backward_weight_winograd: shape not supported")
    ws = torch.empty(nws, dtype=torch.float32, device=x.device)
    check(c.lib.t2v_conv2d_backward_weight_winograd(c.handle, _stream(), ctypes.byref(desc), B, _p(x), x_cs, _p(dy), dy_cs,
                                                    _p(dw), int(accumulate_into is not None), _p(ws)),
          "conv2d_backward_weight_winograd")
    return dw


def backward_weight_winograd_workspace(desc, x_cs, batch, device):
    n = _lib.load().t2v_conv_backward_weight_winograd_workspace_floats(ctypes.byref(desc), x_cs, batch)
    if n == 0:
        raise RuntimeError("backward_weight_winograd_workspace: shape not supported")
    return torch.empty(n, dtype=torch.float32, device=device)


def conv2d_backward_weight_winograd_stages(x, dy, desc, ws, batch, b0, reduce, out=None, accumulate=False):
    """Staged form: transform the images x, dy ([nb,H,W,C] / [nb,Ho,Wo,Cout]) into slots [b0, b0+nb) of `ws`
    (backward_weight_winograd_workspace(desc, x_cs, batch)); with reduce=True also run the reduction over all
    `batch` slots and return dW in torch layout, else return None."""
    c = context()
    if x.dim() == 3:
        x, dy = x.unsqueeze(0), dy.unsqueeze(0)
    _chk(x, "x")
    _chk(dy, "dy")
    dw = (out if out is not None else torch.empty(desc.Cout, desc.Cin, 3, 3, dtype=torch.float32, device=x.device)) \
        if reduce else None
    check(c.lib.t2v_conv2d_backward_weight_winograd_stages(c.handle, _stream(), ctypes.byref(desc), batch, b0, x.shape[0],
                                                           _p(x), x.shape[-1], _p(dy), dy.shape[-1], _p(dw),
                                                           int(bool(accumulate and out is not None)), _p(ws),
                                                           3 if reduce else 1),
          "conv2d_backward_weight_winograd_stages")
    return dw


def conv2d_backward_weight_winograd_dy(dy, desc, ws, batch, slot, x_cs):
    """A dy A^T of one image ([Ho,Wo,Cout] or [1,Ho,Wo,Cout]) into slot `slot` of `ws`, whose V slot the forward pass has
    filled already (conv2d_winograd(keep_v=...))."""
    c = context()
    if dy.dim() == 3:
        dy = dy.unsqueeze(0)
    _chk(dy, "dy")
    check(c.lib.t2v_conv2d_backward_weight_winograd_stages(c.handle, _stream(), ctypes.byref(desc), batch, slot, 1, None, x_cs,
                                                           _p(dy), dy.shape[-1], None, 0, _p(ws), 1),
          "conv2d_backward_weight_winograd_stages")


def conv2d_backward_weight_winograd_dy_norm(conv_out, dy, mean_rstd, gamma, beta, relu, sums, desc, ws, batch, slot, x_cs):
    """conv2d_backward_weight_winograd_dy of the gradient in FRONT of the layer's norm, formed on the fly from the gradient
    behind it (`dy`), the conv's raw output and the sums of instance_norm_backward(..., sums_only=True): one image."""
    c = context()
    _chk(conv_out, "conv_out")
    _chk(dy, "dy")
    assert conv_out.numel() == dy.numel() and conv_out.shape[-1] == desc.Cout
    check(c.lib.t2v_conv2d_backward_weight_winograd_dy_norm(c.handle, _stream(), ctypes.byref(desc), batch, slot, x_cs, _p(conv_out),
                                                            _p(dy), _p(mean_rstd), _p(gamma), _p(beta), int(relu), _p(sums), _p(ws)),
          "conv2d_backward_weight_winograd_dy_norm")


def conv2d_backward_weight_winograd_reduce(desc, ws, batch, x_cs, dy_cs, out=None, accumulate=False):
    """Reduction stage alone over the `batch` slots already transformed into `ws` -> dW in torch layout."""
    c = context()
    dw = out if out is not None else torch.empty(desc.Cout, desc.Cin, 3, 3, dtype=torch.float32, device=ws.device)
    check(c.lib.t2v_conv2d_backward_weight_winograd_stages(c.handle, _stream(), ctypes.byref(desc), batch, 0, 0, None, x_cs,
                                                           None, dy_cs, _p(dw), int(bool(accumulate and out is not None)),
                                                           _p(ws), 2),
          "conv2d_backward_weight_winograd_stages")
    return dw


def backward_data_winograd_supported(desc, x_cs, dy_cs):
    return bool(_lib.load().t2v_conv_backward_data_winograd_supported(ctypes.byref(desc), x_cs, dy_cs))


def pack_conv_weight_transposed(w, desc, x_cs):
    """U^T of a forward 3x3 layer (torch weight [Cout,Cin,3,3] on the device) for conv2d_backward_data_winograd."""
    c = context()
    n = c.lib.t2v_conv_backward_data_winograd_weight_floats(ctypes.byref(desc), x_cs)
    out = torch.empty(n, dtype=torch.float32, device=w.device)
    check(c.lib.t2v_conv_pack_weight_transposed(c.handle, _stream(), ctypes.byref(desc), x_cs, _p(w.contiguous()), _p(out)),
          "conv_pack_weight_transposed")
    return out


def backward_data_winograd_takes_forward_weights(desc, x_cs, dy_cs):
    """the data gradient reads the forward layer's own F(4x4) packing (pack_conv_weight) in place: no transposed copy"""
    return bool(_lib.load().t2v_conv_backward_data_winograd_takes_forward_weights(ctypes.byref(desc), x_cs, dy_cs))


def backward_data_winograd_scratch(desc, x_cs, device):
    n = _lib.load().t2v_conv_backward_data_winograd_scratch_floats(ctypes.byref(desc), x_cs)
    return torch.empty(n, dtype=torch.float32, device=device)


def conv2d_backward_data_winograd(desc, batch, slot, wgrad_ws, x_cs, ut, out=None, forward_weights=False, scratch=None):
    """dx [H,W,x_cs] of image `slot` of a batch whose A dy A^T already sits in the weight gradient's workspace `wgrad_ws`
    (conv2d_backward_weight_winograd_stages): the transposed Winograd algorithm (include/t2v.h).  `ut`: the transposed
    packing (pack_conv_weight_transposed), or with forward_weights the forward layer's own F(4x4) packing.  `scratch`
    (backward_data_winograd_scratch): where dV = U^T dM lands, [36][Tp][Cin] first (its own buffer by default)."""
    c = context()
    dx = torch.empty(desc.H, desc.W, x_cs, dtype=torch.float32, device=wgrad_ws.device) if out is None else out
    if scratch is None:
        scratch = backward_data_winograd_scratch(desc, x_cs, wgrad_ws.device)
    fn = c.lib.t2v_conv2d_backward_data_winograd_fw if forward_weights else c.lib.t2v_conv2d_backward_data_winograd
    check(fn(c.handle, _stream(), ctypes.byref(desc), batch, slot, _p(wgrad_ws), x_cs, _p(ut), _p(scratch), _p(dx)),
          "conv2d_backward_data_winograd")
    return dx


def maxpool2x2(x):
    """MaxPool2d(2,2) on [H,W,C] or [B,H,W,C] (H even for a batch: the images are pooled as one tall image)."""
    c = context()
    _chk(x, "x")
    if x.dim() == 4:
        B, H, W, C = x.shape
        assert H % 2 == 0, "batched maxpool2x2 needs an even height"
        return maxpool2x2(x.reshape(B * H, W, C)).reshape(B, H // 2, W // 2, C)
    H, W, C = x.shape
    y = torch.empty(H // 2, W // 2, C, dtype=torch.float32, device=x.device)
    check(c.lib.t2v_maxpool2x2(c.handle, _stream(), _p(x), _p(y), H, W, C), "maxpool2x2")
    return y


def maxpool2x2_backward(x, dy):
    c = context()
    _chk(x, "x")
    _chk(dy, "dy")
    if x.dim() == 4:
        B, H, W, C = x.shape
        return maxpool2x2_backward(x.reshape(B * H, W, C), dy.reshape(B * (H // 2), W // 2, C)).reshape(B, H, W, C)
    H, W, C = x.shape
    dx = torch.empty_like(x)
    check(c.lib.t2v_maxpool2x2_backward(c.handle, _stream(), _p(x), _p(dy), _p(dx), H, W, C), "maxpool2x2_backward")
    return dx


def unpack_conv_weight(packed, desc, x_cs=None):
    """packed layout -> torch layout ([Cout,Cin,kH,kW] or [Cin,Cout,3,3])."""
    c = context()
    x_cs = round_up(desc.Cin, 4) if x_cs is None else x_cs
    shape = (desc.Cin, desc.Cout, desc.kH, desc.kW) if desc.transposed else (desc.Cout, desc.Cin, desc.kH, desc.kW)
    w = torch.empty(shape, dtype=torch.float32, device=packed.device)
    check(c.lib.t2v_conv_unpack_weight(c.handle, _stream(), ctypes.byref(desc), x_cs, _p(packed), _p(w)),
          "conv_unpack_weight")
    return w


def unpack_conv_weight_into(packed, desc, x_cs, out, accumulate):
    """packed layout -> torch layout written (or added, accumulate=True) into `out`: a contiguous tensor of the weight's
    torch shape, e.g. the parameter's slice of a flat gradient bucket."""
    c = context()
    check(c.lib.t2v_conv_unpack_weight_into(c.handle, _stream(), ctypes.byref(desc), x_cs, _p(packed), _p(out), int(accumulate)),
          "conv_unpack_weight_into")
    return out


def accumulate_(dst, src, overwrite=False):
    """dst = src (overwrite) or dst += src, in place on contiguous fp32 tensors of equal size."""
    c = context()
    assert dst.numel() == src.numel() and dst.is_contiguous() and src.is_contiguous()
    check(c.lib.t2v_accumulate(c.handle, _stream(), _p(dst), _p(src), dst.numel(), int(overwrite)), "accumulate")
    return dst


def unzip2_(src, dst0, dst1, overwrite=False):
    """src [C,2] -> dst0 (+)= src[:,0], dst1 (+)= src[:,1]"""
    c = context()
    check(c.lib.t2v_unzip2(c.handle, _stream(), _p(src), _p(dst0), _p(dst1), dst0.numel(), int(overwrite)), "unzip2")


def scale_(x, s):
    c = context()
    assert x.is_contiguous()
    check(c.lib.t2v_scale(c.handle, _stream(), _p(x), x.numel(), float(s)), "scale")
    return x


GRAD_FOLD_OPEN, GRAD_FOLD_ADD, GRAD_FOLD_CLOSE = _gradfoldlib.OPEN, _gradfoldlib.ADD, _gradfoldlib.CLOSE


def grad_fold(grad, acc, mode, scale=1.0):
    """One clip's gradients `grad` folded into the accumulator `acc` of an optimiser step over several clips (libt2v_gradfold.so,
    include/t2v_grad_fold.h), on flat fp32 device tensors of equal size: GRAD_FOLD_OPEN acc = grad; GRAD_FOLD_ADD
    acc = acc + grad; GRAD_FOLD_CLOSE grad = (acc + grad) * scale, one fp32 addition and one fp32 multiplication per element."""
    c = context()
    _chk(grad, "grad")
    _chk(acc, "acc")
    if grad.numel() != acc.numel():
        raise ValueError("grad_fold: grad has %d elements, acc %d" % (grad.numel(), acc.numel()))
    check(_gradfoldlib.load().t2v_grad_fold(c.handle, _stream(), _p(grad), _p(acc), grad.numel(), int(mode), float(scale)),
          "grad_fold")
    return grad if mode == GRAD_FOLD_CLOSE else acc


def zero_(x):
    c = context()
    assert x.is_contiguous()
    check(c.lib.t2v_zero(c.handle, _stream(), _p(x), x.numel() * x.element_size()), "zero")
    return x


def channel_sum(x, C=None, out=None):
    """sum over all pixels per channel of an NHWC tensor (bias gradient)."""
    c = context()
    _chk(x, "x")
    cs = x.shape[-1]
    C = cs if C is None else C
    out = torch.empty(C, dtype=torch.float32, device=x.device) if out is None else out
    scratch = torch.empty(256 * C, dtype=torch.float32, device=x.device)
    check(c.lib.t2v_channel_sum(c.handle, _stream(), _p(x), x.numel() // cs, C, cs, _p(scratch), _p(out)),
          "channel_sum")
    return out


def reflect_pad_backward(dxp, pad, out=None):
    """adjoint of ReflectionPad2d(pad): [H+2p, W+2p, C] -> [H, W, C]."""
    c = context()
    _chk(dxp, "dxp")
    Hp, Wp, C = dxp.shape
    H, W = Hp - 2 * pad, Wp - 2 * pad
    dx = out if out is not None else torch.empty(H, W, C, dtype=torch.float32, device=dxp.device)
    _chk(dx, "dx")
    check(c.lib.t2v_reflect_pad_backward(c.handle, _stream(), _p(dxp), _p(dx), H, W, C, pad), "reflect_pad_backward")
    return dx


def instance_norm_backward(x, dy, mean_rstd, gamma=None, beta=None, relu=0, out=None, affine_into=None, sums_only=False):
    """x, dy: [..., C] (all leading dims are the pixels of ONE statistics group).  Returns
    (dx, dbeta_dgamma [C,2]).  affine_into = (d_beta, d_gamma, overwrite): the two sums also land in those gradient
    tensors (written or added) inside the same launches.  sums_only: dx is None -- its consumer forms it
    (conv2d_backward_weight_winograd_dy_norm)."""
    c = context()
    _chk(x, "x")
    _chk(dy, "dy")
    C = x.shape[-1]
    npix = x.numel() // C
    dx = None if sums_only else (out if out is not None else torch.empty_like(x))
    if dx is not None:
        _chk(dx, "dx")
    sums = torch.empty(C, 2, dtype=torch.float32, device=x.device)
    scratch = torch.empty(128 * C * 2, dtype=torch.float32, device=x.device)
    if affine_into is not None:
        d_beta, d_gamma, overwrite = affine_into
        check(c.lib.t2v_instance_norm_backward_affine(c.handle, _stream(), _p(x), _p(dy), _p(mean_rstd), _p(gamma), _p(beta),
                                                      int(relu), npix, C, _p(scratch), _p(dx), _p(sums), _p(d_beta), _p(d_gamma),
                                                      int(bool(overwrite))), "instance_norm_backward_affine")
        return dx, sums
    check(c.lib.t2v_instance_norm_backward(c.handle, _stream(), _p(x), _p(dy), _p(mean_rstd), _p(gamma), _p(beta),
                                           int(relu), npix, C, _p(scratch), _p(dx), _p(sums)), "instance_norm_backward")
    return dx, sums


def act_backward(dy, y, act, slope=1.0):
    c = context()
    dpre = torch.empty_like(dy)
    check(c.lib.t2v_act_backward(c.handle, _stream(), _p(dy), _p(y), act, slope, dy.numel(), _p(dpre)), "act_backward")
    return dpre


def avgpool3x3s2_backward(dy, H, W):
    c = context()
    C = dy.shape[-1]
    dx = torch.empty(H, W, C, dtype=torch.float32, device=dy.device)
    check(c.lib.t2v_avgpool3x3s2_backward(c.handle, _stream(), _p(dy), _p(dx), H, W, C), "avgpool3x3s2_backward")
    return dx


def sum_sq_diff_const_backward(x, c0, scale):
    c = context()
    dx = torch.empty_like(x)
    check(c.lib.t2v_sum_sq_diff_const_backward(c.handle, _stream(), _p(x), float(c0), float(scale), x.numel(), _p(dx)),
          "sum_sq_diff_const_backward")
    return dx


def sum_abs_diff_backward(a, b, scale):
    c = context()
    da = torch.empty_like(a)
    check(c.lib.t2v_sum_abs_diff_backward(c.handle, _stream(), _p(a), _p(b), float(scale), a.numel(), _p(da)),
          "sum_abs_diff_backward")
    return da
