"""Extra storage channels are IGNORED, not just zero on arrival: the twin runs of tests/storage_lanes.py.

Per case (storage_lanes.case_ids(): the Case entries of LANES and the Python-layer cases):
  * run A has zeros in every extra input lane, run B junk -- once per pattern of storage_lanes.PATTERNS (finite values only:
    randn * 1e3, and a mix of +-FLT_MAX, +-1e30, +-2^-149, -0.0 and randn).  Every run starts from NaN-poisoned output
    buffers of the same shapes;
  * the logical outputs of A and B are EQUAL element by element (torch.equal on values: +-0 compare equal) and finite:
    finalised (mean, rstd) tables, scalar sums, unpacked weight gradients and bias gradients included.  No tolerance:
    0 * finite is exactly 0 and s + 0 is exactly s, so equality is derived, not measured, and run A is what the float64
    tests of the suite already pin;
  * the output lanes the header says are written as zero are zero in both runs; destination channels it says are not touched
    still hold their poison; the guard floats around every poisoned buffer are untouched;
  * A and B ran the same set of t2v:: kernels (torch.profiler), printed per case and pattern.

Two things a twin run cannot compare bit for bit, said where they occur: d_prev of t2v_flow_warp_composite_backward is
accumulated with atomic adds (t2v.h: "its summation order is not fixed"), so only its untouched channels are asserted;
packing entries have no input lane -- their cases assert that the packed buffer holds exactly the weight's non-zeros."""
import ctypes

import numpy as np
import pytest
import torch

import kernel_variants as kv
import storage_lanes as sl

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64          # floats in front of and behind every poisoned buffer (256 bytes: alignment is kept)


class Fill:
    """what a run puts into the lanes: 'zero' (run A) or one of the junk patterns (run B); every call draws another seed"""

    def __init__(self, pattern):
        self.pattern, self.n = pattern, 0

    def lanes(self, t, C):
        return self.outside(t, 0, C)

    def outside(self, t, c0, C):
        self.n += 1
        return sl.with_lanes_outside(t, c0, C, self.pattern, seed=self.n)


class Poison:
    """a NaN-filled device buffer with NaN guards on both sides; .t is the view the kernel writes"""

    def __init__(self, *shape):
        n = int(np.prod(shape))
        self.whole = torch.full((n + 2 * GUARD,), float("nan"), device=DEV)
        self.t = self.whole[GUARD:GUARD + n].view(*shape)

    def guards(self):
        return torch.cat([self.whole[:GUARD], self.whole[-GUARD:]])


def _profiled(fn):
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    return {kv.normalise(e.name) for e in prof.events() if "t2v::" in e.name}, out


def _result(equal=None, zero=None, poison=None, expect=None):
    cpu = lambda d: {k: v.detach().cpu().clone() if torch.is_tensor(v) else v for k, v in (d or {}).items()}
    return {"equal": cpu(equal), "zero": cpu(zero), "poison": cpu(poison),
            "expect": {k: tuple(t.detach().cpu().clone() if torch.is_tensor(t) else t for t in v) for k, v in (expect or {}).items()}}


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---- forward convolutions -------------------------------------------------------------------------------------------------
def _conv(cid):
    case = kv.CASE_BY_ID[sl.CONV_GEOMETRY[cid]]._replace(batch=2)

    def run(P):
        from text2video_amd import ops
        x, w, b = kv.case_tensors(case)
        desc = ops.conv_desc(case.H, case.W, case.Cin, case.Cout, case.k, case.stride, case.pad,
                             ops.PAD_REFLECT if case.reflect else ops.PAD_ZERO, case.transposed, ops.ACT_NONE, 1.0,
                             output_padding=case.op)
        xcs, ycs = kv.x_cs(case), ops.round_up(case.Cout, 4)
        assert xcs > case.Cin or ycs > case.Cout
        xs = torch.zeros(2, case.H, case.W, xcs)
        xs[..., :case.Cin] = x.permute(0, 2, 3, 1)
        xs = P.lanes(xs, case.Cin).to(DEV)
        pw, bd = ops.pack_conv_weight(w.to(DEV), desc, xcs), b.to(DEV)
        ho, wo = ops.conv_out_dims(desc)
        y1, yb = Poison(ho, wo, ycs), Poison(2, ho, wo, ycs)
        n = ops.conv_stats_buffer(desc, DEV).numel() if case.stats else 0
        s1, sb = (Poison(n), Poison(2 * n)) if case.stats else (None, None)
        ops.conv2d(xs[0], pw, bd, desc, y_cs=ycs, stats=s1.t if s1 else None, out=y1.t)
        ops.conv2d_batch(xs, pw, bd, desc, y_cs=ycs, stats=sb.t if sb else None, out=yb.t)
        equal = {"y": y1.t[..., :case.Cout], "y_batch": yb.t[..., :case.Cout]}
        poison = {"y guard": y1.guards(), "y_batch guard": yb.guards()}
        if case.stats:
            equal["mean_rstd"] = ops.instance_norm_finalize(s1.t, desc).view(-1, 2)[:case.Cout]
            for i in range(2):
                equal["mean_rstd_batch%d" % i] = ops.instance_norm_finalize(sb.t[i * n:(i + 1) * n], desc).view(-1, 2)[:case.Cout]
            poison.update({"stats guard": s1.guards(), "stats_batch guard": sb.guards()})
        return _result(equal, {"y lanes": y1.t[..., case.Cout:], "y_batch lanes": yb.t[..., case.Cout:]}, poison)
    return run


# ---- weight packing ---------------------------------------------------------------------------------------------------------
def _pack(H, W, Cin, Cout, k, stride, pad, transposed=False, adjoint=False):
    def run(P):
        from text2video_amd import ops
        desc = ops.conv_desc(H, W, Cin, Cout, k, stride, pad, ops.PAD_ZERO, transposed)
        xcs = ops.round_up(Cin, 4)
        assert xcs > Cin
        w = _rand(*((Cin, Cout, k, k) if transposed or adjoint else (Cout, Cin, k, k)), seed=11)
        w[w == 0] = 1.0
        wd = w.to(DEV)
        c = ops.context()
        n = c.lib.t2v_conv_packed_weight_floats(ctypes.byref(desc), xcs)
        packed = Poison(n)
        fn = c.lib.t2v_conv_pack_weight_adjoint if adjoint else c.lib.t2v_conv_pack_weight
        ops.check(fn(c.handle, ops._stream(), ctypes.byref(desc), xcs, wd.data_ptr(), packed.t.data_ptr()), "pack")
        # (a slot left unwritten is NaN, which counts as a non-zero)
        nnz = torch.count_nonzero(packed.t).cpu()
        want = w.transpose(0, 1).flip(2, 3).contiguous() if adjoint else w          # t2v.h: 180-degree flip, in/out transpose
        expect = {"non-zeros of the packed buffer": (nnz, torch.tensor(w.numel())),
                  "unpack(pack(w))": (ops.unpack_conv_weight(packed.t, desc, xcs), want)}
        into = Poison(*want.shape)
        ops.unpack_conv_weight_into(packed.t, desc, xcs, into.t, False)
        expect["unpack_into(pack(w))"] = (into.t, want)
        return _result(expect=expect, poison={"packed guard": packed.guards(), "unpack_into guard": into.guards()})
    return run


# ---- weight gradient, bias gradient, data gradient ----------------------------------------------------------------------------
def _fwd_desc(ops, H, W, Cin, Cout, k, stride, pad, reflect, transposed):
    return ops.conv_desc(H, W, Cin, Cout, k, stride, pad, ops.PAD_REFLECT if reflect else ops.PAD_ZERO, transposed)


def _wgrad(H, W, Cin, Cout, k, stride, pad, reflect, B, pair, transposed=False):
    def run(P):
        from text2video_amd import ops
        desc = _fwd_desc(ops, H, W, Cin, Cout, k, stride, pad, reflect, transposed)
        xcs, ycs = ops.round_up(Cin, 4), ops.round_up(Cout, 4)
        assert xcs > Cin and ycs > Cout
        ho, wo = ops.conv_out_dims(desc)
        xs = P.lanes(_rand(B, H, W, xcs, seed=12), Cin).to(DEV)
        dys = P.lanes(_rand(B, ho, wo, ycs, seed=13), Cout).to(DEV)
        equal = {"dW": ops.unpack_conv_weight(ops.conv2d_backward_weight(xs, dys, desc), desc, xcs),
                 "dbias": ops.channel_sum(dys, Cout)}
        if pair:
            assert B == 2 and ops.backward_weight_strided_supported(desc, xcs, ycs)
            x0, x1, d0, d1 = xs[0].clone(), xs[1].clone(), dys[0].clone(), dys[1].clone()
            equal["dW strided"] = ops.unpack_conv_weight(ops.conv2d_backward_weight_pair(x0, d0, x1, d1, desc), desc, xcs)
        return _result(equal)
    return run


def _channel_sum(npix, C, cs):
    def run(P):
        from text2video_amd import ops
        x = P.lanes(_rand(npix, cs, seed=14), C).to(DEV)
        out = Poison(C)
        ops.channel_sum(x, C, out=out.t)
        return _result({"sum": out.t}, poison={"out guard": out.guards()})
    return run


def _dgrad(H, W, Cin, Cout, k, stride, pad, reflect, transposed):
    def run(P):
        from text2video_amd import ops
        from text2video_amd.backward import ConvDataGrad
        desc = _fwd_desc(ops, H, W, Cin, Cout, k, stride, pad, reflect, transposed)
        w = _rand(*((Cin, Cout, k, k) if transposed else (Cout, Cin, k, k)), seed=15) * 0.1
        dg = ConvDataGrad(desc).refresh(w.to(DEV))
        ho, wo = ops.conv_out_dims(desc)
        ycs, xcs = ops.round_up(Cout, 4), ops.round_up(Cin, 4)
        assert ycs > Cout and xcs > Cin
        dy = P.lanes(_rand(ho, wo, ycs, seed=16), Cout).to(DEV)
        dx = Poison(H, W, xcs)
        dg(dy, out=dx.t)
        return _result({"dx": dx.t[..., :Cin]}, {"dx lanes": dx.t[..., Cin:]}, {"dx guard": dx.guards()})
    return run


# ---- warp, masked L1, activation backward ---------------------------------------------------------------------------------------
def _warp_inputs(P, H, W, prev_cs, c0):
    raw = torch.zeros(H, W, 4)
    raw[..., :3] = torch.tanh(_rand(H, W, 3, seed=17))
    fw = torch.zeros(H, W, 4)
    fw[..., :2] = _rand(H, W, 2, seed=18) * 3.0          # up to ~10 px: some positions leave the 37 x 45 image
    fw[..., 2] = torch.sigmoid(_rand(H, W, seed=19))
    prev = torch.zeros(H, W, prev_cs)
    prev[..., c0:c0 + 3] = torch.tanh(_rand(H, W, 3, seed=20))
    return P.lanes(raw, 3).to(DEV), P.lanes(fw, 3).to(DEV), P.outside(prev, c0, 3).to(DEV)


def _flow_warp_composite(P):
    from text2video_amd import ops
    H, W, c0 = 37, 45, 3
    raw, fw, prev = _warp_inputs(P, H, W, 8, c0)
    c = ops.context()
    out, warp, only = Poison(H, W, 4), Poison(H, W, 4), Poison(H, W, 4)
    ops.check(c.lib.t2v_flow_warp_composite(c.handle, ops._stream(), raw.data_ptr(), fw.data_ptr(), prev.data_ptr(), 8, c0,
                                            out.t.data_ptr(), warp.t.data_ptr(), H, W), "flow_warp_composite")
    ops.flow_warp(fw, prev, c0, out=only.t)            # raw == NULL: plain resample
    return _result({"out": out.t[..., :3], "warp_out": warp.t[..., :3], "resample": only.t[..., :3]},
                   {"out ch 3": out.t[..., 3], "warp_out ch 3": warp.t[..., 3], "resample ch 3": only.t[..., 3]},
                   {"out guard": out.guards(), "warp_out guard": warp.guards(), "resample guard": only.guards()})


def _flow_warp_composite_backward(P):
    from text2video_amd import ops
    H, W, c0 = 37, 45, 3
    raw, fw, prev = _warp_inputs(P, H, W, 8, c0)
    d_out = P.lanes(_rand(H, W, 4, seed=21), 3).to(DEV)
    d_warp = P.lanes(_rand(H, W, 4, seed=22), 3).to(DEV)
    d_raw, d_fw, d_prev = ops.flow_warp_composite_backward(d_out, d_warp, raw, fw, prev, c0, want_d_prev=True)
    # d_prev: atomic adds, "its summation order is not fixed" (t2v.h) -- only the channels it must leave alone are compared
    keep = [i for i in range(8) if not c0 <= i < c0 + 3]
    return _result({"d_raw": d_raw[..., :3], "d_fw": d_fw[..., :3]},
                   {"d_raw ch 3": d_raw[..., 3], "d_fw ch 3": d_fw[..., 3], "d_prev outside [c0, c0 + 3)": d_prev[..., keep]},
                   expect={"d_prev is finite": (torch.isfinite(d_prev).all(), torch.tensor(True))})


def _masked_inputs(P, npix, cs, c0, C):
    a = P.outside(_rand(npix, cs, seed=23), c0, C).to(DEV)
    b = P.outside(_rand(npix, cs, seed=24), c0, C).to(DEV)
    return a, b, torch.rand(npix, generator=torch.Generator().manual_seed(25)).to(DEV)


def _sum_abs_diff_masked(P):
    from text2video_amd import ops
    a, b, mask = _masked_inputs(P, 1231, 8, 2, 3)
    return _result({"masked": ops.sum_abs_diff_masked(a, b, mask, 2, 3), "zero target": ops.sum_abs_diff_masked(a, None, None, 2, 3)})


def _sum_abs_diff_masked_backward(P):
    from text2video_amd import ops
    a, b, mask = _masked_inputs(P, 1231, 8, 2, 3)
    da = ops.sum_abs_diff_masked_backward(a, b, mask, 2, 3, 0.125)
    return _result({"da": da[..., 2:5]}, {"da outside [c0, c0 + C)": da[..., [0, 1, 5, 6, 7]]})


def _act_backward_flow_w(P):
    from text2video_amd import ops
    n = 1537
    y = torch.zeros(n, 4)
    y[..., :2] = _rand(n, 2, seed=26) * 20
    y[..., 2] = torch.sigmoid(_rand(n, seed=27))
    dy = P.lanes(_rand(n, 4, seed=28), 3).to(DEV)
    dpre = ops.act_backward(dy, P.lanes(y, 3).to(DEV), 4, 20.0)
    return _result({"dpre": dpre[..., :3]}, {"dpre ch 3": dpre[..., 3]})


# ---- layout and conversion entries --------------------------------------------------------------------------------------------
def _nhwc_to_nchw(P):
    from text2video_amd import ops
    src = P.lanes(_rand(7, 5, 12, seed=29), 10)
    got = ops.nhwc_to_nchw(src.to(DEV), 10)
    return _result({"dst": got}, expect={"dst": (got, src[..., :10].permute(2, 0, 1))})


def _nchw_to_nhwc(P):
    from text2video_amd import ops
    src = _rand(10, 7, 5, seed=30)
    dst = Poison(7, 5, 12)
    ops.nchw_to_nhwc(src.to(DEV), 12, out=dst.t)
    return _result({"dst": dst.t[..., :10]}, {"dst channels [C, dst_cs): written as zero": dst.t[..., 10:]},
                   {"dst guard": dst.guards()}, {"dst": (dst.t[..., :10], src.permute(1, 2, 0))})


def _pose_u8_to_f32(P):
    from text2video_amd import ops
    src = torch.randint(0, 256, (9, 11, 3), generator=torch.Generator().manual_seed(31), dtype=torch.uint8)
    dst = Poison(9, 11, 8)
    ops.pose_u8_to_f32(src.to(DEV), dst.t, 3)
    return _result({"dst": dst.t[..., 3:6]}, None, {"dst outside [c0, c0 + 3): not touched": dst.t[..., [0, 1, 2, 6, 7]],
                                                   "dst guard": dst.guards()},
                   {"dst": (dst.t[..., 3:6], (src.float() / 255.0 - 0.5) / 0.5)})


def _copy_channels(P):
    from text2video_amd import ops
    src = P.outside(_rand(63, 12, seed=32), 3, 5)
    dst = Poison(63, 8)
    ops.copy_channels(src.to(DEV), 3, dst.t, 1, 5)
    return _result({"dst": dst.t[..., 1:6]}, None, {"dst outside [dst_c0, dst_c0 + nc): not touched": dst.t[..., [0, 6, 7]],
                                                   "dst guard": dst.guards()}, {"dst": (dst.t[..., 1:6], src[..., 3:8])})


def _resample_crop_normalize_u8(P):
    from text2video_amd import ops
    src = torch.randint(0, 256, (2, 20, 24, 3), generator=torch.Generator().manual_seed(33), dtype=torch.uint8).to(DEV)
    dst, ref = Poison(2, 10, 12, 8), Poison(2, 10, 12, 4)
    ops.resample_crop_normalize_u8(src, (16, 12), (2, 1), (12, 10), out=dst.t, c0=2)
    ops.resample_crop_normalize_u8(src, (16, 12), (2, 1), (12, 10), out=ref.t, c0=0)
    return _result({"dst": dst.t[..., 2:5]}, None, {"dst outside [dst_c0, dst_c0 + 3): not touched": dst.t[..., [0, 1, 5, 6, 7]],
                                                   "dst guard": dst.guards()}, {"dst": (dst.t[..., 2:5], ref.t[..., :3])})


# ---- optical flow -------------------------------------------------------------------------------------------------------------
def _smooth(H, W, seed):
    """a low-pass random texture in [-1, 1], and the same texture moved by about (1.5, -1) px"""
    t = torch.nn.functional.avg_pool2d(_rand(1, 3, H + 16, W + 16, seed=seed), 7, 1, 3)
    t = torch.nn.functional.avg_pool2d(t, 5, 1, 2)
    t = t / t.abs().max()
    return t[0, :, 8:8 + H, 8:8 + W].permute(1, 2, 0), t[0, :, 7:7 + H, 10:10 + W].permute(1, 2, 0)


def _optical_flow(refine_iters):
    def run(P):
        from text2video_amd import ops
        H, W = 48, 64
        a, b = _smooth(H, W, 34)
        cur, prev = torch.zeros(H, W, 8), torch.zeros(H, W, 12)
        cur[..., 2:5], prev[..., 7:10] = a, b
        cur, prev = P.outside(cur, 2, 3).to(DEV), P.outside(prev, 7, 3).to(DEV)
        out = Poison(H, W, 4)
        ops.optical_flow(cur, prev, cur_c0=2, prev_c0=7, out=out.t, refine_iters=refine_iters)
        moved = out.t[..., :2].abs().max() > 0.25
        return _result({"flow": out.t[..., :2]}, {"flow_out channels 2, 3": out.t[..., 2:]}, {"flow_out guard": out.guards()},
                       {"the flow is not trivially zero": (moved, torch.tensor(True))})
    return run


# ---- generator frame and train step -------------------------------------------------------------------------------------------
_generators = {}


def _generator(no_flow):
    def run(P):
        from text2video_amd.generator import GeneratorSpec, HipGenerator, synthetic_state_dict
        if no_flow not in _generators:          # (the smallest spec tests/test_gpu_generator.py uses)
            spec = GeneratorSpec(ngf=16, n_downsample=2, n_blocks=2, no_flow=no_flow, norm="batch")
            _generators[no_flow] = HipGenerator(spec, DEV).load_state_dict(synthetic_state_dict(spec, 3, "vid2vid", 0.1))
        net = _generators[no_flow]
        H = W = 64
        want = ("out", "raw") if no_flow else ("out", "raw", "flow_w")
        ins = []
        for i in range(2):
            pose, prev = torch.zeros(H, W, 12), torch.zeros(H, W, 8)
            pose[..., :9] = torch.rand(H, W, 9, generator=torch.Generator().manual_seed(40 + i)) * 2 - 1
            prev[..., :6] = torch.tanh(_rand(H, W, 6, seed=42 + i))
            ins.append((P.lanes(pose, 9).to(DEV), P.lanes(prev, 6).to(DEV)))
        one = net.forward(ins[0][0], ins[0][1], False, want=want)
        two = net.forward_batch([p for p, _ in ins], [q for _, q in ins], [False, False], want=want)
        equal, zero = {}, {}
        for tag, res in (("frame", one), ("batch0", two[0]), ("batch1", two[1])):
            for name in want:
                equal["%s %s" % (tag, name)] = res[name][..., :3]
                if name != "flow_w":
                    zero["%s %s ch 3" % (tag, name)] = res[name][..., 3]
        return _result(equal, zero)
    return run


def _train_step_64(P):
    from text2video_amd import train as T
    from text2video_amd.options import TrainOptions
    from test_gpu_optical_flow_refine import TRAIN_ARGS
    H = W = 64
    real_prev, real = [torch.zeros(1, H, W, 4) for _ in range(2)]
    a, b = _smooth(H, W, 50)
    real[0, ..., :3], real_prev[0, ..., :3] = a, b
    pose, prev_in = torch.zeros(1, H, W, 12), torch.zeros(1, H, W, 8)
    pose[..., :9] = torch.rand(1, H, W, 9, generator=torch.Generator().manual_seed(51)) * 2 - 1
    prev_in[..., :6] = torch.tanh(_rand(1, H, W, 6, seed=52))
    tr = T.Vid2VidTrainer(TrainOptions().parse(TRAIN_ARGS + ["--max_frames_per_gpu", "1", "--n_scales_temporal", "0"]), DEV, seed=7)
    losses = tr.train_step(P.lanes(pose, 9).to(DEV), P.lanes(real, 3).to(DEV), None, P.lanes(prev_in, 6).to(DEV),
                           real_prev=P.lanes(real_prev, 3).to(DEV))[0]
    torch.cuda.synchronize()
    equal = {"loss %s" % k: torch.tensor(float(v)) for k, v in sorted(losses.items())}
    equal["gradient bucket G"], equal["gradient bucket D"] = tr.bucketsG.flat, tr.bucketsD.flat
    return _result(equal, expect={"G received gradients": (tr.bucketsG.flat.abs().max() > 0, torch.tensor(True)),
                                  "D received gradients": (tr.bucketsD.flat.abs().max() > 0, torch.tensor(True))})


RUNNERS = dict({cid: _conv(cid) for cid in sl.CONV_GEOMETRY}, **{
    "pack_conv_k4s2_cin6": _pack(16, 16, 6, 64, 4, 2, 2),
    "pack_convT_cin5": _pack(9, 11, 5, 32, 3, 2, 1, transposed=True),
    "pack_adjoint_cin30": _pack(17, 19, 30, 6, 3, 1, 1, adjoint=True),       # the data-gradient conv of a 6 -> 30 layer
    "wgrad_s2_cin6_cout30": _wgrad(32, 32, 6, 30, 3, 2, 1, False, 2, False),
    # (the strided entry takes no folded taps: a regular conv needs x_cs >= 64 there, a transposed one any x_cs)
    "wgrad_strided_convT_cin6_cout30": _wgrad(16, 16, 6, 30, 3, 2, 1, False, 2, True, transposed=True),
    "wgrad_reflect_k7_cin9_cout30": _wgrad(12, 13, 9, 30, 7, 1, 3, True, 1, False),
    "channel_sum_c6_cs8": _channel_sum(37 * 41, 6, 8),
    "channel_sum_c30_cs32": _channel_sum(64 * 64, 30, 32),
    "dgrad_s2_cout30": _dgrad(16, 16, 6, 30, 4, 2, 2, False, False),
    "dgrad_reflect_cout30": _dgrad(17, 19, 6, 30, 3, 1, 1, True, False),
    "dgrad_convT_cout30": _dgrad(9, 11, 6, 30, 3, 2, 1, False, True),
    "flow_warp_composite": _flow_warp_composite,
    "flow_warp_composite_backward": _flow_warp_composite_backward,
    "sum_abs_diff_masked": _sum_abs_diff_masked,
    "sum_abs_diff_masked_backward": _sum_abs_diff_masked_backward,
    "act_backward_flow_w": _act_backward_flow_w,
    "nhwc_to_nchw": _nhwc_to_nchw,
    "nchw_to_nhwc": _nchw_to_nhwc,
    "pose_u8_to_f32": _pose_u8_to_f32,
    "copy_channels": _copy_channels,
    "resample_crop_normalize_u8": _resample_crop_normalize_u8,
    "optical_flow": _optical_flow(0),
    "optical_flow_refined": _optical_flow(5),
    "generator_frame_noflow": _generator(True),
    "generator_frame_flow": _generator(False),
    "train_step_64": _train_step_64,
})


# cases whose first run also packs weights, which the later ones find cached: one run before the profiled ones
WARM_UP = ("generator_frame_noflow", "generator_frame_flow")


def _check_one(cid, pattern, res):
    for name, t in res["equal"].items():
        assert torch.isfinite(t).all(), "%s / %s: %s is not finite (NaN poison left, or junk reached it)" % (cid, pattern, name)
    for name, t in res["zero"].items():
        assert t.numel() == 0 or (t == 0).all(), "%s / %s: %s must be zero" % (cid, pattern, name)
    for name, t in res["poison"].items():
        assert torch.isnan(t).all(), "%s / %s: %s was written" % (cid, pattern, name)
    for name, (got, want) in res["expect"].items():
        assert torch.equal(got, want), "%s / %s: %s" % (cid, pattern, name)


@pytest.mark.parametrize("cid", sl.case_ids())
def test_junk_in_the_storage_lanes_changes_nothing(cid):
    assert torch.cuda.is_available(), "GPU test without a GPU"
    from text2video_amd import ops
    ops.context()                       # (the library's start-up self-test launches a kernel of its own)
    run = RUNNERS[cid]
    if cid in WARM_UP:
        run(Fill("zero"))
    ran_a, a = _profiled(lambda: run(Fill("zero")))
    assert ran_a, "%s: no t2v:: kernel ran" % cid
    _check_one(cid, "zero", a)
    for pattern in sl.PATTERNS:
        ran_b, b = _profiled(lambda: run(Fill(pattern)))
        print("storage_lanes %s | %s | %s" % (cid, pattern, " ".join(sorted(ran_b))))
        _check_one(cid, pattern, b)
        assert ran_b == ran_a, "%s / %s: kernels differ: %s" % (cid, pattern, sorted(ran_a ^ ran_b))
        assert sorted(a["equal"]) == sorted(b["equal"])
        for name, t in a["equal"].items():
            u = b["equal"][name]
            assert torch.equal(t, u), "%s / %s: %s differs at %d of %d places (max |d| %.3g)" % (
                cid, pattern, name, int((t != u).sum()), t.numel(), (t.double() - u.double()).abs().max().item())
