"""The other half of the channel-storage convention of include/t2v.h: "cs" arguments are a storage stride, a multiple of 4
that is at least the logical channel count, and the extra channels (the "lanes") "must hold finite values and are ignored /
written as zero".  The suite asserts "written as zero" in many places and fed exact zeros to the lanes nearly everywhere,
where 0 * 0 hides a loader that multiplies a lane by a weight slot that is not zero, a packing kernel that leaves a value in
a pad K slot, a reduction over cs instead of C and a flat sum over [npix, cs].

A plain helper module (no fixtures, no pytest hooks), imported by tests/test_cpu_storage_lanes.py and
tests/test_gpu_storage_lanes.py.

  * the two junk patterns (finite, seeded) and with_lanes / with_lanes_outside, which fill the lanes of a tensor;
  * LANES: every parameter named cs, *_cs, c0 or *_c0 of every entry point of the four headers -> what checks that the
    entry ignores the lanes that parameter creates:
      Case(ids)             twin runs of tests/test_gpu_storage_lanes.py (zeros in the lanes, then junk: equal outputs);
      Existing(nodeids)     a test that already feeds non-zero lanes;
      NotApplicable(reason) the entry refuses cs > C: no lane exists.  The reason quotes the condition;
      Query(reason)         the entry computes a size or answers yes / no from the stride and is handed no tensor;
  * PYTHON_CASES: the twin runs of the Python layer (data gradient, generator frame, train step);
  * the fault-sensitivity helpers: an im2col conv over padded channel storage in float64 with the four faults the twin
    run exists to see.

Junk is data, never an index: no shape, offset or count is ever junk, and no value is NaN or Inf."""
import collections
import zlib

import torch
import torch.nn.functional as F

HEADERS = ("t2v.h", "t2v_flow_refine.h", "t2v_bf16x2.h", "t2v_grad_fold.h")
PATTERNS = ("moderate", "extreme")
FLT_MAX = float(torch.finfo(torch.float32).max)      # 3.4028235e38
EXTREMES = (FLT_MAX, -FLT_MAX, 1e30, -1e30, 2.0 ** -149, -2.0 ** -149, -0.0)


def junk(shape, pattern, seed=0):
    """fp32 tensor of `shape`: 'zero'; 'moderate' = randn * 1e3; 'extreme' = a random mix of +-FLT_MAX, +-1e30, +-2^-149, -0.0
    and randn.  Finite everywhere; the same (shape, pattern, seed) gives the same values."""
    if pattern == "zero":
        return torch.zeros(shape)
    g = torch.Generator().manual_seed(zlib.crc32(("%s %s %d" % (tuple(shape), pattern, seed)).encode()))
    r = torch.randn(shape, generator=g)
    if pattern == "moderate":
        out = r * 1e3
    elif pattern == "extreme":
        pick = torch.randint(0, len(EXTREMES) + 1, tuple(shape), generator=g)
        table = torch.tensor(EXTREMES + (0.0,), dtype=torch.float32)
        out = torch.where(pick < len(EXTREMES), table[pick], r)
    else:
        raise ValueError("unknown pattern %r" % (pattern,))
    assert torch.isfinite(out).all()
    return out


def with_lanes(t, C, pattern, seed=0):
    """t with [..., C:] filled with the pattern (a copy; t keeps its values)"""
    return with_lanes_outside(t, 0, C, pattern, seed)


def with_lanes_outside(t, c0, C, pattern, seed=0):
    """t with every channel outside [c0, c0 + C) filled with the pattern (a copy)"""
    cs = t.shape[-1]
    assert 0 <= c0 and c0 + C <= cs
    out = t.clone()
    j = junk(t.shape, pattern, seed).to(t.dtype)
    out[..., :c0] = j[..., :c0]
    out[..., c0 + C:] = j[..., c0 + C:]
    return out


# ---- the table -------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "ids")
Existing = collections.namedtuple("Existing", "nodeids")
NotApplicable = collections.namedtuple("NotApplicable", "reason")
Query = collections.namedtuple("Query", "reason")

_T = "t2v.h"
_R = "t2v_flow_refine.h"
_WINO_X = ('t2v.h, t2v_conv_winograd_supported: "Cin % 32 == 0 == x_cs"; every other algorithm of the *_winograd entries '
           'asks the same (t2v_conv_polyphase_supported: "x_cs == Cin", t2v_conv_direct_bf16x2_supported: "x_cs == Cin")')
_WINO_Y = ('t2v.h, t2v_conv2d_forward_winograd: every form that runs through the *_winograd entries asks "y_cs == Cout" '
           '(capi.hip: "winograd forward: output channel storage must equal Cout")')
_WGRAD_W = ('t2v.h, t2v_conv_backward_weight_winograd_supported: "the forward conditions of F(4x4,3x3) plus dy_cs == Cout", and '
            'those conditions hold "Cin % 32 == 0 == x_cs"')
_DGRAD_W = ('capi.hip, dgrad_winograd_ok rests on winograd_supported: "x_cs != d->Cin" is refused '
            '(t2v.h: "Cin % 32 == 0 == x_cs"), and dy_cs == Cout')
_QUERY = "computes a size or a yes / no from the descriptor and the stride; it is handed no tensor"
_CONV = ("conv_stem_cin6", "conv_stem_cin7", "conv_stem_cin9", "conv_stem_cin11", "conv_igemm_cin3_k3_reflect",
         "conv_igemm_cin6_k4s2p2", "conv_igemm_cin9_k3s2", "conv_igemm_cin5_convT", "conv_igemm_cin6_cout30")
_U8_IMG = ("tests/test_gpu_image_metrics.py::test_whole_frame_against_reference",)
_U8_TMP = ("tests/test_gpu_temporal_metrics.py::test_whole_frame_against_reference",)
_U8_FLOW = ("tests/test_gpu_temporal_metrics.py::test_optical_flow_u8_is_bit_equal_to_optical_flow_on_the_converted_frames",)
_U8_REFINED = ("tests/test_gpu_optical_flow_refine.py::test_u8_entry_is_bit_equal_to_the_fp32_entry_on_the_converted_frames",)

LANES = {
    (_T, "t2v_conv_packed_weight_floats", "x_cs"): Query(_QUERY),
    (_T, "t2v_conv_pack_weight", "x_cs"): Case(("pack_conv_k4s2_cin6", "pack_convT_cin5")),
    (_T, "t2v_conv_pack_weight_adjoint", "x_cs"): Case(("pack_adjoint_cin30",)),
    (_T, "t2v_conv2d_forward", "x_cs"): Case(_CONV),
    (_T, "t2v_conv2d_forward", "y_cs"): Case(("conv_igemm_cin6_cout30",)),
    (_T, "t2v_conv2d_forward_batch", "x_cs"): Case(_CONV),
    (_T, "t2v_conv2d_forward_batch", "y_cs"): Case(("conv_igemm_cin6_cout30",)),
    (_T, "t2v_conv2d_forward_head_norm", "x_cs"): NotApplicable(
        't2v.h: "mean_rstd [x_cs][2] as t2v_*_norm_finalize writes it" -- one row per channel of the conv whose raw output x is, '
        'so x_cs == Cin: x has no lane (and "x_cs % 16 == 0")'),
    (_T, "t2v_conv2d_forward_head_norm", "y_cs"): Existing(
        ("tests/test_gpu_head_norm.py::test_head_on_raw_map_is_apply_then_head",)),
    (_T, "t2v_conv_winograd_supported", "x_cs"): Query(_QUERY),
    (_T, "t2v_conv_winograd_bf16x2_supported", "x_cs"): Query(_QUERY),
    (_T, "t2v_conv_polyphase_supported", "x_cs"): Query(_QUERY),
    (_T, "t2v_conv_polyphase_bf16x2_supported", "x_cs"): Query(_QUERY),
    (_T, "t2v_conv_best_algo", "x_cs"): Query(_QUERY),
    (_T, "t2v_conv_winograd_workspace_floats", "x_cs"): Query(_QUERY),
    (_T, "t2v_conv_winograd_batch_workspace_floats", "x_cs"): Query(_QUERY),
    (_T, "t2v_conv2d_forward_winograd", "x_cs"): NotApplicable(_WINO_X),
    (_T, "t2v_conv2d_forward_winograd", "y_cs"): NotApplicable(_WINO_Y),
    (_T, "t2v_conv2d_forward_winograd_stages", "x_cs"): NotApplicable(_WINO_X),
    (_T, "t2v_conv2d_forward_winograd_stages", "y_cs"): NotApplicable(_WINO_Y),
    (_T, "t2v_conv2d_forward_winograd_batch_stages", "x_cs"): NotApplicable(_WINO_X),
    (_T, "t2v_conv2d_forward_winograd_batch_stages", "y_cs"): NotApplicable(_WINO_Y),
    (_T, "t2v_conv2d_forward_winograd_keep_v", "x_cs"): NotApplicable(_WINO_X),
    (_T, "t2v_conv2d_forward_winograd_keep_v", "y_cs"): NotApplicable(_WINO_Y),
    (_T, "t2v_flow_warp_composite", "prev_cs"): Case(("flow_warp_composite",)),
    (_T, "t2v_flow_warp_composite", "prev_c0"): Case(("flow_warp_composite",)),
    (_T, "t2v_flow_warp_composite_backward", "prev_cs"): Case(("flow_warp_composite_backward",)),
    (_T, "t2v_flow_warp_composite_backward", "prev_c0"): Case(("flow_warp_composite_backward",)),
    (_T, "t2v_conv_backward_weight_workspace_floats", "x_cs"): Query(_QUERY),
    (_T, "t2v_conv2d_backward_weight", "x_cs"): Case(("wgrad_s2_cin6_cout30", "wgrad_reflect_k7_cin9_cout30",
                                                       "wgrad_strided_convT_cin6_cout30")),
    (_T, "t2v_conv2d_backward_weight", "dy_cs"): Case(("wgrad_s2_cin6_cout30", "wgrad_reflect_k7_cin9_cout30",
                                                        "wgrad_strided_convT_cin6_cout30")),
    (_T, "t2v_conv_backward_weight_strided_supported", "x_cs"): Query(_QUERY),
    (_T, "t2v_conv_backward_weight_strided_supported", "dy_cs"): Query(_QUERY),
    (_T, "t2v_conv2d_backward_weight_strided", "x_cs"): Case(("wgrad_strided_convT_cin6_cout30",)),
    (_T, "t2v_conv2d_backward_weight_strided", "dy_cs"): Case(("wgrad_strided_convT_cin6_cout30",)),
    (_T, "t2v_conv_backward_weight_winograd_supported", "x_cs"): Query(_QUERY),
    (_T, "t2v_conv_backward_weight_winograd_supported", "dy_cs"): Query(_QUERY),
    (_T, "t2v_conv_backward_weight_winograd_workspace_floats", "x_cs"): Query(_QUERY),
    (_T, "t2v_conv2d_backward_weight_winograd", "x_cs"): NotApplicable(_WGRAD_W),
    (_T, "t2v_conv2d_backward_weight_winograd", "dy_cs"): NotApplicable(_WGRAD_W),
    (_T, "t2v_conv2d_backward_weight_winograd_stages", "x_cs"): NotApplicable(_WGRAD_W),
    (_T, "t2v_conv2d_backward_weight_winograd_stages", "dy_cs"): NotApplicable(_WGRAD_W),
    (_T, "t2v_conv2d_backward_weight_winograd_dy_norm", "x_cs"): NotApplicable(_WGRAD_W),
    (_T, "t2v_conv_backward_data_winograd_supported", "x_cs"): Query(_QUERY),
    (_T, "t2v_conv_backward_data_winograd_supported", "dy_cs"): Query(_QUERY),
    (_T, "t2v_conv_backward_data_winograd_weight_floats", "x_cs"): Query(_QUERY),
    (_T, "t2v_conv_backward_data_winograd_scratch_floats", "x_cs"): Query(_QUERY),
    (_T, "t2v_conv_pack_weight_transposed", "x_cs"): NotApplicable(_DGRAD_W),
    (_T, "t2v_conv2d_backward_data_winograd", "x_cs"): NotApplicable(_DGRAD_W),
    (_T, "t2v_conv_backward_data_winograd_takes_forward_weights", "x_cs"): Query(_QUERY),
    (_T, "t2v_conv_backward_data_winograd_takes_forward_weights", "dy_cs"): Query(_QUERY),
    (_T, "t2v_conv2d_backward_data_winograd_fw", "x_cs"): NotApplicable(_DGRAD_W),
    (_T, "t2v_conv_unpack_weight", "x_cs"): Case(("pack_conv_k4s2_cin6", "pack_convT_cin5", "pack_adjoint_cin30")),
    (_T, "t2v_conv_unpack_weight_into", "x_cs"): Case(("pack_conv_k4s2_cin6", "pack_convT_cin5")),
    (_T, "t2v_channel_sum", "cs"): Case(("channel_sum_c6_cs8", "channel_sum_c30_cs32")),
    (_T, "t2v_sum_abs_diff_masked", "c0"): Case(("sum_abs_diff_masked",)),
    (_T, "t2v_sum_abs_diff_masked", "cs"): Case(("sum_abs_diff_masked",)),
    (_T, "t2v_sum_abs_diff_masked_backward", "c0"): Case(("sum_abs_diff_masked_backward",)),
    (_T, "t2v_sum_abs_diff_masked_backward", "cs"): Case(("sum_abs_diff_masked_backward",)),
    (_T, "t2v_nchw_to_nhwc", "dst_cs"): Case(("nchw_to_nhwc",)),
    (_T, "t2v_nhwc_to_nchw", "src_cs"): Case(("nhwc_to_nchw",)),
    (_T, "t2v_pose_u8_to_f32", "dst_cs"): Case(("pose_u8_to_f32",)),
    (_T, "t2v_pose_u8_to_f32", "c0"): Case(("pose_u8_to_f32",)),
    (_T, "t2v_copy_channels", "src_cs"): Case(("copy_channels",)),
    (_T, "t2v_copy_channels", "src_c0"): Case(("copy_channels",)),
    (_T, "t2v_copy_channels", "dst_cs"): Case(("copy_channels",)),
    (_T, "t2v_copy_channels", "dst_c0"): Case(("copy_channels",)),
    (_T, "t2v_generator_layer_desc", "x_cs"): Query("an int* the call WRITES the layer's input storage stride through; no tensor"),
    (_T, "t2v_optical_flow", "cur_cs"): Case(("optical_flow",)),
    (_T, "t2v_optical_flow", "cur_c0"): Case(("optical_flow",)),
    (_T, "t2v_optical_flow", "prev_cs"): Case(("optical_flow",)),
    (_T, "t2v_optical_flow", "prev_c0"): Case(("optical_flow",)),
    (_T, "t2v_optical_flow_u8", "cur_cs"): Existing(_U8_FLOW),
    (_T, "t2v_optical_flow_u8", "prev_cs"): Existing(_U8_FLOW),
    (_T, "t2v_resample_crop_normalize_u8", "dst_cs"): Case(("resample_crop_normalize_u8",)),
    (_T, "t2v_resample_crop_normalize_u8", "dst_c0"): Case(("resample_crop_normalize_u8",)),
    (_T, "t2v_image_metrics_u8", "a_cs"): Existing(_U8_IMG),
    (_T, "t2v_image_metrics_u8", "b_cs"): Existing(_U8_IMG),
    (_T, "t2v_temporal_metrics_u8", "a_cur_cs"): Existing(_U8_TMP),
    (_T, "t2v_temporal_metrics_u8", "a_prev_cs"): Existing(_U8_TMP),
    (_T, "t2v_temporal_metrics_u8", "b_cur_cs"): Existing(_U8_TMP),
    (_T, "t2v_temporal_metrics_u8", "b_prev_cs"): Existing(_U8_TMP),
    # entries whose storage stride travels in a table or a struct, not in a parameter of that name
    (_T, "t2v_act_backward", "dy"): Case(("act_backward_flow_w",)),
    (_T, "t2v_loss_terms", "term_ints"): Existing(
        ("tests/test_gpu_loss_terms.py::test_values_against_float64_and_seeds_bit_for_bit_in_one_run",)),
    (_T, "t2v_generator_forward", "io"): Case(("generator_frame_noflow", "generator_frame_flow")),
    (_T, "t2v_generator_forward_batch", "ios"): Case(("generator_frame_noflow", "generator_frame_flow")),
    (_R, "t2v_optical_flow_refined", "cur_cs"): Case(("optical_flow_refined",)),
    (_R, "t2v_optical_flow_refined", "cur_c0"): Case(("optical_flow_refined",)),
    (_R, "t2v_optical_flow_refined", "prev_cs"): Case(("optical_flow_refined",)),
    (_R, "t2v_optical_flow_refined", "prev_c0"): Case(("optical_flow_refined",)),
    (_R, "t2v_optical_flow_refined_u8", "cur_cs"): Existing(_U8_REFINED),
    (_R, "t2v_optical_flow_refined_u8", "prev_cs"): Existing(_U8_REFINED),
    ("t2v_bf16x2.h", "t2v_conv_direct_bf16x2_supported", "x_cs"): Query(_QUERY),
}

# the Python layer: (module, callable) -> case ids
PYTHON_CASES = {
    ("text2video_amd/backward.py", "ConvDataGrad.__call__"): ("dgrad_s2_cout30", "dgrad_reflect_cout30", "dgrad_convT_cout30"),
    ("text2video_amd/train.py", "Vid2VidTrainer.train_step"): ("train_step_64",),
}

# the geometry of the forward-conv cases: ids of kernel_variants.CONV_CASES (float64-pinned there)
CONV_GEOMETRY = {
    "conv_stem_cin6": "stem_cs8_cin6_c64", "conv_stem_cin7": "stem_cs8_cin7_c64", "conv_stem_cin9": "stem_cs12_cin9_c64",
    "conv_stem_cin11": "stem_cs12_cin11_c64", "conv_igemm_cin3_k3_reflect": "Q1_stats_reflect_k3_cin3",
    "conv_igemm_cin6_k4s2p2": "Q1_stats_k4s2p2_cin6_disc", "conv_igemm_cin9_k3s2": "Q1_stats_k3s2_cin9_cout96",
    "conv_igemm_cin5_convT": "Q2_stats_convT_cin5_r3", "conv_igemm_cin6_cout30": "Q1_zero_s2_cin6_cout30",
}


def case_ids():
    """every twin-run case id, in the table's order, once"""
    out = []
    for entry in list(LANES.values()) + [Case(ids) for ids in PYTHON_CASES.values()]:
        if isinstance(entry, Case):
            out += [i for i in entry.ids if i not in out]
    return out


# ---- fault sensitivity: an im2col conv over padded channel storage, float64 -------------------------------------------------
FAULTS = ("pad weight slot 2^-20", "K loop over cs, neighbouring tap's weight", "channel sum over cs folded into C-1",
          "flat sum |a - b| over [npix, cs]")


def im2col_conv(x, w, b, cs, k, pad, fault=None):
    """y [Cout, Ho, Wo] of a k x k zero-padded stride-1 conv as the implicit GEMM sees it: K index = tap * cs + c over the
    padded channel storage.  x [cs, H, W] float64 with its lanes filled as the caller chose, w [Cout, Cin, k, k], b [Cout].
    The unfaulted form multiplies the lanes by weight slots that are exactly zero.  Faults:
      FAULTS[0]: the pad weight slots hold 2^-20 instead of 0;
      FAULTS[1]: the pad weight slots hold the neighbouring tap's weight of the same lane index (a K loop that runs over cs
                 with a weight matrix packed over Cin)."""
    Cout, Cin = w.shape[:2]
    taps = k * k
    cols = F.unfold(F.pad(x[None].double(), (pad,) * 4), k)[0]                  # [cs * taps, L], index c * taps + tap
    L = cols.shape[-1]
    cols = cols.view(cs, taps, L).permute(1, 0, 2).reshape(taps * cs, L)
    wd = torch.zeros(Cout, cs, k, k, dtype=torch.float64)
    wd[:, :Cin] = w.double()
    wm = wd.view(Cout, cs, taps).permute(0, 2, 1).reshape(Cout, taps * cs).clone()
    if fault == FAULTS[0]:
        wm.view(Cout, taps, cs)[:, :, Cin:] = 2.0 ** -20
    elif fault == FAULTS[1]:
        tight = w.double().reshape(Cout, Cin, taps).permute(0, 2, 1).reshape(Cout, taps * Cin)      # packed over Cin
        tight = torch.cat([tight, torch.zeros(Cout, cs)], 1)
        for t in range(taps):           # slot (t, c >= Cin) reads on into tap t + 1's first channels
            wm.view(Cout, taps, cs)[:, t, Cin:] = tight[:, (t + 1) * Cin:(t + 1) * Cin + cs - Cin]
    elif fault is not None:
        raise ValueError(fault)
    H, W = x.shape[1:]
    return (wm @ cols + b.double()[:, None]).view(Cout, H + 2 * pad - k + 1, W + 2 * pad - k + 1)


def channel_sum(x, C, fault=None):
    """out [C] = sum over the pixels of x [npix, cs]; FAULTS[2]: the sum runs over cs and the lanes fold into channel C - 1"""
    s = x.double().sum(0)
    out = s[:C].clone()
    if fault == FAULTS[2]:
        out[C - 1] += s[C:].sum()
    elif fault is not None:
        raise ValueError(fault)
    return out


def sum_abs_diff(a, b, C, fault=None):
    """sum |a - b| over the pixels and the channels [0, C) of [npix, cs] tensors; FAULTS[3]: over the flat buffers"""
    d = (a.double() - b.double()).abs()
    if fault == FAULTS[3]:
        return d.sum()
    if fault is not None:
        raise ValueError(fault)
    return d[:, :C].sum()
