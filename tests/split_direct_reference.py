"""Float64 restatement and bounds of T2V_ALGO_DIRECT_BF16X2 (text2video_amd/csrc/conv_igemm_split.hip): the direct 3x3 stride-2
conv and the transposed conv (k3, s2, p1, output_padding 1) with zero padding, their contraction in the split-bf16 arithmetic of
split_reference.

    (xh, xl) = split(x), (wh, wl) = split(w)                                  split_reference.split
    y = conv(xh, wh) + conv(xh, wl) + conv(xl, wh) + bias                     xl * wl dropped

Operand layout ("pairs"): every fp32 channel pair (c, c + 1) of a map [..., C] -- and every K pair of a packed weight -- holds,
in its 8 bytes, the dwords {hi[c] | hi[c + 1] << 16, lo[c] | lo[c + 1] << 16} of bf16 bit patterns.
"""
import torch
import torch.nn.functional as F

import kernel_variants as kv
import split_polyphase_reference as spr
import split_reference as sr

conv64 = spr.conv64          # the exact layer: (x [H, W, Cin], w torch layout, b, up) -> [Ho, Wo, Cout] float64


def pairs_i16(v):
    """fp32 tensor [..., C] (C even) -> int16 [..., C / 2, 4]: (hi[c], hi[c + 1], lo[c], lo[c + 1]) bit patterns per pair, the
    little-endian halves of the two dwords"""
    p = sr.split_planes_i16(v)                                   # [2, ..., C]
    hi, lo = p[0].reshape(*v.shape[:-1], -1, 2), p[1].reshape(*v.shape[:-1], -1, 2)
    return torch.cat([hi, lo], -1).contiguous()


def pairs_i32(v):
    """... as int32 [..., C]: the dwords as the kernels store them (dword 2j = the hi pair, 2j + 1 = the lo pair)"""
    return pairs_i16(v).view(torch.int32).reshape(v.shape)


def unpairs(buf, *shape):
    """an fp32 (or int32) buffer in the pair layout -> (hi, lo) fp32 tensors of `shape` ([..., C])"""
    q = buf.contiguous().view(torch.int16).reshape(*shape[:-1], shape[-1] // 2, 4)
    hi = q[..., :2].contiguous().view(torch.bfloat16).float().reshape(shape)
    lo = q[..., 2:].contiguous().view(torch.bfloat16).float().reshape(shape)
    return hi, lo


def split_conv64(x, w, b, up, drop=None):
    """the split conv in float64 -> [Ho, Wo, Cout].  drop (fault injection): "product" leaves xl * wh out."""
    (xh, xl), (wh, wl) = sr.split(x), sr.split(w)
    z = torch.zeros_like(b)
    y = conv64(xh, wh, b, up) + conv64(xh, wl, z, up)
    return y if drop == "product" else y + conv64(xl, wh, z, up)


def taps(up, Ho, Wo):
    """filter taps that reach output pixel (oy, ox), as [Ho, Wo, 1]: 9 for the stride-2 conv (padding taps count: they are
    terms of the kernel's sum, zeros); 1 | 2 | 2 | 4 for the sub-pixel phases of the transposed conv (oy = 2 iy - 1 + kh: kh = 1
    on even rows, kh in {0, 2} on odd ones)"""
    if not up:
        return torch.full((Ho, Wo, 1), 9.0, dtype=torch.float64)
    ty = 1.0 + (torch.arange(Ho) % 2).double()
    tx = 1.0 + (torch.arange(Wo) % 2).double()
    return (ty[:, None] * tx[None, :])[..., None]


def abs_sum(xh, xl, wh, wl, up):
    """sum over the three kept products of |a| |b|: what the kernel's fp32 accumulation order is measured against"""
    z = torch.zeros(wh.shape[1] if up else wh.shape[0], dtype=torch.float64)
    return conv64(xh.abs(), wh.abs(), z, up) + conv64(xh.abs(), wl.abs(), z, up) + conv64(xl.abs(), wh.abs(), z, up)


def split_gemm_bound(xh, xl, wh, wl, up):
    """split_reference.split_gemm_bound for the conv's contraction: K = taps * Cin per output pixel, 3K exact products
    accumulated in fp32 in the kernel's order"""
    S = abs_sum(xh, xl, wh, wl, up)
    K = taps(up, S.shape[0], S.shape[1]) * xh.shape[-1]
    return kv.sum_bound(S, 3 * K)


def split_gemm_rms_bound(xh, xl, wh, wl, up):
    """split_reference.split_gemm_rms_bound, per group of outputs with one K (the whole map | each sub-pixel phase):
    [(mask [Ho, Wo], bound)]"""
    S = abs_sum(xh, xl, wh, wl, up)
    t = taps(up, S.shape[0], S.shape[1])[..., 0]
    out = []
    for n in sorted(set(t.flatten().tolist())):
        m = t == n
        out.append((m, (3 * n * xh.shape[-1]) ** 0.5 * 2.0 ** -24 * S[m].pow(2).mean().sqrt().item()))
    return out


def split_direct_bound(x, w, b, up):
    """|y - exact| for the whole layer, S = |x| (*) |w|:
      * the split: SPLIT_TERM * S (split_reference: the dropped lo * lo and the two roundings of each operand);
      * the accumulation: 3K exact products, |hi| <= (1 + 2^-9) |v| and |lo| <= 2^-9 |v|, so their absolute sum is within
        (1 + 2^-9)^2 + 2^-8 < 1 + 2^-7 of S; the bias is one more term: sum_bound((1 + 2^-7) S + |b|, 3K + 1)."""
    z = torch.zeros_like(b, dtype=torch.float64)
    S = conv64(x.abs(), w.abs(), z, up)
    K = taps(up, S.shape[0], S.shape[1]) * x.shape[-1]
    return kv.sum_bound((1 + 2.0 ** -7) * S + b.double().abs(), 3 * K + 1) + sr.SPLIT_TERM * S


def taps_in_range(H, W, up):
    """taps whose input pixel lies inside the H x W map, per output pixel [Ho, Wo]: the conv of ones with ones"""
    one = torch.ones(H, W, 1)
    w = torch.ones(1, 1, 3, 3)
    return conv64(one, w, torch.zeros(1), up)[..., 0]


# ---- the kernel census of libt2v_split.so (tests/test_cpu_split_direct_library.py): every instantiation -> the tests that pin
# it, in the form of kernel_variants.TABLE, whose census covers libt2v_hip.so
_T = "tests/test_gpu_split_direct.py::"
SPLIT_LIBRARY_TABLE = {
    # t2v_split_launch_conv: <true> with a statistics buffer (the whole-conv test), <false> without (emulation, padding)
    "t2v::conv_igemm_split_kernel<false>":
        kv.Existing((_T + "test_conv_against_the_emulation_of_its_own_operands", _T + "test_zero_padding_is_exact_on_ones",)),
    "t2v::conv_igemm_split_kernel<true>":
        kv.Existing((_T + "test_whole_conv_against_float64",)),
    # the packed weights in place, the single-layer entry's input into its workspace
    "t2v::split_pairs_kernel":
        kv.Existing((_T + "test_packed_weights_are_the_pair_layout_of_the_fp32_packing", _T + "test_split_pass_of_the_single_layer_entry",)),
    "t2v::inorm_apply_split_kernel":
        kv.Existing((_T + "test_split_emitting_apply_pass_is_the_pair_layout_of_the_fp32_pass",
                     _T + "test_generator_outer_scope_against_the_float64_oracle",)),
}
