"""Float64 emulation and bounds of T2V_ALGO_POLYPHASE_BF16X2 (text2video_amd/csrc/polyphase_split.hip): the polyphase F(4,2)
pipeline of kernel_variants with its 81 GEMMs in the split-bf16 arithmetic of split_reference.

    V = fp32(B d B^T), U = fp32(G g G^T)        the fp32 pipeline's transforms, rounded as the kernels round them
    (vh, vl) = split(V), (uh, ul) = split(U)    split_reference.split
    M = sum_k (vh uh + vh ul + vl uh)           split_reference.split_gemm64
    y = A M A^T + bias
"""
import torch

import kernel_variants as kv
import split_reference as sr


def geometry(H, W, up):
    """real tiles T, padded tile rows Tt, TH, TW, Ho, Wo of a polyphase layer on an H x W input map"""
    TH, TW = (-(-H // 4), -(-W // 4)) if up else (-(-(H // 2) // 4), -(-(W // 2) // 4))
    Ho, Wo = (2 * H, 2 * W) if up else (H // 2, W // 2)
    return TH * TW, kv.pad_tiles(TH * TW), TH, TW, Ho, Wo


def split_conv64(x, w, b, up):
    """the split polyphase conv of x [H, W, C] in float64 -> y [Ho, Wo, Cout]; w in torch layout (up: ConvTranspose2d's)"""
    H, W, _ = x.shape
    _, _, TH, TW, Ho, Wo = geometry(H, W, up)
    V, _, _ = kv.polyphase_input64(x.double(), H, W, up)
    Uw = kv.weight64(w, kv.PP["kGU" if up else "kGD"], transposed_layout=up)
    (vh, vl), (uh, ul) = sr.split(V.float()), sr.split(Uw.float())
    M = sr.split_gemm64(vh, vl, uh, ul)
    return kv.output64(M, kv.PP["kAU" if up else "kAD"], TH, TW, Ho, Wo, b)[0]


def split_pipeline_bound(x, w, b, up):
    """kernel_variants.pipeline_bound("down" | "up") with the GEMM stage in split arithmetic, as
    split_reference.split_pipeline_bound does for F(4x4,3x3): the fp32 accumulation is 3K terms deep instead of K and the split
    adds SPLIT_TERM |V| |U|^T; input, weight and output transform terms are the fp32 pipeline's."""
    H, W, C = x.shape
    AV, TH, TW = kv.polyphase_input64(x.double().abs(), H, W, up, absolute=True)
    AU = kv.weight64(w.abs(), kv.PP["kGU" if up else "kGD"].abs(), transposed_layout=up)
    BT, AT = kv.PP["kBU" if up else "kBD"], kv.PP["kAU" if up else "kAD"]
    Ho, Wo = (2 * H, 2 * W) if up else (H // 2, W // 2)
    eU = kv.U * AU
    nB, nA = kv.nnz_rows(BT), kv.nnz_rows(AT)
    eV = kv.gamma(2 * nB) * AV
    AM = kv.gemm64(AV, AU)
    full = kv.gemm64(AV + eV, AU + eU)
    eM = kv.sum_bound(full, 3 * C) + sr.SPLIT_TERM * full + kv.gemm64(eV, AU) + kv.gemm64(AV, eU) + kv.gemm64(eV, eU)
    zb = torch.zeros(AU.shape[1], dtype=torch.float64)
    _, aM = kv.output64(eM, AT.abs(), TH, TW, Ho, Wo, zb)
    _, aY = kv.output64(AM, AT.abs(), TH, TW, Ho, Wo, b.double().abs())
    return aM * (1 + kv.gamma(2 * nA + 1)) + kv.gamma(2 * nA + 1) * aY


def conv64(x, w, b, up):
    """the exact layer in float64: F.conv2d(stride 2, pad 1) | F.conv_transpose2d(3, 2, 1, output_padding 1) -> [Ho, Wo, Cout]"""
    import torch.nn.functional as F
    xd = x.double().permute(2, 0, 1)[None]
    if up:
        y = F.conv_transpose2d(xd, w.double(), b.double(), stride=2, padding=1, output_padding=1)
    else:
        y = F.conv2d(xd, w.double(), b.double(), stride=2, padding=1)
    return y[0].permute(1, 2, 0)
