"""Float64 emulation of the split-bf16 arithmetic of T2V_ALGO_WINOGRAD_F4_BF16X2 (text2video_amd/csrc/winograd_split.hip), the
definition every layer and test shares:

    hi = bf16_rne(v),  lo = bf16_rne(v - float(hi))          (the subtraction is exact in fp32)
    contraction over K:  sum_k (ah*bh + ah*bl + al*bh), al*bl dropped; every product of two bf16 values is exact in fp32

The split is torch's `.bfloat16()` (round to nearest even).  Bounds:
  * against the emulation on the kernel's own planes: the GPU accumulates the 3K exact products in fp32 in an order of its
    own, so |got - emu| <= sum_bound(|ah||bh|^T + |ah||bl|^T + |al||bh|^T, 3K) (kernel_variants.sum_bound) for every
    element, and rms(got - emu) <= sqrt(3K) 2^-24 rms of that absolute sum per position (split_gemm_rms_bound);
  * of the emulation against the exact product: |v - hi - lo| <= 2^-18 |v| (two roundings of 2^-9), so the three dropped or
    rounded terms are within (2 * 2^-18 + 2^-18 + O(2^-27)) |a||b| per product: SPLIT_TERM = 3.5 * 2^-18 of |a| . |b|^T.
"""
import torch

import kernel_variants as kv

SPLIT_TERM = 3.5 * 2.0 ** -18


def split(v):
    """fp32 tensor -> (hi, lo) as fp32 tensors holding bf16 values"""
    v = v.float()
    hi = v.bfloat16().float()
    lo = (v - hi).bfloat16().float()
    return hi, lo


def split_planes_i16(v):
    """fp32 tensor -> int16 tensor [2, *v.shape]: the bit patterns of the hi and lo planes as the kernels store them"""
    hi, lo = split(v)
    return torch.stack([hi.bfloat16().view(torch.int16), lo.bfloat16().view(torch.int16)])


def planes_to_float(p):
    """int16 planes [2, ...] -> (hi, lo) fp32"""
    return p[0].view(torch.bfloat16).float(), p[1].view(torch.bfloat16).float()


def bmm_t(a, b):
    return torch.bmm(a.double(), b.double().transpose(1, 2))


def split_gemm64(ah, al, bh, bl, drop=None):
    """M[pos][t][n] = sum_k (ah bh + ah bl + al bh) in float64; planes [pos][T][K] and [pos][N][K].
    drop (fault injection): "product" leaves al*bh out."""
    m = bmm_t(ah, bh) + bmm_t(ah, bl)
    return m if drop == "product" else m + bmm_t(al, bh)


def _abs_sum(ah, al, bh, bl):
    return bmm_t(ah.abs(), bh.abs()) + bmm_t(ah.abs(), bl.abs()) + bmm_t(al.abs(), bh.abs())


def split_gemm_bound(ah, al, bh, bl, K):
    """fp32 accumulation of the 3K exact products: sum_bound over their absolute sum"""
    return kv.sum_bound(_abs_sum(ah, al, bh, bl), 3 * K)


def rms(t):
    """root mean square over everything but the leading (position) axis"""
    return t.double().pow(2).mean(dim=tuple(range(1, t.dim()))).sqrt()


def split_gemm_rms_bound(ah, al, bh, bl, K):
    """The typical-case companion of split_gemm_bound, per position: rms over the outputs of |got - emu|.  The products are
    exact, so the deviation is the roundings of at most 3K fp32 additions; each is at most half an ulp of a partial sum,
    2^-24 |partial|, and every partial sum, in whatever order, is at most the absolute sum S of the element's terms.
    Roundings of distinct additions are independent and of either sign, so they add in quadrature:
        rms(got - emu) <= sqrt(3K) * 2^-24 * rms(S).
    The worst-case bound grows as K * S and cannot tell a missing lo product (2^-9 of a random sum, ~sqrt(K)) from rounding
    beyond one K stage; this one grows as sqrt(K) * S and can (tests/test_cpu_split_bf16.py)."""
    return (3 * K) ** 0.5 * 2.0 ** -24 * rms(_abs_sum(ah, al, bh, bl))


def split_pipeline_bound(x, w, b, pad=1, reflect=True):
    """kernel_variants.pipeline_bound for "F4" with the GEMM stage in split arithmetic: the fp32 accumulation is 3K terms
    deep instead of K, and the split itself adds SPLIT_TERM |V| |U|^T; both are carried through |A^T| . |A| like every
    other part of e_M.  Input, weight and output transform terms are the fp32 pipeline's."""
    H, W, C = x.shape
    mats = kv.F4
    AV, TH, TW = kv.wino_input64(x.double().abs(), H, W, pad, reflect, m=4, BT=mats["kBT"].abs())
    AU = kv.weight64(w.abs(), mats["kG"].abs())
    BT, AT = mats["kBT"], mats["kAT"]
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    eU = kv.U * AU
    nB, nA = kv.nnz_rows(BT), kv.nnz_rows(AT)
    eV = kv.gamma(2 * nB) * AV
    AM = kv.gemm64(AV, AU)
    full = kv.gemm64(AV + eV, AU + eU)
    eM = kv.sum_bound(full, 3 * C) + SPLIT_TERM * full + kv.gemm64(eV, AU) + kv.gemm64(AV, eU) + kv.gemm64(eV, eU)
    zb = torch.zeros(AU.shape[1], dtype=torch.float64)
    _, aM = kv.output64(eM, AT.abs(), TH, TW, Ho, Wo, zb)
    _, aY = kv.output64(AM, AT.abs(), TH, TW, Ho, Wo, b.double().abs())
    return aM * (1 + kv.gamma(2 * nA + 1)) + kv.gamma(2 * nA + 1) * aY
