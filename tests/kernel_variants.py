"""Which test reaches which compiled kernel instantiation, and the float64 yardstick those tests use.

A plain helper module (no fixtures, no pytest hooks), imported by tests/test_cpu_kernel_variants.py and
tests/test_gpu_kernel_variants.py.

TABLE maps every `t2v::` kernel instantiation of libt2v_hip.so (the `__device_stub__` symbols, names normalised by
normalise()) to one of
  * Cases(...)       the ids of CONV_CASES below -- tests/test_gpu_kernel_variants.py runs each one, asserts with the
                     profiler that exactly this instantiation of its family ran, and compares with float64 elementwise;
  * Existing(...)    node ids of tests that compare this instantiation's own output, at operator level, with a
                     reference (torch / autograd / float64 / an exact identity).  Those in tests/test_gpu_kernel_variants.py
                     also assert with the profiler that the kernel ran; the others were seen to launch it in a profiled
                     run of the suite.  Bit-for-bit twins and end-to-end frame or train-step tests do not count;
  * Uncovered(...)   a reachable instantiation with no such test yet -- said plainly, not presented as covered.  Most are
                     forms of the Winograd / polyphase pipelines, which still want pinned float64 cases with the
                     transform-pipeline bound;
  * Unreachable(...) a reason read off the dispatch code (launch_pad, launch_conv_igemm, build_conv_plan,
                     run_conv_batch) for why no call selects the instantiation.
"""
import collections
import math
import re

import torch
import torch.nn.functional as F

U = 2.0 ** -24          # unit roundoff of fp32
TINY_PER_TERM = 2.0 ** -126   # a flushed subnormal product or partial sum
# A K-term sum evaluated as fma chains and pairwise partial sums in any order satisfies |fl(s) - s| <= gamma_n * sum|t_i|
# with n the longest chain of roundings a term goes through (<= K) and gamma_n = n u / (1 - n u) <= 1.01 n u while
# n u <= 0.01.  If the matrix core rounds each product before it adds it (no fused multiply-add), every term meets two
# roundings: gamma_2K <= 2.02 K u.  C_DIRECT covers that case; K counts the bias as one more term.
C_DIRECT = 2.1


def normalise(name):
    """'void t2v::f<t2v::T<1, 2>, 3>(t2v::P)' -> 't2v::f<t2v::T<1,2>,3>': no 'void ', no argument list, no whitespace;
    '__device_stub__' removed (nm's host-side stub names)."""
    name = name.replace("__device_stub__", "").strip()
    if name.startswith("void "):
        name = name[5:]
    depth = 0
    for i, ch in enumerate(name):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            name = name[:i]
            break
    return re.sub(r"\s+", "", name)


def family(name):
    """'t2v::conv_igemm_kernel<...>' -> 'conv_igemm_kernel'"""
    return normalise(name).split("<")[0].split("::")[-1]


# ---- conv_igemm_kernel<Cfg, MODE, STATS, REFLECT, RING> ----------------------------------------------------------------
TILE_CFG = {"L": "t2v::TileCfg<32,2,2,2,2>",    # 128 x 128
            "Q": "t2v::TileCfg<32,2,2,1,1>",    # 64 x 64
            "S": "t2v::TileCfg<16,4,1,4,1>"}    # 256 x 16


def igemm(cfg, mode, stats, reflect, ring):
    return "t2v::conv_igemm_kernel<%s,%d,%s,%s,%d>" % (TILE_CFG[cfg], mode, str(bool(stats)).lower(),
                                                      str(bool(reflect)).lower(), ring)


def stem(cs, nt, cr):
    return "t2v::conv_stem7x7_kernel<%d,%d,%d>" % (cs, nt, cr)


def head(cpl):
    return "t2v::conv_head7x7_strip_kernel<%d>" % cpl


def cout1(ks, cpl):
    return "t2v::conv_cout1_kernel<%d,%d>" % (ks, cpl)


ConvCase = collections.namedtuple(
    "ConvCase", "id H W Cin Cout k stride pad reflect transposed stats batch op offset expect note")


def _case(id, H, W, Cin, Cout, k, stride, pad, reflect, transposed, stats, expect, batch=1, op=None, offset=0.0, note=""):
    if op is None:
        op = 1 if transposed else 0
    return ConvCase(id, H, W, Cin, Cout, k, stride, pad, reflect, transposed, stats, batch, op, offset, expect, note)


def x_cs(case):
    return (case.Cin + 3) // 4 * 4


def taps(case):
    """products per output channel and input channel: all k*k taps of a direct conv, the largest sub-pixel phase of a
    stride-2 transposed conv (ceil(k/2)^2)"""
    return ((case.k + 1) // 2) ** 2 if case.transposed else case.k * case.k


def k_stages(case):
    """K stages (32 packed K elements each) of the implicit-GEMM kernel: one value, or one per transposed phase"""
    cs = x_cs(case)
    if not case.transposed:
        return [-(-case.k * case.k * cs // 32)]
    per_axis = [(case.k + 1 - p) // 2 for p in (0, 1)] if case.k == 3 else [2, 2]
    return sorted({-(-a * b * cs // 32) for a in per_axis for b in per_axis})


# The kernel each case must select is written out, not derived: the profiler check then catches a dispatch rule that moved.
# Blocks = tiles per phase x phases x batch.  Rings (launch_pad): 128x128 tiles take 2 slots from 1024 blocks, or above 256
# blocks with one phase; 64x64 tiles take 2 slots with one phase or from 4096 blocks; the 256x16 tile always 3.
# nk = packed K / 32: {1, 2, RING, RING + 1} appear for every reachable ring.  "mod8" notes the tile count mod 8 (XCD bands).
CONV_CASES = [
    # --- 128x128 tiles (Cout > 64; 205..256 single-phase blocks keep them, launch_pad: 3 slots; 257+: 2 slots) ---
    _case("L0_zero_k2p1_nk4_r3", 130, 206, 32, 96, 2, 1, 1, False, False, False, igemm("L", 0, 0, 0, 3),
          note="212 tiles (mod8 4), N tail 96/128, nk = RING + 1"),
    _case("L0_zero_1x1_nk1_r3", 150, 180, 32, 128, 1, 1, 0, False, False, False, igemm("L", 0, 0, 0, 3),
          note="211 tiles (mod8 3), nk 1"),
    _case("L0_zero_1x1_nk2_b2_r2", 150, 180, 64, 128, 1, 1, 0, False, False, False, igemm("L", 0, 0, 0, 2), batch=2,
          note="2 x 211 blocks crosses 256: 2 slots; nk 2 = RING"),
    _case("L0_zero_1x1_nk3_512t_r2", 256, 256, 96, 70, 1, 1, 0, False, False, False, igemm("L", 0, 0, 0, 2),
          note="512 tiles in one image, Cout % 4 != 0, nk 3 = RING + 1"),
    _case("L0_zero_convT_odd_768b_r3", 128, 192, 32, 96, 3, 2, 1, False, True, False, igemm("L", 0, 0, 0, 3), op=0,
          note="transposed, odd 255x383 output (masked store), 4 x 192 blocks < 1024"),
    _case("L0_reflect_k2p1_nk4_r3", 130, 206, 32, 96, 2, 1, 1, True, False, False, igemm("L", 0, 0, 1, 3)),
    _case("L0_reflect_1x1p1_b2_r2", 148, 178, 32, 128, 1, 1, 1, True, False, False, igemm("L", 0, 0, 1, 2), batch=2),
    _case("L0_stats_1x1_nk2_offset_r3", 150, 180, 64, 96, 1, 1, 0, False, False, True, igemm("L", 0, 1, 0, 3),
          offset=100.0, note="input mean 100, std 1"),
    _case("L0_stats_k2p1_b2_r2", 150, 180, 32, 128, 2, 1, 1, False, False, True, igemm("L", 0, 1, 0, 2), batch=2),
    _case("L0_stats_convT_b2_r2", 128, 192, 32, 96, 3, 2, 1, False, True, True, igemm("L", 0, 1, 0, 2), batch=2,
          note="4 phases x 192 x 2 = 1536 blocks"),
    _case("L0_stats_convT_768b_r3", 128, 192, 32, 128, 3, 2, 1, False, True, True, igemm("L", 0, 1, 0, 3)),
    _case("L0_stats_reflect_k2p1_nk4_r3", 130, 206, 32, 96, 2, 1, 1, True, False, True, igemm("L", 0, 1, 1, 3)),
    _case("L0_stats_reflect_1x1p1_512t_r2", 254, 254, 32, 128, 1, 1, 1, True, False, True, igemm("L", 0, 1, 1, 2)),
    _case("L1_zero_k3_nk2_r3", 130, 207, 4, 96, 3, 1, 1, False, False, False, igemm("L", 1, 0, 0, 3),
          note="211 tiles, Cin 4: nk 2"),
    _case("L1_zero_k3_nk2_b2_r2", 130, 207, 4, 96, 3, 1, 1, False, False, False, igemm("L", 1, 0, 0, 2), batch=2),
    _case("L1_reflect_k3_nk3_r3", 130, 207, 8, 96, 3, 1, 1, True, False, False, igemm("L", 1, 0, 1, 3),
          note="Cin 8: nk 3 = RING"),
    _case("L1_reflect_k3_nk3_b2_r2", 130, 207, 8, 100, 3, 1, 1, True, False, False, igemm("L", 1, 0, 1, 2), batch=2,
          note="nk 3 = RING + 1"),
    _case("L1_stats_1x1_nk1_r3", 150, 180, 4, 96, 1, 1, 0, False, False, True, igemm("L", 1, 1, 0, 3)),
    _case("L1_stats_s2_odd_b2_r2", 301, 361, 4, 128, 3, 2, 1, False, False, True, igemm("L", 1, 1, 0, 2), batch=2,
          note="stride 2 on an odd input: 151 x 181"),
    _case("L1_stats_reflect_k3_offset_r3", 130, 207, 4, 96, 3, 1, 1, True, False, True, igemm("L", 1, 1, 1, 3),
          offset=100.0),
    _case("L1_stats_reflect_k3_nk4_b2_r2", 130, 207, 12, 96, 3, 1, 1, True, False, True, igemm("L", 1, 1, 1, 2), batch=2,
          note="Cin 12: nk 4"),
    _case("L2_convT_odd_r3", 128, 192, 4, 96, 3, 2, 1, False, True, False, igemm("L", 2, 0, 0, 3), op=0),
    _case("L2_convT_b2_r2", 128, 192, 4, 96, 3, 2, 1, False, True, False, igemm("L", 2, 0, 0, 2), batch=2),
    _case("L2_stats_convT_nk124_r3", 128, 192, 28, 96, 3, 2, 1, False, True, True, igemm("L", 2, 1, 0, 3),
          note="Cin 28: the phases have nk 1, 2, 2, 4"),
    _case("L2_stats_convT_b2_r2", 128, 192, 8, 128, 3, 2, 1, False, True, True, igemm("L", 2, 1, 0, 2), batch=2),
    # --- 64x64 tiles (Cout <= 64, or 128x128 tiles that would fill the chip poorly) ---
    _case("Q0_zero_s2_odd", 33, 47, 32, 40, 3, 2, 1, False, False, False, igemm("Q", 0, 0, 0, 2),
          note="7 tiles, N tail 40/64"),
    _case("Q0_zero_k4s2p2_disc", 16, 16, 64, 64, 4, 2, 2, False, False, False, igemm("Q", 0, 0, 0, 2),
          note="the discriminators' geometry"),
    _case("Q0_zero_convT_odd_r3", 7, 9, 32, 36, 3, 2, 1, False, True, False, igemm("Q", 0, 0, 0, 3), op=0),
    _case("Q0_zero_convT_k4s2p2_r3", 9, 9, 32, 64, 4, 2, 2, False, True, False, igemm("Q", 0, 0, 0, 3), op=0,
          note="data gradient of a discriminator layer: 16x16 output"),
    _case("Q0_reflect_min_h2", 2, 37, 32, 64, 3, 1, 1, True, False, False, igemm("Q", 0, 0, 1, 2),
          note="H = pad + 1"),
    _case("Q0_reflect_fallback_cout128", 12, 20, 64, 128, 3, 1, 1, True, False, False, igemm("Q", 0, 0, 1, 2),
          note="4 blocks of 128x128 fill the chip poorly: 64x64 tiles, 8 tiles (mod8 0), nk 18"),
    _case("Q0_stats_k2p1_nk4", 24, 29, 32, 64, 2, 1, 1, False, False, True, igemm("Q", 0, 1, 0, 2)),
    _case("Q0_stats_convT_r3", 10, 13, 32, 64, 3, 2, 1, False, True, True, igemm("Q", 0, 1, 0, 3)),
    _case("Q0_stats_reflect_offset", 20, 23, 32, 48, 3, 1, 1, True, False, True, igemm("Q", 0, 1, 1, 2), offset=100.0,
          note="N tail 48/64"),
    _case("Q0_stats_reflect_b3", 9, 11, 32, 64, 3, 1, 1, True, False, True, igemm("Q", 0, 1, 1, 2), batch=3),
    _case("Q1_zero_s2_odd_cout30", 35, 41, 4, 30, 3, 2, 1, False, False, False, igemm("Q", 1, 0, 0, 2),
          note="Cout % 4 != 0"),
    _case("Q1_zero_k3_nk4_b2", 17, 19, 12, 64, 3, 1, 1, False, False, False, igemm("Q", 1, 0, 0, 2), batch=2),
    _case("Q1_reflect_min_h2_nk3", 2, 70, 8, 24, 3, 1, 1, True, False, False, igemm("Q", 1, 0, 1, 2)),
    _case("Q1_stats_1x1_nk1", 40, 40, 4, 64, 1, 1, 0, False, False, True, igemm("Q", 1, 1, 0, 2)),
    _case("Q1_stats_reflect_nk4_offset", 33, 17, 12, 64, 3, 1, 1, True, False, True, igemm("Q", 1, 1, 1, 2), offset=100.0),
    _case("Q2_convT_odd_r3", 9, 11, 4, 32, 3, 2, 1, False, True, False, igemm("Q", 2, 0, 0, 3), op=0),
    _case("Q2_convT_b15_3840b_r3", 64, 64, 4, 32, 3, 2, 1, False, True, False, igemm("Q", 2, 0, 0, 3), batch=15,
          note="4 phases x 64 tiles x 15 = 3840 blocks < 4096"),
    _case("Q2_convT_b16_4096b_r2", 64, 64, 4, 32, 3, 2, 1, False, True, False, igemm("Q", 2, 0, 0, 2), batch=16,
          note="4096 blocks: 2 slots"),
    _case("Q2_convT_k4s2p2_r3", 9, 9, 8, 64, 4, 2, 2, False, True, False, igemm("Q", 2, 0, 0, 3), op=0),
    _case("Q2_stats_convT_nk124_r3", 8, 12, 28, 64, 3, 2, 1, False, True, True, igemm("Q", 2, 1, 0, 3)),
    _case("Q2_stats_convT_b16_r2", 64, 64, 8, 32, 3, 2, 1, False, True, True, igemm("Q", 2, 1, 0, 2), batch=16),
    # --- 256x16 tiles (Cout <= 16, no statistics) ---
    _case("S0_zero_s2_odd", 21, 15, 32, 8, 3, 2, 1, False, False, False, igemm("S", 0, 0, 0, 3)),
    _case("S0_zero_b2", 20, 30, 32, 16, 1, 1, 0, False, False, False, igemm("S", 0, 0, 0, 3), batch=2),
    _case("S0_reflect_cout6", 20, 30, 64, 6, 3, 1, 1, True, False, False, igemm("S", 0, 0, 1, 3)),
    _case("S1_zero_k4s2p2_cout2", 16, 16, 4, 2, 4, 2, 2, False, False, False, igemm("S", 1, 0, 0, 3)),
    _case("S1_reflect_k7_cin12_min_h4", 4, 9, 12, 3, 7, 1, 3, True, False, False, igemm("S", 1, 0, 1, 3),
          note="the head geometry with Cin 12 (no multiple of 16: not the head kernel), H = pad + 1"),
    _case("S2_convT_odd_cout3", 11, 6, 8, 3, 3, 2, 1, False, True, False, igemm("S", 2, 0, 0, 3), op=0),
    # --- 7x7 stems (conv_stem.hip; statistics requested): <storage, Cout / 32, real channels the K loop skips to> ---
    _case("stem_cs12_cin9_c64", 17, 33, 9, 64, 7, 1, 3, True, False, True, stem(12, 2, 9)),
    _case("stem_cs12_cin9_c128_offset", 16, 16, 9, 128, 7, 1, 3, True, False, True, stem(12, 4, 9), offset=100.0),
    _case("stem_cs12_cin11_c64", 20, 19, 11, 64, 7, 1, 3, True, False, True, stem(12, 2, 12)),
    _case("stem_cs12_cin12_c128", 16, 35, 12, 128, 7, 1, 3, True, False, True, stem(12, 4, 12)),
    _case("stem_cs8_cin6_c64", 33, 16, 6, 64, 7, 1, 3, True, False, True, stem(8, 2, 6)),
    _case("stem_cs8_cin6_c128", 18, 18, 6, 128, 7, 1, 3, True, False, True, stem(8, 4, 6)),
    _case("stem_cs8_cin7_c64", 16, 17, 7, 64, 7, 1, 3, True, False, True, stem(8, 2, 8)),
    _case("stem_cs8_cin8_c128_offset", 31, 16, 8, 128, 7, 1, 3, True, False, True, stem(8, 4, 8), offset=100.0),
    # --- 7x7 heads (conv_head.hip; Cout <= 3, Cin storage a multiple of 16, no statistics) ---
    _case("head_cs128_cout3", 13, 21, 128, 3, 7, 1, 3, True, False, False, head(128)),
    _case("head_cs64_cout2_min_h4", 4, 4, 64, 2, 7, 1, 3, True, False, False, head(64), note="H = W = pad + 1"),
    _case("head_cs32_cout1", 9, 30, 32, 1, 7, 1, 3, True, False, False, head(0)),
    # --- one output channel, k4 p2 zero padding (conv_head.hip: a wave per output pixel) ---
    _case("cout1_cs256_s1", 9, 13, 256, 1, 4, 1, 2, False, False, False, cout1(4, 1)),
    _case("cout1_cs512_s2_odd", 17, 13, 512, 1, 4, 2, 2, False, False, False, cout1(4, 2)),
    _case("cout1_cs512_s1_3x3", 3, 3, 512, 1, 4, 1, 2, False, False, False, cout1(4, 2)),
]
CASE_BY_ID = {c.id: c for c in CONV_CASES}


# ---- float64 reference and the elementwise bound -------------------------------------------------------------------------
def case_tensors(case, seed=0):
    """fp32 input [B, Cin, H, W] (mean `offset`, std 1), weight, bias -- the values the GPU test uploads."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(case.batch, case.Cin, case.H, case.W, generator=g) + case.offset
    wshape = (case.Cin, case.Cout, case.k, case.k) if case.transposed else (case.Cout, case.Cin, case.k, case.k)
    w = torch.randn(*wshape, generator=g) * (1.0 / math.sqrt(case.Cin * taps(case)))
    b = torch.randn(case.Cout, generator=g) * 0.1
    return x, w, b


def conv64(case, x, w, b, pad_mode=None):
    """the case's convolution in float64 on the CPU; x [B, Cin, H, W] -> [B, Cout, Ho, Wo]"""
    x, w, b = x.double(), w.double(), b.double()
    reflect = case.reflect if pad_mode is None else pad_mode == "reflect"
    if case.transposed:
        return F.conv_transpose2d(x, w, b, stride=case.stride, padding=case.pad, output_padding=case.op)
    if case.pad > 0 and reflect:
        return F.conv2d(F.pad(x, (case.pad,) * 4, mode="reflect"), w, b, stride=case.stride)
    return F.conv2d(x, w, b, stride=case.stride, padding=case.pad)


def terms(case):
    """K: products accumulated per output (the largest count over outputs) plus the bias"""
    return taps(case) * case.Cin + 1


def depth(case):
    """the longest chain of roundings a product meets on its way to an output.  K (terms()) for the matrix-core kernels,
    whose order inside an MFMA is not specified.  The two VALU kernels' summation trees are read off conv_head.hip:
      conv_head7x7_strip_kernel: a lane's fma chain takes 2 of every 16 channels of all 49 taps (each wave a quarter of
        the channels, two lanes of a packed pair), then .x + .y, 4 wave partials added in turn, the bias: 49 Cin_s / 8 + 6;
      conv_cout1_kernel: each float4 component of a lane chains k*k * Cin_s / 256 products, then 2 adds over the
        components, 6 cross-lane shuffle adds, the bias: k*k * Cin_s / 256 + 9."""
    fam = family(case.expect)
    if fam == "conv_head7x7_strip_kernel":
        return 49 * x_cs(case) // 8 + 6
    if fam == "conv_cout1_kernel":
        return case.k * case.k * x_cs(case) // 256 + 9
    return terms(case)


def sum_bound(A, n, K=None, c=C_DIRECT):
    """|fl(s) - s| <= c u n A + K tiny for a sum of K terms whose absolute values sum to A, n roundings deep (n <= K)"""
    return c * U * n * A + (n if K is None else K) * TINY_PER_TERM


def bound(case, x, w, b, c=C_DIRECT):
    """elementwise |y - r| bound c u n A + K tiny: A = the same conv in float64 on |x|, |w|, |b|, n = depth() <= K"""
    return sum_bound(conv64(case, x.abs(), w.abs(), b.abs()), depth(case), terms(case), c)


def stats_bounds(r, bnd, parts):
    """Bounds for the instance-norm (mean, rstd) of one image's fp32 output, given its fp64 value r [C, Ho, Wo] and the
    elementwise bound bnd: the fp32 partials are tree sums over <= 256 pixels (depth 8), one two-pass M2 per block, and a
    combine over `parts` blocks; every level adds one rounding (depth d), so
      |mean - m| <= max(bnd) + d u mean|r|            (E_m)
      |var - v|  <= 2 sqrt(v) E + E^2 + d u v,  E = max(bnd) + E_m + 2 u max|r|   (the rounded block mean, subtracted)
      |rstd - s| <= s (|var - v| / (2 (v + eps)) + 4 u)."""
    d = 8 + 4 + math.ceil(math.log2(max(parts, 2))) + 2
    m = r.mean((1, 2))
    v = r.var((1, 2), unbiased=False)
    emax = bnd.flatten(1).max(1).values
    e_m = emax + d * U * r.abs().mean((1, 2))
    E = emax + e_m + 2 * U * r.abs().flatten(1).max(1).values
    e_v = 2 * v.sqrt() * E + E * E + d * U * v
    s = 1.0 / torch.sqrt(v + 1e-5)
    e_s = s * (e_v / (2 * (v + 1e-5)) + 4 * U)
    return m, s, e_m, e_s


# ---- the table ----------------------------------------------------------------------------------------------------------
Cases = collections.namedtuple("Cases", "ids")
Existing = collections.namedtuple("Existing", "nodeids")
Uncovered = collections.namedtuple("Uncovered", "reason")
Unreachable = collections.namedtuple("Unreachable", "reason")


_MODE2_REFLECT = ("MODE 2 means several phases, i.e. a transposed conv, and build_conv_plan gives transposed plans "
                  "T2V_PAD_ZERO only")
_Q_SINGLE_RING3 = ("64x64 tiles with one phase always take RING 2 in launch_pad (Cfg::BM == 64 && nphases == 1)")
_Q_REFLECT_RING3 = ("64x64 tiles take RING 3 only with several phases (transposed), and transposed plans are zero-padded")

# Written out entry by entry (a reviewer can diff it against `nm -C libt2v_hip.so | grep __device_stub__`).
_PIPELINE = ('a form of the Winograd / polyphase pipeline: exercised by operator and end-to-end tests, but no pinned float64 case with the transform-pipeline bound yet')

TABLE = {
    "t2v::accumulate_kernel":
        Existing(("tests/test_gpu_kernel_variants.py::test_layout_and_reduction_forms_against_float64",)),
    "t2v::act_backward_kernel":
        Existing(("tests/test_gpu_backward.py::test_pointwise_and_pooling_backward", "tests/test_gpu_backward.py::test_masked_l1_and_flow_head_activation_backward",)),
    "t2v::adam_kernel":
        Existing(("tests/test_gpu_train_pieces.py::test_fused_adam_matches_torch041_semantics",)),
    "t2v::adam_multi_kernel":
        Uncovered('compared with adam_kernel bit for bit and inside train-step oracle tests only; no float64 case of its own'),
    "t2v::add_kernel":
        Uncovered('no Python entry point; reached only inside generator frames compared end to end with the oracle'),
    "t2v::avgpool3s2_backward_kernel":
        Existing(("tests/test_gpu_backward.py::test_pointwise_and_pooling_backward",)),
    "t2v::avgpool3s2_kernel":
        Existing(("tests/test_gpu_ops.py::test_avgpool_count_include_pad_false",)),
    "t2v::bn_running_update_kernel":
        Existing(("tests/test_gpu_kernel_variants.py::test_scalar_channel_forms_against_float64",)),
    "t2v::channel_sum_final_kernel":
        Existing(("tests/test_gpu_backward.py::test_channel_sum_matches_a_float64_sum",)),
    "t2v::channel_sum_partial4_kernel":
        Existing(("tests/test_gpu_backward.py::test_channel_sum_matches_a_float64_sum",)),
    "t2v::channel_sum_partial_kernel":
        Existing(("tests/test_gpu_backward.py::test_channel_sum_matches_a_float64_sum",)),
    "t2v::conv_cout1_kernel<4,1>":
        Cases(("cout1_cs256_s1",)),
    "t2v::conv_cout1_kernel<4,2>":
        Cases(("cout1_cs512_s2_odd", "cout1_cs512_s1_3x3",)),
    "t2v::conv_head7x7_strip_kernel<0>":
        Cases(("head_cs32_cout1",)),
    "t2v::conv_head7x7_strip_kernel<128>":
        Cases(("head_cs128_cout3",)),
    "t2v::conv_head7x7_strip_kernel<64>":
        Cases(("head_cs64_cout2_min_h4",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<16,4,1,4,1>,0,false,false,3>":
        Cases(("S0_zero_s2_odd", "S0_zero_b2",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<16,4,1,4,1>,0,false,true,3>":
        Cases(("S0_reflect_cout6",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<16,4,1,4,1>,1,false,false,3>":
        Cases(("S1_zero_k4s2p2_cout2",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<16,4,1,4,1>,1,false,true,3>":
        Cases(("S1_reflect_k7_cin12_min_h4",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<16,4,1,4,1>,2,false,false,3>":
        Cases(("S2_convT_odd_cout3",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<16,4,1,4,1>,2,false,true,3>":
        Unreachable(_MODE2_REFLECT),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,0,false,false,2>":
        Cases(("Q0_zero_s2_odd", "Q0_zero_k4s2p2_disc",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,0,false,false,3>":
        Cases(("Q0_zero_convT_odd_r3", "Q0_zero_convT_k4s2p2_r3",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,0,false,true,2>":
        Cases(("Q0_reflect_min_h2", "Q0_reflect_fallback_cout128",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,0,false,true,3>":
        Unreachable(_Q_REFLECT_RING3),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,0,true,false,2>":
        Cases(("Q0_stats_k2p1_nk4",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,0,true,false,3>":
        Cases(("Q0_stats_convT_r3",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,0,true,true,2>":
        Cases(("Q0_stats_reflect_offset", "Q0_stats_reflect_b3",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,0,true,true,3>":
        Unreachable(_Q_REFLECT_RING3),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,1,false,false,2>":
        Cases(("Q1_zero_s2_odd_cout30", "Q1_zero_k3_nk4_b2",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,1,false,false,3>":
        Unreachable('64x64 tiles with one phase always take RING 2 in launch_pad (Cfg::BM == 64 && nphases == 1); MODE 1 is single-phase by definition'),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,1,false,true,2>":
        Cases(("Q1_reflect_min_h2_nk3",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,1,false,true,3>":
        Unreachable('64x64 tiles with one phase always take RING 2 in launch_pad (Cfg::BM == 64 && nphases == 1); MODE 1 is single-phase by definition'),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,1,true,false,2>":
        Cases(("Q1_stats_1x1_nk1",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,1,true,false,3>":
        Unreachable('64x64 tiles with one phase always take RING 2 in launch_pad (Cfg::BM == 64 && nphases == 1); MODE 1 is single-phase by definition'),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,1,true,true,2>":
        Cases(("Q1_stats_reflect_nk4_offset",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,1,true,true,3>":
        Unreachable('64x64 tiles with one phase always take RING 2 in launch_pad (Cfg::BM == 64 && nphases == 1); MODE 1 is single-phase by definition'),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,2,false,false,2>":
        Cases(("Q2_convT_b16_4096b_r2",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,2,false,false,3>":
        Cases(("Q2_convT_odd_r3", "Q2_convT_b15_3840b_r3", "Q2_convT_k4s2p2_r3",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,2,false,true,2>":
        Unreachable(_MODE2_REFLECT),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,2,false,true,3>":
        Unreachable(_MODE2_REFLECT),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,2,true,false,2>":
        Cases(("Q2_stats_convT_b16_r2",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,2,true,false,3>":
        Cases(("Q2_stats_convT_nk124_r3",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,2,true,true,2>":
        Unreachable(_MODE2_REFLECT),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,2,true,true,3>":
        Unreachable(_MODE2_REFLECT),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,2,2>,0,false,false,2>":
        Cases(("L0_zero_1x1_nk2_b2_r2", "L0_zero_1x1_nk3_512t_r2",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,2,2>,0,false,false,3>":
        Cases(("L0_zero_k2p1_nk4_r3", "L0_zero_1x1_nk1_r3", "L0_zero_convT_odd_768b_r3",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,2,2>,0,false,true,2>":
        Cases(("L0_reflect_1x1p1_b2_r2",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,2,2>,0,false,true,3>":
        Cases(("L0_reflect_k2p1_nk4_r3",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,2,2>,0,true,false,2>":
        Cases(("L0_stats_k2p1_b2_r2", "L0_stats_convT_b2_r2",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,2,2>,0,true,false,3>":
        Cases(("L0_stats_1x1_nk2_offset_r3", "L0_stats_convT_768b_r3",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,2,2>,0,true,true,2>":
        Cases(("L0_stats_reflect_1x1p1_512t_r2",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,2,2>,0,true,true,3>":
        Cases(("L0_stats_reflect_k2p1_nk4_r3",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,2,2>,1,false,false,2>":
        Cases(("L1_zero_k3_nk2_b2_r2",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,2,2>,1,false,false,3>":
        Cases(("L1_zero_k3_nk2_r3",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,2,2>,1,false,true,2>":
        Cases(("L1_reflect_k3_nk3_b2_r2",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,2,2>,1,false,true,3>":
        Cases(("L1_reflect_k3_nk3_r3",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,2,2>,1,true,false,2>":
        Cases(("L1_stats_s2_odd_b2_r2",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,2,2>,1,true,false,3>":
        Cases(("L1_stats_1x1_nk1_r3",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,2,2>,1,true,true,2>":
        Cases(("L1_stats_reflect_k3_nk4_b2_r2",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,2,2>,1,true,true,3>":
        Cases(("L1_stats_reflect_k3_offset_r3",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,2,2>,2,false,false,2>":
        Cases(("L2_convT_b2_r2",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,2,2>,2,false,false,3>":
        Cases(("L2_convT_odd_r3",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,2,2>,2,false,true,2>":
        Unreachable(_MODE2_REFLECT),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,2,2>,2,false,true,3>":
        Unreachable(_MODE2_REFLECT),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,2,2>,2,true,false,2>":
        Cases(("L2_stats_convT_b2_r2",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,2,2>,2,true,false,3>":
        Cases(("L2_stats_convT_nk124_r3",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,2,2>,2,true,true,2>":
        Unreachable(_MODE2_REFLECT),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,2,2>,2,true,true,3>":
        Unreachable(_MODE2_REFLECT),
    "t2v::conv_stem7x7_kernel<12,2,12>":
        Cases(("stem_cs12_cin11_c64",)),
    "t2v::conv_stem7x7_kernel<12,2,9>":
        Cases(("stem_cs12_cin9_c64",)),
    "t2v::conv_stem7x7_kernel<12,4,12>":
        Cases(("stem_cs12_cin12_c128",)),
    "t2v::conv_stem7x7_kernel<12,4,9>":
        Cases(("stem_cs12_cin9_c128_offset",)),
    "t2v::conv_stem7x7_kernel<8,2,6>":
        Cases(("stem_cs8_cin6_c64",)),
    "t2v::conv_stem7x7_kernel<8,2,8>":
        Cases(("stem_cs8_cin7_c64",)),
    "t2v::conv_stem7x7_kernel<8,4,6>":
        Cases(("stem_cs8_cin6_c128",)),
    "t2v::conv_stem7x7_kernel<8,4,8>":
        Cases(("stem_cs8_cin8_c128_offset",)),
    "t2v::conv_wgrad_kernel<false,16,4>":
        Existing(("tests/test_gpu_kernel_variants.py::test_direct_weight_gradient_against_float64",)),
    "t2v::conv_wgrad_kernel<true,16,4>":
        Existing(("tests/test_gpu_kernel_variants.py::test_direct_weight_gradient_against_float64",)),
    "t2v::copy_channels_kernel":
        Existing(("tests/test_gpu_kernel_variants.py::test_layout_and_reduction_forms_against_float64",)),
    "t2v::dispatch_order_kernel":
        Uncovered('the fixed-grid dispatch-order self-test run by t2v_create: it writes tickets, no numerical output'),
    "t2v::inorm_apply_kernel":
        Existing(("tests/test_gpu_ops.py::test_instance_norm_affine_residual_matches_trainmode_batchnorm", "tests/test_gpu_ops.py::test_instance_norm_large_mean_is_stable",)),
    "t2v::inorm_bwd_apply_kernel":
        Existing(("tests/test_gpu_backward.py::test_norm_backward_with_fused_activation",)),
    "t2v::inorm_bwd_final_kernel":
        Existing(("tests/test_gpu_backward.py::test_norm_backward_with_fused_activation",)),
    "t2v::inorm_bwd_reduce_kernel":
        Existing(("tests/test_gpu_backward.py::test_norm_backward_with_fused_activation",)),
    "t2v::inorm_finalize_kernel":
        Existing(("tests/test_gpu_ops.py::test_instance_norm_affine_residual_matches_trainmode_batchnorm", "tests/test_gpu_ops.py::test_instance_norm_large_mean_is_stable",)),
    "t2v::inorm_finalize_merge_kernel":
        Uncovered('reached only by full-size frames compared end to end with the oracle'),
    "t2v::loss_backward_kernel":
        Existing(("tests/test_gpu_backward.py::test_pointwise_and_pooling_backward",)),
    "t2v::loss_terms_final_kernel":
        Uncovered('reached only inside train steps compared end to end with the device oracle'),
    "t2v::loss_terms_kernel":
        Uncovered('reached only inside train steps compared end to end with the device oracle'),
    "t2v::masked_l1_backward_kernel":
        Existing(("tests/test_gpu_backward.py::test_masked_l1_and_flow_head_activation_backward",)),
    "t2v::maxpool2x2_backward_kernel":
        Existing(("tests/test_gpu_train_pieces.py::test_maxpool2x2_forward_backward_matches_torch",)),
    "t2v::maxpool2x2_kernel":
        Existing(("tests/test_gpu_train_pieces.py::test_maxpool2x2_forward_backward_matches_torch",)),
    "t2v::nchw_to_nhwc_kernel":
        Existing(("tests/test_gpu_ops.py::test_conv_with_norm_stats",)),
    "t2v::nhwc_to_nchw_kernel":
        Existing(("tests/test_gpu_kernel_variants.py::test_layout_and_reduction_forms_against_float64",)),
    "t2v::pack_convT_weight_kernel":
        Existing(("tests/test_gpu_backward.py::test_conv_data_gradient_via_adjoint_forward_conv",)),
    "t2v::pack_conv_weight_kernel":
        Existing(("tests/test_gpu_ops.py::test_conv_with_norm_stats",)),
    "t2v::pad_copy_kernel":
        Existing(("tests/test_gpu_backward.py::test_conv_weight_and_bias_gradient",)),
    "t2v::polyphase_input_kernel<false,false>":
        Uncovered(_PIPELINE),
    "t2v::polyphase_input_kernel<false,true>":
        Uncovered(_PIPELINE),
    "t2v::polyphase_input_kernel<true,false>":
        Uncovered(_PIPELINE),
    "t2v::polyphase_input_kernel<true,true>":
        Uncovered(_PIPELINE),
    "t2v::polyphase_output_down_kernel":
        Existing(("tests/test_gpu_ops.py::test_polyphase_winograd_matches_torch_and_the_direct_kernel",)),
    "t2v::polyphase_output_up_kernel":
        Existing(("tests/test_gpu_ops.py::test_polyphase_winograd_matches_torch_and_the_direct_kernel",)),
    "t2v::polyphase_weight_kernel<false>":
        Uncovered(_PIPELINE),
    "t2v::polyphase_weight_kernel<true>":
        Uncovered(_PIPELINE),
    "t2v::reduce_final_kernel":
        Existing(("tests/test_gpu_kernel_variants.py::test_layout_and_reduction_forms_against_float64",)),
    "t2v::reduce_masked_l1_kernel":
        Existing(("tests/test_gpu_backward.py::test_masked_l1_and_flow_head_activation_backward",)),
    "t2v::reduce_partial_kernel<0>":
        Existing(("tests/test_gpu_kernel_variants.py::test_layout_and_reduction_forms_against_float64",)),
    "t2v::reduce_partial_kernel<1>":
        Existing(("tests/test_gpu_kernel_variants.py::test_layout_and_reduction_forms_against_float64",)),
    "t2v::reflect_pad_backward_kernel<HIP_vector_type<float,4u>>":
        Existing(("tests/test_gpu_kernel_variants.py::test_layout_and_reduction_forms_against_float64",)),
    "t2v::reflect_pad_backward_kernel<float>":
        Existing(("tests/test_gpu_kernel_variants.py::test_scalar_channel_forms_against_float64",)),
    "t2v::scale_kernel":
        Existing(("tests/test_gpu_kernel_variants.py::test_scalar_channel_forms_against_float64",)),
    "t2v::to_u8_kernel":
        Existing(("tests/test_gpu_ops.py::test_pose_u8_and_tensor2im_roundtrip",)),
    "t2v::u8_pose_to_f32_kernel":
        Existing(("tests/test_gpu_ops.py::test_pose_u8_and_tensor2im_roundtrip",)),
    "t2v::unpack_convT_weight_kernel":
        Existing(("tests/test_gpu_backward.py::test_conv_weight_and_bias_gradient",)),
    "t2v::unpack_conv_weight_kernel":
        Existing(("tests/test_gpu_backward.py::test_conv_weight_and_bias_gradient",)),
    "t2v::unzip2_kernel":
        Existing(("tests/test_gpu_kernel_variants.py::test_layout_and_reduction_forms_against_float64",)),
    "t2v::warp_composite_backward_kernel":
        Existing(("tests/test_gpu_backward.py::test_flow_warp_composite_backward_matches_oracle_autograd",)),
    "t2v::warp_composite_kernel":
        Existing(("tests/test_gpu_ops.py::test_flow_warp_composite_vs_grid_sample",)),
    "t2v::wgrad_reduce_kernel":
        Existing(("tests/test_gpu_backward.py::test_conv_weight_and_bias_gradient",)),
    "t2v::wino_gemm_sk_kernel<t2v::TileCfg<32,1,4,5,1>,3,false>":
        Uncovered(_PIPELINE),
    "t2v::wino_gemm_sk_kernel<t2v::TileCfg<32,1,4,8,1>,3,false>":
        Uncovered(_PIPELINE),
    "t2v::wino_gemm_sk_kernel<t2v::TileCfg<32,2,2,2,2>,2,false>":
        Uncovered(_PIPELINE),
    "t2v::wino_gemm_sk_kernel<t2v::TileCfg<32,2,2,2,2>,2,true>":
        Uncovered(_PIPELINE),
    "t2v::wino_gemm_sk_kernel<t2v::TileCfg<32,2,2,3,1>,2,false>":
        Uncovered(_PIPELINE),
    "t2v::wino_gemm_skr_kernel<2>":
        Uncovered(_PIPELINE),
    "t2v::wino_gemm_skt_kernel<3>":
        Uncovered(_PIPELINE),
    "t2v::wino_wgrad_sk_kernel<16,4>":
        Uncovered('compared with the one-block-per-tile form bit for bit and inside train steps only'),
    "t2v::winograd4_dgrad_output_kernel<false>":
        Uncovered(_PIPELINE),
    "t2v::winograd4_dgrad_output_kernel<true>":
        Uncovered(_PIPELINE),
    "t2v::winograd4_dw_kernel":
        Existing(("tests/test_gpu_backward.py::test_weight_gradient_in_winograd_domain",)),
    "t2v::winograd4_dy_kernel<false>":
        Uncovered(_PIPELINE),
    "t2v::winograd4_dy_kernel<true>":
        Uncovered(_PIPELINE),
    "t2v::winograd4_input_kernel<0,false>":
        Uncovered(_PIPELINE),
    "t2v::winograd4_input_kernel<0,true>":
        Uncovered(_PIPELINE),
    "t2v::winograd4_input_kernel<1,false>":
        Uncovered(_PIPELINE),
    "t2v::winograd4_input_kernel<1,true>":
        Uncovered(_PIPELINE),
    "t2v::winograd4_input_kernel<2,false>":
        Uncovered(_PIPELINE),
    "t2v::winograd4_input_kernel<2,true>":
        Uncovered(_PIPELINE),
    "t2v::winograd4_output_kernel":
        Existing(("tests/test_gpu_ops.py::test_winograd_conv_matches_direct_and_reference",)),
    "t2v::winograd4_weight_adjoint_kernel<false>":
        Uncovered(_PIPELINE),
    "t2v::winograd4_weight_adjoint_kernel<true>":
        Uncovered(_PIPELINE),
    "t2v::winograd4_weight_kernel":
        Existing(("tests/test_gpu_ops.py::test_winograd_conv_matches_direct_and_reference",)),
    "t2v::winograd_input_kernel":
        Existing(("tests/test_gpu_ops.py::test_winograd_conv_matches_direct_and_reference",)),
    "t2v::winograd_output_kernel":
        Existing(("tests/test_gpu_ops.py::test_winograd_conv_matches_direct_and_reference",)),
    "t2v::winograd_weight_kernel":
        Existing(("tests/test_gpu_ops.py::test_winograd_conv_matches_direct_and_reference",)),
}
