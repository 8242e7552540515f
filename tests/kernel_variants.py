"""Which test reaches which compiled kernel instantiation, and the float64 yardstick those tests use.

A plain helper module (no fixtures, no pytest hooks), imported by tests/test_cpu_kernel_variants.py,
tests/test_gpu_kernel_variants.py and tests/test_gpu_pipeline_variants.py.

TABLE maps every `t2v::` kernel instantiation of libt2v_hip.so (the `__device_stub__` symbols, those of
`t2v::(anonymous namespace)::` included; names normalised by normalise()) to one of
  * Cases(...)       the ids of CONV_CASES or PIPE_CASES below -- tests/test_gpu_kernel_variants.py and
                     tests/test_gpu_pipeline_variants.py run each one, assert with the profiler that exactly this
                     instantiation of its family ran, and compare with float64 elementwise;
  * Existing(...)    node ids of tests that compare this instantiation's own output, at operator level, with a
                     reference (torch / autograd / float64 / an exact identity).  Those in tests/test_gpu_kernel_variants.py
                     also assert with the profiler that the kernel ran; the others were seen to launch it in a profiled
                     run of the suite.  Bit-for-bit twins and end-to-end frame or train-step tests do not count;
  * Uncovered(...)   a reachable instantiation with no such test yet -- said plainly, not presented as covered;
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
    '__device_stub__' removed (nm's host-side stub names).  Every '(anonymous namespace)::' component goes first of all (its
    '(' would otherwise be taken for the argument list): a kernel of `namespace t2v { namespace { ... } }` has the name
    't2v::f' whether nm spells it ('t2v::(anonymous namespace)::__device_stub__f(...)') or the profiler does."""
    name = name.replace("(anonymous namespace)::", "").replace("__device_stub__", "").strip()
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
    # Cin % 4 != 0 (x_cs > Cin: the pad K slots of every tap meet the storage lanes; tests/storage_lanes.py runs these
    # geometries with junk in the lanes)
    _case("Q1_stats_reflect_k3_cin3", 17, 19, 3, 64, 3, 1, 1, True, False, True, igemm("Q", 1, 1, 1, 2),
          note="Cin 3 -> storage 4: nk 2"),
    _case("Q1_stats_k4s2p2_cin6_disc", 16, 16, 6, 64, 4, 2, 2, False, False, True, igemm("Q", 1, 1, 0, 2),
          note="the discriminators' first layer: Cin 6 -> storage 8, nk 4"),
    _case("Q1_stats_k3s2_cin9_cout96", 33, 47, 9, 96, 3, 2, 1, False, False, True, igemm("Q", 1, 1, 0, 2),
          note="Cin 9 -> storage 12; Cout 96 asks for 128x128 tiles, 4 of them fill the chip poorly: 64x64, N tail 32/64"),
    _case("Q1_zero_s2_cin6_cout30", 35, 41, 6, 30, 3, 2, 1, False, False, False, igemm("Q", 1, 0, 0, 2),
          note="Cin 6 -> storage 8 and Cout 30 -> storage 32"),
    _case("Q2_convT_odd_r3", 9, 11, 4, 32, 3, 2, 1, False, True, False, igemm("Q", 2, 0, 0, 3), op=0),
    _case("Q2_stats_convT_cin5_r3", 9, 11, 5, 32, 3, 2, 1, False, True, True, igemm("Q", 2, 1, 0, 3),
          note="Cin 5 -> storage 8: the phases have nk 1, 1, 1, 1 with 1, 2, 2, 4 taps"),
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


# ---- the Winograd / polyphase pipelines: float64 stage references and their bounds ------------------------------------
# Each reference takes the fp32 buffers the kernel actually read (its own V, U, M, dV, dU out of the workspace) and returns
# the stage's output in float64; each bound is derived from the arithmetic the kernel does (winograd.hip, polyphase.hip,
# conv_igemm.hip, conv_wgrad.hip) and written next to its formula.  gamma(n) = n u / (1 - n u): a value that went through n
# roundings, each relative to what it rounded, is within gamma(n) of the exact result times the magnitudes it was formed
# from; chains compose as gamma(a) + gamma(b) + gamma(a) gamma(b) <= gamma(a + b).
import os

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "text2video_amd", "csrc")
TINY = 2.0 ** -149      # one flushed or subnormal result per rounding


def gamma(n):
    return n * U / (1 - n * U)


LEAKY32 = float(torch.tensor(0.2, dtype=torch.float32))    # the LeakyReLU slope as the kernels hold it: float32(0.2), not 0.2


def read_consts(path):
    """{name: float64 tensor} of the `constexpr double kX[r][c] = {...};` tables of a generated header"""
    src = open(path).read()
    out = {}
    for m in re.finditer(r"constexpr double (\w+)\[(\d+)\]\[(\d+)\] = \{(.*?)\};", src, re.S):
        name, r, c, body = m.group(1), int(m.group(2)), int(m.group(3)), m.group(4)
        vals = []
        for tok in re.findall(r"-?[\d.]+(?:\s*/\s*[\d.]+)?", body):
            num, _, den = tok.partition("/")
            vals.append(float(num) / (float(den) if den else 1.0))
        assert len(vals) == r * c, (name, len(vals))
        out[name] = torch.tensor(vals, dtype=torch.float64).view(r, c)
    return out


F4 = read_consts(os.path.join(_CSRC, "winograd_f4_consts.h"))          # kAT 4x6, kG 6x3, kBT 6x6
PP = read_consts(os.path.join(_CSRC, "polyphase_consts.h"))             # kBD 9x9, kGD 9x3, kAD 4x9, kBU 9x5, kGU 9x3, kAU 8x9
# F(2x2,3x3): written out in winograd.hip's comments and code, not in a header
F2 = {"kAT": torch.tensor([[1., 1., 1., 0.], [0., 1., -1., -1.]], dtype=torch.float64),
      "kG": torch.tensor([[1., 0., 0.], [.5, .5, .5], [.5, -.5, .5], [0., 0., 1.]], dtype=torch.float64),
      "kBT": torch.tensor([[1., 0., -1., 0.], [0., 1., 1., 0.], [0., -1., 1., 0.], [0., 1., 0., -1.]], dtype=torch.float64)}


def nnz_rows(m):
    """the longest cdot chain of a transform matrix applied row by row: its most nonzeros in one row (zero taps are skipped
    at compile time, winograd.hip: cdot)"""
    return int((m != 0).sum(1).max())


def pad_tiles(T):
    """wino_pad_tiles (t2v_internal.h): 64 or 128 multiple"""
    a, b = -(-T // 64) * 64, -(-T // 128) * 128
    return a if (b - a) * 8 >= b else b


def patch_index(n, tiles, step, size, start, reflect):
    """[tiles, size] source indices and validity of the patch rows (or columns) the input kernels read: row step*t - start + k;
    reflected as |i| then min(i, 2n - 2 - i) clamped at 0 (past the reflected border: a ragged tile's masked outputs), or
    zero outside [0, n)"""
    i = torch.arange(tiles)[:, None] * step - start + torch.arange(size)[None, :]
    if reflect:
        j = i.abs()
        return torch.clamp(torch.minimum(j, 2 * n - 2 - j), min=0), torch.ones_like(i, dtype=torch.bool)
    ok = (i >= 0) & (i < n)
    return i.clamp(0, n - 1), ok


def gather_patches(x, rows, cols):
    """x [H, W, C] -> [TH, P, TW, Q, C] patches (zeros where the index is not valid)"""
    (ry, oky), (rx, okx) = rows, cols
    d = x[ry.reshape(-1)][:, rx.reshape(-1)].view(ry.shape[0], ry.shape[1], rx.shape[0], rx.shape[1], x.shape[-1])
    m = (oky[:, :, None, None] & okx[None, None, :, :]).to(d.dtype)
    return d * m[..., None]


def transform_in(d, BL, BR=None):
    """V[p*Q'+q][tile][c] = (BL d BR^T)[p][q] of patches d [TH, P, TW, Q, C] -> [P' Q', TH TW, C]"""
    BR = BL if BR is None else BR
    v = torch.einsum("ia,jb,yaxbc->ijyxc", BL, BR, d)
    return v.reshape(BL.shape[0] * BR.shape[0], d.shape[0] * d.shape[2], d.shape[-1])


def wino_input64(x, H, W, pad, reflect, m=4, BT=None, d=None):
    """F(m x m, 3x3) input transform of x [H, W, C] (fp32 values) in float64: [pos][T][C] over the real tiles.  The tile grid
    covers the output (H + 2 pad - 2) x (W + 2 pad - 2); patch rows m*t - pad ... m*t - pad + m + 1.  d: the map the
    patches are cut from, if not x itself (the normalised map of the lazy modes)."""
    BT = (F4 if m == 4 else F2)["kBT"] if BT is None else BT
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    TH, TW = -(-Ho // m), -(-Wo // m)
    src = x if d is None else d
    p = gather_patches(src, patch_index(H, TH, m, m + 2, pad, reflect), patch_index(W, TW, m, m + 2, pad, reflect))
    return transform_in(p, BT), TH, TW


def input_bound(Aabs, n, e_d=None):
    """Input transform: two cdot levels (rows, then columns), each a chain of <= n roundings (the product by a dyadic
    constant and n - 1 additions): |V - V64| <= gamma(2n) |B^T| |d| |B| = gamma(2n) Aabs.  Lazy forms: d itself carries the
    elementwise error e_d of forming it in fp32, carried through |B^T| . |B| (transform_in of e_d, passed in already
    transformed) and rounded on the way: + (1 + gamma(2n)) e_d."""
    b = gamma(2 * n) * Aabs + 2 * n * TINY
    return b if e_d is None else b + (1 + gamma(2 * n)) * e_d


def lazy_d64(x, mean_rstd, gamma_=None, beta=None, relu=False, res=None, res2=None):
    """d = [act]((x - mean) * rstd [* gamma + beta]) [+ res] [+ res2] in float64 from the fp32 operands, and its elementwise
    error bound in fp32: x - mean (1 rounding), * rstd (2), * gamma (3), + beta (4), + res (5); each rounding is relative to
    the value it rounds, all of which are <= |x - mean| rstd |gamma| + |beta| (+ |res|); ReLU is 1-Lipschitz: e_d <= gamma(5)
    (that sum).  relu: 0 / False none, 1 / True ReLU, 2 LeakyReLU with the slope float32(0.2) the kernels multiply by (norm_act,
    transform_common.h) -- v > 0 ? v : slope v is 1-Lipschitz too, so a v and v64 on two sides of 0 differ after it by no more
    than before; the product by the slope is one more rounding, and the reference may as well take the slope as 0.2: the two
    differ by 7.5e-9 relative, inside one more u (gamma(7)).  A second residual is one more addition (+1).
    x [.., C], mean_rstd [C, 2]."""
    m, r = mean_rstd[:, 0].double(), mean_rstd[:, 1].double()
    t = (x.double() - m) * r
    mag = (x.double() - m).abs() * r
    n = 5
    if gamma_ is not None:
        t = t * gamma_.double() + beta.double()
        mag = mag * gamma_.double().abs() + beta.double().abs()
    if int(relu) == 1:
        t = t.clamp(min=0)
    elif int(relu) == 2:
        t = torch.where(t > 0, t, t * LEAKY32)
        n += 2
    if res is not None:
        t = t + res.double()
        mag = mag + res.double().abs()
    if res2 is not None:
        t = t + res2.double()
        mag = mag + res2.double().abs()
        n += 1
    return t, gamma(n) * mag + n * TINY


def weight64(w, G, transposed_layout=False, flip=False):
    """U[pos][n][c] = (G g G^T) of the torch-layout weight: w [Cout][Cin][3][3], or [Cin][Cout][3][3] (transposed_layout:
    the adjoint / ConvTranspose2d layouts, U[.][n][c] from w[c][n]); flip rotates each 3x3 by 180 degrees"""
    g = w.double()
    if transposed_layout:
        g = g.transpose(0, 1)
    if flip:
        g = g.flip(-1).flip(-2)
    u = torch.einsum("ia,jb,ncab->ijnc", G, G, g)
    return u.reshape(G.shape[0] ** 2, g.shape[0], g.shape[1])


def weight_bound(U64, Aabs):
    """F(4x4) and polyphase weight transforms run in fp64 and round once (winograd4_weight_store, polyphase_weight_kernel):
    |U - U64| <= u |U64| + 2^-149, plus the fp64 chain itself (<= 6 roundings of 2^-53 relative to |G| |g| |G^T| = Aabs)"""
    return U * U64.abs() + TINY + 8 * 2.0 ** -53 * Aabs


def weight_bound_f2(Aabs):
    """F(2x2) weight transform in fp32 (winograd_weight_kernel): per level 0.5 * (g0 + g1 + g2): 2 roundings (the halving is
    exact), two levels: gamma(4) |G| |g| |G^T|"""
    return gamma(4) * Aabs + 4 * TINY


def gemm64(V, Ub):
    """M[pos][t][n] = V[pos][t] . U[pos][n]^T in float64 (on V's device).  V [pos][T][K], Ub [pos][N][K]."""
    return torch.bmm(V.double(), Ub.double().transpose(1, 2))


def gemm_bound(V, Ub, K):
    """the batched GEMMs are K-term MFMA sums: sum_bound(|V| |U|^T, K) with C_DIRECT (conv_igemm.hip; the stream-K forms add
    one block's partial to another's, which is one more order of the same K terms)"""
    return sum_bound(torch.bmm(V.double().abs(), Ub.double().abs().transpose(1, 2)), K)


def output64(M, A, TH, TW, Ho, Wo, bias):
    """y = A M A^T + bias per tile, M [pos][T][N] (real tiles) -> y [Ho, Wo, N] (ragged tiles cropped); also returns the same
    on |M|, |bias| (the magnitude the bound scales)"""
    e, k = A.shape
    N = M.shape[-1]
    m = M.double().view(k, k, TH, TW, N)
    y = torch.einsum("ia,jb,abyxn->yixjn", A, A, m).reshape(TH * e, TW * e, N)[:Ho, :Wo] + bias.double()
    a = torch.einsum("ia,jb,abyxn->yixjn", A.abs(), A.abs(), m.abs()).reshape(TH * e, TW * e, N)[:Ho, :Wo] + bias.double().abs()
    return y, a


def output_bound(Aabs, n, slope=None):
    """output transform: two cdot levels of <= n roundings, then + bias: gamma(2n + 1) (|A| |M| |A^T| + |bias|).
    With the LeakyReLU of winograd4_output_kernel (v < 0 ? v * slope : v, slope <= 1: 1-Lipschitz, so a v and v64 on two
    sides of 0 differ after it by no more than before) the product by the slope is one more rounding: gamma(2n + 2)."""
    k = 2 * n + 1 if slope is None else 2 * n + 2
    return gamma(k) * Aabs + k * TINY


def leaky64(y, slope):
    return torch.where(y < 0, y * slope, y)


def dy64(dy, Ho, Wo):
    """winograd4_dy_kernel: Md[a*6+b][tile][n] = (A dy A^T)[a][b] = sum_ij AT[i][a] dy[i][j] AT[j][b] over the 4x4 dy tile
    (zeros outside the map).  dy [Ho, Wo, N] float64 -> [36][T][N], and the same on |dy|."""
    AT = F4["kAT"]
    TH, TW = -(-Ho // 4), -(-Wo // 4)
    d = torch.zeros(TH * 4, TW * 4, dy.shape[-1], dtype=torch.float64, device=dy.device)
    d[:Ho, :Wo] = dy
    d = d.view(TH, 4, TW, 4, -1)
    A = AT.to(dy.device)
    f = lambda t, M: torch.einsum("ia,jb,yixjn->abyxn", M, M, t).reshape(36, TH * TW, -1)
    return f(d, A), f(d.abs(), A.abs())


def dy_bound(Aabs, e_d=None):
    """A dy A^T: rows then columns, each a chain of <= n = 4 roundings (a column of A^T has <= 4 nonzeros): gamma(8) |A| |dy|
    |A^T|; the NORM form adds the error of the gradient it forms (dy_front64), carried through |A| . |A^T|"""
    b = gamma(8) * Aabs + 8 * TINY
    return b if e_d is None else b + (1 + gamma(8)) * e_d


def dy_front64(dy, x, mean_rstd, gamma_, beta, relu, sums, npix):
    """the gradient in front of the norm (winograd.hip, DyNormBackward): rstd gamma (g - S0/N - xhat S1/N), g = dy act'(gamma
    xhat + beta), in float64 from the fp32 operands, and its error bound.  Roundings: invn = 1/N (1), k0 = S0 invn (2),
    xh = (x - m) r (2), k1 (2), xh k1 (5), g - k0 (+1), - xh k1 (+1), rstd * gamma (1), the product (+1): every term <= 9:
    e <= gamma(9) |r gamma| (|g| + |k0| + |xh| |k1|).
    The activation's branch: the reference takes it from pre = gamma xhat + beta in float64.  The kernel decides on its own
    fp32 pre, which is within gamma(4) (|gamma xhat| + |beta|) of that (two roundings for xhat, one each for the product and
    the sum); where |pre| is no larger than that the two may disagree, and the bound there also admits the other branch:
    + |r gamma dy| |act'(+) - act'(-)|."""
    xh, pre, act, lo, near, r, ga = norm_pre64(x, mean_rstd, gamma_, beta, relu)
    g = dy.double() * act
    k0, k1 = sums[:, 0].double() / npix, sums[:, 1].double() / npix
    front = r * ga * (g - k0 - xh * k1)
    err = gamma(9) * (r * ga).abs() * (g.abs() + k0.abs() + xh.abs() * k1.abs()) + 9 * TINY
    err = err + near.double() * (r * ga * dy.double()).abs() * (1.0 - lo)
    return front, err


def norm_pre64(x, mean_rstd, gamma_, beta, relu):
    """what dy_front64 and the norm backward's sums share: xhat, pre = gamma xhat + beta and act'(pre) in float64 (the
    convention at exactly zero is the kernels' `pre > 0`: ReLU' gives 0 and Leaky gives 0.2 at pre == 0), the lower slope
    `lo`, and the `near` mask inside which the kernel's own fp32 pre may fall on the other side of zero.  Also r, gamma."""
    m, r = mean_rstd[:, 0].double(), mean_rstd[:, 1].double()
    ga = gamma_.double() if gamma_ is not None else torch.ones_like(m)
    be = beta.double() if beta is not None else torch.zeros_like(m)
    xh = (x.double() - m) * r
    pre = ga * xh + be
    lo = 0.0 if relu == 1 else LEAKY32 if relu == 2 else 1.0      # float32(0.2), the kernels' constant; 7.5e-9 from 0.2: inside u
    act = torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, lo))
    near =pre.abs() <= gamma(4) * ((ga * xh).abs() + be.abs()) + TINY
    return xh, pre, act, lo, near, r, ga


def dgrad_output64(dV, TH, TW):
    """winograd4_dgrad_output_kernel: the transposed algorithm's scatter -- per tile dd = B dV B^T (6x6, B = (B^T)^T), added
    into the padded map dxp [(4 TH + 2), (4 TW + 2)] at rows 4 ty.., columns 4 tx.. (two rows / columns of overlap).
    dV [36][T][C] (real tiles, float64) -> dxp, and the same on |dV|."""
    BT = F4["kBT"].to(dV.device)
    C = dV.shape[-1]

    def scat(v, B):
        dd = torch.einsum("ai,bj,abyxc->yixjc", B, B, v.view(6, 6, TH, TW, C))      # [TH, 6, TW, 6, C]
        out = torch.zeros(4 * TH + 2, 4 * TW + 2, C, dtype=torch.float64, device=dV.device)
        for r in range(6):
            for q in range(6):
                out[r:r + 4 * TH:4, q:q + 4 * TW:4] += dd[:, r, :, q]
        return out
    return scat(dV.double(), BT), scat(dV.double().abs(), BT.abs())


def dgrad_output_bound(Aabs):
    """dd = B dV B^T: two cdot levels of <= n roundings (n = the most nonzeros in a column of B^T), then up to 4 overlapping
    contributions added to a zero start (3 more roundings): gamma(2n + 3) times the scatter of |B| |dV| |B^T|"""
    n = nnz_rows(F4["kBT"].t())
    return gamma(2 * n + 3) * Aabs + (2 * n + 3) * TINY


def dw64(dU):
    """winograd4_dw_kernel: dg[n][c] = G^T dU[.][n][c] G in fp64, rounded once.  dU [36][Cout][Cin] -> [Cout][Cin][3][3]"""
    G = F4["kG"].to(dU.device)
    d = dU.double().view(6, 6, dU.shape[1], dU.shape[2])
    return torch.einsum("ai,bj,abnc->ncij", G, G, d), torch.einsum("ai,bj,abnc->ncij", G.abs(), G.abs(), d.abs())


def reflect_fold(t):
    """the adjoint of ReflectionPad2d(1) (what reflect_pad_backward computes): [(H + 2), (W + 2), C] -> [H, W, C]"""
    H, W = t.shape[0] - 2, t.shape[1] - 2
    z = torch.zeros(1, t.shape[2], H, W, dtype=t.dtype, device=t.device, requires_grad=True)
    F.pad(z, (1, 1, 1, 1), mode="reflect").backward(t.permute(2, 0, 1)[None])
    return z.grad[0].permute(1, 2, 0)


def _abs_gemm_bound(AA, AB, eA, eB, K):
    """|fl(A B^T) - A B^T| for inputs within eA, eB of |A| <= AA, |B| <= AB: the K-term sum's own rounding on the inputs'
    magnitudes, plus the inputs' errors carried through the product"""
    return sum_bound(gemm64(AA + eA, AB + eB), K) + gemm64(eA, AB) + gemm64(AA, eB) + gemm64(eA, eB)


def dgrad64(dy, w):
    """the data gradient of a 3x3 ReflectionPad(1) conv by the transposed algorithm, in float64: dy [H, W, Cout] (H, W multiples
    of 4), w [Cout][Cin][3][3] -> dx [H, W, Cin] = fold(scatter(B (U^T (A dy A^T)) B^T)) -- the composition of dy64, the
    GEMM with U^T (weight64 of the transposed layout), dgrad_output64 and reflect_fold"""
    H, W = dy.shape[:2]
    Md, _ = dy64(dy.double(), H, W)
    Ut = weight64(w.to(dy.device), F4["kG"].to(dy.device), transposed_layout=True)
    return reflect_fold(dgrad_output64(gemm64(Md, Ut), H // 4, W // 4)[0])


def dgrad_bound(dy, w):
    """End-to-end bound of the F(4x4) data gradient, the stage bounds composed on absolute values as in pipeline_bound:
      A dy A^T:   e_Md = gamma(8) A_Md,  A_Md = |A| |dy| |A^T|
      U^T:        e_U = u A_U  (fp64, one rounding),  A_U = |G| |w| |G^T|
      dV = Md U:  e_dV = C_DIRECT u Cout (A_Md + e_Md)(A_U + e_U) + e_Md A_U + A_Md e_U + e_Md e_U,  A_dV = A_Md A_U
      scatter:    e_p = S(e_dV) (1 + g) + g S(A_dV),  S = the scatter of |B| . |B^T|,  g = gamma(2 nB + 3)
      fold:       <= 4 terms per pixel: e_dx = R(e_p) (1 + gamma(3)) + gamma(3) R(S(A_dV)),  R = reflect_fold
    dy [H, W, Cout] fp32 values, w [Cout][Cin][3][3]; returns [H, W, Cin]."""
    H, W, Cout = dy.shape
    dev = dy.device
    _, AMd = dy64(dy.double(), H, W)
    AU = weight64(w.to(dev).abs(), F4["kG"].to(dev).abs(), transposed_layout=True)
    eMd, eU = gamma(8) * AMd, U * AU
    AdV = gemm64(AMd, AU)
    edV = _abs_gemm_bound(AMd, AU, eMd, eU, Cout)
    g = gamma(2 * nnz_rows(F4["kBT"].t()) + 3)
    Sa = dgrad_output64(AdV, H // 4, W // 4)[1]
    ep = dgrad_output64(edV, H // 4, W // 4)[1] * (1 + g) + g * Sa
    return reflect_fold(ep) * (1 + gamma(3)) + gamma(3) * reflect_fold(Sa) + 16 * TINY


def wgrad64(x, dy):
    """the weight gradient of a 3x3 ReflectionPad(1) conv in the Winograd domain, in float64: x [B, H, W, Cin], dy [B, H, W, Cout]
    -> dw [Cout][Cin][3][3] = G^T (sum over images and tiles of (A dy A^T)^T (B^T d B)) G -- wino_input64, dy64, the reduction
    over tiles and dw64 composed"""
    dU = 0
    for b in range(x.shape[0]):
        V, _, _ = wino_input64(x[b].double(), x.shape[1], x.shape[2], 1, True)
        Md, _ = dy64(dy[b].double(), dy.shape[1], dy.shape[2])
        dU = dU + gemm64(Md.transpose(1, 2), V.transpose(1, 2))
    return dw64(dU)[0]


def wgrad_bound(x, dy, Tp):
    """End-to-end bound of the F(4x4) weight gradient, the stage bounds composed on absolute values:
      V = B^T d B:   e_V = gamma(2 nB) A_V;   Md = A dy A^T:  e_Md = gamma(8) A_Md
      dU = sum_t Md^T V over the batch's B Tp tile rows (K terms, padding rows zero):
                     e_dU = C_DIRECT u K (A_Md + e_Md)^T (A_V + e_V) + e_Md^T A_V + A_Md^T e_V + e_Md^T e_V
      dw = G^T dU G in fp64, rounded once:  e_dw = |G^T| e_dU |G| + (u + 2^-50) |G^T| (A_dU + e_dU) |G|
    x [B, H, W, Cin], dy [B, H, W, Cout] fp32 values, Tp the padded tiles per image; returns [Cout][Cin][3][3]."""
    nB = nnz_rows(F4["kBT"])
    AV = torch.cat([wino_input64(x[b].double().abs(), x.shape[1], x.shape[2], 1, True, BT=F4["kBT"].abs())[0]
                    for b in range(x.shape[0])], 1)
    AMd = torch.cat([dy64(dy[b].double(), dy.shape[1], dy.shape[2])[1] for b in range(dy.shape[0])], 1)
    AMdT, AVT = AMd.transpose(1, 2), AV.transpose(1, 2)
    eMdT, eVT = gamma(8) * AMdT, gamma(2 * nB) * AVT
    AdU = gemm64(AMdT, AVT)
    edU = _abs_gemm_bound(AMdT, AVT, eMdT, eVT, x.shape[0] * Tp)
    absG = lambda t: dw64(t)[1]
    return absG(edU) + (U + 2.0 ** -50) * absG(AdU + edU) + TINY


def pipeline_bound(x, w, b, algo, pad=1, reflect=True):
    """End-to-end bound of a whole pipeline, composed from the stage bounds by running the same pipeline on absolute values:
    |V| <= A_V = |B^T| |x| |B|, |U| <= A_U = |G| |w| |G^T|, |M| <= A_M = A_V . A_U (K terms), |y| <= |A^T| A_M |A| + |b|.
    Each stage's error enters the next one's inputs and is carried through the absolute values:
      e_V = gamma(2 nB) A_V,  e_U = u A_U (fp64 + one rounding; F(2x2): gamma(4) A_U),
      e_M = C_DIRECT u K (A_V + e_V)(A_U + e_U) + e_V A_U + A_V e_U + e_V e_U,
      e_y = |A^T| e_M |A| (1 + gamma(2 nA + 1)) + gamma(2 nA + 1) (|A^T| A_M |A| + |b|).
    algo: "F4" | "F2" (x [H, W, C] fp32, w [Cout][Cin][3][3], the reflect / zero pad of the forward conv) | "down" | "up"
    (polyphase: zero pad 1; "up" takes ConvTranspose2d's w [Cin][Cout][3][3]).  Returns the bound [Ho, Wo, Cout]."""
    H, W, C = x.shape
    if algo in ("down", "up"):
        up = algo == "up"
        AV, TH, TW = polyphase_input64(x.double().abs(), H, W, up, absolute=True)
        AU = weight64(w.abs(), PP["kGU" if up else "kGD"].abs(), transposed_layout=up)
        BT, AT = PP["kBU" if up else "kBD"], PP["kAU" if up else "kAD"]
        Ho, Wo = (2 * H, 2 * W) if up else (H // 2, W // 2)
        eU = U * AU
    else:
        mats = F4 if algo == "F4" else F2
        AV, TH, TW = wino_input64(x.double().abs(), H, W, pad, reflect, m=4 if algo == "F4" else 2, BT=mats["kBT"].abs())
        AU = weight64(w.abs(), mats["kG"].abs())
        BT, AT = mats["kBT"], mats["kAT"]
        Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
        eU = (U if algo == "F4" else gamma(4)) * AU
    nB, nA = nnz_rows(BT), nnz_rows(AT)
    eV = gamma(2 * nB) * AV
    AM = gemm64(AV, AU)
    eM = sum_bound(gemm64(AV + eV, AU + eU), C) + gemm64(eV, AU) + gemm64(AV, eU) + gemm64(eV, eU)
    zb = torch.zeros(AU.shape[1], dtype=torch.float64)
    _, aM = output64(eM, AT.abs(), TH, TW, Ho, Wo, zb)
    _, aY = output64(AM, AT.abs(), TH, TW, Ho, Wo, b.double().abs())
    return aM * (1 + gamma(2 * nA + 1)) + gamma(2 * nA + 1) * aY


def polyphase_input64(x, H, W, up, d=None, absolute=False):
    """polyphase_input_kernel: V[pr*9+pc][tile][c] = (B d B^T), down: B = kBD on the 9x9 patch at (8 ty - 1, 8 tx - 1) (zero
    padding), tiles = 4x4 outputs of the H/2 x W/2 map; up: B = kBU on the 5x5 patch at (4 ty, 4 tx) (zeros past the map),
    tiles = 4x4 inputs.  x [H, W, C] -> [81][T][C], TH, TW.  absolute: with |B| (the magnitude a bound scales)"""
    src = x if d is None else d
    f = (lambda m: m.abs()) if absolute else (lambda m: m)
    if up:
        TH, TW = -(-H // 4), -(-W // 4)
        p = gather_patches(src, patch_index(H, TH, 4, 5, 0, False), patch_index(W, TW, 4, 5, 0, False))
        return transform_in(p, f(PP["kBU"])), TH, TW
    TH, TW = -(-(H // 2) // 4), -(-(W // 2) // 4)
    p = gather_patches(src, patch_index(H, TH, 8, 9, 1, False), patch_index(W, TW, 8, 9, 1, False))
    return transform_in(p, f(PP["kBD"])), TH, TW


# ---- pinned Winograd / polyphase stage cases (tests/test_gpu_pipeline_variants.py) ------------------------------------
# stage: which call runs (the test's STAGES); algo: "F4" | "F2" | "down" | "up"; H, W, Cin, Cout of the forward conv (the data
# gradient: of the conv whose gradient it is); pad / reflect of that conv; nimg: packed forward images (the batch entry);
# batch / slot: the weight gradient's workspace; opts: "affine" (gamma / beta), "relu", "res" (mode 2), "hint" (overlap hint
# 1), "fw" (forward weights); env: T2V_* switches; expect: the pipeline instantiations that must run, and nothing else of
# PIPE_FAMILIES.
# the fixed-grid GEMM geometries (H, W, Cin, Cout) of the 3x3 reflect-pad F(4x4) convs the generator runs, shared with
# tests/test_gpu_ops.py (the fixed-grid forms against one block per tile, bit for bit); the GEMM stage cases below take theirs
FG_GEOMS = [(64, 64, 1024, 1024), (64, 88, 640, 640), (128, 128, 256, 256), (64, 128, 512, 1024), (128, 128, 512, 256),
            (64, 40, 1024, 1024), (64, 40, 512, 384), (128, 128, 1024, 1024), (64, 85, 1024, 1024), (64, 56, 1024, 1024),
            (64, 114, 1024, 1024), (60, 52, 256, 384)]
PipeCase = collections.namedtuple("PipeCase", "id stage algo H W Cin Cout pad reflect nimg batch slot opts env expect note")
PIPE_FAMILIES = ("winograd_weight_kernel", "winograd_input_kernel", "winograd_output_kernel", "winograd4_weight_kernel",
                 "winograd4_weight_adjoint_kernel", "winograd4_input_kernel", "winograd4_output_kernel", "winograd4_dy_kernel",
                 "winograd4_dgrad_output_kernel", "winograd4_dw_kernel", "polyphase_weight_kernel", "polyphase_input_kernel",
                 "polyphase_output_down_kernel", "polyphase_output_up_kernel", "wino_gemm_sk_kernel", "wino_gemm_skr_kernel",
                 "wino_gemm_skt_kernel", "wino_wgrad_sk_kernel", "conv_igemm_kernel", "conv_wgrad_kernel")
_SK = (("T2V_WINO_GEMM_SK", "2"),)


def _pc(id, stage, algo, H, W, Cin, Cout, expect, pad=1, reflect=True, nimg=1, batch=1, slot=0, opts=(), env=(), note=""):
    if algo in ("down", "up"):
        pad, reflect = 1, False
    return PipeCase(id, stage, algo, H, W, Cin, Cout, pad, reflect, nimg, batch, slot, tuple(opts), tuple(env),
                    tuple(expect) if isinstance(expect, (tuple, list)) else (expect,), note)


def wi(mode, xcd):
    return "t2v::winograd4_input_kernel<%d,%s>" % (mode, str(bool(xcd)).lower())


def ppi(up, norm):
    return "t2v::polyphase_input_kernel<%s,%s>" % (str(bool(up)).lower(), str(bool(norm)).lower())


SK_L = "t2v::wino_gemm_sk_kernel<t2v::TileCfg<32,2,2,2,2>,2,false>"
SK_L_BKN = "t2v::wino_gemm_sk_kernel<t2v::TileCfg<32,2,2,2,2>,2,true>"
SK_W = "t2v::wino_gemm_sk_kernel<t2v::TileCfg<32,2,2,3,1>,2,false>"
SK_T160 = "t2v::wino_gemm_sk_kernel<t2v::TileCfg<32,1,4,5,1>,3,false>"
SK_T256 = "t2v::wino_gemm_sk_kernel<t2v::TileCfg<32,1,4,8,1>,3,false>"
SKR = "t2v::wino_gemm_skr_kernel<2>"
SKT = "t2v::wino_gemm_skt_kernel<3>"
_NOXCD = (("T2V_XCD_SLICES", "1"),)

PIPE_CASES = [
    # --- weight transforms ---
    _pc("w4_fwd", "weight", "F4", 8, 8, 96, 100, "t2v::winograd4_weight_kernel", note="Cout_p 128: 28 zero rows"),
    _pc("w4_adjoint_flip", "weight_adjoint", "F4", 8, 8, 64, 36, "t2v::winograd4_weight_adjoint_kernel<true>",
        note="data-gradient conv (zero pad 2) of a 36 -> 64 layer: the last 8 x 32 LDS tile partial in n"),
    _pc("w4_transposed", "weight_transposed", "F4", 8, 8, 96, 64, "t2v::winograd4_weight_adjoint_kernel<false>",
        note="U^T of a 96 -> 64 layer: rows 96 of Cout_p 128 (the data gradient asks Cout % 32 == 0)"),
    _pc("w2_fwd", "weight", "F2", 8, 8, 32, 36, "t2v::winograd_weight_kernel"),
    _pc("wp_down", "weight", "down", 8, 8, 32, 128, "t2v::polyphase_weight_kernel<false>"),
    _pc("wp_up", "weight", "up", 4, 4, 64, 128, "t2v::polyphase_weight_kernel<true>"),
    # --- forward input transforms (MODE 0) ---
    _pc("in4_reflect_ragged", "input", "F4", 10, 14, 32, 32, wi(0, 0), note="3 x 4 tiles, ragged: reflected clamps"),
    _pc("in4_reflect_h2", "input", "F4", 2, 7, 32, 32, wi(0, 0), note="H = 2, the smallest reflect size"),
    _pc("in4_zero_p0", "input", "F4", 9, 13, 32, 32, wi(0, 0), pad=0, reflect=False),
    _pc("in4_zero_p1", "input", "F4", 11, 6, 64, 32, wi(0, 0), pad=1, reflect=False),
    _pc("in4_zero_p2", "input", "F4", 7, 9, 32, 32, wi(0, 0), pad=2, reflect=False, note="the data-gradient conv's padding"),
    _pc("in4_pack2", "input", "F4", 17, 18, 32, 32, wi(0, 0), nimg=2, note="2 x 25 tiles packed into 64 rows"),
    _pc("in4_pack3", "input", "F4", 10, 10, 32, 32, wi(0, 0), nimg=3, note="3 x 9 tiles packed into 64 rows"),
    _pc("in4_xcd", "input", "F4", 13, 16, 1024, 32, wi(0, 1), env=_NOXCD, note="C2 = 512: channel slices per XCD"),
    _pc("in4_xcd_pack2", "input", "F4", 8, 12, 1024, 32, wi(0, 1), nimg=2, env=_NOXCD),
    _pc("in2_reflect_ragged", "input", "F2", 9, 11, 32, 32, "t2v::winograd_input_kernel"),
    _pc("in2_zero_p2", "input", "F2", 6, 5, 32, 32, "t2v::winograd_input_kernel", pad=2, reflect=False),
    # --- lazy-norm input transforms (the batch entry) ---
    _pc("in4_lazy1", "input", "F4", 10, 13, 64, 32, wi(1, 0), opts=("relu",)),
    _pc("in4_lazy1_affine_pack2", "input", "F4", 9, 10, 32, 32, wi(1, 0), nimg=2, opts=("relu", "affine")),
    _pc("in4_lazy1_zero_p1", "input", "F4", 9, 7, 32, 32, wi(1, 0), pad=1, reflect=False, opts=("relu", "affine"),
        note="beta != 0: a normalised padding would not be 0"),
    _pc("in4_lazy1_xcd", "input", "F4", 8, 9, 1024, 32, wi(1, 1), opts=("relu", "affine"), env=_NOXCD),
    _pc("in4_lazy2", "input", "F4", 10, 14, 32, 32, wi(2, 0), opts=("res",)),
    _pc("in4_lazy2_affine_pack3", "input", "F4", 9, 6, 64, 32, wi(2, 0), nimg=3, opts=("res", "affine")),
    _pc("in4_lazy2_xcd_pack2", "input", "F4", 7, 8, 1024, 32, wi(2, 1), nimg=2, opts=("res", "affine"), env=_NOXCD),
    # --- polyphase input transforms ---
    _pc("inp_down_ragged", "input", "down", 14, 10, 32, 128, ppi(0, 0), note="7 x 5 outputs: 2 x 2 ragged tiles"),
    _pc("inp_up_odd", "input", "up", 7, 9, 32, 128, ppi(1, 0)),
    _pc("inp_up_ragged", "input", "up", 10, 14, 64, 128, ppi(1, 0)),
    _pc("inp_down_lazy", "input", "down", 10, 14, 32, 128, ppi(0, 1), opts=("relu", "affine"),
        note="beta != 0: the zero padding must stay 0 after the norm"),
    _pc("inp_up_lazy", "input", "up", 7, 9, 32, 128, ppi(1, 1), opts=("affine",)),
    _pc("inp_up_lazy_relu_wide", "input", "up", 8, 85, 32, 128, ppi(1, 1), opts=("relu",)),
    # --- batched GEMMs: the fixed-grid forms (T2V_WINO_GEMM_SK=2: wherever the shape allows) ---
    # (the F(4x4) forms at FG_GEOMS entries: the same shapes test_gpu_ops.py checks bit for bit against one block per tile)
    _pc("gemm_sk_128", "gemm", "F4", *FG_GEOMS[0], SK_L, env=_SK + (("T2V_WINO_GEMM_SK_RAGGED", "1"),),
        note="256 rows, 576 tiles on 512 blocks: stream-K hand-over"),
    _pc("gemm_sk_192x64", "gemm", "F4", *FG_GEOMS[6], SK_W, env=_SK + (("T2V_WINO_GEMM_SK_RAGGED", "0"),),
        note="160 rows padded to 192, 108 tiles: too few for one block per CU"),
    _pc("gemm_sk_160", "gemm", "F4", *FG_GEOMS[5], SK_T160, env=_SK + (("T2V_WINO_GEMM_SK_RAGGED", "0"),),
        note="160 rows, 288 tiles: one block per CU"),
    _pc("gemm_sk_256_pack2", "gemm", "F4", *FG_GEOMS[0], SK_T256, nimg=2, opts=("hint",),
        env=_SK + (("T2V_WINO_GEMM_SK_RAGGED", "0"),), note="two packed images: 512 rows, the overlap hint"),
    _pc("gemm_skr", "gemm", "F4", *FG_GEOMS[11], SKR, env=_SK + (("T2V_WINO_GEMM_SK_RAGGED", "1"),),
        note="195 rows: 7 fragments"),
    _pc("gemm_skt", "gemm", "F4", *FG_GEOMS[9], SKT, env=_SK + (("T2V_WINO_GEMM_SK_RAGGED", "2"),),
        note="224 rows: 4 + 3 fragments"),
    # (polyphase: no FG_GEOMS entry -- a stride-2 map whose 81-position GEMM has whole 128-row tiles)
    _pc("gemm_sk_down", "gemm", "down", 64, 128, 128, 256, SK_L, env=_SK + (("T2V_WINO_GEMM_SK_RAGGED", "0"),)),
    # --- output transforms ---
    _pc("out4_ragged_stats", "output", "F4", 10, 14, 32, 96, "t2v::winograd4_output_kernel", opts=("stats",)),
    _pc("out4_pack2_stats", "output", "F4", 9, 13, 32, 64, "t2v::winograd4_output_kernel", nimg=2, opts=("stats",)),
    _pc("out4_lrelu", "output", "F4", 11, 10, 32, 68, "t2v::winograd4_output_kernel", opts=("lrelu",),
        note="the VGG19 loss network's LeakyReLU in the output transform (no statistics with an activation)"),
    _pc("out2_ragged_stats", "output", "F2", 9, 11, 32, 72, "t2v::winograd_output_kernel", opts=("stats",)),
    _pc("outp_down_stats", "output", "down", 14, 10, 32, 128, "t2v::polyphase_output_down_kernel", opts=("stats",)),
    _pc("outp_up_stats", "output", "up", 7, 9, 32, 128, "t2v::polyphase_output_up_kernel", opts=("stats",)),
    # --- weight gradient: A dy A^T, the reduction over tiles, G^T dU G ---
    _pc("dy_plain", "dy", "F4", 10, 14, 32, 36, "t2v::winograd4_dy_kernel<false>", batch=2, slot=1),
    _pc("dy_norm_relu_affine", "dy_norm", "F4", 12, 9, 32, 40, "t2v::winograd4_dy_kernel<true>", batch=2, slot=1,
        opts=("relu", "affine")),
    _pc("dy_norm_plain", "dy_norm", "F4", 8, 8, 32, 32, "t2v::winograd4_dy_kernel<true>"),
    _pc("wgrad_sk", "wgrad", "F4", 16, 20, 128, 256, ("t2v::wino_wgrad_sk_kernel<16,4>", "t2v::winograd4_dw_kernel"),
        batch=2, env=(("T2V_WGRAD_SK", "2"),)),
    _pc("wgrad_tile_per_block", "wgrad", "F4", 12, 10, 64, 36, ("t2v::conv_wgrad_kernel<false,16,4>",
                                                                "t2v::winograd4_dw_kernel"),
        batch=3, env=(("T2V_WGRAD_SK", "0"),)),
    # --- data gradient by the transposed algorithm: dV = dM U^T (GEMM), the scatter B dV B^T ---
    _pc("dgrad_bkn", "dgrad", "F4", 64, 64, 128, 128, (SK_L_BKN, "t2v::winograd4_dgrad_output_kernel<false>"), batch=2,
        slot=1, opts=("fw",), env=_SK + (("T2V_XCD_SLICES", "0"),), note="forward weights as B [K][N]"),
    _pc("dgrad_xcd", "dgrad", "F4", 8, 12, 1024, 64, ("t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,0,false,false,2>",
                                                      "t2v::winograd4_dgrad_output_kernel<true>"),
        env=(("T2V_WINO_GEMM_SK", "0"),) + _NOXCD, note="C = 1024: channel slices per XCD; every border block touched"),
]
PIPE_BY_ID = {c.id: c for c in PIPE_CASES}
# end to end, one per algorithm: the whole pipeline against F.conv2d / conv_transpose2d / autograd in float64 under
# pipeline_bound() / dgrad_bound() / wgrad_bound() (catches a wrong matrix or a wrong adjoint, which the stage cases -- each
# against the header's own matrices and the stage references' own algebra -- cannot): (algo, H, W, Cin, Cout)
E2E_CASES = [("F4", 13, 18, 64, 96), ("F2", 9, 11, 32, 64), ("down", 14, 18, 64, 128), ("up", 7, 9, 64, 128),
             ("F4_dgrad", 16, 20, 64, 128), ("F4_wgrad", 13, 18, 32, 64)]


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

TABLE = {
    "t2v::accumulate_kernel":
        Existing(("tests/test_gpu_kernel_variants.py::test_layout_and_reduction_forms_against_float64",)),
    "t2v::act_backward_kernel":
        Existing(("tests/test_gpu_elementwise_float64.py::test_act_backward_against_float64", "tests/test_gpu_backward.py::test_pointwise_and_pooling_backward", "tests/test_gpu_backward.py::test_masked_l1_and_flow_head_activation_backward",)),
    "t2v::adam_kernel":
        Existing(("tests/test_gpu_train_pieces.py::test_fused_adam_matches_torch041_semantics",)),
    "t2v::adam_multi_kernel":
        Existing(("tests/test_gpu_train_pieces.py::test_multi_tensor_adam_against_float64_on_both_paths",)),
    "t2v::add_kernel":
        Existing(("tests/test_gpu_elementwise_float64.py::test_norm_join_is_two_applies_and_an_add", "tests/test_gpu_elementwise_float64.py::test_add_strides_past_the_grid_cap",)),
    "t2v::avgpool3s2_backward_kernel":
        Existing(("tests/test_gpu_elementwise_float64.py::test_avgpool_forward_and_backward_against_float64", "tests/test_gpu_backward.py::test_pointwise_and_pooling_backward",)),
    "t2v::avgpool3s2_kernel":
        Existing(("tests/test_gpu_elementwise_float64.py::test_avgpool_forward_and_backward_against_float64", "tests/test_gpu_ops.py::test_avgpool_count_include_pad_false",)),
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
        Cases(("Q1_zero_s2_odd_cout30", "Q1_zero_k3_nk4_b2", "Q1_zero_s2_cin6_cout30",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,1,false,false,3>":
        Unreachable('64x64 tiles with one phase always take RING 2 in launch_pad (Cfg::BM == 64 && nphases == 1); MODE 1 is single-phase by definition'),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,1,false,true,2>":
        Cases(("Q1_reflect_min_h2_nk3",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,1,false,true,3>":
        Unreachable('64x64 tiles with one phase always take RING 2 in launch_pad (Cfg::BM == 64 && nphases == 1); MODE 1 is single-phase by definition'),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,1,true,false,2>":
        Cases(("Q1_stats_1x1_nk1", "Q1_stats_k4s2p2_cin6_disc", "Q1_stats_k3s2_cin9_cout96",)),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,1,true,false,3>":
        Unreachable('64x64 tiles with one phase always take RING 2 in launch_pad (Cfg::BM == 64 && nphases == 1); MODE 1 is single-phase by definition'),
    "t2v::conv_igemm_kernel<t2v::TileCfg<32,2,2,1,1>,1,true,true,2>":
        Cases(("Q1_stats_reflect_nk4_offset", "Q1_stats_reflect_k3_cin3",)),
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
        Cases(("Q2_stats_convT_nk124_r3", "Q2_stats_convT_cin5_r3",)),
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
        Existing(("tests/test_gpu_elementwise_float64.py::test_norm_apply_against_float64", "tests/test_gpu_elementwise_float64.py::test_norm_join_is_two_applies_and_an_add", "tests/test_gpu_ops.py::test_instance_norm_affine_residual_matches_trainmode_batchnorm", "tests/test_gpu_ops.py::test_instance_norm_large_mean_is_stable",)),
    "t2v::inorm_bwd_apply_kernel":
        Existing(("tests/test_gpu_elementwise_float64.py::test_norm_backward_against_float64", "tests/test_gpu_backward.py::test_norm_backward_with_fused_activation",)),
    "t2v::inorm_bwd_final_kernel":
        Existing(("tests/test_gpu_elementwise_float64.py::test_norm_backward_against_float64", "tests/test_gpu_backward.py::test_norm_backward_with_fused_activation",)),
    "t2v::inorm_bwd_reduce_kernel":
        Existing(("tests/test_gpu_elementwise_float64.py::test_norm_backward_against_float64", "tests/test_gpu_backward.py::test_norm_backward_with_fused_activation",)),
    "t2v::inorm_finalize_kernel":
        Existing(("tests/test_gpu_ops.py::test_instance_norm_affine_residual_matches_trainmode_batchnorm", "tests/test_gpu_ops.py::test_instance_norm_large_mean_is_stable",
                  "tests/test_gpu_norm_finalize_grouped.py::test_grouped_tables_against_float64_and_the_single_kernel_form",)),
    "t2v::inorm_finalize_merge_kernel":
        Existing(("tests/test_gpu_norm_finalize_grouped.py::test_grouped_tables_against_float64_and_the_single_kernel_form",)),
    "t2v::loss_backward_kernel":
        Existing(("tests/test_gpu_elementwise_float64.py::test_loss_backward_past_the_grid_cap", "tests/test_gpu_backward.py::test_pointwise_and_pooling_backward",)),
    "t2v::loss_terms_final_kernel":
        Existing(("tests/test_gpu_loss_terms.py::test_values_against_float64_and_seeds_bit_for_bit_in_one_run",)),
    "t2v::loss_terms_kernel":
        Existing(("tests/test_gpu_loss_terms.py::test_values_against_float64_and_seeds_bit_for_bit_in_one_run",)),
    "t2v::masked_l1_backward_kernel":
        Existing(("tests/test_gpu_elementwise_float64.py::test_masked_l1_and_its_backward_against_float64", "tests/test_gpu_backward.py::test_masked_l1_and_flow_head_activation_backward",)),
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
        Cases(("inp_down_ragged",)),
    "t2v::polyphase_input_kernel<false,true>":
        Cases(("inp_down_lazy",)),
    "t2v::polyphase_input_kernel<true,false>":
        Cases(("inp_up_odd", "inp_up_ragged",)),
    "t2v::polyphase_input_kernel<true,true>":
        Cases(("inp_up_lazy", "inp_up_lazy_relu_wide",)),
    "t2v::polyphase_output_down_kernel":
        Cases(("outp_down_stats",)),
    "t2v::polyphase_output_up_kernel":
        Cases(("outp_up_stats",)),
    "t2v::polyphase_weight_kernel<false>":
        Cases(("wp_down",)),
    "t2v::polyphase_weight_kernel<true>":
        Cases(("wp_up",)),
    "t2v::reduce_final_kernel":
        Existing(("tests/test_gpu_kernel_variants.py::test_layout_and_reduction_forms_against_float64",)),
    "t2v::reduce_masked_l1_kernel":
        Existing(("tests/test_gpu_elementwise_float64.py::test_masked_l1_and_its_backward_against_float64", "tests/test_gpu_backward.py::test_masked_l1_and_flow_head_activation_backward",)),
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
        Existing(("tests/test_gpu_elementwise_float64.py::test_flow_warp_forward_and_backward_against_float64", "tests/test_gpu_backward.py::test_flow_warp_composite_backward_matches_oracle_autograd",)),
    "t2v::warp_composite_kernel":
        Existing(("tests/test_gpu_elementwise_float64.py::test_flow_warp_forward_and_backward_against_float64", "tests/test_gpu_ops.py::test_flow_warp_composite_vs_grid_sample",)),
    "t2v::wgrad_reduce_kernel":
        Existing(("tests/test_gpu_backward.py::test_conv_weight_and_bias_gradient",)),
    "t2v::wino_gemm_sk_kernel<t2v::TileCfg<32,1,4,5,1>,3,false>":
        Cases(("gemm_sk_160",)),
    "t2v::wino_gemm_sk_kernel<t2v::TileCfg<32,1,4,8,1>,3,false>":
        Cases(("gemm_sk_256_pack2",)),
    "t2v::wino_gemm_sk_kernel<t2v::TileCfg<32,2,2,2,2>,2,false>":
        Cases(("gemm_sk_128", "gemm_sk_down",)),
    "t2v::wino_gemm_sk_kernel<t2v::TileCfg<32,2,2,2,2>,2,true>":
        Cases(("dgrad_bkn",)),
    "t2v::wino_gemm_sk_kernel<t2v::TileCfg<32,2,2,3,1>,2,false>":
        Cases(("gemm_sk_192x64",)),
    "t2v::wino_gemm_skr_kernel<2>":
        Cases(("gemm_skr",)),
    "t2v::wino_gemm_skt_kernel<3>":
        Cases(("gemm_skt",)),
    "t2v::wino_wgrad_sk_kernel<16,4>":
        Cases(("wgrad_sk",)),
    "t2v::winograd4_dgrad_output_kernel<false>":
        Cases(("dgrad_bkn",)),
    "t2v::winograd4_dgrad_output_kernel<true>":
        Cases(("dgrad_xcd",)),
    "t2v::winograd4_dw_kernel":
        Cases(("wgrad_sk", "wgrad_tile_per_block",)),
    "t2v::winograd4_dy_kernel<false>":
        Cases(("dy_plain",)),
    "t2v::winograd4_dy_kernel<true>":
        Cases(("dy_norm_relu_affine", "dy_norm_plain",)),
    "t2v::winograd4_input_kernel<0,false>":
        Cases(("in4_reflect_ragged", "in4_reflect_h2", "in4_zero_p0", "in4_zero_p1", "in4_zero_p2", "in4_pack2", "in4_pack3",)),
    "t2v::winograd4_input_kernel<0,true>":
        Cases(("in4_xcd", "in4_xcd_pack2",)),
    "t2v::winograd4_input_kernel<1,false>":
        Cases(("in4_lazy1", "in4_lazy1_affine_pack2", "in4_lazy1_zero_p1",)),
    "t2v::winograd4_input_kernel<1,true>":
        Cases(("in4_lazy1_xcd",)),
    "t2v::winograd4_input_kernel<2,false>":
        Cases(("in4_lazy2", "in4_lazy2_affine_pack3",)),
    "t2v::winograd4_input_kernel<2,true>":
        Cases(("in4_lazy2_xcd_pack2",)),
    "t2v::winograd4_output_kernel":
        Cases(("out4_ragged_stats", "out4_pack2_stats", "out4_lrelu",)),
    "t2v::winograd4_weight_adjoint_kernel<false>":
        Cases(("w4_transposed",)),
    "t2v::winograd4_weight_adjoint_kernel<true>":
        Cases(("w4_adjoint_flip",)),
    "t2v::winograd4_weight_kernel":
        Cases(("w4_fwd",)),
    "t2v::winograd_input_kernel":
        Cases(("in2_reflect_ragged", "in2_zero_p2",)),
    "t2v::winograd_output_kernel":
        Cases(("out2_ragged_stats",)),
    "t2v::winograd_weight_kernel":
        Cases(("w2_fwd",)),
}

# ---- kernels of `namespace t2v { namespace { ... } }` (optical_flow, image_metrics, temporal_metrics, train_visuals,
# image_resample, winograd_split, polyphase_split .hip): nm spells them 't2v::(anonymous namespace)::...', normalise() drops
# that component.  Which parametrisation reaches which template instantiation is read off the dispatch code named in each
# comment and was confirmed with the profiler on an MI355X (profiles/ledger_float64.txt).
_OF = "tests/test_gpu_optical_flow.py::"
_S4 = "tests/test_gpu_split_bf16.py::"
_S5 = "tests/test_gpu_split_polyphase.py::"
_IN_PLANES = "test_input_transform_planes_are_the_split_of_the_fp32_transform"
_W_PLANES = "test_packed_weight_planes_are_the_split_of_the_fp32_packing"
_GEMM_EMU = "test_gemm_stage_against_the_emulation_of_its_own_planes"
_WHOLE = "test_whole_conv_against_float64"
TABLE.update({
    # launch_flow (optical_flow.hip): <0> is the coarsest level's first iteration (every call); <1> every iteration k > 0
    # (iters >= 2: cases A, B with the default 3, C with 2); <2> the first iteration of every finer level (levels >= 2: A, B, C
    # take the default rule's 3 levels).  Float64 restatement at every pixel.
    "t2v::flow_lk_kernel<0>":
        Existing((_OF + "test_kernel_matches_the_float64_restatement_at_every_pixel",
                  _OF + "test_kernel_matches_the_float64_restatement_at_the_edges_of_its_geometry",)),
    "t2v::flow_lk_kernel<1>":
        Existing((_OF + "test_kernel_matches_the_float64_restatement_at_every_pixel",)),
    "t2v::flow_lk_kernel<2>":
        Existing((_OF + "test_kernel_matches_the_float64_restatement_at_every_pixel",)),
    "t2v::flow_grey_kernel":
        Existing((_OF + "test_kernel_matches_the_float64_restatement_at_every_pixel",)),
    "t2v::flow_pool_kernel":
        Existing((_OF + "test_kernel_matches_the_float64_restatement_at_every_pixel",)),
    "t2v::flow_out_kernel":
        Existing((_OF + "test_kernel_matches_the_float64_restatement_at_every_pixel",)),
    # an exact identity: the flow of the bytes == the flow of the frames u8_pose_to_f32_kernel converts (both pinned)
    "t2v::flow_grey_u8_kernel":
        Existing(("tests/test_gpu_temporal_metrics.py::test_optical_flow_u8_is_bit_equal_to_optical_flow_on_the_converted_frames",)),
    "t2v::image_metrics_u8_kernel":
        Existing(("tests/test_gpu_image_metrics.py::test_whole_frame_against_reference",
                  "tests/test_gpu_image_metrics.py::test_boxes_equal_the_cropped_pair",)),
    "t2v::image_metrics_finalize_kernel":
        Existing(("tests/test_gpu_image_metrics.py::test_whole_frame_against_reference",)),
    "t2v::temporal_metrics_u8_kernel":
        Existing(("tests/test_gpu_temporal_metrics.py::test_whole_frame_against_reference",
                  "tests/test_gpu_temporal_metrics.py::test_boxes_equal_the_reference_on_the_box",)),
    "t2v::temporal_metrics_finalize_kernel":
        Existing(("tests/test_gpu_temporal_metrics.py::test_whole_frame_against_reference",)),
    "t2v::train_visuals_minmax_kernel":
        Existing(("tests/test_gpu_train_display.py::test_eight_panels_against_the_reference",)),
    "t2v::train_visuals_render_kernel":
        Existing(("tests/test_gpu_train_display.py::test_eight_panels_against_the_reference",)),
    "t2v::resample_crop_normalize_u8_kernel":
        Existing(("tests/test_gpu_image_resample.py::test_kernel_equals_pillow_crop_normalize_bitwise",)),
    # the 36- and 81-position split GEMM: the float64 emulation of its own bf16 planes
    "t2v::wino_split_gemm_kernel":
        Existing((_S4 + _GEMM_EMU, _S5 + _GEMM_EMU,)),
    # launch_winograd4_input_split (winograd_split.hip): MODE 0 = no lazy norm ("plain"), 1 = mean_rstd without a residual
    # ("relu", "relu_affine"), 2 = with res / xout ("res"); XCD = xcd_slice_grid() != 0, i.e. C / 2 % 512 == 0: the
    # 1024-channel maps, every other map takes <MODE, false>.  The planes must be split() -- tests/split_reference.py's own
    # restatement -- of what the float64-pinned fp32 kernel stores, bit for bit; the whole conv is then held to float64.
    "t2v::winograd4_input_split_kernel<0,false>":
        Existing((_S4 + _IN_PLANES, _S4 + _WHOLE,)),
    "t2v::winograd4_input_split_kernel<0,true>":
        Existing((_S4 + _IN_PLANES,)),
    "t2v::winograd4_input_split_kernel<1,false>":
        Existing((_S4 + _IN_PLANES,)),
    "t2v::winograd4_input_split_kernel<1,true>":
        Existing((_S4 + _IN_PLANES,)),
    "t2v::winograd4_input_split_kernel<2,false>":
        Existing((_S4 + _IN_PLANES,)),
    "t2v::winograd4_input_split_kernel<2,true>":
        Existing((_S4 + _IN_PLANES,)),
    "t2v::winograd4_weight_split_kernel":
        Existing((_S4 + _W_PLANES, _S4 + _WHOLE,)),
    # launch_polyphase_input_split (polyphase_split.hip): UP = the desc is transposed (INPUT_MAPS' up column), NORM =
    # mean_rstd given ("relu", "relu_affine"; "plain" takes <UP, false>)
    "t2v::polyphase_input_split_kernel<false,false>":
        Existing((_S5 + _IN_PLANES, _S5 + _WHOLE,)),
    "t2v::polyphase_input_split_kernel<false,true>":
        Existing((_S5 + _IN_PLANES,)),
    "t2v::polyphase_input_split_kernel<true,false>":
        Existing((_S5 + _IN_PLANES, _S5 + _WHOLE,)),
    "t2v::polyphase_input_split_kernel<true,true>":
        Existing((_S5 + _IN_PLANES,)),
    # launch_polyphase_weight_split: <false> the "conv2d" id, <true> the "convtranspose2d" id
    "t2v::polyphase_weight_split_kernel<false>":
        Existing((_S5 + _W_PLANES, _S5 + _WHOLE,)),
    "t2v::polyphase_weight_split_kernel<true>":
        Existing((_S5 + _W_PLANES, _S5 + _WHOLE,)),
})
