// conv_igemm_split.hip -- T2V_ALGO_DIRECT_BF16X2: the direct 3x3 stride-2 / transposed convolution (conv_igemm.hip, MODE 0,
// zero padding) with its contraction on the bf16 matrix cores, in the split-bf16 arithmetic of winograd_split.hip:
//   hi = bf16_rne(v), lo = bf16_rne(v - hi);  sum_k (ah*bh + ah*bl + al*bh)  with v_mfma_f32_32x32x16_bf16, fp32 accumulators.
// Operand layout: every fp32 channel pair (8 bytes) of the input map and of the packed weight [Cout][Kp] is replaced IN PLACE by
// the two dwords split_bf16x2 returns, {hi.x, hi.y | lo.x, lo.y}.  A split tensor therefore has the byte geometry of the fp32
// one: the loaders (per-lane source offsets, hardware zero fill for padding and ragged edges, the 16-byte XOR swizzle), the
// K index tap * Cin + c, the phase decomposition of the transposed conv, the epilogue (bias, statistics partials) and the
// XCD-aware tile walk are conv_igemm_kernel's, and no workspace grows.  A 16-byte LDS slot holds four channels as
// [hi01 lo01 hi23 lo23]; an MFMA operand (8 bf16 = 8 k per lane) is the hi -- or the lo -- dwords of two slots, chosen, not
// shuffled.  The k order inside a 32-deep stage is permuted identically for A and B.
// Shared text: the loader waves' K loop (loader_k_loop), xcd_band, dma16 and the dynamic-LDS opt-in are k_loops.h's, the split
// stores transform_common.h's.  The loader geometry and the epilogue are copies of conv_igemm_kernel's, and the MFMA waves' loop
// is wino_split_gemm_kernel's written out again: shared, together with the loader loop, it cost that kernel 0.4 % (see there).
//   split_pairs_kernel        : fp32 -> the pair layout (the single-layer entry's input pass; the packed weights, in place)
//   conv_igemm_split_kernel   : 128 x 128 output tile per block, 4 MFMA waves (64 x 64 each) + 4 loader waves, a ring of three
//                               32 KiB stages: one block per CU (64 accumulator + 64 fragment registers per lane), as
//                               wino_split_gemm_kernel.  One block per tile, nothing shared between blocks: every output is one
//                               block's fixed-order chain, two calls give the same bits.
//   inorm_apply_split_kernel  : the norm apply pass in front of such a layer inside the generator: inorm_apply_kernel's body
//                               (norm_apply.h) with the split store, in place
// The kernels of this opt-in form are a library of their own, libt2v_split.so, which libt2v_hip.so loads as a dependency: what
// it exports are the three launches at the end of this file, which report a hipError_t; arguments are checked by their callers
// in libt2v_hip.so (capi.hip: launch_conv_igemm_split, launch_split_pairs; elementwise.hip: launch_inorm_apply_split).
#include "t2v_internal.h"
#include "k_loops.h"
#include "transform_common.h"
#include "norm_apply.h"

namespace t2v {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(256) void split_pairs_kernel(const float4* x, uint4* y, long n4) {   // (y == x allowed)
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) store_split_quad(y, i, x[i]);
}

// the same pass with the split store: y receives {hi.x, hi.y | lo.x, lo.y} per channel pair; y == x is
// allowed (every thread reads its float4 before it writes it), so neither is __restrict__
__global__ __launch_bounds__(256) void inorm_apply_split_kernel(const float4* x, const float4* __restrict__ mean_rstd,
                                                                const float4* __restrict__ gamma,
                                                                const float4* __restrict__ beta,
                                                                const float4* __restrict__ res1, uint4* y, long n4, int C4,
                                                                int relu) {
    y += (long)blockIdx.y * n4;
    inorm_apply_body(x, mean_rstd, gamma, beta, res1, nullptr, n4, C4, relu, NormJoinSide{},
                     [&](long i, float4 v) { store_split_quad(y, i, v); });
}


constexpr int kBM = 128, kBN = 128, kMF = 32, kTM = 2, kTN = 2, kRing = 3;
constexpr int kStageBytes = (kBM + kBN) * 128;      // 32 KiB: [A | B][128 rows][32 k as 16 {hi, lo} dword pairs]
constexpr int kSplitLds = kRing * kStageBytes;      // 96 KiB
constexpr int kAIters = kBM / 32, kBPerWave = kBN / 32, kLd = kAIters + kBPerWave;   // DMA instructions per loader wave and stage

template <bool STATS>
__global__ __launch_bounds__(512) void conv_igemm_split_kernel(const ConvKParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // 0..7
    const bool is_loader = wave >= 4;
    const int wid = wave & 3;

    // ---- block -> (phase, tile): conv_igemm_kernel's walk (phases heaviest first, tiles banded per XCD) ----
    const int tiles_per_phase = p.mtiles * p.ntiles;
    const int phase = blockIdx.x / tiles_per_phase;
    const int rem = xcd_band(blockIdx.x - phase * tiles_per_phase, tiles_per_phase);
    const int mt = rem / p.ntiles;
    const int nt = rem - mt * p.ntiles;
    const int m0 = mt * kBM, n0 = nt * kBN;
    const ConvPhase ph = p.ph[phase];
    const float* __restrict__ wbase = p.w + ph.w_off;

    if (is_loader) {
        // ---- loader lane geometry: conv_igemm_kernel's MODE 0 (a stage lies inside one tap), zero padding.  A lane whose
        // tap falls outside the image or whose pixel lies past M fetches from kOOB: the hardware writes zeros, and the split
        // of 0.f is the zero pair.
        constexpr int kOOB = 0x7fff0000;  // >= num_records of both SRDs (direct_split_supported)
        const int lrow = lane >> 3, lslot = lane & 7;
        const int x_bytes = p.Hin * p.Win * p.Cin_s * 4;
        const int w_bytes = p.ntiles * kBN * ph.Kp * 4;
        int a_by[kAIters], a_bx[kAIters], a_coff[kAIters], a_voff[kAIters], b_voff[kBPerWave];
        bool a_ok[kAIters];
#pragma unroll
        for (int i = 0; i < kAIters; ++i) {
            const int r = wid * (kBM / 4) + i * 8 + lrow;
            const int m = m0 + r;
            a_ok[i] = m < p.M;
            const int my = m / p.Wm, mx = m - my * p.Wm;
            a_by[i] = my * p.stride;
            a_bx[i] = mx * p.stride;
            a_coff[i] = (lslot ^ ((r >> 1) & 7)) * 4;
            a_voff[i] = kOOB;
        }
#pragma unroll
        for (int i = 0; i < kBPerWave; ++i) {
            const int r = (wid * kBPerWave + i) * 8 + lrow;
            b_voff[i] = ((n0 + r) * ph.Kp + (lslot ^ ((r >> 1) & 7)) * 4) * 4;
        }
        const int cpt = p.Cin_s >> 5;   // stages per tap
        int cur_tap = -1;
        auto issue_stage = [&](int kt, int buf) {
            const int tap = kt / cpt;
            if (tap != cur_tap) {
                const int dy = p.tdy[ph.tap0 + tap], dx = p.tdx[ph.tap0 + tap];
#pragma unroll
                for (int i = 0; i < kAIters; ++i) {
                    const int iy = a_by[i] + dy, ix = a_bx[i] + dx;
                    const bool ok = a_ok[i] && (unsigned)iy < (unsigned)p.Hin && (unsigned)ix < (unsigned)p.Win;
                    a_voff[i] = ok ? ((iy * p.Win + ix) * p.Cin_s + a_coff[i]) * 4 : kOOB;
                }
                cur_tap = tap;
            }
            char* dstA = smem + buf * kStageBytes + wid * (kBM / 4) * 128;
            char* dstB = smem + buf * kStageBytes + kBM * 128 + wid * kBPerWave * 8 * 128;
            const int c0 = (kt - tap * cpt) << 5;
#pragma unroll
            for (int i = 0; i < kAIters; ++i) dma16(p.x, x_bytes, dstA + i * 8 * 128, a_voff[i], c0 * 4);
#pragma unroll
            for (int i = 0; i < kBPerWave; ++i) dma16(wbase, w_bytes, dstB + i * 8 * 128, b_voff[i], kt * (kBK * 4));
        };
        loader_k_loop<kRing, kLd>(0, ph.nk, issue_stage);
        __syncthreads();  // the epilogue reuses the LDS ring
        // (the barrier count of the statistics reduction below: s_barrier counts arrivals of all 8 waves)
        if constexpr (STATS) {
            __syncthreads(); __syncthreads(); __syncthreads(); __syncthreads();
        }
        return;
    }

    // ---- MFMA waves ----
    const int wm = wid >> 1, wn = wid & 1;
    const int fr = lane & (kMF - 1);  // row (A) / column (B) inside the MFMA tile
    const int g = lane >> 5;          // k group: 8 of the 16 k of an MFMA
    const int fsw = (fr >> 1) & 7;    // tile bases are multiples of 16 rows, so swizzle(row) = swizzle(fr)
    const int a_row0 = wm * (kTM * kMF) + fr;
    const int b_row0 = wn * (kTN * kMF) + fr;

    f32x16 acc[kTM][kTN];
#pragma unroll
    for (int i = 0; i < kTM; ++i)
#pragma unroll
        for (int j = 0; j < kTN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // half stage q (16 k): lane group g takes the logical slots 4q + 2g, 4q + 2g + 1 (8 channels) of its rows
    u32x4 af[2][kTM][2], bfr[2][kTN][2];   // [register set][fragment][slot]
    auto load_frags = [&](int buf, int q, int set) {
        const char* sA = smem + buf * kStageBytes;
        const char* sB = sA + kBM * 128;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int slot = ((4 * q + 2 * g + t) ^ fsw) * 16;
#pragma unroll
            for (int i = 0; i < kTM; ++i) af[set][i][t] = *reinterpret_cast<const u32x4*>(sA + (a_row0 + i * kMF) * 128 + slot);
#pragma unroll
            for (int j = 0; j < kTN; ++j) bfr[set][j][t] = *reinterpret_cast<const u32x4*>(sB + (b_row0 + j * kMF) * 128 + slot);
        }
    };
    auto hi_of = [](const u32x4 (&s)[2]) { return __builtin_bit_cast(bf16x8, u32x4{s[0][0], s[0][2], s[1][0], s[1][2]}); };
    auto lo_of = [](const u32x4 (&s)[2]) { return __builtin_bit_cast(bf16x8, u32x4{s[0][1], s[0][3], s[1][1], s[1][3]}); };
    auto mfmas = [&](int set) {      // lo*hi, hi*lo, hi*hi per 16-deep half stage
        bf16x8 ah[kTM], al[kTM], bh[kTN], bl[kTN];
#pragma unroll
        for (int i = 0; i < kTM; ++i) {
            ah[i] = hi_of(af[set][i]);
            al[i] = lo_of(af[set][i]);
        }
#pragma unroll
        for (int j = 0; j < kTN; ++j) {
            bh[j] = hi_of(bfr[set][j]);
            bl[j] = lo_of(bfr[set][j]);
        }
#pragma unroll
        for (int i = 0; i < kTM; ++i)
#pragma unroll
            for (int j = 0; j < kTN; ++j) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
            }
    };

    const int nk = ph.nk;
    __syncthreads();   // B0
    load_frags(0, 0, 0);
    int buf = 0;
    for (int kt = 0; kt < nk; ++kt) {
        const int nbuf = buf == kRing - 1 ? 0 : buf + 1;
        __builtin_amdgcn_sched_barrier(0);
        load_frags(buf, 1, 1);
        mfmas(0);
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();   // barrier(kt): slot `buf` fully read, stage kt + 1 visible
        __builtin_amdgcn_sched_barrier(0);
        load_frags(nbuf, 0, 0);      // (after the last stage: the re-fetched last stage, read and dropped)
        mfmas(1);
        buf = nbuf;
    }
    __syncthreads();  // the epilogue reuses the LDS ring

    // ---- epilogue: conv_igemm_kernel's (bias, statistics partials, buffer stores), no activation ----
    float bias_v[kTN];
    int col[kTN];
#pragma unroll
    for (int j = 0; j < kTN; ++j) {
        col[j] = n0 + wn * (kTN * kMF) + j * kMF + fr;
        bias_v[j] = (col[j] < p.Cout && p.bias) ? p.bias[col[j]] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < kTM; ++i)
#pragma unroll
        for (int j = 0; j < kTN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] += bias_v[j];
    auto row_of = [&](int i, int r) { return wm * (kTM * kMF) + i * kMF + (r & 3) + 8 * (r >> 2) + 4 * g; };

    if constexpr (STATS) {
        // per-block, per-channel mean and M2 over the block's valid pixels, two passes over the accumulators, pairwise sums
        float* red = reinterpret_cast<float*>(smem);  // [2][BN]
        const int cnt = min(kBM, p.M - m0);
        const float inv_cnt = 1.f / (float)cnt;
        float mean_b[kTN];
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
            for (int j = 0; j < kTN; ++j) {
                float tsum[kTM * 16];
#pragma unroll
                for (int i = 0; i < kTM; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float v = acc[i][j][r];
                        if (pass == 1) {
                            v -= mean_b[j];
                            v *= v;
                        }
                        tsum[i * 16 + r] = (row_of(i, r) < cnt) ? v : 0.f;
                    }
#pragma unroll
                for (int w = kTM * 16 / 2; w >= 1; w >>= 1)
#pragma unroll
                    for (int i = 0; i < w; ++i) tsum[i] += tsum[i + w];
                float s = tsum[0];
                s += __shfl_xor(s, 32);
                if (g == 0) red[wm * kBN + wn * (kTN * kMF) + j * kMF + fr] = s;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < kTN; ++j) {
                const int c = wn * (kTN * kMF) + j * kMF + fr;
                const float tot = red[c] + red[kBN + c];
                if (pass == 0) {
                    mean_b[j] = tot * inv_cnt;
                } else if (wm == 0 && g == 0 && col[j] < p.Cout) {
                    const size_t part = (size_t)phase * p.mtiles + mt;
                    float2* dst = reinterpret_cast<float2*>(p.stats) + part * p.Cout + col[j];
                    *dst = make_float2(mean_b[j], tot);
                }
            }
            __syncthreads();
        }
    }

    const __amdgpu_buffer_rsrc_t ysrd = __builtin_amdgcn_make_buffer_rsrc(p.y, 0, p.Hout * p.Wout * p.Cout_s * 4, 0x00020000);
    constexpr unsigned kDrop = 0x7fffff00u;   // past every output map (< 0x7fff0000 bytes); offsets are unsigned
    const bool fastdiv = p.M <= (1 << 20);
    const unsigned long long magic = (1ull << 40) / (unsigned)p.Wm + 1;
    unsigned coff[kTN];
#pragma unroll
    for (int j = 0; j < kTN; ++j) coff[j] = col[j] < p.Cout ? (unsigned)col[j] * 4u : kDrop;
#pragma unroll
    for (int i = 0; i < kTM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + row_of(i, r);
            const int my = fastdiv ? (int)(((unsigned long long)(unsigned)m * magic) >> 40) : m / p.Wm;
            const int mx = m - my * p.Wm;
            const int oy = my * p.ostride + ph.oy0, ox = mx * p.ostride + ph.ox0;
            const bool ok = m < p.M && oy < p.Hout && ox < p.Wout;
            const unsigned poff = (unsigned)((oy * p.Wout + ox) * p.Cout_s) * 4u;
#pragma unroll
            for (int j = 0; j < kTN; ++j)
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc[i][j][r]), ysrd, (int)(ok ? poff + coff[j] : kDrop), 0, 0);
        }
}

template <bool STATS>
hipError_t launch_split(hipStream_t s, const ConvKParams& p) {
    constexpr auto kern = conv_igemm_split_kernel<STATS>;
    const hipError_t e = optin_dynamic_lds<kern>(kSplitLds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(p.mtiles * p.ntiles * p.nphases), dim3(512), kSplitLds, s, p);
    return hipGetLastError();
}

}  // namespace
}  // namespace t2v

using namespace t2v;

extern "C" {

int t2v_split_interface(void) { return kSplitInterface; }

int t2v_split_launch_pairs(hipStream_t s, const float* x, float* y, long n4, int grid) {
    hipLaunchKernelGGL(split_pairs_kernel, dim3(grid), dim3(256), 0, s, reinterpret_cast<const float4*>(x), reinterpret_cast<uint4*>(y), n4);
    return (int)hipGetLastError();
}

int t2v_split_launch_conv(hipStream_t s, const ConvKParams* p) {
    return (int)(p->stats ? launch_split<true>(s, *p) : launch_split<false>(s, *p));
}

int t2v_split_launch_norm_apply(hipStream_t s, const float* x, const float* mean_rstd, const float* gamma, const float* beta,
                                const float* res1, float* y, long n4, int C4, int relu, int grid, int nimg) {
    hipLaunchKernelGGL(inorm_apply_split_kernel, dim3(grid, nimg), dim3(256), 0, s, reinterpret_cast<const float4*>(x),
                       reinterpret_cast<const float4*>(mean_rstd), reinterpret_cast<const float4*>(gamma),
                       reinterpret_cast<const float4*>(beta), reinterpret_cast<const float4*>(res1), reinterpret_cast<uint4*>(y), n4,
                       C4, relu);
    return (int)hipGetLastError();
}

}  // extern "C"
