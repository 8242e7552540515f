// winograd_split.hip -- T2V_ALGO_WINOGRAD_F4_BF16X2: the F(4x4,3x3) convolution with its 36 GEMMs on the bf16 matrix cores.
//
// An fp32 value v is split into two bf16 terms, hi = bf16_rne(v) and lo = bf16_rne(v - float(hi)) (the subtraction is exact
// in fp32), and a contraction over K is evaluated as  sum_k (ah*bh + ah*bl + al*bh)  with v_mfma_f32_32x32x16_bf16: every
// product of two bf16 values is exact in the fp32 accumulator, al*bl (<= 2^-18 of the term) is dropped.  Everything outside
// the GEMMs stays fp32 and is the arithmetic of winograd.hip: the input transform and the filter transform call the same
// device functions (transform_common.h) and split the finished fp32 value on its way out, the output transform is
// winograd4_output_kernel itself.
//   winograd4_input_split_kernel  : V planes [2][36][Tt][C] bf16 (hi plane, lo plane) -- the bytes of the fp32 V
//   winograd4_weight_split_kernel : U planes [2][36][Cout][Cin] bf16                   -- the bytes of the fp32 U
//   wino_split_gemm_kernel        : M[pos][t][n] = V[pos][t] . U[pos][n], fp32 [npos][Tt][N]; npos = 36 here, 81 for the
//                                   polyphase F(4,2) layers, whose split-emitting transforms are in polyphase_split.hip
// One block per 128 x 128 output tile, nothing shared between blocks: every output is one block's fixed-order chain.
#include "t2v_internal.h"
#include "k_loops.h"
#include "transform_common.h"

namespace t2v {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// winograd4_input_kernel<MODE> (winograd.hip) with the split store; packed batch layout (image i owns rows [i*T, (i+1)*T) of
// every position, the last image also the rows that pad the total to Tt).  Vp: [2][36][Tt][C2] channel pairs.
// XCD: the channel-slice grid of winograd4_input_kernel<MODE, true> (C2 % 512 == 0; grid.x = xcd_slice_grid()).
template <int MODE, bool XCD>
__global__ __launch_bounds__(256) void winograd4_input_split_kernel(const float2* __restrict__ x, unsigned* __restrict__ Vp, int H,
                                                                    int W, int C2, int TW, int T, int pad, int reflect, int Tt,
                                                                    const float2* __restrict__ mean_rstd,
                                                                    const float2* __restrict__ gamma,
                                                                    const float2* __restrict__ beta,
                                                                    const float2* __restrict__ res, float2* __restrict__ xout,
                                                                    long img_stride, int last_tiles) {
    const long im = blockIdx.y;
    x += im * img_stride;
    const int t0 = (int)im * T;
    if (MODE) mean_rstd += im * 2 * C2;
    if (MODE == 2) {
        res += im * img_stride;
        xout += im * img_stride;
    }
    const int ntiles = blockIdx.y == gridDim.y - 1 ? last_tiles : T;
    const Wino4Input in{x, H, W, C2, TW, T, pad, reflect, mean_rstd, gamma, beta, res, xout};
    const long plane = (long)36 * Tt * C2;
    auto item = [&](const long tile, const int c2) {
        winograd4_input_item<MODE>(in, tile, c2, [&](int xi, float2 v) {
            const SplitPair sp = split_bf16x2(v);
            const long at = ((long)xi * Tt + t0 + tile) * C2 + c2;
            Vp[at] = sp.hi;
            Vp[plane + at] = sp.lo;
        });
    };
    if constexpr (XCD) {
        // a wave = one tile x one 64-pair slice, XCD x (block b runs on XCD b % 8) owns the slices {x, x + 8, ..} of all tiles
        const long it = (long)(blockIdx.x >> 3) * 4 + (threadIdx.x >> 6);
        if (it < (long)(C2 >> 9) * ntiles) {
            const int sl = (int)(it / ntiles);
            item(it - (long)sl * ntiles, ((sl << 3) + (int)(blockIdx.x & 7)) * 64 + (int)(threadIdx.x & 63));
        }
    } else {
        const long total = (long)ntiles * C2;
        const long stride = (long)gridDim.x * blockDim.x;
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
            const long tile = i / C2;
            item(tile, (int)(i - tile * C2));
        }
    }
}

// winograd4_weight_kernel (winograd.hip) with the split store: Up [2][36][Cout_p][Cin_s] bf16
__global__ void winograd4_weight_split_kernel(const float* __restrict__ w, u16* __restrict__ Up, int Cout, int Cin, int Cout_p,
                                              int Cin_s) {
    const long total = (long)Cout_p * Cin_s;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int n = (int)(i / Cin_s), c = (int)(i - (long)n * Cin_s);
        double g[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) g[a][b] = (n < Cout && c < Cin) ? (double)w[(((size_t)n * Cin + c) * 3 + a) * 3 + b] : 0.0;
        winograd4_weight_transform(g, [&](int pos, float u) {
            store_split_planes(Up, (size_t)pos * total + i, (size_t)36 * total, u);
        });
    }
}

// ---- the GEMM stage.  128 x 128 output tile per block; 4 MFMA waves (64 x 64 each, 2 x 2 fragments of 32 x 32) and 4 loader
// waves.  The loaders fill a ring of kRing stages of K = 32 by LDS-DMA (buffer_load ... lds, 16 bytes per lane): a stage is
// [plane][A | B][64 LDS rows][128 bytes], an LDS row holding two 32-element bf16 matrix rows, its eight 16-byte slots XOR-swizzled
// with the row index on the SOURCE address so that a fragment read (ds_read_b128 per lane) is conflict-free.  Synchronisation:
// the loaders keep kRing - 1 stages in flight, wait with a counted vmcnt until all but the newest have landed and meet the MFMA
// waves at ONE barrier per stage; a slot is refilled only after the barrier behind its last read.  Both wave kinds execute
// nk + 1 barriers for every nk >= 1 (stages past the end re-load the last one: same instruction count per stage, so the
// vmcnt constants hold for K / 32 below the ring depth as well).  The loaders' loop is k_loops.h's loader_k_loop.  The
// MFMA waves' loop below is conv_igemm_split_kernel's written out a second time, on purpose: with both loops shared this kernel's
// GEMM stage ran 0.4 % slower at the trunk shapes (0.8 % with the guard on the last prefetch kept, 0.45 % with this loop
// inline and the guard dropped); with the loader loop alone shared it runs as before (profiles/split_shared_times.txt).
// A trailing half tile (Tt % 128 == 64): its loaders re-read rows 0..63 for the missing ones, the MFMA waves of those rows
// skip their work (not their barriers) and store nothing.
constexpr int kBM = 128, kBN = 128, kSBK = 32, kRing = 3;
constexpr int kStageBytes = 2 * 2 * 64 * 128;      // [plane][A|B][64 LDS rows][128 B] = 32 KiB
constexpr int kLd = 8;                             // DMA instructions per loader wave and stage
constexpr int kSplitGemmLds = kRing * kStageBytes; // 96 KiB

__global__ __launch_bounds__(512) void wino_split_gemm_kernel(const u16* __restrict__ A, const u16* __restrict__ B,
                                                              float* __restrict__ C, int npos, int Tt, int N, int K,
                                                              int mtiles, int ntiles) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool is_loader = wave >= 4;
    const int wid = wave & 3;
    // block -> tile: a contiguous run of tiles per XCD (block b runs on XCD b % 8: relied on for speed only)
    const int tile = xcd_band(blockIdx.x, gridDim.x);
    const int per_pos = mtiles * ntiles;
    const int p = tile / per_pos, rest = tile - p * per_pos;
    const int mt = rest / ntiles, nt = rest - mt * ntiles;
    const int m0 = mt * kBM, n0 = nt * kBN;
    const int nk = K / kSBK;
    const bool half = m0 + 64 >= Tt;      // only rows m0 .. m0 + 63 exist

    if (is_loader) {
        const unsigned a_bytes = (unsigned)((size_t)2 * npos * Tt * K * 2), b_bytes = (unsigned)((size_t)2 * npos * N * K * 2);
        int voff[kLd];
#pragma unroll
        for (int n = 0; n < kLd; ++n) {
            const int plane = n / 4, op = (n % 4) / 2, rb = ((n % 4) % 2) * 4 + wid;
            const int rho = rb * 8 + (lane >> 3), slot = lane & 7;
            const int sp = slot ^ ((rho >> 1) & 7);
            int r = 2 * rho + (sp >> 2);
            const int kc = sp & 3;
            if (op == 0 && half) r &= 63;
            voff[n] = op == 0 ? (((plane * npos + p) * Tt + m0 + r) * K + kc * 8) * 2 : (((plane * npos + p) * N + n0 + r) * K + kc * 8) * 2;
        }
        auto issue_stage = [&](int kt, int slot) {
#pragma unroll
            for (int n = 0; n < kLd; ++n) {
                const int plane = n / 4, op = (n % 4) / 2, rb = ((n % 4) % 2) * 4 + wid;
                char* dst = smem + slot * kStageBytes + ((plane * 2 + op) * 64 + rb * 8) * 128;
                if (op == 0)
                    dma16(A, a_bytes, dst, voff[n], kt * (kSBK * 2));
                else
                    dma16(B, b_bytes, dst, voff[n], kt * (kSBK * 2));
            }
        };
        loader_k_loop<kRing, kLd>(0, nk, issue_stage);   // (ends with vmcnt(0): nothing lands in this block's LDS after it)
        return;
    }

    const int wm = wid >> 1, wn = wid & 1;
    const int fr = lane & 31, g = lane >> 5;
    const int fsw = (fr >> 2) & 7;
    const bool active = !(half && wm == 1);
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    bf16x8 af[2][2][2], bfr[2][2][2];   // [register set][fragment][plane]
    auto load_frags = [&](int buf, int q, int set) {
        const char* st = smem + buf * kStageBytes;
        const int slot = ((((fr & 1) * 4) + 2 * q + g) ^ fsw) * 16;
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
                af[set][i][pl] = *reinterpret_cast<const bf16x8*>(st + ((pl * 2 + 0) * 64 + wm * 32 + i * 16 + (fr >> 1)) * 128 + slot);
#pragma unroll
            for (int j = 0; j < 2; ++j)
                bfr[set][j][pl] = *reinterpret_cast<const bf16x8*>(st + ((pl * 2 + 1) * 64 + wn * 32 + j * 16 + (fr >> 1)) * 128 + slot);
        }
    };
    auto mfmas = [&](int set) {      // lo*hi, hi*lo, hi*hi per 16-deep half stage
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[set][i][1], bfr[set][j][0], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[set][i][0], bfr[set][j][1], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[set][i][0], bfr[set][j][0], acc[i][j], 0, 0, 0);
            }
    };

    __syncthreads();   // B0
    if (active) load_frags(0, 0, 0);
    int buf = 0;
    for (int kt = 0; kt < nk; ++kt) {
        const int nbuf = buf == kRing - 1 ? 0 : buf + 1;
        __builtin_amdgcn_sched_barrier(0);
        if (active) {
            load_frags(buf, 1, 1);
            mfmas(0);
        }
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();   // barrier(kt): slot `buf` fully read, stage kt + 1 visible
        __builtin_amdgcn_sched_barrier(0);
        if (active) {
            if (kt + 1 < nk) load_frags(nbuf, 0, 0);
            mfmas(1);
        }
        buf = nbuf;
    }
    if (!active) return;

#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * g;
                const int col = n0 + wn * 64 + j * 32 + fr;
                C[((size_t)p * Tt + row) * N + col] = acc[i][j][r];
            }
}

}  // namespace

int launch_winograd4_input_split(hipStream_t s, int mode, const float* x, float* V, int H, int W, int C, const TileGrid& tg,
                                 int pad, int reflect, int Tt, int nimg, long img_stride, int last_tiles, const LazyNorm& ln,
                                 unsigned xcd_grid) {
    // xcd_grid: grid.x of the channel-slice form for this shape (winograd.hip: xcd_slice_grid), 0 where it does not apply
    auto kern = xcd_grid ? (mode == 0 ? winograd4_input_split_kernel<0, true> : mode == 1 ? winograd4_input_split_kernel<1, true> : winograd4_input_split_kernel<2, true>)
                         : (mode == 0 ? winograd4_input_split_kernel<0, false> : mode == 1 ? winograd4_input_split_kernel<1, false> : winograd4_input_split_kernel<2, false>);
    const long most = last_tiles > tg.T ? last_tiles : tg.T;
    hipLaunchKernelGGL(kern, dim3(xcd_grid ? xcd_grid : capped_grid(most * (C / 2), 256, 4096), nimg), dim3(256), 0, s,
                       reinterpret_cast<const float2*>(x), reinterpret_cast<unsigned*>(V), H, W, C / 2, tg.TW, tg.T, pad, reflect, Tt,
                       reinterpret_cast<const float2*>(ln.mean_rstd), reinterpret_cast<const float2*>(ln.gamma),
                       reinterpret_cast<const float2*>(ln.beta), reinterpret_cast<const float2*>(ln.res),
                       reinterpret_cast<float2*>(ln.xout), img_stride / 2, last_tiles);
    T2V_HIP_CHECK(hipGetLastError());
    return T2V_OK;
}

int launch_winograd4_weight_split(hipStream_t s, const float* w, float* U, int Cout, int Cin, int Cout_p, int Cin_s) {
    hipLaunchKernelGGL(winograd4_weight_split_kernel, dim3(capped_grid((long)Cout_p * Cin_s, 256, 4096)), dim3(256), 0, s, w,
                       reinterpret_cast<u16*>(U), Cout, Cin, Cout_p, Cin_s);
    T2V_HIP_CHECK(hipGetLastError());
    return T2V_OK;
}

// npos transform positions: 36 (F(4x4,3x3)) | 81 (polyphase F(4,2))
bool wino_split_gemm_ok(int npos, int Tt, int K, int N) {
    return (npos == 36 || npos == 81) && Tt >= 64 && Tt % 64 == 0 && N >= kBN && N % kBN == 0 && K >= kSBK && K % kSBK == 0 &&
           // 32-bit byte offsets into each operand's buffer resource (two planes of npos * rows * K bf16: the bytes of the
           // fp32 tensor), and a 31-bit grid
           (long)npos * Tt * K * 4 < 0x7fff0000L && (long)npos * N * K * 4 < 0x7fff0000L &&
           (long)npos * ((Tt + kBM - 1) / kBM) * (N / kBN) < 0x7fffffffL;
}

// V planes [2][npos][Tt][K], U planes [2][npos][N][K] (bf16) -> M [npos][Tt][N] fp32
int launch_wino_split_gemm(hipStream_t s, int npos, const float* V, const float* U, float* M, int Tt, int K, int N) {
    T2V_REQUIRE(wino_split_gemm_ok(npos, Tt, K, N), "split-bf16 gemm: %d positions, Tt=%d (%% 64), K=%d (%% 32), N=%d (%% 128) not supported",
                npos, Tt, K, N);
    T2V_HIP_CHECK(optin_dynamic_lds<wino_split_gemm_kernel>(kSplitGemmLds));
    const int mtiles = (Tt + kBM - 1) / kBM, ntiles = N / kBN;
    hipLaunchKernelGGL(wino_split_gemm_kernel, dim3(npos * mtiles * ntiles), dim3(512), kSplitGemmLds, s,
                       reinterpret_cast<const u16*>(V), reinterpret_cast<const u16*>(U), M, npos, Tt, N, K, mtiles, ntiles);
    T2V_HIP_CHECK(hipGetLastError());
    return T2V_OK;
}

}  // namespace t2v
