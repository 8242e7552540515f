// polyphase.hip -- polyphase Winograd F(4,2) for the generator's stride-2 3x3 convolutions ("down") and their transposed
// counterparts ConvTranspose2d(3, stride 2, pad 1, output_padding 1) ("up") on gfx950.  SURVEY.md section 8a rows a6 / a8.
//
// Per dimension a stride-2 3x3 conv is a 2-tap correlation on the odd input samples (taps 0 and 2) plus a 1-tap one on the
// even samples (tap 1); the transposed conv is a 2-tap correlation that makes the odd outputs (taps 2 and 0) plus a 1-tap one
// that makes the even outputs.  The 2-tap parts run as Winograd F(4,2) -- 5 products per 4 outputs --, the 1-tap parts as they
// are: 9 "positions" per dimension, 81 per tile (4x4 outputs of a down conv = a 9x9 input patch at stride 8; 8x8 outputs of an
// up conv = a 5x5 input patch at stride 4) against the direct form's 144 multiply-adds per tile and channel pair: 0.5625x the
// MFMA work, and milder in fp32 than F(4x4,3x3) (2.0e-6 against the direct conv's 1.4e-6 on unit-variance data).
//   V[pos][tile][c] = (B d B^T)[pr][pc]        input transform (this file)
//   M[pos][tile][n] = sum_c V[pos][tile][c] U[pos][n][c]     81 batched GEMMs [T x Cin] x [Cin x Cout]: the fixed-grid kernel
//                                                             of the ResnetBlock convs (conv_igemm.hip: wino_gemm_sk_kernel)
//   y = A M A^T + bias, norm statistics partials              output transform (this file)
// with pos = pr * 9 + pc; pr, pc in 0..4 = the F(4,2) positions, 5..8 = the four 1-tap samples.  Matrices: polyphase_consts.h
// (scripts/gen_polyphase_consts.py; checked against torch in fp64 there).  It pays where the transforms (V is 81/64 of a down
// conv's input and M 81/16 of its output; 81/16 and 81/64 for an up conv) are small against the GEMM: the 512<->1024 and
// 256<->512 layers (csrc/capi.hip: polyphase_supported); the wider, shallower maps stay on the implicit-GEMM kernel.
#include "t2v_internal.h"
#include "norm_pool.h"
#include "polyphase_consts.h"
#include "transform_common.h"

namespace t2v {

// at most 65535 x 16 blocks: the cap decides how many tiles a thread of the grid-stride transforms walks
static inline int pp_grid(long n, int block) { return capped_grid(n, block, 65535L * 16); }

// B^T of F(4,2) (5 x 5) = rows 0..4 of pp::kBU;  A^T (4 x 5) = the first five columns of pp::kAD: cdot takes both in place

// ---- weights: U[pr*9+pc][n][c] = sum_{a,b} G[pr][a] G[pc][b] g[a][b], in fp64, rounded once ---------------------------------------
// UP = false: w is Conv2d's [Cout][Cin][3][3]; UP = true: ConvTranspose2d's [Cin][Cout][3][3]
template <bool UP>
__global__ void polyphase_weight_kernel(const float* __restrict__ w, float* __restrict__ U, int Cout, int Cin, int Cout_p,
                                        int Cin_s) {
    const long total = (long)Cout_p * Cin_s;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int n = (int)(i / Cin_s), c = (int)(i - (long)n * Cin_s);
        double g[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const size_t at = UP ? (((size_t)c * Cout + n) * 3 + a) * 3 + b : (((size_t)n * Cin + c) * 3 + a) * 3 + b;
                g[a][b] = (n < Cout && c < Cin) ? (double)w[at] : 0.0;
            }
        polyphase_weight_transform<UP>(g, [&](int pos, float u) { U[(size_t)pos * Cout_p * Cin_s + (size_t)n * Cin_s + c] = u; });
    }
}
int launch_polyphase_weight(hipStream_t s, const float* w, float* U, int Cout, int Cin, int Cout_p, int Cin_s, int up,
                            bool split) {
    const int grid = pp_grid((long)Cout_p * Cin_s, 256);
    if (split) return launch_polyphase_weight_split(s, w, U, Cout, Cin, Cout_p, Cin_s, up, grid);
    if (up)
        hipLaunchKernelGGL(polyphase_weight_kernel<true>, dim3(grid), dim3(256), 0, s, w, U, Cout, Cin, Cout_p, Cin_s);
    else
        hipLaunchKernelGGL(polyphase_weight_kernel<false>, dim3(grid), dim3(256), 0, s, w, U, Cout, Cin, Cout_p, Cin_s);
    T2V_HIP_CHECK(hipGetLastError());
    return T2V_OK;
}

// ---- input transform --------------------------------------------------------------------------------------------------------------
// UP: one thread = one tile x 2 channels; DOWN: one thread = one of the tile's four sub-blocks x 2 channels (below).
// DOWN: the tile's 9 x 9 patch starts at input (8 ty - 1, 8 tx - 1) (zero padding 1); its
// even patch indices 0, 2, .., 8 are the odd-phase samples (F(4,2) input, 5 of them), the odd indices 1, 3, 5, 7 the even-phase
// samples (taken as they are).  UP: the 5 x 5 patch starts at input (4 ty, 4 tx) (zeros past the map); all five samples feed
// F(4,2), the first four are also the 1-tap samples.  The four (transformed | plain) x (transformed | plain) sub-blocks are
// done one after the other, so that at most 25 values per channel are live.  The DOWN form gives each sub-block a thread of its
// own (sub-block = bits above the channel pair of the flat index, uniform over a wave): four times the threads with 16-25 loads
// each instead of 81 -- the 512 -> 1024 layer's 256 tiles x 256 channel pairs are 1024 blocks instead of 256 -- and every V
// element comes from the same cdot calls on the same loads as before.
// NORM: x is the previous layer's conv output that has not gone through its norm layer yet; the transform applies
// relu((x - mean) * rstd [* gamma + beta]) on the fly -- by norm_apply (transform_common.h), the function inorm_apply_kernel
// calls, so the result is bit-identical to apply-then-transform -- and that layer's apply pass (a read and a write of the map) is dropped.  The zero
// padding pads the NORMALISED map: samples outside stay exact zeros.
template <bool UP, bool NORM>
__global__ __launch_bounds__(256) void polyphase_input_kernel(const float2* __restrict__ x, float2* __restrict__ V, int H, int W,
                                                             int C2, int TW, int T, int Tt,
                                                             const float2* __restrict__ mean_rstd,
                                                             const float2* __restrict__ gamma,
                                                             const float2* __restrict__ beta, int relu) {
    constexpr int NSUB = UP ? 1 : 4;
    const PolyInput in{x, H, W, C2, TW, T, mean_rstd, gamma, beta, relu};
    const long total = (long)Tt * NSUB * C2, pitch = (long)Tt * C2;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const long ts = i / C2;
        const int c2 = (int)(i - ts * C2);
        const long tile = ts / NSUB;
        const int sub = (int)(ts - tile * NSUB);      // DOWN: 0 = (1), .., 3 = (4) of polyphase_input_item; UP: all four
        float2* const Vt = V + (tile * C2 + c2);      // this thread's element of position 0; the positions are Tt * C2 apart
        polyphase_input_item<UP, NORM>(in, tile, sub, c2, [&](int pos, float2 v) { Vt[pos * pitch] = v; });
    }
}
// H, W: the INPUT map; tiles: 4x4 outputs of the H/2 x W/2 map (down) | 4x4 inputs (up); Tt = padded tile rows of V.
// lazy != null: x still has to go through its norm layer (relu: 0 | 1 after it)
int launch_polyphase_input(hipStream_t s, const float* x, float* V, int H, int W, int C, int up, int Tt, const LazyNorm* lazy,
                           bool split) {
    const LazyNorm none{};
    const LazyNorm& ln = lazy ? *lazy : none;
    T2V_REQUIRE((ln.gamma == nullptr) == (ln.beta == nullptr) && (ln.relu == 0 || ln.relu == 1) && !ln.res && !ln.xout,
                "polyphase_input: bad norm arguments");
    const TileGrid tg = up ? tile_grid(H, W, 4) : tile_grid(H / 2, W / 2, 4);
    const int grid = pp_grid((long)Tt * (up ? 1 : 4) * (C / 2), 256);
    if (split) return launch_polyphase_input_split(s, x, V, H, W, C, up, tg, Tt, ln, grid);
    auto kern = up ? (ln.mean_rstd ? polyphase_input_kernel<true, true> : polyphase_input_kernel<true, false>)
                   : (ln.mean_rstd ? polyphase_input_kernel<false, true> : polyphase_input_kernel<false, false>);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, s, reinterpret_cast<const float2*>(x), reinterpret_cast<float2*>(V), H, W,
                       C / 2, tg.TW, tg.T, Tt, reinterpret_cast<const float2*>(ln.mean_rstd),
                       reinterpret_cast<const float2*>(ln.gamma), reinterpret_cast<const float2*>(ln.beta), ln.relu);
    T2V_HIP_CHECK(hipGetLastError());
    return T2V_OK;
}

// ---- output transform, down: y (4 x 4 per tile) = A M A^T + bias; block = 64 channels x 4 tile lanes, 8 tiles = 128 pixels ------
__global__ __launch_bounds__(256) void polyphase_output_down_kernel(const float* __restrict__ Mm, const float* __restrict__ bias,
                                                                    float* __restrict__ y, float2* __restrict__ stats, int Ho,
                                                                    int Wo, int N, int TW, int T, int Tt) {
    __shared__ float sh[4][64];
    output_transform_4x4<9>(pp::kAD, Mm, bias, y, stats, Ho, Wo, N, TW, T, Tt, sh, [](float v) { return v; });
}

// ---- output transform, up: y (8 x 8 per tile) = A M A^T + bias; a thread makes HALF a tile (4 output rows x 8 columns = 32
// values), block = 64 channels x 4 lanes = 2 tiles = 128 pixels: the statistics partial of 8 x 8 tiles (wm = 8) ------------------
__global__ __launch_bounds__(256) void polyphase_output_up_kernel(const float* __restrict__ Mm, const float* __restrict__ bias,
                                                                  float* __restrict__ y, float2* __restrict__ stats, int Ho,
                                                                  int Wo, int N, int TW, int T, int Tt) {
    __shared__ float sh[4][64];
    const int cl = threadIdx.x & 63, tl = threadIdx.x >> 6;
    const int n = blockIdx.y * 64 + cl;
    const bool ok = n < N;
    const float bv = (ok && bias) ? bias[n] : 0.f;
    const long tile = (long)blockIdx.x * 2 + (tl >> 1);
    const int half = tl & 1;                     // output rows 4*half .. 4*half + 3 of the tile
    const bool tv = tile < T;
    // the four output rows of this half: 8h (plain 2h), 8h+1 (F(4,2) output 2h), 8h+2 (plain 2h+1), 8h+3 (F(4,2) output 2h+1)
    float r[4][9];
#pragma unroll
    for (int pc = 0; pc < 9; ++pc) {
        float m[5];
#pragma unroll
        for (int pr = 0; pr < 5; ++pr) m[pr] = (ok && tv) ? Mm[((long)(pr * 9 + pc) * Tt + tile) * N + n] : 0.f;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int q = 2 * half + k;                                  // plain sample / F(4,2) output index 0..3
            r[2 * k][pc] = (ok && tv) ? Mm[((long)((5 + q) * 9 + pc) * Tt + tile) * N + n] : 0.f;
            r[2 * k + 1][pc] = half ? (k ? cdot<5>(pp::kAD[3], m) : cdot<5>(pp::kAD[2], m)) : (k ? cdot<5>(pp::kAD[1], m) : cdot<5>(pp::kAD[0], m));
        }
    }
    const int ty = (int)(tile / TW), tx = (int)(tile - (long)ty * TW);
    float out[32];
    unsigned mask = 0;
#pragma unroll
    for (int i2 = 0; i2 < 4; ++i2)
#pragma unroll
        for (int j2 = 0; j2 < 8; ++j2) {
            const float v = cdot<9>(pp::kAU[j2], r[i2]) + bv;
            out[i2 * 8 + j2] = v;
            const int oy = 8 * ty + 4 * half + i2, ox = 8 * tx + j2;
            if (tv && oy < Ho && ox < Wo) {
                mask |= 1u << (i2 * 8 + j2);
                if (ok) y[((long)oy * Wo + ox) * N + n] = v;
            }
        }
    block_stats_128(out, mask, sh, tl, cl, ok, stats, N, n);
}
// Ho, Wo: the OUTPUT map
int launch_polyphase_output(hipStream_t s, const float* Mm, const float* bias, float* y, float* stats, int Ho, int Wo, int N,
                            int up, int Tt) {
    const TileGrid tg = tile_grid(Ho, Wo, up ? 8 : 4);
    const int TW = tg.TW, T = tg.T, Tp = tg.Tp;
    if (up)
        hipLaunchKernelGGL(polyphase_output_up_kernel, dim3(Tp / 2, (N + 63) / 64), dim3(256), 0, s, Mm, bias, y,
                           reinterpret_cast<float2*>(stats), Ho, Wo, N, TW, T, Tt);
    else
        hipLaunchKernelGGL(polyphase_output_down_kernel, dim3(Tp / 8, (N + 63) / 64), dim3(256), 0, s, Mm, bias, y,
                           reinterpret_cast<float2*>(stats), Ho, Wo, N, TW, T, Tt);
    T2V_HIP_CHECK(hipGetLastError());
    return T2V_OK;
}

}  // namespace t2v
