// transform_common.h -- device functions shared by the transform passes around the batched per-position GEMM (winograd.hip,
// polyphase.hip) and by the norm kernels whose arithmetic those passes fold in (elementwise.hip).  Every piece exists once:
// a kernel that applies a norm "on the fly" calls the function the stand-alone norm kernel calls, so the two agree bit for
// bit by construction (the build uses -ffp-contract=off: inlining into different kernels cannot change a result).
#pragma once
#include <hip/hip_runtime.h>
#include "polyphase_consts.h"
#include "winograd_f4_consts.h"

namespace t2v {

// sum_k row[k] * v[k] over the first K entries of a row of a constant matrix.  Zero coefficients are skipped and the first
// term is not an add (compile-time after unrolling: x * 0 is not foldable under IEEE rules).
template <int K, int R>
__device__ __forceinline__ float cdot(const double (&row)[R], const float (&v)[K]) {
    static_assert(K <= R, "cdot: more values than coefficients");
    float acc = 0.f;
    bool first = true;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (row[k] != 0.0) {
            const float t = (float)row[k] * v[k];
            acc = first ? t : acc + t;
            first = false;
        }
    }
    return acc;
}
// ... down column `col` of the matrix: sum_k m[k][col] * v[k], the product with the transposed matrix.  V: float, or float2
// for a channel pair (component-wise)
template <int K, int R, int C, class V>
__device__ __forceinline__ V cdot_col(const double (&m)[R][C], int col, const V (&v)[K]) {
    static_assert(K <= R, "cdot_col: more values than coefficients");
    V acc{};
    bool first = true;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (m[k][col] != 0.0) {
            const V t = (float)m[k][col] * v[k];
            acc = first ? t : acc + t;
            first = false;
        }
    }
    return acc;
}

// The consumer side of a norm layer, per value, in two steps: (x - mean) * rstd [* gamma + beta], then the activation
// (relu: 0 none, 1 ReLU, 2 LeakyReLU(0.2)).  inorm_apply_kernel and the input transforms that take a conv output before
// its norm all call these.
__device__ __forceinline__ float norm_scale(float x, float mean, float rstd) { return (x - mean) * rstd; }
__device__ __forceinline__ float norm_affine(float v, float gamma, float beta) { return v * gamma + beta; }
__device__ __forceinline__ float norm_act(float v, int relu) {
    return relu == 1 ? fmaxf(v, 0.f) : (relu == 2 ? (v > 0.f ? v : 0.2f * v) : v);
}
__device__ __forceinline__ float norm_apply(float x, float mean, float rstd, bool affine, float gamma, float beta, int relu) {
    const float v = norm_scale(x, mean, rstd);
    return norm_act(affine ? norm_affine(v, gamma, beta) : v, relu);
}

// The norm backward, per value: xhat and g = dy * act'(gamma * xhat + beta) (what the per-channel sums S0 = sum g,
// S1 = sum g * xhat are made of), then dx = rstd * gamma * (g - S0/N - xhat * S1/N) with k0 = S0/N, k1 = S1/N.
__device__ __forceinline__ float act_grad(float pre, int relu) {
    return relu == 1 ? (pre > 0.f ? 1.f : 0.f) : (relu == 2 ? (pre > 0.f ? 1.f : 0.2f) : 1.f);
}
struct NormBwdTerms {
    float xh, g;
};
__device__ __forceinline__ NormBwdTerms norm_bwd_terms(float x, float dy, float mean, float rstd, float gamma, float beta,
                                                       int relu) {
    const float xh = (x - mean) * rstd;
    return {xh, dy * act_grad(gamma * xh + beta, relu)};
}
__device__ __forceinline__ float norm_bwd_dx(const NormBwdTerms& t, float rstd, float gamma, float k0, float k1) {
    return rstd * gamma * (t.g - k0 - t.xh * k1);
}

// (mean, M2) of a block's <= 128 valid output pixels per channel: each of the 4 tile lanes holds 32 pixel
// slots, `mask` marks the ones inside the image (all of them except in ragged / padding tiles).  Two passes,
// tree-summed (exact for constant maps over power-of-two counts), written as the partial inorm_finalize
// merges; the partial's pixel count is recomputed there from the geometry.
__device__ __forceinline__ void block_stats_128(const float (&val)[32], unsigned mask, float (*sh)[64], int tl, int cl,
                                                bool ok, float2* __restrict__ stats, int N, int n) {
    if (stats == nullptr) return;
    sh[tl][cl] = (float)__popc(mask);
    __syncthreads();
    const float cnt = (sh[0][cl] + sh[1][cl]) + (sh[2][cl] + sh[3][cl]);
    __syncthreads();
    const float inv_cnt = cnt > 0.f ? 1.f / cnt : 0.f;
    float mean_b = 0.f;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        float v[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const float dlt = val[i] - mean_b;
            v[i] = ((mask >> i) & 1u) ? (pass ? dlt * dlt : val[i]) : 0.f;
        }
#pragma unroll
        for (int w = 16; w >= 1; w >>= 1)
#pragma unroll
            for (int i = 0; i < w; ++i) v[i] += v[i + w];
        sh[tl][cl] = v[0];
        __syncthreads();
        const float tot = (sh[0][cl] + sh[1][cl]) + (sh[2][cl] + sh[3][cl]);
        __syncthreads();
        if (pass == 0) {
            mean_b = tot * inv_cnt;
        } else if (tl == 0 && ok) {
            stats[(size_t)blockIdx.x * N + n] = make_float2(mean_b, tot);
        }
    }
}

// Output transform of tiles of 4x4 outputs from P x P positions: y = AT M AT^T + bias with AT [4][P] (F(4x4,3x3): P = 6,
// polyphase down: P = 9).  Block = 64 channels x 4 tile lanes, 8 tiles (2 per thread) = 128 output pixels => one
// (mean_b, M2_b) statistics partial per block.  Mm is [P*P][Tt][N] and its first T tile rows are this map's; y [Ho][Wo][N]
// receives act(v) (the statistics see v).  sh: the block's __shared__ float [4][64].
template <int P, class Act>
__device__ __forceinline__ void output_transform_4x4(const double (&AT)[4][P], const float* Mm, const float* bias, float* y,
                                                     float2* stats, int Ho, int Wo, int N, int TW, int T, int Tt,
                                                     float (*sh)[64], Act act) {
    const int cl = threadIdx.x & 63, tl = threadIdx.x >> 6;
    const int n = blockIdx.y * 64 + cl;
    const bool ok = n < N;
    const float bv = (ok && bias) ? bias[n] : 0.f;
    float out[32];
    unsigned mask = 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const long tile = (long)blockIdx.x * 8 + tl + 4 * i;
        const bool tv = tile < T;
        float r[4][P];   // r[i2][b] = sum_a AT[i2][a] m[a][b]
#pragma unroll
        for (int b = 0; b < P; ++b) {
            float m[P];
#pragma unroll
            for (int a = 0; a < P; ++a) m[a] = (ok && tv) ? Mm[((long)(a * P + b) * Tt + tile) * N + n] : 0.f;
#pragma unroll
            for (int i2 = 0; i2 < 4; ++i2) r[i2][b] = cdot<P>(AT[i2], m);
        }
        const int ty = (int)(tile / TW), tx = (int)(tile - (long)ty * TW);
#pragma unroll
        for (int i2 = 0; i2 < 4; ++i2)
#pragma unroll
            for (int j2 = 0; j2 < 4; ++j2) {
                const float v = cdot<P>(AT[j2], r[i2]) + bv;
                out[i * 16 + i2 * 4 + j2] = v;
                const int oy = 4 * ty + i2, ox = 4 * tx + j2;
                if (tv && oy < Ho && ox < Wo) {
                    mask |= 1u << (i * 16 + i2 * 4 + j2);
                    if (ok) y[((long)oy * Wo + ox) * N + n] = act(v);
                }
            }
    }
    block_stats_128(out, mask, sh, tl, cl, ok, stats, N, n);
}

// ---- F(4x4,3x3) input and weight transforms with a store policy: the fp32 kernels of winograd.hip and the split-bf16 ones
// of winograd_split.hip run the same arithmetic and differ only in what `store` does with a finished value.
// U[pos] = (G g G^T)[pos] of one (n, c) filter: transformed in fp64, rounded once; store(pos, u)
template <class Store>
__device__ __forceinline__ void winograd4_weight_transform(const double (&g)[3][3], Store store) {
    double t[6][3];
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) t[a][b] = f4::kG[a][0] * g[0][b] + f4::kG[a][1] * g[1][b] + f4::kG[a][2] * g[2][b];
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            const double u = t[a][0] * f4::kG[b][0] + t[a][1] * f4::kG[b][1] + t[a][2] * f4::kG[b][2];
            store(a * 6 + b, (float)u);
        }
}

// One image's view of an F(4x4) input transform launch (the per-image pointers already advanced)
struct Wino4Input {
    const float2* x;
    int H, W, C2, TW, T, pad, reflect;
    const float2* mean_rstd;   // MODE 1 | 2
    const float2* gamma;       // both or neither
    const float2* beta;
    const float2* res;         // MODE 2
    float2* xout;              // MODE 2
};
// V[a*6+b] = (B^T d B)[a][b] of tile `tile` (row-major in the TW-wide tile grid; tile >= T: a padding tile, zeros) for the
// channel pair c2; store(pos, v) receives the 36 values.  MODE as winograd4_input_kernel: 0 plain, 1 lazy norm + ReLU,
// 2 lazy norm + residual with the tile's own 4x4 pixels written to xout.
template <int MODE, class Store>
__device__ __forceinline__ void winograd4_input_item(const Wino4Input& p, const long tile, const int c2, Store store) {
    const int H = p.H, W = p.W, C2 = p.C2, pad = p.pad;
    if (tile >= p.T) {   // padding tiles: zeros
#pragma unroll
        for (int xi = 0; xi < 36; ++xi) store(xi, make_float2(0.f, 0.f));
        return;
    }
    const int ty = (int)(tile / p.TW), tx = (int)(tile - (long)ty * p.TW);
    int ry[6], rx[6];
    bool oky[6], okx[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        int yy = 4 * ty - pad + k, xx = 4 * tx - pad + k;
        oky[k] = p.reflect || ((unsigned)yy < (unsigned)H);
        okx[k] = p.reflect || ((unsigned)xx < (unsigned)W);
        yy = yy < 0 ? -yy : yy;
        xx = xx < 0 ? -xx : xx;
        ry[k] = max(min(yy, 2 * H - 2 - yy), 0);   // past the reflected border: ragged tile, outputs masked
        rx[k] = max(min(xx, 2 * W - 2 - xx), 0);
    }
    float2 mr0, mr1, gm = make_float2(1.f, 1.f), bt = make_float2(0.f, 0.f);
    if (MODE) {
        mr0 = p.mean_rstd[2 * c2];
        mr1 = p.mean_rstd[2 * c2 + 1];
        if (p.gamma) {
            gm = p.gamma[c2];
            bt = p.beta[c2];
        }
    }
    // rows first: r[a][j] = sum_b B^T[j][b] d[a][b]
    float rxv[6][6], ryv[6][6];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        float2 d[6], r[6];
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            const long at = ((long)ry[a] * W + rx[b]) * C2 + c2;
            d[b] = (oky[a] && okx[b]) ? p.x[at] : make_float2(0.f, 0.f);
            if (MODE == 2) r[b] = (oky[a] && okx[b]) ? p.res[at] : make_float2(0.f, 0.f);
        }
        float dx[6], dy[6];
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            float2 v = d[b];
            if (MODE && oky[a] && okx[b]) {
                v.x = norm_apply(v.x, mr0.x, mr0.y, p.gamma != nullptr, gm.x, bt.x, MODE == 1);
                v.y = norm_apply(v.y, mr1.x, mr1.y, p.gamma != nullptr, gm.y, bt.y, MODE == 1);
                if (MODE == 2) {
                    v.x += r[b].x;
                    v.y += r[b].y;
                    // the tile's own pixels: rows / columns pad .. pad+3 of the patch, inside the map
                    if (a >= pad && a < pad + 4 && b >= pad && b < pad + 4 && 4 * ty - pad + a < H && 4 * tx - pad + b < W)
                        p.xout[((long)ry[a] * W + rx[b]) * C2 + c2] = v;
                }
            }
            dx[b] = v.x;
            dy[b] = v.y;
        }
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            rxv[a][j] = cdot<6>(f4::kBT[j], dx);
            ryv[a][j] = cdot<6>(f4::kBT[j], dy);
        }
    }
    // columns: v[a2][j] = sum_a B^T[a2][a] r[a][j]
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        float cx[6], cy[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            cx[a] = rxv[a][j];
            cy[a] = ryv[a][j];
        }
#pragma unroll
        for (int a2 = 0; a2 < 6; ++a2) store(a2 * 6 + j, make_float2(cdot<6>(f4::kBT[a2], cx), cdot<6>(f4::kBT[a2], cy)));
    }
}

// U[pr*9+pq] = sum_{a,b} G[pr][a] G[pq][b] g[a][b] of one (n, c) filter of a polyphase layer (UP: the transposed conv's
// matrices): transformed in fp64, rounded once; store(pos, u)
template <bool UP, class Store>
__device__ __forceinline__ void polyphase_weight_transform(const double (&g)[3][3], Store store) {
    double t[9][3];
#pragma unroll
    for (int p = 0; p < 9; ++p)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const double(&G)[9][3] = UP ? pp::kGU : pp::kGD;
            t[p][b] = G[p][0] * g[0][b] + G[p][1] * g[1][b] + G[p][2] * g[2][b];
        }
#pragma unroll
    for (int p = 0; p < 9; ++p)
#pragma unroll
        for (int q = 0; q < 9; ++q) {
            const double(&G)[9][3] = UP ? pp::kGU : pp::kGD;
            const double u = t[p][0] * G[q][0] + t[p][1] * G[q][1] + t[p][2] * G[q][2];
            store(p * 9 + q, (float)u);
        }
}

// ---- the split-bf16 form of an fp32 value (winograd_split.hip, polyphase_split.hip): hi = bf16_rne(v), lo = bf16_rne(v - hi)
// round to nearest even (finite values: what torch's .bfloat16() computes)
__device__ __forceinline__ unsigned bf16_rne(float x) {
    unsigned u = __float_as_uint(x);
    u += 0x7fffu + ((u >> 16) & 1u);
    return u >> 16;
}
__device__ __forceinline__ float bf16_float(unsigned h) { return __uint_as_float(h << 16); }
struct SplitPair {
    unsigned hi, lo;   // two bf16 each: .x in the low half
};
__device__ __forceinline__ SplitPair split_bf16x2(float2 v) {
    const unsigned hx = bf16_rne(v.x), hy = bf16_rne(v.y);
    const unsigned lx = bf16_rne(v.x - bf16_float(hx)), ly = bf16_rne(v.y - bf16_float(hy));
    return {hx | (hy << 16), lx | (ly << 16)};
}
// the two stores of a finished fp32 value in that form: four channels as the 16-byte slot {hi01, lo01, hi23, lo23} of the
// direct kernels (conv_igemm_split.hip), one value as a bf16 in the hi plane and one `plane` elements on in the lo plane
// (the filter transforms of winograd_split.hip and polyphase_split.hip)
__device__ __forceinline__ void store_split_quad(uint4* y, long i, float4 v) {
    const SplitPair a = split_bf16x2(make_float2(v.x, v.y)), b = split_bf16x2(make_float2(v.z, v.w));
    y[i] = make_uint4(a.hi, a.lo, b.hi, b.lo);
}
typedef unsigned short u16;
__device__ __forceinline__ void store_split_planes(u16* hi_plane, size_t at, size_t plane, float v) {
    const unsigned hi = bf16_rne(v), lo = bf16_rne(v - bf16_float(hi));
    hi_plane[at] = (u16)hi;
    hi_plane[plane + at] = (u16)lo;
}

// ---- polyphase F(4,2) input transform (polyphase.hip) with a store policy, as winograd4_input_item above: the fp32 kernel
// stores the finished value, the split-bf16 one (polyphase_split.hip) its two bf16 terms.
struct PolyInput {
    const float2* x;
    int H, W, C2, TW, T;
    const float2* mean_rstd;   // NORM
    const float2* gamma;       // both or neither
    const float2* beta;
    int relu;
};
// The positions of sub-block `sub` (DOWN; UP: all four sub-blocks) of tile `tile` (tile >= T: a padding tile, zeros) for the
// channel pair c2; out(pos, v) receives them, pos = pr * 9 + pc.
template <bool UP, bool NORM, class Out>
__device__ __forceinline__ void polyphase_input_item(const PolyInput& in, const long tile, const int sub, const int c2, Out out) {
    const float2* __restrict__ x = in.x;
    const float2* __restrict__ mean_rstd = in.mean_rstd;
    const float2* __restrict__ gamma = in.gamma;
    const float2* __restrict__ beta = in.beta;
    const int H = in.H, W = in.W, C2 = in.C2, TW = in.TW, T = in.T, relu = in.relu;
    auto mine = [&](int s) { return UP || sub == s; };
    if (tile >= T) {   // padding tiles: zeros (each sub-block's thread its own positions)
#pragma unroll 1
        for (int pos = 0; pos < 81; ++pos)
            if (mine((pos / 9 >= 5 ? 2 : 0) + (pos % 9 >= 5 ? 1 : 0))) out(pos, make_float2(0.f, 0.f));
        return;
    }
    const int ty = (int)(tile / TW), tx = (int)(tile - (long)ty * TW);
    // sample k of the F(4,2) set / of the plain set, per dimension -> input index
    auto wrow = [&](int k, int t) { return UP ? 4 * t + k : 8 * t - 1 + 2 * k; };       // k = 0..4
    auto prow = [&](int k, int t) { return UP ? 4 * t + k : 8 * t + 2 * k; };           // k = 0..3
    float2 mr0 = make_float2(0.f, 1.f), mr1 = make_float2(0.f, 1.f), gm = make_float2(1.f, 1.f), bt = make_float2(0.f, 0.f);
    if (NORM) {
        mr0 = mean_rstd[2 * c2];
        mr1 = mean_rstd[2 * c2 + 1];
        if (gamma) {
            gm = gamma[c2];
            bt = beta[c2];
        }
    }
    auto load = [&](int yy, int xx) {
        if (!((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W)) return make_float2(0.f, 0.f);
        float2 v = x[((long)yy * W + xx) * C2 + c2];
        if (NORM) {
            v.x = norm_apply(v.x, mr0.x, mr0.y, gamma != nullptr, gm.x, bt.x, relu == 1);
            v.y = norm_apply(v.y, mr1.x, mr1.y, gamma != nullptr, gm.y, bt.y, relu == 1);
        }
        return v;
    };
    auto store = [&](int pr, int pc, float vx, float vy) { out(pr * 9 + pc, make_float2(vx, vy)); };
    // (1) transformed rows x transformed columns: 5 x 5 -> 5 x 5
    if (mine(0)) {
        float rx[5][5], ry[5][5];
#pragma unroll
        for (int a = 0; a < 5; ++a) {
            float dx[5], dy[5];
#pragma unroll
            for (int b = 0; b < 5; ++b) {
                const float2 v = load(wrow(a, ty), wrow(b, tx));
                dx[b] = v.x;
                dy[b] = v.y;
            }
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                rx[a][q] = cdot<5>(pp::kBU[q], dx);
                ry[a][q] = cdot<5>(pp::kBU[q], dy);
            }
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            float cx[5], cy[5];
#pragma unroll
            for (int a = 0; a < 5; ++a) {
                cx[a] = rx[a][q];
                cy[a] = ry[a][q];
            }
#pragma unroll
            for (int p = 0; p < 5; ++p) store(p, q, cdot<5>(pp::kBU[p], cx), cdot<5>(pp::kBU[p], cy));
        }
    }
    // (2) transformed rows x plain columns: per plain column a 5-vector down the rows
    if (mine(1))
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        float cx[5], cy[5];
#pragma unroll
        for (int a = 0; a < 5; ++a) {
            const float2 v = load(wrow(a, ty), prow(b, tx));
            cx[a] = v.x;
            cy[a] = v.y;
        }
#pragma unroll
        for (int p = 0; p < 5; ++p) store(p, 5 + b, cdot<5>(pp::kBU[p], cx), cdot<5>(pp::kBU[p], cy));
    }
    // (3) plain rows x transformed columns
    if (mine(2))
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        float dx[5], dy[5];
#pragma unroll
        for (int b = 0; b < 5; ++b) {
            const float2 v = load(prow(a, ty), wrow(b, tx));
            dx[b] = v.x;
            dy[b] = v.y;
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) store(5 + a, q, cdot<5>(pp::kBU[q], dx), cdot<5>(pp::kBU[q], dy));
    }
    // (4) plain x plain: copies
    if (mine(3))
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const float2 v = load(prow(a, ty), prow(b, tx));
            store(5 + a, 5 + b, v.x, v.y);
        }
}

}  // namespace t2v
