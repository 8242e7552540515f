// libt2v_flow.so: t2v_optical_flow_refined / _u8 (include/t2v_flow_refine.h) -- the coarse-to-fine Lucas-Kanade flow of
// optical_flow.hip with a Horn-Schunck refinement of every level's estimate, which fills the textureless regions a local
// estimator leaves to its smoothing.  tests/flow_refine_reference.py restates the algorithm in float64.
//
// A library of its own that links libt2v_hip.so (its error message, its shape rules, and t2v_optical_flow itself for
// refine_iters == 0).  The LK kernels are optical_flow_kernels.h's, compiled here a second time from the same text with one
// more form: MODE 3, a finer level's first iteration starting from a REFINED coarser flow, which nobody smooths.
//
// Planes per level: the LK ones (optical_flow.hip) and, behind all of them, (u0, v0), (gx, gy), (It0, 1 / denominator).
// Launches per call: include/t2v_flow_refine.h.
#include "../../include/t2v_flow_refine.h"
#include "optical_flow_kernels.h"

namespace t2v {
namespace {

// ---------------------------------------------------------------------------------------------------------------------
// Variational (Horn-Schunck) refinement of a level's LK estimate.
// Per level, after the LK iterations: one preparation launch (u0 = the smoothed LK flow, gx, gy, It0 and 1 / (alpha^2 + |g|^2)
// per pixel), then ceil(refine_iters / k) launches of k Jacobi steps each.  A refined plane is nobody's to smooth: the next
// finer level reads it with MODE 3, the output pass copies it.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void flow_hs_prep_kernel(const float* __restrict__ cur, const float* __restrict__ prev,
                                                           const float2* __restrict__ raw, float2* __restrict__ uv0,
                                                           float2* __restrict__ gxy, float2* __restrict__ itinv, int h, int w,
                                                           float alpha2) {
    const int total = h * w;
    const int stride = gridDim.x * blockDim.x;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int y = i / w, x = i - y * w;
        float su = 0.f, sv = 0.f;
        int n = 0;
        for (int dy = -1; dy <= 1; ++dy) {
            if ((unsigned)(y + dy) >= (unsigned)h) continue;
            for (int dx = -1; dx <= 1; ++dx) {
                if ((unsigned)(x + dx) >= (unsigned)w) continue;
                const float2 f = raw[(y + dy) * w + x + dx];
                su += f.x;
                sv += f.y;
                ++n;
            }
        }
        const float u0 = su / (float)n, v0 = sv / (float)n;
        const Tap tx = clamped_tap((float)x + u0, w), ty = clamped_tap((float)y + v0, h);
        const float* p0 = prev + ty.i0 * w;
        const float* p1 = prev + ty.i1 * w;
        const float wv = lerp2(p0[tx.i0], p0[tx.i1], p1[tx.i0], p1[tx.i1], tx.f, ty.f);
        const float* c = cur + y * w;
        const float gx = 0.5f * (c[min(x + 1, w - 1)] - c[max(x - 1, 0)]);
        const float gy = 0.5f * (cur[min(y + 1, h - 1) * w + x] - cur[max(y - 1, 0) * w + x]);
        uv0[i] = make_float2(u0, v0);
        gxy[i] = make_float2(gx, gy);
        itinv[i] = make_float2(wv - c[x], 1.0f / (alpha2 + gx * gx + gy * gy));
    }
}

// one Jacobi step of one pixel: the ONLY statement of the update, whichever launch form runs it (the library is built with
// -ffp-contract=off, so the expression is also its own contraction)
__device__ __forceinline__ float2 hs_step(float2 n, float2 s, float2 e, float2 w, float2 ne, float2 nw, float2 se, float2 sw,
                                          float gx, float gy, float it, float inv, float u0, float v0) {
    const float ub = (n.x + s.x + e.x + w.x) * (1.0f / 6.0f) + (ne.x + nw.x + se.x + sw.x) * (1.0f / 12.0f);
    const float vb = (n.y + s.y + e.y + w.y) * (1.0f / 6.0f) + (ne.y + nw.y + se.y + sw.y) * (1.0f / 12.0f);
    const float t = (gx * (ub - u0) + gy * (vb - v0) + it) * inv;
    return make_float2(ub - gx * t, vb - gy * t);
}

struct HsArgs {
    const float2* gxy;      // per-pixel constants of the level (flow_hs_prep_kernel)
    const float2* itinv;
    const float2* uv0;
    const float2* src;      // the iterate to start from
    float2* dst;            // ... and the one K steps later
    int h, w;
};

#ifndef T2V_HS_TILE
#define T2V_HS_TILE 16      // measured against 24 and 32 (-D builds; the same bits): profiles/flow_refine_times.txt
#endif
constexpr int kHsTile = T2V_HS_TILE;      // output tile (square) of a 256-thread block
constexpr int kHsMaxFused = T2V_FLOW_REFINE_MAX_FUSED;
constexpr int kHsDefaultFused = 8;      // profiles/flow_refine_times.txt

// K Jacobi steps in one launch.  The block stages its tile plus a ring of K cells of the iterate in LDS (region R x R,
// R = tile + 2K), each thread keeps the constants of the NC cells it owns in registers, and step s = 1..K updates the cells at
// least s away from the region's edge between two LDS buffers; step K is the tile itself and goes to memory.
// A cell outside the image is not a cell: it is never loaded, never updated and never read -- a neighbour offset that would
// leave the IMAGE is zero (replicate = the cell itself or its in-image neighbour of the same iterate), at every step.  Such a
// clamped neighbour is no further from the cell than the unclamped one, so it is valid whenever the unclamped one would be.
template <int K>
__global__ __launch_bounds__(256) void flow_hs_kernel(HsArgs a) {
    constexpr int R = kHsTile + 2 * K, NC = (R * R + 255) / 256;
    __shared__ float2 s_uv[2][R * R];
    const int tid = threadIdx.x;
    const int ox = blockIdx.x * kHsTile - K, oy = blockIdx.y * kHsTile - K;
    const int h = a.h, w = a.w;
    float gx[NC], gy[NC], it[NC], inv[NC], u0[NC], v0[NC];
    int margin[NC];      // cells of the region's edge the cell is away from; -1: not a cell
    int nb[NC];          // bit 0: x > 0, 1: x < w - 1, 2: y > 0, 3: y < h - 1
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int i = tid + j * 256;
        const int cy = i / R, cx = i - cy * R;
        const int x = ox + cx, y = oy + cy;
        const bool in = i < R * R && (unsigned)x < (unsigned)w && (unsigned)y < (unsigned)h;
        margin[j] = -1;
        nb[j] = 0;
        gx[j] = gy[j] = it[j] = inv[j] = u0[j] = v0[j] = 0.f;
        if (in) {
            const int p = y * w + x;
            const float2 g = a.gxy[p], c = a.itinv[p], f0 = a.uv0[p];
            gx[j] = g.x;
            gy[j] = g.y;
            it[j] = c.x;
            inv[j] = c.y;
            u0[j] = f0.x;
            v0[j] = f0.y;
            margin[j] = min(min(cx, R - 1 - cx), min(cy, R - 1 - cy));
            nb[j] = (x > 0 ? 1 : 0) | (x < w - 1 ? 2 : 0) | (y > 0 ? 4 : 0) | (y < h - 1 ? 8 : 0);
            s_uv[0][i] = a.src[p];
        }
    }
    __syncthreads();
#pragma unroll 1
    for (int s = 1; s <= K; ++s) {
        const float2* in = s_uv[(s - 1) & 1];
        float2* out = s_uv[s & 1];
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            if (margin[j] < s) continue;
            const int i = tid + j * 256;
            const int xm = -(nb[j] & 1), xp = (nb[j] >> 1) & 1;
            const int ym = (nb[j] & 4) ? -R : 0, yp = (nb[j] & 8) ? R : 0;
            const float2 r = hs_step(in[i + ym], in[i + yp], in[i + xp], in[i + xm], in[i + ym + xp], in[i + ym + xm],
                                     in[i + yp + xp], in[i + yp + xm], gx[j], gy[j], it[j], inv[j], u0[j], v0[j]);
            if (s == K) {
                const int cy = i / R, cx = i - cy * R;
                a.dst[(oy + cy) * w + ox + cx] = r;
            } else {
                out[i] = r;
            }
        }
        __syncthreads();
    }
}

template <int K>
void launch_hs_k(hipStream_t s, dim3 grid, int k, const HsArgs& a) {
    if (k == K)
        hipLaunchKernelGGL(flow_hs_kernel<K>, grid, dim3(256), 0, s, a);
    else if constexpr (K > 1)
        launch_hs_k<K - 1>(s, grid, k, a);
}

// out [H][W][4] = (u, v, 0, 0) of a refined plane
__global__ __launch_bounds__(256) void flow_out_plain_kernel(const float2* __restrict__ uv, float4* __restrict__ out, int total) {
    const int stride = gridDim.x * blockDim.x;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const float2 f = uv[i];
        out[i] = make_float4(f.x, f.y, 0.f, 0.f);
    }
}

}  // namespace

// the LK planes plus, per level and behind ALL of them (their layout stays what it is): (u0, v0), (gx, gy), (It0, 1 / denominator)
static size_t optical_flow_refined_workspace_floats(int H, int W, int levels) { return 2 * optical_flow_workspace_floats(H, W, levels); }

namespace {

struct Refine {
    float alpha;
    int iters;      // >= 1 (0 is t2v_optical_flow itself and never comes here)
    int fused;      // Jacobi steps per launch, 0: kHsDefaultFused
};

// launch_flow of optical_flow.hip with the refinement behind every level's LK iterations: grey(g_cur, g_prev) enqueues the one
// launch that writes the finest level's grey images
template <class GreyLaunch>
int launch_flow(hipStream_t s, GreyLaunch grey, int H, int W, int levels, int iters, int radius, float lambda, Refine rf,
                float* workspace, float* flow_out) {
    if (levels == 0) levels = optical_flow_default_levels(H, W);
    int hs[kMaxLevels], ws[kMaxLevels];
    float *g_cur[kMaxLevels], *g_prev[kMaxLevels];
    float2* uv[kMaxLevels][2];
    float2* hsp[kMaxLevels][3];      // (u0, v0), (gx, gy), (It0, 1 / denominator)
    float* p = workspace;
    for (int l = 0, h = H, w = W; l < levels; ++l, h = (h + 1) / 2, w = (w + 1) / 2) {
        const size_t n = (size_t)h * w;
        hs[l] = h;
        ws[l] = w;
        g_cur[l] = p;
        g_prev[l] = p + n;
        uv[l][0] = reinterpret_cast<float2*>(p + 2 * n);
        uv[l][1] = reinterpret_cast<float2*>(p + 4 * n);
        p += 6 * n;
    }
    for (int l = 0; l < levels; ++l) {
        const size_t n = (size_t)hs[l] * ws[l];
        for (int j = 0; j < 3; ++j) hsp[l][j] = reinterpret_cast<float2*>(p + 2 * j * n);
        p += 6 * n;
    }
    grey(g_cur[0], g_prev[0]);
    for (int l = 1; l < levels; ++l)
        hipLaunchKernelGGL(flow_pool_kernel, dim3(blocks_for((long)hs[l] * ws[l]), 2), dim3(256), 0, s, g_cur[l - 1],
                           g_prev[l - 1], g_cur[l], g_prev[l], hs[l - 1], ws[l - 1], hs[l], ws[l]);
    const float lam_n = (float)((double)lambda * (2 * radius + 1) * (2 * radius + 1));
    const int last = (iters - 1) % 2;          // the (u, v) plane a level's last iteration writes
    const int fused = rf.fused ? rf.fused : kHsDefaultFused;
    const float2* coarser = nullptr;           // the refined flow the next finer level starts from
    for (int l = levels - 1; l >= 0; --l) {
        const dim3 grid((ws[l] + kTW - 1) / kTW, (hs[l] + kTH - 1) / kTH);
        for (int k = 0; k < iters; ++k) {
            LkArgs a;
            a.cur = g_cur[l];
            a.prev = g_prev[l];
            a.h = hs[l];
            a.w = ws[l];
            a.dst = uv[l][k % 2];
            a.r = radius;
            a.lam_n = lam_n;
            if (k > 0) {
                a.src = uv[l][(k - 1) % 2];
                a.sh = hs[l];
                a.sw = ws[l];
                hipLaunchKernelGGL(flow_lk_kernel<1>, grid, dim3(256), 0, s, a);
            } else if (l < levels - 1) {
                a.src = coarser;
                a.sh = hs[l + 1];
                a.sw = ws[l + 1];
                hipLaunchKernelGGL(flow_lk_kernel<3>, grid, dim3(256), 0, s, a);
            } else {
                a.src = nullptr;
                a.sh = a.sw = 0;
                hipLaunchKernelGGL(flow_lk_kernel<0>, grid, dim3(256), 0, s, a);
            }
        }
        hipLaunchKernelGGL(flow_hs_prep_kernel, dim3(blocks_for((long)hs[l] * ws[l])), dim3(256), 0, s, g_cur[l], g_prev[l],
                           uv[l][last], hsp[l][0], hsp[l][1], hsp[l][2], hs[l], ws[l], rf.alpha * rf.alpha);
        // the LK planes are free from here on: the Jacobi launches go (u0, v0) -> uv[l][0] -> uv[l][1] -> uv[l][0] ...
        const dim3 hgrid((ws[l] + kHsTile - 1) / kHsTile, (hs[l] + kHsTile - 1) / kHsTile);
        coarser = hsp[l][0];
        for (int done = 0, j = 0; done < rf.iters; ++j) {
            const int k = rf.iters - done < fused ? rf.iters - done : fused;
            HsArgs a;
            a.uv0 = hsp[l][0];
            a.gxy = hsp[l][1];
            a.itinv = hsp[l][2];
            a.src = coarser;
            a.dst = uv[l][j % 2];
            a.h = hs[l];
            a.w = ws[l];
            launch_hs_k<kHsMaxFused>(s, hgrid, k, a);
            coarser = a.dst;
            done += k;
        }
    }
    hipLaunchKernelGGL(flow_out_plain_kernel, dim3(blocks_for((long)H * W)), dim3(256), 0, s, coarser,
                       reinterpret_cast<float4*>(flow_out), H * W);
    T2V_HIP_CHECK(hipGetLastError());
    return T2V_OK;
}

}  // namespace

static int launch_optical_flow_refined(hipStream_t s, const float* cur, int cur_cs, int cur_c0, const float* prev, int prev_cs,
                                int prev_c0, int H, int W, int levels, int iters, int radius, float lambda, float alpha,
                                int refine_iters, int iters_per_launch, float* workspace, float* flow_out) {
    return launch_flow(
        s,
        [&](float* g_cur, float* g_prev) {
            hipLaunchKernelGGL(flow_grey_kernel, dim3(blocks_for((long)H * W), 2), dim3(256), 0, s, cur, cur_cs, cur_c0, prev,
                               prev_cs, prev_c0, g_cur, g_prev, (long)H * W);
        },
        H, W, levels, iters, radius, lambda, Refine{alpha, refine_iters, iters_per_launch}, workspace, flow_out);
}

static int launch_optical_flow_refined_u8(hipStream_t s, const uint8_t* cur, int cur_cs, const uint8_t* prev, int prev_cs, int H, int W,
                                   int levels, int iters, int radius, float lambda, float alpha, int refine_iters,
                                   int iters_per_launch, float* workspace, float* flow_out) {
    return launch_flow(
        s,
        [&](float* g_cur, float* g_prev) {
            hipLaunchKernelGGL(flow_grey_u8_kernel, dim3(blocks_for((long)H * W), 2), dim3(256), 0, s, cur, cur_cs, prev, prev_cs,
                               g_cur, g_prev, (long)H * W);
        },
        H, W, levels, iters, radius, lambda, Refine{alpha, refine_iters, iters_per_launch}, workspace, flow_out);
}

}  // namespace t2v

using namespace t2v;

extern "C" {

int t2v_flow_refine_abi_version(void) { return T2V_FLOW_REFINE_ABI_VERSION; }

size_t t2v_optical_flow_refined_workspace_floats(int H, int W, int levels) {
    return optical_flow_shape_ok(H, W, levels) ? optical_flow_refined_workspace_floats(H, W, levels) : 0;
}
#define T2V_REQUIRE_REFINE(name)                                                                                              \
    T2V_REQUIRE(alpha > 0.f && alpha * alpha > 0.f && __builtin_isfinite(alpha * alpha),                                       \
                name ": alpha and alpha^2 must be finite and > 0 in fp32");                                                    \
    T2V_REQUIRE(refine_iters >= 0 && refine_iters <= 1024, name ": refine_iters must be in 0..1024 (got %d)", refine_iters);   \
    T2V_REQUIRE(iters_per_launch >= 0 && iters_per_launch <= T2V_FLOW_REFINE_MAX_FUSED,                                        \
                name ": iters_per_launch must be in 0..%d (got %d)", T2V_FLOW_REFINE_MAX_FUSED, iters_per_launch)
int t2v_optical_flow_refined(t2v_ctx* ctx, void* stream, const float* cur, int cur_cs, int cur_c0, const float* prev,
                             int prev_cs, int prev_c0, int H, int W, int levels, int iters, int radius, float lambda,
                             float alpha, int refine_iters, int iters_per_launch, float* workspace, float* flow_out) {
    T2V_REQUIRE(ctx && cur && prev && workspace && flow_out, "optical_flow_refined: null pointer");
    T2V_REQUIRE(H >= 8 && W >= 8, "optical_flow_refined: H, W must be >= 8 (got %d x %d)", H, W);
    T2V_REQUIRE(optical_flow_shape_ok(H, W, levels), "optical_flow_refined: unsupported size %d x %d or level count %d", H, W,
                levels);
    T2V_REQUIRE(radius >= 1 && radius <= 7, "optical_flow_refined: radius must be in 1..7 (got %d)", radius);
    T2V_REQUIRE(iters >= 1, "optical_flow_refined: iters must be >= 1 (got %d)", iters);
    T2V_REQUIRE(lambda > 0.f, "optical_flow_refined: lambda must be > 0");
    T2V_REQUIRE(cur_c0 >= 0 && cur_c0 + 3 <= cur_cs && prev_c0 >= 0 && prev_c0 + 3 <= prev_cs,
                "optical_flow_refined: the three channels from c0 must lie inside the channel stride");
    T2V_REQUIRE_REFINE("optical_flow_refined");
    if (refine_iters == 0)      // the LK entry's own launches
        return launch_optical_flow((hipStream_t)stream, cur, cur_cs, cur_c0, prev, prev_cs, prev_c0, H, W, levels, iters, radius,
                                   lambda, workspace, flow_out);
    return launch_optical_flow_refined((hipStream_t)stream, cur, cur_cs, cur_c0, prev, prev_cs, prev_c0, H, W, levels, iters,
                                       radius, lambda, alpha, refine_iters, iters_per_launch, workspace, flow_out);
}
int t2v_optical_flow_refined_u8(t2v_ctx* ctx, void* stream, const uint8_t* cur, int cur_cs, const uint8_t* prev, int prev_cs,
                                int H, int W, int levels, int iters, int radius, float lambda, float alpha, int refine_iters,
                                int iters_per_launch, float* workspace, float* flow_out) {
    T2V_REQUIRE(ctx && cur && prev && workspace && flow_out, "optical_flow_refined_u8: null pointer");
    T2V_REQUIRE(H >= 8 && W >= 8, "optical_flow_refined_u8: H, W must be >= 8 (got %d x %d)", H, W);
    T2V_REQUIRE(optical_flow_shape_ok(H, W, levels), "optical_flow_refined_u8: unsupported size %d x %d or level count %d", H, W,
                levels);
    T2V_REQUIRE(radius >= 1 && radius <= 7, "optical_flow_refined_u8: radius must be in 1..7 (got %d)", radius);
    T2V_REQUIRE(iters >= 1, "optical_flow_refined_u8: iters must be >= 1 (got %d)", iters);
    T2V_REQUIRE(lambda > 0.f, "optical_flow_refined_u8: lambda must be > 0");
    T2V_REQUIRE((cur_cs == 3 || cur_cs == 4) && (prev_cs == 3 || prev_cs == 4),
                "optical_flow_refined_u8: channel strides must be 3 or 4 (got %d and %d)", cur_cs, prev_cs);
    T2V_REQUIRE_REFINE("optical_flow_refined_u8");
    if (refine_iters == 0)
        return launch_optical_flow_u8((hipStream_t)stream, cur, cur_cs, prev, prev_cs, H, W, levels, iters, radius, lambda,
                                      workspace, flow_out);
    return launch_optical_flow_refined_u8((hipStream_t)stream, cur, cur_cs, prev, prev_cs, H, W, levels, iters, radius, lambda,
                                          alpha, refine_iters, iters_per_launch, workspace, flow_out);
}
#undef T2V_REQUIRE_REFINE

}  // extern "C"
