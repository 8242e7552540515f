// The kernels of the dense Lucas-Kanade flow (optical_flow.hip, t2v_optical_flow), shared with its refined form
// (optical_flow_refine.hip, t2v_optical_flow_refined, a library of its own): every translation unit that includes this compiles
// its own copy from the one text, so both libraries run the same arithmetic.
#pragma once
#include "t2v_internal.h"

namespace t2v {
namespace {

constexpr int kTW = 32, kTH = 8;            // output tile of a 256-thread block
constexpr int kMaxR = 7;                     // largest window radius
constexpr int kHaloW = kTW + 2 * kMaxR, kHaloH = kTH + 2 * kMaxR;     // tile + window halo
constexpr int kRawW = kHaloW + 2, kRawH = kHaloH + 2;                 // ... + the smoothing's ring
constexpr int kRowPitch = kTW + 1;           // row sums: odd pitch, the column pass reads down a column without conflicts
constexpr int kMaxLevels = 8;

__device__ __forceinline__ int floor_half(int v) { return (v + 16) / 2 - 8; }      // floor(v / 2) for v >= -16

// (R + G + B) / 3 of both images: blockIdx.y = 0 cur, 1 prev
__global__ __launch_bounds__(256) void flow_grey_kernel(const float* __restrict__ cur, int cur_cs, int cur_c0,
                                                        const float* __restrict__ prev, int prev_cs, int prev_c0,
                                                        float* __restrict__ g_cur, float* __restrict__ g_prev, long npix) {
    const float* src = blockIdx.y ? prev : cur;
    const int cs = blockIdx.y ? prev_cs : cur_cs, c0 = blockIdx.y ? prev_c0 : cur_c0;
    float* dst = blockIdx.y ? g_prev : g_cur;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += stride) {
        const float* p = src + i * cs + c0;
        dst[i] = (p[0] + p[1] + p[2]) / 3.0f;
    }
}

// the same grey images from uint8 HWC frames (t2v_optical_flow_u8): x_c = (v_c / 255 - 0.5) / 0.5 as t2v_pose_u8_to_f32 forms
// it (the true quotient), then (x0 + x1 + x2) / 3 -- bit for bit flow_grey_kernel on the fp32 image of the same bytes
__global__ __launch_bounds__(256) void flow_grey_u8_kernel(const uint8_t* __restrict__ cur, int cur_cs,
                                                           const uint8_t* __restrict__ prev, int prev_cs,
                                                           float* __restrict__ g_cur, float* __restrict__ g_prev, long npix) {
    const uint8_t* src = blockIdx.y ? prev : cur;
    const int cs = blockIdx.y ? prev_cs : cur_cs;
    float* dst = blockIdx.y ? g_prev : g_cur;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += stride) {
        const uint8_t* p = src + i * cs;
        const float x0 = ((float)p[0] / 255.0f - 0.5f) / 0.5f;
        const float x1 = ((float)p[1] / 255.0f - 0.5f) / 0.5f;
        const float x2 = ((float)p[2] / 255.0f - 0.5f) / 0.5f;
        dst[i] = (x0 + x1 + x2) / 3.0f;
    }
}

// AvgPool2d(3, 2, 1, count_include_pad=False) of both grey images: blockIdx.y = 0 cur, 1 prev
__global__ __launch_bounds__(256) void flow_pool_kernel(const float* __restrict__ src_cur, const float* __restrict__ src_prev,
                                                        float* __restrict__ dst_cur, float* __restrict__ dst_prev, int H,
                                                        int W, int Ho, int Wo) {
    const float* x = blockIdx.y ? src_prev : src_cur;
    float* y = blockIdx.y ? dst_prev : dst_cur;
    const int total = Ho * Wo;
    const int stride = gridDim.x * blockDim.x;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int oy = i / Wo, ox = i - oy * Wo;
        float s = 0.f;
        int n = 0;
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = oy * 2 - 1 + ky;
            if ((unsigned)iy >= (unsigned)H) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = ox * 2 - 1 + kx;
                if ((unsigned)ix >= (unsigned)W) continue;
                s += x[iy * W + ix];
                ++n;
            }
        }
        y[i] = s / (float)n;
    }
}

// bilinear tap of a clamped position: p in [0, n - 1] -> (i0, i1, weight of i1)
struct Tap {
    int i0, i1;
    float f;
};
// the clamp goes through fminf / fmaxf BEFORE the value becomes an index: a non-finite position lands on 0 (fmaxf returns its
// other operand for a NaN), never outside the plane
__device__ __forceinline__ Tap clamped_tap(float p, int n) {
    p = fminf(fmaxf(p, 0.0f), (float)(n - 1));
    const float f0 = floorf(p);
    Tap t;
    t.i0 = (int)f0;
    t.i1 = min(t.i0 + 1, n - 1);
    t.f = p - f0;
    return t;
}
__device__ __forceinline__ float lerp2(float a00, float a10, float a01, float a11, float fx, float fy) {
    const float top = (1.0f - fx) * a00 + fx * a10;
    const float bot = (1.0f - fx) * a01 + fx * a11;
    return (1.0f - fy) * top + fy * bot;
}

struct LkArgs {
    const float* cur;      // grey planes of this level
    const float* prev;
    int h, w;
    const float2* src;     // flow to start from, before its smoothing: MODE 1 this level's, MODE 2 the coarser level's
    int sh, sw;            // ... and that plane's size
    float2* dst;           // this iteration's flow, before its smoothing
    int r;
    float lam_n;           // lambda * (2r+1)^2
};

// MODE 0: the incoming flow is zero (coarsest level, first iteration); 1: smooth3x3(src), src on this level's grid;
// 2: 2 * bilinear(smooth3x3(src); x/2, y/2), src on the coarser grid (a finer level's first iteration); 3: as 2 without the
// smoothing (the coarser level's flow is a refined one, t2v_optical_flow_refined, which nobody smooths).
// s_sm holds smooth3x3(src) (MODE 3: src) over the region [sox, sox + SW) x [soy, ...) of src's grid.
template <int MODE>
__device__ __forceinline__ float2 incoming_flow(const float2* s_sm, int x, int y, int sox, int soy, int SW, int sw, int sh) {
    if (MODE == 0) return make_float2(0.f, 0.f);
    if (MODE == 1) return s_sm[(y - soy) * SW + (x - sox)];
    const Tap tx = clamped_tap((float)x * 0.5f, sw), ty = clamped_tap((float)y * 0.5f, sh);
    const float2 a00 = s_sm[(ty.i0 - soy) * SW + (tx.i0 - sox)], a10 = s_sm[(ty.i0 - soy) * SW + (tx.i1 - sox)];
    const float2 a01 = s_sm[(ty.i1 - soy) * SW + (tx.i0 - sox)], a11 = s_sm[(ty.i1 - soy) * SW + (tx.i1 - sox)];
    return make_float2(2.0f * lerp2(a00.x, a10.x, a01.x, a11.x, tx.f, ty.f),
                       2.0f * lerp2(a00.y, a10.y, a01.y, a11.y, tx.f, ty.f));
}

template <int MODE>
__global__ __launch_bounds__(256) void flow_lk_kernel(LkArgs a) {
    __shared__ float2 s_raw[kRawH * kRawW];
    __shared__ float2 s_sm[kHaloH * kHaloW];
    __shared__ float s_gx[kHaloH * kHaloW], s_gy[kHaloH * kHaloW], s_it[kHaloH * kHaloW];
    __shared__ float s_row[5][kHaloH * kRowPitch];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    const int r = a.r, h = a.h, w = a.w;
    const int HW = kTW + 2 * r, HH = kTH + 2 * r;        // tile + halo, origin (x0 - r, y0 - r)
    // region of src's grid whose smoothed flow this block reads
    const int sox = MODE >= 2 ? floor_half(x0 - r) : x0 - r, soy = MODE >= 2 ? floor_half(y0 - r) : y0 - r;
    const int SW = MODE >= 2 ? HW / 2 + 2 : HW, SH = MODE >= 2 ? HH / 2 + 2 : HH;
    if (MODE != 0) {
        const int RW = SW + 2, RH = SH + 2;              // ... plus the ring its 3x3 smoothing reaches
        for (int i = tid; i < RW * RH; i += 256) {
            const int ry = i / RW, rx = i - ry * RW;
            const int sx = sox - 1 + rx, sy = soy - 1 + ry;
            const bool in = (unsigned)sx < (unsigned)a.sw && (unsigned)sy < (unsigned)a.sh;
            s_raw[i] = in ? a.src[sy * a.sw + sx] : make_float2(0.f, 0.f);
        }
        __syncthreads();
        // 3x3 mean over the taps inside the image
        for (int i = tid; i < SW * SH; i += 256) {
            const int py = i / SW, px = i - py * SW;
            const int sx = sox + px, sy = soy + py;
            if ((unsigned)sx >= (unsigned)a.sw || (unsigned)sy >= (unsigned)a.sh) continue;      // never read
            if (MODE == 3) {
                s_sm[i] = s_raw[(py + 1) * RW + px + 1];
                continue;
            }
            float su = 0.f, sv = 0.f;
            int n = 0;
            for (int dy = -1; dy <= 1; ++dy) {
                if ((unsigned)(sy + dy) >= (unsigned)a.sh) continue;
                for (int dx = -1; dx <= 1; ++dx) {
                    if ((unsigned)(sx + dx) >= (unsigned)a.sw) continue;
                    const float2 f = s_raw[(py + 1 + dy) * RW + px + 1 + dx];
                    su += f.x;
                    sv += f.y;
                    ++n;
                }
            }
            s_sm[i] = make_float2(su / (float)n, sv / (float)n);
        }
        __syncthreads();
    }
    // gx, gy (central differences of cur, replicate border) and it = warp(prev; u, v) - cur over tile + halo; zero outside
    // the image (the window sums run over the image only)
    for (int i = tid; i < HW * HH; i += 256) {
        const int hy = i / HW, hx = i - hy * HW;
        const int x = x0 - r + hx, y = y0 - r + hy;
        float gx = 0.f, gy = 0.f, it = 0.f;
        if ((unsigned)x < (unsigned)w && (unsigned)y < (unsigned)h) {
            const float2 f = incoming_flow<MODE>(s_sm, x, y, sox, soy, SW, a.sw, a.sh);
            const Tap tx = clamped_tap((float)x + f.x, w), ty = clamped_tap((float)y + f.y, h);
            const float* p0 = a.prev + ty.i0 * w;
            const float* p1 = a.prev + ty.i1 * w;
            const float wv = lerp2(p0[tx.i0], p0[tx.i1], p1[tx.i0], p1[tx.i1], tx.f, ty.f);
            const float* c = a.cur + y * w;
            it = wv - c[x];
            gx = 0.5f * (c[min(x + 1, w - 1)] - c[max(x - 1, 0)]);
            gy = 0.5f * (a.cur[min(y + 1, h - 1) * w + x] - a.cur[max(y - 1, 0) * w + x]);
        }
        s_gx[i] = gx;
        s_gy[i] = gy;
        s_it[i] = it;
    }
    __syncthreads();
    // window sums, separably: along the rows ...
    const int n1 = 2 * r + 1;
    for (int i = tid; i < HH * kTW; i += 256) {
        const int hy = i / kTW, tx = i - hy * kTW;
        const int base = hy * HW + tx;
        float sxx = 0.f, syy = 0.f, sxy = 0.f, sxt = 0.f, syt = 0.f;
        for (int j = 0; j < n1; ++j) {
            const float gx = s_gx[base + j], gy = s_gy[base + j], it = s_it[base + j];
            sxx += gx * gx;
            syy += gy * gy;
            sxy += gx * gy;
            sxt += gx * it;
            syt += gy * it;
        }
        const int o = hy * kRowPitch + tx;
        s_row[0][o] = sxx;
        s_row[1][o] = syy;
        s_row[2][o] = sxy;
        s_row[3][o] = sxt;
        s_row[4][o] = syt;
    }
    __syncthreads();
    // ... then down the columns, the 2x2 solve and the clamped step
    const int tx = tid % kTW, ty = tid / kTW;
    const int x = x0 + tx, y = y0 + ty;
    if (x >= w || y >= h) return;
    float sxx = 0.f, syy = 0.f, sxy = 0.f, sxt = 0.f, syt = 0.f;
    for (int j = 0; j < n1; ++j) {
        const int o = (ty + j) * kRowPitch + tx;
        sxx += s_row[0][o];
        syy += s_row[1][o];
        sxy += s_row[2][o];
        sxt += s_row[3][o];
        syt += s_row[4][o];
    }
    sxx += a.lam_n;
    syy += a.lam_n;
    const float det = sxx * syy - sxy * sxy;          // >= lam_n^2 > 0
    const float bx = -sxt, by = -syt;
    const float du = (syy * bx - sxy * by) / det, dv = (sxx * by - sxy * bx) / det;
    const float m = fmaxf(1.0f, sqrtf(du * du + dv * dv));
    const float2 f = incoming_flow<MODE>(s_sm, x, y, sox, soy, SW, a.sw, a.sh);
    a.dst[y * w + x] = make_float2(f.x + du / m, f.y + dv / m);
}

// out [H][W][4] = (smooth3x3(u), smooth3x3(v), 0, 0) of the finest level's last iteration
__global__ __launch_bounds__(256) void flow_out_kernel(const float2* __restrict__ raw, float4* __restrict__ out, int H, int W) {
    const int total = H * W;
    const int stride = gridDim.x * blockDim.x;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int y = i / W, x = i - y * W;
        float su = 0.f, sv = 0.f;
        int n = 0;
        for (int dy = -1; dy <= 1; ++dy) {
            if ((unsigned)(y + dy) >= (unsigned)H) continue;
            for (int dx = -1; dx <= 1; ++dx) {
                if ((unsigned)(x + dx) >= (unsigned)W) continue;
                const float2 f = raw[(y + dy) * W + x + dx];
                su += f.x;
                sv += f.y;
                ++n;
            }
        }
        out[i] = make_float4(su / (float)n, sv / (float)n, 0.f, 0.f);
    }
}

inline int blocks_for(long n) { return capped_grid(n, 256, 4096); }

}  // namespace
}  // namespace t2v
