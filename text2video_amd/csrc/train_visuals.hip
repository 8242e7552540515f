// The pictures a training run shows of its last frame (t2v_train_visuals_u8, include/t2v.h): up to 8 panels of one
// H x W frame -- fp32 NHWC tensors read from a channel offset -- rendered as uint8 RGB into one contiguous buffer
// [n][H/scale][W/scale][3].  IMAGE is util.tensor2im's byte, UNIT a [0,1] map as grey, FLOW a flow field as HSV with
// hue = direction, value = the panel's min-max-normalised magnitude (float64), saturation 1.
//
// Two launches on the caller's stream.  (1) one block per (FLOW panel, slice of its pixels): the min and max of the
// magnitude over the slice's finite pixels -> `scratch` [panel][block][lo, hi].  (2) the output as one flat run of
// n * Ho * Wo pixels, four consecutive pixels = 12 bytes = three whole dwords per thread; a block first reduces the
// partials of the FLOW panels its pixels lie in (one wave per panel, <= 64 partials each), then renders.  With scale s
// an output byte is the rounded mean of the s x s full-resolution bytes.  min / max do not depend on the order, nothing
// is accumulated in floating point: two calls give the same bytes.  No atomics, no allocation, no host synchronisation.
#include <math.h>

#include "t2v_internal.h"

namespace t2v {
namespace {

constexpr int kMaxPanels = T2V_VISUALS_MAX_PANELS;
constexpr int kThreads = 256;
constexpr int kPixPerThread = 4;             // 12 output bytes = 3 dwords
constexpr int kMaxSlices = 64;               // min/max partials per FLOW panel: one wave reduces them
constexpr int kSlicePixels = 1024;           // pixels a slice holds before the slices grow instead of their number

struct VisualsArgs {
    const float* ptr[kMaxPanels];
    int kind[kMaxPanels], c0[kMaxPanels], cs[kMaxPanels], vec[kMaxPanels];      // vec: floats per aligned load at c0 (1, 2, 4)
    int flow_panel[kMaxPanels];              // launch 1: blockIdx.y -> panel
    int npanels, H, W, scale, Ho, Wo, nslices;
    double* partials;                        // [npanels][nslices][2]
    uint8_t* out;
};

struct Dwords3 { uint32_t a, b, c; };

__device__ __forceinline__ bool finite2(float u, float v) { return isfinite(u) && isfinite(v); }

__device__ __forceinline__ void load2(const float* q, int vec, float& a, float& b) {
    if (vec >= 2) {
        const float2 t = *reinterpret_cast<const float2*>(q);
        a = t.x;
        b = t.y;
    } else {
        a = q[0];
        b = q[1];
    }
}

__device__ __forceinline__ void load3(const float* q, int vec, float& a, float& b, float& c) {
    if (vec == 4) {
        const float4 t = *reinterpret_cast<const float4*>(q);
        a = t.x;
        b = t.y;
        c = t.z;
    } else {
        load2(q, vec, a, b);
        c = q[2];
    }
}

__device__ __forceinline__ double wave_min(double v) {
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_down(v, off, 64));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
    return v;
}

// launch 1: grid (nslices, FLOW panels)
__global__ __launch_bounds__(kThreads) void train_visuals_minmax_kernel(VisualsArgs p) {
    __shared__ double red[2][kThreads / 64];
    const int panel = p.flow_panel[blockIdx.y];
    const float* src = p.ptr[panel] + p.c0[panel];
    const int cs = p.cs[panel], vec = p.vec[panel];
    const long npix = (long)p.H * p.W;
    double lo = INFINITY, hi = -INFINITY;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < npix; i += (long)gridDim.x * kThreads) {
        float u, v;
        load2(src + (size_t)i * cs, vec, u, v);
        if (finite2(u, v)) {
            const double m = sqrt((double)u * (double)u + (double)v * (double)v);
            lo = fmin(lo, m);
            hi = fmax(hi, m);
        }
    }
    lo = wave_min(lo);
    hi = wave_max(hi);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        red[0][wave] = lo;
        red[1][wave] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kThreads / 64; ++w) {
            lo = fmin(lo, red[0][w]);
            hi = fmax(hi, red[1][w]);
        }
        double* dst = p.partials + ((size_t)panel * p.nslices + blockIdx.x) * 2;
        dst[0] = lo;
        dst[1] = hi;
    }
}

// the three bytes of full-resolution pixel `pix` of a panel, packed r | g << 8 | b << 16
__device__ __forceinline__ uint32_t pixel_bytes(const float* base, int kind, int cs, int vec, size_t pix, double lo, double hi) {
    const float* q = base + pix * cs;
    if (kind == T2V_VISUALS_IMAGE) {
        float x[3];
        load3(q, vec, x[0], x[1], x[2]);
        uint32_t w = 0;
        for (int c = 0; c < 3; ++c) {
            float v = (x[c] + 1.0f) / 2.0f * 255.0f;             // util.tensor2im, as to_u8_kernel (elementwise.hip)
            v = fminf(fmaxf(v, 0.f), 255.f);
            w |= (uint32_t)(uint8_t)v << (8 * c);
        }
        return w;
    }
    if (kind == T2V_VISUALS_UNIT) {
        float v = q[0] * 255.0f;
        v = fminf(fmaxf(v, 0.f), 255.f);                         // (fmaxf drops a NaN: 0)
        return (uint32_t)(uint8_t)v * 0x010101u;
    }
    float uf, vf;
    load2(q, vec, uf, vf);
    if (!finite2(uf, vf) || !(hi > lo)) return 0;
    const double u = (double)uf, v = (double)vf;
    const double V = (sqrt(u * u + v * v) - lo) / (hi - lo);
    double a = atan2(v, u);
    if (a < 0.0) a += 2.0 * M_PI;
    const double h6 = 3.0 * a / M_PI, fl = floor(h6), f = h6 - fl;
    const int sector = (int)fl % 6;                              // (a == 2 pi after rounding: sector 6 -> 0, f = 0)
    double r, g, b;
    switch (sector) {
        case 0: r = 1.0, g = f, b = 0.0; break;
        case 1: r = 1.0 - f, g = 1.0, b = 0.0; break;
        case 2: r = 0.0, g = 1.0, b = f; break;
        case 3: r = 0.0, g = 1.0 - f, b = 1.0; break;
        case 4: r = f, g = 0.0, b = 1.0; break;
        default: r = 1.0, g = 0.0, b = 1.0 - f; break;
    }
    const double s = 255.0 * V;
    return (uint32_t)floor(s * r + 0.5) | (uint32_t)floor(s * g + 0.5) << 8 | (uint32_t)floor(s * b + 0.5) << 16;
}

// launch 2: one thread per four consecutive output pixels of the flat [n * Ho * Wo] run
__global__ __launch_bounds__(kThreads) void train_visuals_render_kernel(VisualsArgs p) {
    __shared__ double s_lo[kMaxPanels], s_hi[kMaxPanels];
    const long per_panel = (long)p.Ho * p.Wo, total = per_panel * p.npanels;
    const long block_first = (long)blockIdx.x * kThreads * kPixPerThread;
    const long block_end = block_first + (long)kThreads * kPixPerThread, block_last = (block_end < total ? block_end : total) - 1;
    const int panel_first = (int)(block_first / per_panel), panel_last = (int)(block_last / per_panel);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int panel = panel_first + wave; panel <= panel_last; panel += kThreads / 64) {      // (wave-uniform)
        if (p.kind[panel] != T2V_VISUALS_FLOW) continue;
        const double* src = p.partials + (size_t)panel * p.nslices * 2;
        const double lo = wave_min(lane < p.nslices ? src[2 * lane] : INFINITY);
        const double hi = wave_max(lane < p.nslices ? src[2 * lane + 1] : -INFINITY);
        if (lane == 0) {
            s_lo[panel] = lo;
            s_hi[panel] = hi;
        }
    }
    __syncthreads();

    const long g0 = block_first + (long)threadIdx.x * kPixPerThread;
    if (g0 >= total) return;
    const int s = p.scale, s2 = s * s;
    uint32_t px[kPixPerThread];
    for (int j = 0; j < kPixPerThread; ++j) {
        const long g = g0 + j;
        px[j] = 0;
        if (g >= total) break;
        const int panel = (int)(g / per_panel);
        const long i = g - (long)panel * per_panel;
        const int oy = (int)(i / p.Wo), ox = (int)(i - (long)oy * p.Wo);
        const int kind = p.kind[panel], cs = p.cs[panel], vec = p.vec[panel];
        const float* base = p.ptr[panel] + p.c0[panel];
        double lo = 0.0, hi = 0.0;
        if (kind == T2V_VISUALS_FLOW) {
            lo = s_lo[panel];
            hi = s_hi[panel];
        }
        if (s == 1) {
            px[j] = pixel_bytes(base, kind, cs, vec, (size_t)oy * p.W + ox, lo, hi);
            continue;
        }
        uint32_t sr = 0, sg = 0, sb = 0;                         // <= 16 * 255
        for (int dy = 0; dy < s; ++dy)
            for (int dx = 0; dx < s; ++dx) {
                const uint32_t w = pixel_bytes(base, kind, cs, vec, (size_t)(oy * s + dy) * p.W + (ox * s + dx), lo, hi);
                sr += w & 255u;
                sg += w >> 8 & 255u;
                sb += w >> 16 & 255u;
            }
        px[j] = (sr + s2 / 2) / s2 | (sg + s2 / 2) / s2 << 8 | (sb + s2 / 2) / s2 << 16;
    }
    uint8_t* dst = p.out + (size_t)g0 * 3;                       // 12 * (g0 / 4): dword-aligned with `out`
    if (g0 + kPixPerThread <= total) {
        Dwords3 d;
        d.a = px[0] | px[1] << 24;
        d.b = px[1] >> 8 | px[2] << 16;
        d.c = px[2] >> 16 | px[3] << 8;
        *reinterpret_cast<Dwords3*>(dst) = d;
    } else {                                                     // the run's last, partial group: bytes
        for (int j = 0; j < kPixPerThread && g0 + j < total; ++j) {
            dst[3 * j + 0] = (uint8_t)(px[j] & 255u);
            dst[3 * j + 1] = (uint8_t)(px[j] >> 8 & 255u);
            dst[3 * j + 2] = (uint8_t)(px[j] >> 16 & 255u);
        }
    }
}

int slices(int H, int W) {
    const long n = ((long)H * W + kSlicePixels - 1) / kSlicePixels;
    return (int)(n < 1 ? 1 : (n > kMaxSlices ? kMaxSlices : n));
}

}  // namespace

size_t train_visuals_scratch_doubles(int H, int W, int npanels) { return (size_t)npanels * slices(H, W) * 2; }

int launch_train_visuals_u8(hipStream_t s, const float* const* ptrs, const int32_t* ints, int npanels, int H, int W, int scale,
                            double* scratch, uint8_t* out) {
    VisualsArgs a;
    int nflow = 0;
    for (int i = 0; i < kMaxPanels; ++i) {
        a.ptr[i] = nullptr;
        a.kind[i] = a.c0[i] = a.cs[i] = a.flow_panel[i] = 0;
        a.vec[i] = 1;
        if (i >= npanels) continue;
        a.ptr[i] = ptrs[i];
        a.kind[i] = ints[3 * i + 0];
        a.c0[i] = ints[3 * i + 1];
        a.cs[i] = ints[3 * i + 2];
        // the widest load every pixel's first channel is aligned for (the row pitch, the offset and the base all count)
        const uintptr_t first = (uintptr_t)(ptrs[i] + a.c0[i]);
        if (a.kind[i] != T2V_VISUALS_UNIT) {
            if (a.kind[i] == T2V_VISUALS_IMAGE && a.cs[i] % 4 == 0 && a.c0[i] + 4 <= a.cs[i] && first % 16 == 0) a.vec[i] = 4;
            else if (a.cs[i] % 2 == 0 && first % 8 == 0) a.vec[i] = 2;
        }
        if (a.kind[i] == T2V_VISUALS_FLOW) a.flow_panel[nflow++] = i;
    }
    a.npanels = npanels;
    a.H = H;
    a.W = W;
    a.scale = scale;
    a.Ho = H / scale;
    a.Wo = W / scale;
    a.nslices = slices(H, W);
    a.partials = scratch;
    a.out = out;
    if (nflow) {
        hipLaunchKernelGGL(train_visuals_minmax_kernel, dim3(a.nslices, nflow), dim3(kThreads), 0, s, a);
        T2V_HIP_CHECK(hipGetLastError());
    }
    const long total = (long)a.Ho * a.Wo * npanels, per_block = (long)kThreads * kPixPerThread;
    hipLaunchKernelGGL(train_visuals_render_kernel, dim3((unsigned)((total + per_block - 1) / per_block)), dim3(kThreads), 0, s, a);
    T2V_HIP_CHECK(hipGetLastError());
    return T2V_OK;
}

}  // namespace t2v
