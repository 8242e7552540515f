// Temporal-consistency sums of a generated pair (a_cur, a_prev) read against the real pair (b_cur, b_prev) of the same two
// instants (t2v_temporal_metrics_u8, include/t2v.h), over the whole frame and up to three boxes: the warping error under the
// real pair's flow inside its forward-backward consistency mask (Sundaram et al. 2010; the mask of Ruder et al. 2016 and Lai
// et al. 2018), the same sum on the real pair (the floor the flow's own error leaves), the endpoint error between the
// generated pair's flow and the real pair's (tOF, Chu et al. 2020) and the flow-free flicker term
// sum(((a_cur - a_prev) - (b_cur - b_prev))^2).
//
// One 256-thread block per 32x16 tile of pixels, two pixels per thread (rows ty and ty + 8).  Per pixel: one 16-byte read of
// flow_fwd (and of flow_a), the bytes of the four images at the pixel -- all coalesced along the row -- and, at the position
// the forward flow points to, four taps of flow_bwd, a_prev and b_prev, which go through the caches (the flows are a few
// pixels long: a tile's taps lie in the tile's own neighbourhood).  Everything is evaluated in fp64 from the fp32 / uint8
// inputs.  Every gather position is clamped (fmin / fmax, which return the other operand for a NaN) BEFORE it becomes an
// index: a non-finite or huge flow makes its pixel invalid and can never address outside a plane.
// Every block writes one partial per (region, quantity) to `scratch`; a second launch adds them in a fixed order.  The three
// integer quantities are carried as doubles: every partial sum is an integer below 2^53, so they are exact in any order.
// No atomics, no allocation, no host synchronisation: two calls give the same bits, and row 0 does not depend on the boxes.
#include <math.h>

#include "t2v_internal.h"

namespace t2v {
namespace {

constexpr int kTileW = 32, kTileH = 16;      // pixels per tile
constexpr int kPerThread = kTileH / 8;       // rows ty + 8k of the tile
constexpr int kMaxRegions = 4;               // the frame + T2V_METRICS_MAX_BOXES
constexpr int kQuantities = 6;               // n_valid, warp_sse_a, warp_sse_b, n_flow, epe_sum, tdiff_sse

struct TemporalArgs {
    const uint8_t *a_cur, *a_prev, *b_cur, *b_prev;
    int a_cur_cs, a_prev_cs, b_cur_cs, b_prev_cs;
    const float4 *flow_fwd, *flow_bwd, *flow_a;      // flow_a may be null
    int H, W, nregions;
    int box[kMaxRegions][4];                 // y0, y1, x0, x1 (half-open); region 0 = the frame
    double* partials;                        // [nregions][kQuantities][nblocks]
};

struct FinalizeArgs {
    const double* partials;
    int nblocks;
    double* out;                             // [nregions][kQuantities]
};

__device__ __forceinline__ double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// bilinear tap of a position clamped into [0, n - 1]: a NaN lands on 0, +-Inf and 1e30 on an end
struct Tap {
    int i0, i1;
    double f;
};
__device__ __forceinline__ Tap clamped_tap(double p, int n) {
    p = fmin(fmax(p, 0.0), (double)(n - 1));
    const double f0 = floor(p);
    Tap t;
    t.i0 = (int)f0;
    t.i1 = min(t.i0 + 1, n - 1);
    t.f = p - f0;
    return t;
}
__device__ __forceinline__ double lerp2(double a00, double a10, double a01, double a11, double fx, double fy) {
    const double top = (1.0 - fx) * a00 + fx * a10;
    const double bot = (1.0 - fx) * a01 + fx * a11;
    return (1.0 - fy) * top + fy * bot;
}
__device__ __forceinline__ bool finite2(double u, double v) { return isfinite(u) && isfinite(v); }

// sum over the 3 channels of (cur_c(p) - bilinear(prev_c; tap))^2
__device__ __forceinline__ double warp_sq(const uint8_t* cur_px, const uint8_t* prev, int prev_cs, int W, const Tap& tx,
                                          const Tap& ty) {
    const uint8_t* p00 = prev + ((size_t)ty.i0 * W + tx.i0) * prev_cs;
    const uint8_t* p10 = prev + ((size_t)ty.i0 * W + tx.i1) * prev_cs;
    const uint8_t* p01 = prev + ((size_t)ty.i1 * W + tx.i0) * prev_cs;
    const uint8_t* p11 = prev + ((size_t)ty.i1 * W + tx.i1) * prev_cs;
    double s = 0.0;
    for (int c = 0; c < 3; ++c) {
        const double d = (double)cur_px[c] - lerp2((double)p00[c], (double)p10[c], (double)p01[c], (double)p11[c], tx.f, ty.f);
        s += d * d;
    }
    return s;
}

__global__ __launch_bounds__(256) void temporal_metrics_u8_kernel(TemporalArgs p) {
    __shared__ double red[4][kMaxRegions][kQuantities];
    const int tid = threadIdx.x;
    const int tx = tid % kTileW, ty = tid / kTileW;
    const int x = blockIdx.x * kTileW + tx;

    unsigned n_valid[kMaxRegions] = {0, 0, 0, 0}, n_flow[kMaxRegions] = {0, 0, 0, 0};
    unsigned tdiff[kMaxRegions] = {0, 0, 0, 0};          // <= 2 pixels * 3 channels * 510^2 per thread
    double sse_a[kMaxRegions] = {0.0, 0.0, 0.0, 0.0}, sse_b[kMaxRegions] = {0.0, 0.0, 0.0, 0.0};
    double epe[kMaxRegions] = {0.0, 0.0, 0.0, 0.0};

    for (int k = 0; k < kPerThread; ++k) {
        const int y = blockIdx.y * kTileH + ty + 8 * k;
        if (x >= p.W || y >= p.H) continue;
        unsigned in = 0;                     // bit r: the pixel is counted for region r
        for (int r = 0; r < kMaxRegions; ++r) {
            if (r >= p.nregions) break;
            if (y >= p.box[r][0] && y < p.box[r][1] && x >= p.box[r][2] && x < p.box[r][3]) in |= 1u << r;
        }
        const size_t pix = (size_t)y * p.W + x;
        const uint8_t* ac = p.a_cur + pix * p.a_cur_cs;
        const uint8_t* ap = p.a_prev + pix * p.a_prev_cs;
        const uint8_t* bc = p.b_cur + pix * p.b_cur_cs;
        const uint8_t* bp = p.b_prev + pix * p.b_prev_cs;
        unsigned td = 0;
        for (int c = 0; c < 3; ++c) {
            const int d = ((int)ac[c] - (int)ap[c]) - ((int)bc[c] - (int)bp[c]);
            td += (unsigned)(d * d);
        }

        const float4 f4 = p.flow_fwd[pix];
        const double fu = (double)f4.x, fv = (double)f4.y;
        const bool f_ok = finite2(fu, fv);
        const double qx = (double)x + fu, qy = (double)y + fv;
        const bool inside = f_ok && qx >= 0.0 && qx <= (double)(p.W - 1) && qy >= 0.0 && qy <= (double)(p.H - 1);
        const Tap sx = clamped_tap(qx, p.W), sy = clamped_tap(qy, p.H);      // the position itself for an inside pixel
        const float4 b00 = p.flow_bwd[(size_t)sy.i0 * p.W + sx.i0], b10 = p.flow_bwd[(size_t)sy.i0 * p.W + sx.i1];
        const float4 b01 = p.flow_bwd[(size_t)sy.i1 * p.W + sx.i0], b11 = p.flow_bwd[(size_t)sy.i1 * p.W + sx.i1];
        const double bu = lerp2((double)b00.x, (double)b10.x, (double)b01.x, (double)b11.x, sx.f, sy.f);
        const double bv = lerp2((double)b00.y, (double)b10.y, (double)b01.y, (double)b11.y, sx.f, sy.f);
        const double su = fu + bu, sv = fv + bv;
        const bool valid = inside && finite2(bu, bv) &&
                           su * su + sv * sv <= 0.01 * ((fu * fu + fv * fv) + (bu * bu + bv * bv)) + 0.5;
        double wa = 0.0, wb = 0.0;
        if (valid) {
            wa = warp_sq(ac, p.a_prev, p.a_prev_cs, p.W, sx, sy);
            wb = warp_sq(bc, p.b_prev, p.b_prev_cs, p.W, sx, sy);
        }
        bool flow_ok = false;
        double e = 0.0;
        if (p.flow_a) {
            const float4 g4 = p.flow_a[pix];
            const double gu = (double)g4.x, gv = (double)g4.y;
            flow_ok = f_ok && finite2(gu, gv);
            if (flow_ok) {
                const double du = gu - fu, dv = gv - fv;
                e = sqrt(du * du + dv * dv);
            }
        }
        for (int r = 0; r < kMaxRegions; ++r)
            if (in >> r & 1u) {
                tdiff[r] += td;
                if (valid) {
                    n_valid[r] += 1;
                    sse_a[r] += wa;
                    sse_b[r] += wb;
                }
                if (flow_ok) {
                    n_flow[r] += 1;
                    epe[r] += e;
                }
            }
    }

    // block reduction in a fixed order: lanes by shuffle, then the four waves in order
    const int lane = tid & 63, wave = tid >> 6;
    for (int r = 0; r < kMaxRegions; ++r) {
        if (r >= p.nregions) break;
        const double v0 = wave_sum((double)n_valid[r]), v1 = wave_sum(sse_a[r]), v2 = wave_sum(sse_b[r]);
        const double v3 = wave_sum((double)n_flow[r]), v4 = wave_sum(epe[r]), v5 = wave_sum((double)tdiff[r]);
        if (lane == 0) {
            red[wave][r][0] = v0;
            red[wave][r][1] = v1;
            red[wave][r][2] = v2;
            red[wave][r][3] = v3;
            red[wave][r][4] = v4;
            red[wave][r][5] = v5;
        }
    }
    __syncthreads();
    if (tid < p.nregions * kQuantities) {
        const int r = tid / kQuantities, q = tid - r * kQuantities;
        double v = red[0][r][q];
        for (int wv = 1; wv < 4; ++wv) v += red[wv][r][q];
        const int nblocks = gridDim.x * gridDim.y, blk = blockIdx.y * gridDim.x + blockIdx.x;
        p.partials[(size_t)(r * kQuantities + q) * nblocks + blk] = v;
    }
}

// one block per region: the partials of each quantity added in a fixed order (strided per thread, then a tree)
__global__ __launch_bounds__(256) void temporal_metrics_finalize_kernel(FinalizeArgs p) {
    __shared__ double red[kQuantities][256];
    const int r = blockIdx.x, tid = threadIdx.x;
    for (int q = 0; q < kQuantities; ++q) {
        const double* src = p.partials + (size_t)(r * kQuantities + q) * p.nblocks;
        double v = 0.0;
        for (int i = tid; i < p.nblocks; i += 256) v += src[i];
        red[q][tid] = v;
    }
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s)
            for (int q = 0; q < kQuantities; ++q) red[q][tid] += red[q][tid + s];
        __syncthreads();
    }
    if (tid < kQuantities) p.out[r * kQuantities + tid] = red[tid][0];
}

inline int tiles_w(int n) { return (n + kTileW - 1) / kTileW; }
inline int tiles_h(int n) { return (n + kTileH - 1) / kTileH; }

}  // namespace

size_t temporal_metrics_scratch_doubles(int H, int W, int nbox) {
    return (size_t)tiles_h(H) * tiles_w(W) * (1 + nbox) * kQuantities;
}

int launch_temporal_metrics_u8(hipStream_t s, const uint8_t* a_cur, int a_cur_cs, const uint8_t* a_prev, int a_prev_cs,
                               const uint8_t* b_cur, int b_cur_cs, const uint8_t* b_prev, int b_prev_cs, const float* flow_fwd,
                               const float* flow_bwd, const float* flow_a, int H, int W, const int32_t* boxes, int nbox,
                               double* scratch, double* out) {
    TemporalArgs m;
    m.a_cur = a_cur;
    m.a_prev = a_prev;
    m.b_cur = b_cur;
    m.b_prev = b_prev;
    m.a_cur_cs = a_cur_cs;
    m.a_prev_cs = a_prev_cs;
    m.b_cur_cs = b_cur_cs;
    m.b_prev_cs = b_prev_cs;
    m.flow_fwd = reinterpret_cast<const float4*>(flow_fwd);
    m.flow_bwd = reinterpret_cast<const float4*>(flow_bwd);
    m.flow_a = reinterpret_cast<const float4*>(flow_a);
    m.H = H;
    m.W = W;
    m.nregions = 1 + nbox;
    for (int r = 0; r < kMaxRegions; ++r) {
        int y0 = 0, y1 = 0, x0 = 0, x1 = 0;          // unused regions are empty
        if (r == 0) {
            y1 = H;
            x1 = W;
        } else if (r <= nbox) {
            y0 = boxes[(r - 1) * 4 + 0];
            y1 = boxes[(r - 1) * 4 + 1];
            x0 = boxes[(r - 1) * 4 + 2];
            x1 = boxes[(r - 1) * 4 + 3];
        }
        m.box[r][0] = y0;
        m.box[r][1] = y1;
        m.box[r][2] = x0;
        m.box[r][3] = x1;
    }
    m.partials = scratch;
    const dim3 grid(tiles_w(W), tiles_h(H));
    hipLaunchKernelGGL(temporal_metrics_u8_kernel, grid, dim3(256), 0, s, m);
    T2V_HIP_CHECK(hipGetLastError());
    FinalizeArgs f;
    f.partials = scratch;
    f.nblocks = (int)(grid.x * grid.y);
    f.out = out;
    hipLaunchKernelGGL(temporal_metrics_finalize_kernel, dim3(1 + nbox), dim3(256), 0, s, f);
    T2V_HIP_CHECK(hipGetLastError());
    return T2V_OK;
}

}  // namespace t2v
