// PSNR / SSIM sums of two uint8 HWC images over the whole frame and up to three boxes (t2v_image_metrics_u8,
// include/t2v.h): the integer sums of squared and absolute differences, and the sum of the SSIM index (Wang et al. 2004,
// 11x11 Gaussian window of sigma 1.5, per channel on the 8-bit values) over the window positions that lie wholly inside a
// region.
//
// One 256-thread block per 32x32 tile of pixels.  The block stages its tile and a 5-pixel halo of both images in LDS as
// bytes (pixels outside the frame as zeros: no counted window reaches them), then per channel runs the separable window:
// a row pass that leaves the five horizontal sums (x, y, x^2, y^2, xy) of 42 rows x 32 columns in LDS as fp64, and a column
// pass with one thread per window centre that forms the moments and the SSIM expression, all in fp64 (in fp32 the
// cancellation in sum(w x^2) - mu^2 costs 8e-6 of the index on smooth images).  The integer sums ride along in the column
// pass.  Every block writes one partial per (region, quantity) to `scratch`; a second launch adds them in a fixed order.
// The integer sums are carried as doubles: every partial sum is an integer below 2^53, so they are exact in any order.
// No atomics, no allocation, no host synchronisation: two calls give the same bits, and row 0 does not depend on the boxes.
#include <math.h>

#include "t2v_internal.h"

namespace t2v {
namespace {

constexpr int kTile = 32;                    // pixels per tile side
constexpr int kHalo = 5;                     // window radius
constexpr int kWin = 2 * kHalo + 1;
constexpr int kStage = kTile + 2 * kHalo;    // 42 staged rows / columns
constexpr int kPixPitch = 44;                // bytes per staged row
constexpr int kMaxRegions = 4;               // the frame + T2V_METRICS_MAX_BOXES
constexpr int kQuantities = 3;               // sse, sad, ssim_sum

struct MetricsArgs {
    const uint8_t *a, *b;
    int a_cs, b_cs, H, W, nregions;
    int box[kMaxRegions][4];                 // y0, y1, x0, x1 (half-open); region 0 = the frame
    double w[kWin];                          // the 1-D window, sum 1
    double* partials;                        // [nregions][kQuantities][nblocks]
};

struct FinalizeArgs {
    const double* partials;
    int nblocks, nregions;
    double ssim_n[kMaxRegions];
    double* out;                             // [nregions][4]
};

__device__ __forceinline__ double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__global__ __launch_bounds__(256) void image_metrics_u8_kernel(MetricsArgs p) {
    __shared__ uint8_t pa[3][kStage][kPixPitch];
    __shared__ uint8_t pb[3][kStage][kPixPitch];
    __shared__ double rows[5][kStage][kTile];          // horizontal sums of one channel; reused by the block reduction
    const int tid = threadIdx.x;
    const int tx0 = blockIdx.x * kTile, ty0 = blockIdx.y * kTile;

    for (int i = tid; i < kStage * kStage; i += 256) {
        const int r = i / kStage, c = i - r * kStage;
        const int gy = ty0 - kHalo + r, gx = tx0 - kHalo + c;
        uint8_t va[3] = {0, 0, 0}, vb[3] = {0, 0, 0};
        if (gy >= 0 && gy < p.H && gx >= 0 && gx < p.W) {
            const size_t pix = (size_t)gy * p.W + gx;
            const uint8_t* qa = p.a + pix * p.a_cs;
            const uint8_t* qb = p.b + pix * p.b_cs;
            for (int ch = 0; ch < 3; ++ch) {
                va[ch] = qa[ch];
                vb[ch] = qb[ch];
            }
        }
        for (int ch = 0; ch < 3; ++ch) {
            pa[ch][r][c] = va[ch];
            pb[ch][r][c] = vb[ch];
        }
    }

    // this thread's four pixels / window centres: (ty + 8k, tx); bit r of pix_in / win_in: counted for region r
    const int tx = tid % kTile, ty = tid / kTile;
    unsigned pix_in[4], win_in[4];
    for (int k = 0; k < 4; ++k) {
        const int y = ty0 + ty + 8 * k, x = tx0 + tx;
        pix_in[k] = win_in[k] = 0;
        for (int r = 0; r < kMaxRegions; ++r) {
            if (r >= p.nregions) break;
            const int y0 = p.box[r][0], y1 = p.box[r][1], x0 = p.box[r][2], x1 = p.box[r][3];
            if (y >= y0 && y < y1 && x >= x0 && x < x1) pix_in[k] |= 1u << r;
            if (y - kHalo >= y0 && y + kHalo < y1 && x - kHalo >= x0 && x + kHalo < x1) win_in[k] |= 1u << r;
        }
    }
    // a tile without a window centre whose window lies inside the frame has nothing to add to any SSIM sum
    const bool tile_has_windows = ty0 + kTile > kHalo && ty0 < p.H - kHalo && tx0 + kTile > kHalo && tx0 < p.W - kHalo;

    unsigned sse[kMaxRegions] = {0, 0, 0, 0}, sad[kMaxRegions] = {0, 0, 0, 0};      // <= 12 * 65025 per thread
    double ssim[kMaxRegions] = {0.0, 0.0, 0.0, 0.0};
    const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
    __syncthreads();

    for (int ch = 0; ch < 3; ++ch) {
        for (int k = 0; k < 4; ++k) {
            const int d = (int)pa[ch][kHalo + ty + 8 * k][kHalo + tx] - (int)pb[ch][kHalo + ty + 8 * k][kHalo + tx];
            const unsigned d2 = (unsigned)(d * d), da = (unsigned)(d < 0 ? -d : d);
            for (int r = 0; r < kMaxRegions; ++r)
                if (pix_in[k] >> r & 1u) {
                    sse[r] += d2;
                    sad[r] += da;
                }
        }
        if (!tile_has_windows) continue;       // (block-uniform)
        for (int i = tid; i < kStage * kTile; i += 256) {
            const int r = i / kTile, c = i - r * kTile;
            double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
            for (int j = 0; j < kWin; ++j) {
                const double x = (double)pa[ch][r][c + j], y = (double)pb[ch][r][c + j], wj = p.w[j];
                sx = fma(wj, x, sx);
                sy = fma(wj, y, sy);
                sxx = fma(wj, x * x, sxx);
                syy = fma(wj, y * y, syy);
                sxy = fma(wj, x * y, sxy);
            }
            rows[0][r][c] = sx;
            rows[1][r][c] = sy;
            rows[2][r][c] = sxx;
            rows[3][r][c] = syy;
            rows[4][r][c] = sxy;
        }
        __syncthreads();
        for (int k = 0; k < 4; ++k) {
            if (!win_in[k]) continue;
            const int r0 = ty + 8 * k;           // staged rows r0 .. r0 + 10 are the window of centre row r0 + 5 - 5
            double mx = 0.0, my = 0.0, exx = 0.0, eyy = 0.0, exy = 0.0;
#pragma unroll
            for (int j = 0; j < kWin; ++j) {
                const double wj = p.w[j];
                mx = fma(wj, rows[0][r0 + j][tx], mx);
                my = fma(wj, rows[1][r0 + j][tx], my);
                exx = fma(wj, rows[2][r0 + j][tx], exx);
                eyy = fma(wj, rows[3][r0 + j][tx], eyy);
                exy = fma(wj, rows[4][r0 + j][tx], exy);
            }
            const double vx = exx - mx * mx, vy = eyy - my * my, cxy = exy - mx * my;
            const double s = ((2.0 * mx * my + C1) * (2.0 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2));
            for (int r = 0; r < kMaxRegions; ++r)
                if (win_in[k] >> r & 1u) ssim[r] += s;
        }
        __syncthreads();       // the next channel's row pass overwrites `rows`
    }

    // block reduction in a fixed order: lanes by shuffle, then the four waves in order
    double* red = &rows[0][0][0];                // [4 waves][nregions * kQuantities]
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    for (int r = 0; r < kMaxRegions; ++r) {
        if (r >= p.nregions) break;
        const double v0 = wave_sum((double)sse[r]), v1 = wave_sum((double)sad[r]), v2 = wave_sum(ssim[r]);
        if (lane == 0) {
            red[(wave * kMaxRegions + r) * kQuantities + 0] = v0;
            red[(wave * kMaxRegions + r) * kQuantities + 1] = v1;
            red[(wave * kMaxRegions + r) * kQuantities + 2] = v2;
        }
    }
    __syncthreads();
    if (tid < p.nregions * kQuantities) {
        const int r = tid / kQuantities, q = tid - r * kQuantities;
        double v = red[(0 * kMaxRegions + r) * kQuantities + q];
        for (int wv = 1; wv < 4; ++wv) v += red[(wv * kMaxRegions + r) * kQuantities + q];
        const int nblocks = gridDim.x * gridDim.y, blk = blockIdx.y * gridDim.x + blockIdx.x;
        p.partials[(size_t)(r * kQuantities + q) * nblocks + blk] = v;
    }
}

// one block per region: the partials of each quantity added in a fixed order (strided per thread, then a tree)
__global__ __launch_bounds__(256) void image_metrics_finalize_kernel(FinalizeArgs p) {
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
    if (tid < kQuantities) p.out[r * 4 + tid] = red[tid][0];
    if (tid == kQuantities) p.out[r * 4 + 3] = p.ssim_n[r];
}

inline int tiles(int n) { return (n + kTile - 1) / kTile; }

}  // namespace

size_t image_metrics_scratch_doubles(int H, int W, int nbox) {
    return (size_t)tiles(H) * tiles(W) * (1 + nbox) * kQuantities;
}

int launch_image_metrics_u8(hipStream_t s, const uint8_t* a, int a_cs, const uint8_t* b, int b_cs, int H, int W,
                            const int32_t* boxes, int nbox, double* scratch, double* out) {
    MetricsArgs m;
    m.a = a;
    m.b = b;
    m.a_cs = a_cs;
    m.b_cs = b_cs;
    m.H = H;
    m.W = W;
    m.nregions = 1 + nbox;
    FinalizeArgs f;
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
        const int h = y1 - y0, w = x1 - x0;
        f.ssim_n[r] = (h >= kWin && w >= kWin) ? 3.0 * (double)(h - kWin + 1) * (double)(w - kWin + 1) : 0.0;
    }
    // g[i] = exp(-(i - 5)^2 / (2 sigma^2)), sigma = 1.5, normalised to sum 1 in float64
    double sum = 0.0;
    for (int i = 0; i < kWin; ++i) {
        m.w[i] = exp(-(double)((i - kHalo) * (i - kHalo)) / 4.5);
        sum += m.w[i];
    }
    for (int i = 0; i < kWin; ++i) m.w[i] /= sum;
    m.partials = scratch;
    const dim3 grid(tiles(W), tiles(H));
    hipLaunchKernelGGL(image_metrics_u8_kernel, grid, dim3(256), 0, s, m);
    T2V_HIP_CHECK(hipGetLastError());
    f.partials = scratch;
    f.nblocks = (int)(grid.x * grid.y);
    f.nregions = 1 + nbox;
    f.out = out;
    hipLaunchKernelGGL(image_metrics_finalize_kernel, dim3(1 + nbox), dim3(256), 0, s, f);
    T2V_HIP_CHECK(hipGetLastError());
    return T2V_OK;
}

}  // namespace t2v
