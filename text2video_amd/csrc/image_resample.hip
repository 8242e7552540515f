// Separable 8-bit resampling of a batch of uint8 HWC RGB frames, crop and ToTensor + Normalize(.5, .5) in one launch
// (t2v_resample_crop_normalize_u8, include/t2v.h): what the training loader does on the CPU with
// Image.resize(..., BICUBIC) + crop + (u8.float() / 255.0 - 0.5) / 0.5 on the device.
//
// The arithmetic is Pillow's 8-bit resampler (ImagingResampleHorizontal_8bpc / ImagingResampleVertical_8bpc): integer
// coefficients with 22 fractional bits, a horizontal pass rounded and saturated to uint8, then a vertical pass ON THOSE
// BYTES with the same rounding.  All of it is int32 arithmetic, so the bytes equal Pillow's; the filter lives in the
// host-built tables alone (ops.pillow_bicubic_tables), the kernel knows none.
//
// One 256-thread block per kTW x kTH tile of the crop window and frame (blockIdx.z).  The block runs the horizontal pass
// for its kTW columns over the source rows its vertical taps reach, keeps that strip as bytes in LDS, and runs the
// vertical pass out of LDS: only the columns and source rows the crop window needs are computed.  No atomics, no
// allocation, no host synchronisation: two calls give the same bits.
//
// Every index read from a table is clamped before it addresses memory: tables that are not a resampler's (taps spread
// over more than kResampleStripRows source rows per tile, indices outside the frame) give wrong values, never an access outside
// the frame, the tables or the strip.
#include "t2v_internal.h"

namespace t2v {
namespace {

constexpr int kTW = 32, kTH = 8;             // output tile of a 256-thread block
constexpr int kResampleMaxTaps = 33;                 // T2V_RESAMPLE_MAX_TAPS: ksize of an 8x downscale
// Source rows under one tile: first[Y + 7] - first[Y] <= 7 * scale + 1 and count <= ksize with scale <= (ksize - 1) / 4,
// so at most 7 * 8 + 1 + 33 = 90 rows at 33 taps.
constexpr int kResampleStripRows = 96;
constexpr int kPitch = kTW * 3;              // bytes per strip row
constexpr int kPrecisionBits = 22;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int clip8(int acc) { return clampi(acc >> kPrecisionBits, 0, 255); }      // arithmetic shift

// The trainer's (u8.float() / 255.0 - 0.5) / 0.5 AS THE DEVICE EVALUATES IT: ATen divides a tensor by a host scalar by
// multiplying with the scalar's fp32 reciprocal (div_true_kernel_cuda), so v / 255.0 is v * (1.0f / 255.0f) there -- for some
// bytes one ulp away from the true quotient u8_pose_to_f32_kernel forms (the CPU's, torchvision's ToTensor).  The frames must
// be the numbers the default loader trains on, so this is the form taken; / 0.5 is exact either way.
__device__ __forceinline__ float normalise(int u8) {
    const float v = (float)u8 * (1.0f / 255.0f);
    return (v - 0.5f) / 0.5f;
}

struct ResampleArgs {
    const uint8_t* src;
    int h, w;
    const int *x_first, *x_count, *x_coef;
    const int *y_first, *y_count, *y_coef;
    int kx, ky;
    int crop_x, crop_y, crop_w, crop_h;
    float* dst;
    int dst_cs, dst_c0;
};

__global__ __launch_bounds__(256) void resample_crop_normalize_u8_kernel(ResampleArgs a) {
    __shared__ uint8_t strip[kResampleStripRows * kPitch];
    const int ox0 = blockIdx.x * kTW, oy0 = blockIdx.y * kTH;
    const int ncols = min(kTW, a.crop_w - ox0), nrows_out = min(kTH, a.crop_h - oy0);
    const uint8_t* src = a.src + (size_t)blockIdx.z * a.h * a.w * 3;

    // source rows this tile's vertical taps reach: [r0, r0 + nstrip)
    int r0 = a.h - 1, r1 = 0;
    for (int k = 0; k < nrows_out; ++k) {
        const int Y = a.crop_y + oy0 + k;
        const int f = clampi(a.y_first[Y], 0, a.h - 1);
        const int n = clampi(a.y_count[Y], 0, a.ky);
        r0 = min(r0, f);
        r1 = max(r1, min(f + n, a.h));
    }
    const int nstrip = clampi(r1 - r0, 1, kResampleStripRows);

    // horizontal pass: (strip row, tile column) -> 3 bytes
    for (int i = threadIdx.x; i < nstrip * kTW; i += 256) {
        const int r = i / kTW, col = i - r * kTW;
        if (col >= ncols) continue;
        const int X = a.crop_x + ox0 + col;
        const int f = clampi(a.x_first[X], 0, a.w - 1);
        const int n = min(clampi(a.x_count[X], 0, a.kx), a.w - f);
        const int* kk = a.x_coef + (size_t)X * a.kx;
        const uint8_t* p = src + ((size_t)(r0 + r) * a.w + f) * 3;
        int s0 = 1 << (kPrecisionBits - 1), s1 = s0, s2 = s0;
        for (int j = 0; j < n; ++j) {
            const int c = kk[j];
            s0 += (int)p[3 * j] * c;
            s1 += (int)p[3 * j + 1] * c;
            s2 += (int)p[3 * j + 2] * c;
        }
        uint8_t* q = strip + r * kPitch + col * 3;
        q[0] = (uint8_t)clip8(s0);
        q[1] = (uint8_t)clip8(s1);
        q[2] = (uint8_t)clip8(s2);
    }
    __syncthreads();

    // vertical pass out of the strip, then ToTensor + Normalize: one thread per output pixel
    const int col = threadIdx.x % kTW, row = threadIdx.x / kTW;
    if (col >= ncols || row >= nrows_out) return;
    const int Y = a.crop_y + oy0 + row;
    const int f = clampi(a.y_first[Y], 0, a.h - 1);
    const int n = clampi(a.y_count[Y], 0, a.ky);
    const int* kk = a.y_coef + (size_t)Y * a.ky;
    int s0 = 1 << (kPrecisionBits - 1), s1 = s0, s2 = s0;
    for (int j = 0; j < n; ++j) {
        const uint8_t* q = strip + clampi(f - r0 + j, 0, nstrip - 1) * kPitch + col * 3;
        const int c = kk[j];
        s0 += (int)q[0] * c;
        s1 += (int)q[1] * c;
        s2 += (int)q[2] * c;
    }
    float* d = a.dst + (((size_t)blockIdx.z * a.crop_h + oy0 + row) * a.crop_w + ox0 + col) * a.dst_cs + a.dst_c0;
    d[0] = normalise(clip8(s0));
    d[1] = normalise(clip8(s1));
    d[2] = normalise(clip8(s2));
}

}  // namespace

int resample_max_taps() { return kResampleMaxTaps; }

int launch_resample_crop_normalize_u8(hipStream_t s, const uint8_t* src, int T, int h, int w, const int* x_first,
                                      const int* x_count, const int* x_coef, int kx, const int* y_first, const int* y_count,
                                      const int* y_coef, int ky, int crop_x, int crop_y, int crop_w, int crop_h, float* dst,
                                      int dst_cs, int dst_c0) {
    ResampleArgs a;
    a.src = src;
    a.h = h;
    a.w = w;
    a.x_first = x_first;
    a.x_count = x_count;
    a.x_coef = x_coef;
    a.y_first = y_first;
    a.y_count = y_count;
    a.y_coef = y_coef;
    a.kx = kx;
    a.ky = ky;
    a.crop_x = crop_x;
    a.crop_y = crop_y;
    a.crop_w = crop_w;
    a.crop_h = crop_h;
    a.dst = dst;
    a.dst_cs = dst_cs;
    a.dst_c0 = dst_c0;
    const dim3 grid((crop_w + kTW - 1) / kTW, (crop_h + kTH - 1) / kTH, T);
    hipLaunchKernelGGL(resample_crop_normalize_u8_kernel, grid, dim3(256), 0, s, a);
    T2V_HIP_CHECK(hipGetLastError());
    return T2V_OK;
}

}  // namespace t2v
