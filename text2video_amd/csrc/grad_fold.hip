// libt2v_gradfold.so: t2v_grad_fold (include/t2v_grad_fold.h) -- the fold of a flat gradient bucket into the accumulator of an
// optimiser step that walks several clips per rank (gradients.py, GradBuckets).  A library of its own that links libt2v_hip.so
// for its error message; its one kernel is its own.
//
// One pass over two streams of n floats, bound by memory: a fixed grid (fold_blocks) strides over the 16-byte body, four
// independent 16-byte loads of each operand in flight per lane; the elements in front of the first and behind the last
// 16-byte boundary -- all n of them when the two pointers differ in their alignment modulo 16 -- go one float at a time.
#include <stdint.h>

#include "../../include/t2v_grad_fold.h"
#include "t2v_internal.h"

namespace t2v {
namespace {

constexpr int kFoldThreads = 256;
constexpr int kFoldBlocksPerCu = 8;      // 2048 blocks on 256 compute units: enough loads in flight to fill the memory pipes

// one element of the fold, and four; a + g first, then the product: two roundings, as on the host
template <int MODE>
__device__ __forceinline__ float fold1(float g, float a, float scale) {
    if (MODE == T2V_GRAD_FOLD_OPEN) return g;
    if (MODE == T2V_GRAD_FOLD_ADD) return a + g;
    return (a + g) * scale;
}
template <int MODE>
__device__ __forceinline__ float4 fold4(float4 g, float4 a, float scale) {
    return make_float4(fold1<MODE>(g.x, a.x, scale), fold1<MODE>(g.y, a.y, scale), fold1<MODE>(g.z, a.z, scale),
                       fold1<MODE>(g.w, a.w, scale));
}

// grad, acc: n floats; head: elements in front of the 16-byte body (n when there is none), nvec: float4s of the body.
// OPEN never reads acc, OPEN and ADD write acc only, CLOSE writes grad only.
template <int MODE>
__global__ __launch_bounds__(kFoldThreads) void grad_fold_kernel(float* __restrict__ grad, float* __restrict__ acc, long n,
                                                                 long head, long nvec, float scale) {
    const long stride = (long)gridDim.x * blockDim.x;
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    float4* g4 = reinterpret_cast<float4*>(grad + head);
    float4* a4 = reinterpret_cast<float4*>(acc + head);
    float4* out4 = MODE == T2V_GRAD_FOLD_CLOSE ? g4 : a4;
    long i = t;
    for (; i + 3 * stride < nvec; i += 4 * stride) {
        float4 g[4], a[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) g[u] = g4[i + u * stride];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = MODE != T2V_GRAD_FOLD_OPEN ? a4[i + u * stride] : g[u];
#pragma unroll
        for (int u = 0; u < 4; ++u) out4[i + u * stride] = fold4<MODE>(g[u], a[u], scale);
    }
    for (; i < nvec; i += stride) {
        const float4 g = g4[i];
        float4 a = g;
        if (MODE != T2V_GRAD_FOLD_OPEN) a = a4[i];
        out4[i] = fold4<MODE>(g, a, scale);
    }
    // the scalar elements: [0, head) and [head + 4 nvec, n)
    const long nscalar = n - 4 * nvec;
    float* out = MODE == T2V_GRAD_FOLD_CLOSE ? grad : acc;
    for (long s = t; s < nscalar; s += stride) {
        const long e = s < head ? s : s + 4 * nvec;
        const float g = grad[e];
        float a = g;
        if (MODE != T2V_GRAD_FOLD_OPEN) a = acc[e];
        out[e] = fold1<MODE>(g, a, scale);
    }
}

// the grid: kFoldBlocksPerCu blocks per compute unit of the current device (the one the launch goes to; asked every call:
// nothing is cached across devices or threads), fewer only where that many would have no element
int fold_blocks(long work_items) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        cus <= 0)
        cus = 256;
    const long full = (long)cus * kFoldBlocksPerCu;
    const long need = (work_items + kFoldThreads - 1) / kFoldThreads;
    return (int)(need < full ? (need < 1 ? 1 : need) : full);
}

}  // namespace
}  // namespace t2v

using namespace t2v;

extern "C" {

int t2v_grad_fold_abi_version(void) { return T2V_GRAD_FOLD_ABI_VERSION; }

int t2v_grad_fold(t2v_ctx* ctx, void* stream, float* grad, float* acc, long n, int mode, float scale) {
    T2V_REQUIRE(ctx && grad && acc, "grad_fold: null pointer");
    T2V_REQUIRE(n > 0 && n <= (long)(INTPTR_MAX / 8), "grad_fold: n must be > 0 (got %ld)", n);
    T2V_REQUIRE(mode == T2V_GRAD_FOLD_OPEN || mode == T2V_GRAD_FOLD_ADD || mode == T2V_GRAD_FOLD_CLOSE,
                "grad_fold: mode must be T2V_GRAD_FOLD_OPEN, _ADD or _CLOSE (got %d)", mode);
    T2V_REQUIRE(scale > 0.f && __builtin_isfinite(scale), "grad_fold: scale must be finite and > 0");
    const uintptr_t g = (uintptr_t)grad, a = (uintptr_t)acc, bytes = (uintptr_t)n * 4;
    T2V_REQUIRE(g % 4 == 0 && a % 4 == 0, "grad_fold: grad and acc must be 4-byte aligned");
    T2V_REQUIRE(g + bytes <= a || a + bytes <= g, "grad_fold: grad and acc overlap");
    // the 16-byte body exists where both pointers reach a 16-byte boundary after the same number of floats
    long head = n, nvec = 0;
    if (g % 16 == a % 16) {
        head = (long)((16 - g % 16) % 16 / 4);
        if (head > n) head = n;
        nvec = (n - head) / 4;
    }
    const dim3 grid(fold_blocks(nvec > n - 4 * nvec ? nvec : n - 4 * nvec)), block(kFoldThreads);
    hipStream_t s = (hipStream_t)stream;
    if (mode == T2V_GRAD_FOLD_OPEN)
        hipLaunchKernelGGL(grad_fold_kernel<T2V_GRAD_FOLD_OPEN>, grid, block, 0, s, grad, acc, n, head, nvec, scale);
    else if (mode == T2V_GRAD_FOLD_ADD)
        hipLaunchKernelGGL(grad_fold_kernel<T2V_GRAD_FOLD_ADD>, grid, block, 0, s, grad, acc, n, head, nvec, scale);
    else
        hipLaunchKernelGGL(grad_fold_kernel<T2V_GRAD_FOLD_CLOSE>, grid, block, 0, s, grad, acc, n, head, nvec, scale);
    T2V_HIP_CHECK(hipGetLastError());
    return T2V_OK;
}

}  // extern "C"
