// polyphase_split.hip -- T2V_ALGO_POLYPHASE_BF16X2: the polyphase F(4,2) stride-2 / transposed convolution (polyphase.hip) with
// its 81 GEMMs on the bf16 matrix cores, in the split arithmetic of winograd_split.hip (hi = bf16_rne(v), lo = bf16_rne(v - hi);
// sum_k (ah*bh + ah*bl + al*bh)).  The input transform and the filter transform call the device functions the fp32 kernels
// call (transform_common.h) and split the finished fp32 value on its way out; the GEMM is wino_split_gemm_kernel with 81
// positions, the output transforms are polyphase_output_{down,up}_kernel themselves.
//   polyphase_input_split_kernel  : V planes [2][81][Tt][C] bf16 (hi plane, lo plane) -- the bytes of the fp32 V
//   polyphase_weight_split_kernel : U planes [2][81][Cout_p][Cin_s] bf16              -- the bytes of the fp32 U
#include "t2v_internal.h"
#include "transform_common.h"

namespace t2v {
namespace {

// polyphase_input_kernel<UP, NORM> (polyphase.hip) with the split store: the same thread -> (tile, sub-block, channel pair)
// map, so a padding tile's zeros and every position come from the thread that writes them in the fp32 form.
// Vp: [2][81][Tt][C2] channel pairs.
template <bool UP, bool NORM>
__global__ __launch_bounds__(256) void polyphase_input_split_kernel(const float2* __restrict__ x, unsigned* __restrict__ Vp, int H,
                                                                    int W, int C2, int TW, int T, int Tt,
                                                                    const float2* __restrict__ mean_rstd,
                                                                    const float2* __restrict__ gamma,
                                                                    const float2* __restrict__ beta, int relu) {
    constexpr int NSUB = UP ? 1 : 4;
    const PolyInput in{x, H, W, C2, TW, T, mean_rstd, gamma, beta, relu};
    const long pitch = (long)Tt * C2, plane = 81 * pitch;      // between positions, between the planes
    const long total = (long)Tt * NSUB * C2;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const long ts = i / C2;
        const int c2 = (int)(i - ts * C2);
        const long tile = ts / NSUB;
        const int sub = (int)(ts - tile * NSUB);
        unsigned* const Vt = Vp + (tile * C2 + c2);      // this thread's element of position 0 in the hi plane
        polyphase_input_item<UP, NORM>(in, tile, sub, c2, [&](int pos, float2 v) {
            const SplitPair sp = split_bf16x2(v);
            Vt[pos * pitch] = sp.hi;
            Vt[plane + pos * pitch] = sp.lo;
        });
    }
}

// polyphase_weight_kernel<UP> (polyphase.hip) with the split store: Up [2][81][Cout_p][Cin_s] bf16
template <bool UP>
__global__ void polyphase_weight_split_kernel(const float* __restrict__ w, u16* __restrict__ Up, int Cout, int Cin, int Cout_p,
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
        polyphase_weight_transform<UP>(g, [&](int pos, float u) {
            store_split_planes(Up, (size_t)pos * total + i, (size_t)81 * total, u);
        });
    }
}

}  // namespace

int launch_polyphase_input_split(hipStream_t s, const float* x, float* V, int H, int W, int C, int up, const TileGrid& tg, int Tt,
                                 const LazyNorm& ln, int grid) {
    auto kern = up ? (ln.mean_rstd ? polyphase_input_split_kernel<true, true> : polyphase_input_split_kernel<true, false>)
                   : (ln.mean_rstd ? polyphase_input_split_kernel<false, true> : polyphase_input_split_kernel<false, false>);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, s, reinterpret_cast<const float2*>(x), reinterpret_cast<unsigned*>(V), H, W,
                       C / 2, tg.TW, tg.T, Tt, reinterpret_cast<const float2*>(ln.mean_rstd),
                       reinterpret_cast<const float2*>(ln.gamma), reinterpret_cast<const float2*>(ln.beta), ln.relu);
    T2V_HIP_CHECK(hipGetLastError());
    return T2V_OK;
}

int launch_polyphase_weight_split(hipStream_t s, const float* w, float* U, int Cout, int Cin, int Cout_p, int Cin_s, int up,
                                  int grid) {
    if (up)
        hipLaunchKernelGGL(polyphase_weight_split_kernel<true>, dim3(grid), dim3(256), 0, s, w, reinterpret_cast<u16*>(U), Cout, Cin,
                           Cout_p, Cin_s);
    else
        hipLaunchKernelGGL(polyphase_weight_split_kernel<false>, dim3(grid), dim3(256), 0, s, w, reinterpret_cast<u16*>(U), Cout, Cin,
                           Cout_p, Cin_s);
    T2V_HIP_CHECK(hipGetLastError());
    return T2V_OK;
}

}  // namespace t2v
