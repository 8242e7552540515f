// Dense optical flow between two frames: coarse-to-fine iterative Lucas-Kanade on the grey images (t2v_optical_flow and
// t2v_optical_flow_u8, which differ in the launch that forms the grey images only; include/t2v.h) -- the reference flow of the train step's flow / warp losses, which upstream takes from FlowNet2.
// Fully local: every output pixel is a fixed function of a fixed neighbourhood, no atomics, no global solve, so two
// calls give the same bits.  tests/flow_reference.py restates the algorithm in float64.
//
// Planes (fp32, [h][w], in the caller's workspace), per pyramid level: grey cur, grey prev, and two (u, v) planes the
// iterations ping-pong between.  An iteration WRITES the flow before its 3x3 smoothing; whoever reads a flow plane --
// the next iteration, the next finer level's first iteration, the output pass -- smooths while loading.  So one launch
// per (level, iteration) does everything: smoothing (and, on a level's first iteration, the x2 bilinear upsample) of the
// incoming flow, the bilinear gather of prev, gradients, the five window sums and the 2x2 solve.  (gx, gy and the three
// structure-tensor sums do not change within a level; every iteration forms them again in LDS -- the same values in the same
// order -- which is cheaper than three more planes to write and read.)
//
// Launches per call: levels (grey + pyramid of both images, one per level) + levels * iters + 1 (output pass).
#include "optical_flow_kernels.h"

namespace t2v {

int optical_flow_default_levels(int H, int W) {
    int n = 1;
    while (n < 6 && ((H + 1) / 2 < (W + 1) / 2 ? (H + 1) / 2 : (W + 1) / 2) >= 16) {
        H = (H + 1) / 2;
        W = (W + 1) / 2;
        ++n;
    }
    return n;
}

bool optical_flow_shape_ok(int H, int W, int levels) {
    // (the planes are indexed with ints)
    return H >= 8 && W >= 8 && (long)H * W <= (1L << 28) && levels >= 0 && levels <= kMaxLevels;
}

size_t optical_flow_workspace_floats(int H, int W, int levels) {
    if (levels == 0) levels = optical_flow_default_levels(H, W);
    size_t n = 0;
    for (int l = 0; l < levels; ++l) {
        n += (size_t)6 * H * W;      // grey cur, grey prev, two (u, v) planes
        H = (H + 1) / 2;
        W = (W + 1) / 2;
    }
    return n;
}

namespace {

// everything but the source of the finest level's grey images: grey(g_cur, g_prev) enqueues the one launch that writes them
template <class GreyLaunch>
int launch_flow(hipStream_t s, GreyLaunch grey, int H, int W, int levels, int iters, int radius, float lambda, float* workspace,
                float* flow_out) {
    if (levels == 0) levels = optical_flow_default_levels(H, W);
    int hs[kMaxLevels], ws[kMaxLevels];
    float *g_cur[kMaxLevels], *g_prev[kMaxLevels];
    float2* uv[kMaxLevels][2];
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
    grey(g_cur[0], g_prev[0]);
    for (int l = 1; l < levels; ++l)
        hipLaunchKernelGGL(flow_pool_kernel, dim3(blocks_for((long)hs[l] * ws[l]), 2), dim3(256), 0, s, g_cur[l - 1],
                           g_prev[l - 1], g_cur[l], g_prev[l], hs[l - 1], ws[l - 1], hs[l], ws[l]);
    const float lam_n = (float)((double)lambda * (2 * radius + 1) * (2 * radius + 1));
    const int last = (iters - 1) % 2;          // the (u, v) plane a level's last iteration writes
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
                a.src = uv[l + 1][last];
                a.sh = hs[l + 1];
                a.sw = ws[l + 1];
                hipLaunchKernelGGL(flow_lk_kernel<2>, grid, dim3(256), 0, s, a);
            } else {
                a.src = nullptr;
                a.sh = a.sw = 0;
                hipLaunchKernelGGL(flow_lk_kernel<0>, grid, dim3(256), 0, s, a);
            }
        }
    }
    hipLaunchKernelGGL(flow_out_kernel, dim3(blocks_for((long)H * W)), dim3(256), 0, s, uv[0][last],
                       reinterpret_cast<float4*>(flow_out), H, W);
    T2V_HIP_CHECK(hipGetLastError());
    return T2V_OK;
}

}  // namespace

int launch_optical_flow(hipStream_t s, const float* cur, int cur_cs, int cur_c0, const float* prev, int prev_cs, int prev_c0,
                        int H, int W, int levels, int iters, int radius, float lambda, float* workspace, float* flow_out) {
    return launch_flow(
        s,
        [&](float* g_cur, float* g_prev) {
            hipLaunchKernelGGL(flow_grey_kernel, dim3(blocks_for((long)H * W), 2), dim3(256), 0, s, cur, cur_cs, cur_c0, prev,
                               prev_cs, prev_c0, g_cur, g_prev, (long)H * W);
        },
        H, W, levels, iters, radius, lambda, workspace, flow_out);
}

int launch_optical_flow_u8(hipStream_t s, const uint8_t* cur, int cur_cs, const uint8_t* prev, int prev_cs, int H, int W,
                           int levels, int iters, int radius, float lambda, float* workspace, float* flow_out) {
    return launch_flow(
        s,
        [&](float* g_cur, float* g_prev) {
            hipLaunchKernelGGL(flow_grey_u8_kernel, dim3(blocks_for((long)H * W), 2), dim3(256), 0, s, cur, cur_cs, prev, prev_cs,
                               g_cur, g_prev, (long)H * W);
        },
        H, W, levels, iters, radius, lambda, workspace, flow_out);
}

}  // namespace t2v
